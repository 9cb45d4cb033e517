"""The RD evaluation (batch_test, the reference's test.py) restated with oracle.codec functions and torch, following
the dtype it is given, plus the seeded cases and bounds of the ica_rd_metrics kernel's tests.

Per image (train.RateDistortionLoss(training=False) with N = 1, train.py:50-70):

    bpp     = sum over the likelihood tensors of  sum ln max(lik, 2^-16) / (-ln 2 * H * W)
    mse     = mean((clamp(x_hat, 0, 1) - target)^2)
    msim    = pytorch_msssim.ms_ssim(clamp(x_hat), target)   (oracle.msssim; nan where min(H, W) <= 160)
    psnr    = -10 log10(mse),  msim_dB = -10 log10(1 - msim)  (float64 of the value; 0 gives inf)

``kernel_ref`` gives the kernel's five outputs in a dtype, ``metrics`` the composed per-image numbers from a
codec.forward-style output dict, ``defended`` test.py:37-49 composed from oracle.defend's torch restatements.

Kernel bounds (KERNEL_TOL): each is 4 max(e_ref, 2^-24) rounded up to one digit, e_ref being the distance of the fp32
CPU restatement from the float64 one on the same inputs (rel_err = max |a - b| / max |b| over the batch).  The floor
2^-24 is one fp32 rounding: an fp32 number is no closer to the float64 one than that except by chance, and on the
smallest shapes the CPU sums land closer by chance.  nclamp and the clamped image are compared bit for bit: the
inputs are fp32 numbers both dtypes hold exactly, so the comparison with 2^-16 and the clamp select the same
elements.  tests/test_cpu_rd_eval.py prints the table and checks that the fp32 restatement alone stays inside it.

Composition bounds (FORWARD_TOL): the eval forward's own tolerances of tests/test_gpu_defend.py (bpp and mse
relative 1e-3), and what follows from them through the logarithms:

    psnr = -10 log10(mse):  |d psnr| = 10 |log10(mse' / mse)| <= 10 log10(1 + 1e-3) = 4.341e-3 dB   -> 4.4e-3 dB
    msim: absolute 1e-5, the bound tests/test_gpu_attack.py puts on the same kernel's eval values
    msim_dB = -10 log10(1 - msim):  |d msim_dB| <= 10 log10(1 + 1e-5 / (1 - msim_ref - 1e-5)), from the
              reference's own msim (msim_db_bound); at msim_ref = 0.9 that is 4.3e-4 dB
"""
import math

import torch

from oracle import codec
from oracle import defend as odef
from oracle import msssim as omsssim
from tests import loss_refs as R

LIK_MIN = 2.0 ** -16
ENGINE_FLOOR = 1e-9          # CompressAI's likelihood LowerBound: the smallest value the eval forward emits
# Non-planted likelihoods stay outside (LIK_MIN / BAND, LIK_MIN * BAND)
BAND = 2.0
MSSSIM_MIN_SIDE = 160


def to_dtype(P, dtype):
    return {k: v.to(dtype) for k, v in P.items()}


# --------------------------------------------------------------------------- #
# Restatement
# --------------------------------------------------------------------------- #
def kernel_ref(x_hat, target, lik_y, lik_z=None, dtype=torch.float64):
    """(sse [B], lny [B], lnz [B], nclamp [B] int64, clamp(x_hat, 0, 1)) in dtype."""
    out = torch.clamp(x_hat.to(dtype), 0.0, 1.0)
    sse = ((out - target.to(dtype)) ** 2).flatten(1).sum(1)

    def plane(lik):
        if lik is None:
            return torch.zeros(x_hat.shape[0], dtype=dtype), torch.zeros(x_hat.shape[0], dtype=torch.int64)
        l = lik.to(dtype)
        return torch.log(torch.clamp(l, min=LIK_MIN)).flatten(1).sum(1), (l < LIK_MIN).flatten(1).sum(1)

    (lny, ny), (lnz, nz) = plane(lik_y), plane(lik_z)
    return sse, lny, lnz, ny + nz, out


def neg10log10(v):
    return -10.0 * torch.log10(v.detach().double())


def metrics(output, target):
    """Per-image RateDistortionLoss(output, target, training=False), N = 1, in the dtype of ``output``: a dict of
    [B] tensors (psnr / msim_dB float64)."""
    B, _, H, W = target.shape
    liks = output["likelihoods"]
    sse, lny, lnz, nclamp, out = kernel_ref(output["x_hat"], target, liks["y"], liks.get("z"), output["x_hat"].dtype)
    den = -math.log(2) * (H * W)
    bpp_y, bpp_z = lny / den, lnz / den
    mse = sse / (3 * H * W)
    if min(H, W) > MSSSIM_MIN_SIDE:
        msim = omsssim.ms_ssim_per_image(out, target.to(out.dtype))
    else:
        msim = torch.full_like(mse, float("nan"))
    return {"bpp": bpp_y + bpp_z, "bpp_y": bpp_y, "bpp_z": bpp_z, "mse": mse, "psnr": neg10log10(mse), "msim": msim,
            "msim_dB": neg10log10(1.0 - msim.double()), "nclamp": nclamp, "x_hat": out}


def plain(P, x, model, dtype=torch.float64):
    """test.py:51-52: criterion(net(im), im, training=False) per image."""
    with torch.no_grad():
        return metrics(codec.forward(to_dtype(P, dtype), x.to(dtype), model), x.to(dtype))


def defended(P, x, method, model="hyper", dtype=torch.float64, pre=None, profile=None):
    """test.py:37-49 per image, scored against the original x.  pre (tests): the preprocessed image of 'resize' /
    'bitdepth' as the GPU made it, so that the codec part is compared on identical inputs.  profile: (cmax, cmin)
    [C] of 'range' (attack_rd.py:263-268: clamp_value_naive, likelihoods of the clamped y, g_s(round(y)))."""
    P = to_dtype(P, dtype)
    x = x.to(dtype)
    with torch.no_grad():
        if method == "ensemble":
            outs, best = [], []
            for b in range(x.shape[0]):
                xs = odef.rotates(x[b:b + 1])
                pick = (float("inf"), 0, None)
                for i, xv in enumerate(xs):
                    res = codec.forward(P, xv, model)
                    m = float(torch.mean((xv - res["x_hat"]) ** 2))
                    if m < pick[0]:
                        pick = (m, i, res)
                _, i, res = pick
                back = torch.clamp(odef.rotates(res["x_hat"], reverse=i), 0.0, 1.0)
                outs.append(metrics({"x_hat": back, "likelihoods": res["likelihoods"]}, x[b:b + 1]))
                best.append(i)
            out = {k: torch.cat([o[k] for o in outs], 0) for k in outs[0]}
            out["best_idx"] = best
            return out
        if method == "range":
            cmax, cmin = (t.to(dtype).reshape(1, -1, 1, 1) for t in profile)
            y = codec.g_a(P, x)
            y = torch.where(y > cmax, cmax, y)
            y = torch.where(y < cmin, cmin, y)
            z = codec.h_a(P, torch.abs(y))
            z_hat, z_lik = codec.entropy_bottleneck(P, z)
            _, y_lik = codec.gaussian_conditional(y, codec.h_s(P, z_hat))
            return metrics({"x_hat": codec.g_s(P, torch.round(y)), "likelihoods": {"y": y_lik, "z": z_lik}}, x)
        if pre is not None:
            xp = pre.to(dtype)
        else:
            xp = odef.bitdepth_reduction(x) if method == "bitdepth" else odef.random_resize(x, 243 / 256)
        return metrics(codec.forward(P, xp, model), x)


# --------------------------------------------------------------------------- #
# Composition cases: seeded perturbed quality-1 parameters, g_a's last layer scaled by 40 (as
# tests/test_gpu_rate_attack.py scales it) so that the latents do not all round to 0
# --------------------------------------------------------------------------- #
LATENT_GAIN = 40.0
FORWARD_TOL = dict(bpp=1e-3, mse=1e-3, psnr=4.4e-3, msim=1e-5)
FORWARD_CASES = [   # (model, shape, image seed)
    ("hyper", (2, 3, 64, 64), 71), ("hyper", (1, 3, 64, 128), 72),
    ("factorized", (2, 3, 64, 64), 71), ("factorized", (1, 3, 64, 128), 72),
    ("context", (1, 3, 64, 64), 73), ("cheng2020", (1, 3, 64, 64), 74),
]
MSIM_CASE = ("hyper", (1, 3, 192, 192), 75)   # the smallest multiple of 64 above pytorch_msssim's 160
# Defended cases, hyper.  random_resize(x, 243 / 256) gives back the input size only for sides divisible by 256
# (64 -> 60 -> 63: the reference's mse against the original raises there, and so does rd_eval_defended), so the
# resize case runs at the smallest size the defence is defined for.
DEFEND_CASES = {"ensemble": ((1, 3, 64, 64), 76), "bitdepth": ((1, 3, 64, 64), 77), "range": ((1, 3, 64, 64), 78),
                "resize": ((1, 3, 256, 256), 79)}


def range_profile(P, x, shrink=0.5):
    """(cmax, cmin) [C]: each channel's float64 extremes over x, shrunk so that the clamp changes latents."""
    with torch.no_grad():
        y = codec.g_a(to_dtype(P, torch.float64), x.double())
    return (y.amax(dim=(0, 2, 3)) * shrink).float(), (y.amin(dim=(0, 2, 3)) * shrink).float()


def params(model):
    P = codec.perturb_params(codec.init_params(model, 1, seed=0), seed=1)
    for k in ("g_a.6.weight", "g_a.6.bias"):
        P[k] = P[k] * LATENT_GAIN
    return P


def image(shape, seed):
    return R.rnd(shape, seed)


def msim_db_bound(msim_ref):
    """|d msim_dB| for |d msim| <= FORWARD_TOL['msim'] around the reference's msim (see the module docstring)."""
    d = FORWARD_TOL["msim"]
    return 10.0 * math.log10(1.0 + d / (1.0 - msim_ref - d))


def forward_errors(got, ref):
    """{bpp: rel, mse: rel, psnr: abs dB} of per-image dicts / objects against the float64 reference."""
    g = lambda k: (got[k] if isinstance(got, dict) else getattr(got, k)).detach().double().cpu()
    return {"bpp": float(((g("bpp") - ref["bpp"]).abs() / ref["bpp"].abs()).max()),
            "mse": float(((g("mse") - ref["mse"]).abs() / ref["mse"].abs()).max()),
            "psnr": float((g("psnr") - ref["psnr"]).abs().max())}


# --------------------------------------------------------------------------- #
# Kernel cases
# --------------------------------------------------------------------------- #
# (image shape, y likelihood shape, z likelihood shape or None): the smallest shapes where the kernel can go wrong
# (one element, C not a multiple of 4, more quads than one block's threads, odd sizes, no z plane)
KERNEL_CASES = [
    ((3, 3, 1, 1), (3, 8, 1, 1), (3, 8, 1, 1)),
    ((2, 3, 16, 16), (2, 6, 5, 3), (2, 192, 4, 6)),
    ((2, 3, 33, 47), (2, 320, 4, 6), (2, 6, 5, 3)),
    ((1, 3, 64, 128), (1, 8, 33, 47), None),
    ((2, 3, 33, 47), (2, 192, 4, 6), None),
]
# Planted likelihoods: exactly 2^-16 (not clamped, not counted), the fp32 neighbours above and below it, the
# engine's floor and 1.0
LIK_ABOVE = float(torch.nextafter(torch.tensor(LIK_MIN), torch.tensor(1.0)))
LIK_BELOW = float(torch.nextafter(torch.tensor(LIK_MIN), torch.tensor(0.0)))
LIK_PLANTED = [LIK_MIN, LIK_ABOVE, LIK_BELOW, ENGINE_FLOOR, 1.0]
# Planted reconstructions: below 0, above 1, exactly 0 and 1, and -0.0
XHAT_PLANTED = [-0.25, 1.5, 0.0, 1.0, -0.0, -1e-8, 1.0000001]
XHAT_RANGE = (-0.3, 1.3)


def case_key(case):
    return "+".join("none" if s is None else "x".join(str(v) for v in s) for s in case)


def _plant(t, values):
    """The first elements of the flattened tensor cycle through `values` (as many as fit, at most 3 rounds); the first
    and last element of the last plane (which ends the tensor) get values[-2] / values[-3].  Returns the mask."""
    flat = t.reshape(-1)
    mask = torch.zeros(t.shape, dtype=torch.bool)
    n = min(flat.numel(), 3 * len(values))
    flat[:n] = torch.tensor(values, dtype=t.dtype).repeat(3)[:n]
    mask.reshape(-1)[:n] = True
    B, C, H, W = t.shape
    for (h, w), v in (((0, 0), values[-2]), ((H - 1, W - 1), values[-3])):
        t[B - 1, C - 1, h, w], mask[B - 1, C - 1, h, w] = v, True
    return mask


def lik_case(shape, seed):
    """(lik fp32 NCHW, planted mask): log-uniform in [1e-9, 1], nothing but planted values inside the band."""
    g = R.gen(seed + shape[1] + 7 * shape[2] + shape[0])
    lik = torch.exp(torch.rand(shape, generator=g) * math.log(ENGINE_FLOOR)).clamp(ENGINE_FLOOR, 1.0)
    lik = torch.where(in_band(lik), torch.tensor(0.5), lik)
    return lik, _plant(lik, LIK_PLANTED)


def in_band(lik):
    return (lik > LIK_MIN / BAND) & (lik < LIK_MIN * BAND)


def kernel_case(case, seed=401):
    """dict(x_hat, target, lik_y, lik_z or None, planted_y, planted_z): NCHW fp32."""
    img, ys, zs = case
    g = R.gen(seed + img[2] + 3 * img[0])
    x_hat = XHAT_RANGE[0] + (XHAT_RANGE[1] - XHAT_RANGE[0]) * torch.rand(img, generator=g)
    _plant(x_hat, XHAT_PLANTED)
    target = torch.rand(img, generator=g)
    lik_y, py = lik_case(ys, seed + 11)
    lik_z, pz = lik_case(zs, seed + 23) if zs is not None else (None, None)
    return dict(x_hat=x_hat, target=target, lik_y=lik_y, lik_z=lik_z, planted_y=py, planted_z=pz)


def kernel_errors(got, ref):
    """rel_err of (sse, lny, lnz) tuples; lnz 0 where both are exactly 0 (no z plane)."""
    e = {}
    for k, a, b in zip(("sse", "lny", "lnz"), got, ref):
        e[k] = 0.0 if (not bool(b.any()) and not bool(a.any())) else R.rel_err(a, b)
    return e


# case: bounds of (sse, lny, lnz)                                              e_ref
KERNEL_TOL = {
    "3x3x1x1+3x8x1x1+3x8x1x1": dict(sse=3e-07, lny=3e-07, lnz=3e-07),
    # e_ref 4.41e-08, 9.74e-09, 2.89e-08
    "2x3x16x16+2x6x5x3+2x192x4x6": dict(sse=3e-07, lny=3e-07, lnz=3e-07),
    # e_ref 6.28e-08, 6.01e-08, 3.53e-08
    "2x3x33x47+2x320x4x6+2x6x5x3": dict(sse=3e-07, lny=3e-07, lnz=3e-07),
    # e_ref 6.42e-08, 1.83e-08, 3.15e-08
    "1x3x64x128+1x8x33x47+none": dict(sse=3e-07, lny=3e-07, lnz=0.0),
    # e_ref 1.62e-09, 5.21e-08, no z plane: exactly 0
    "2x3x33x47+2x192x4x6+none": dict(sse=3e-07, lny=3e-07, lnz=0.0),
    # e_ref 6.42e-08, 7.09e-08, no z plane: exactly 0
}
