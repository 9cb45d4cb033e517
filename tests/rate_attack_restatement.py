"""The bitrate attack (attack_rd -r) restated with oracle.codec functions and autograd, following the dtype it is
given, plus the seeded inputs and float64 references of the ica_rate kernels' tests.

Loss of the expensive branch, per image (DESIGN.md "Rate attack"):

    y = g_a(im_in)                                              (no rounding, no noise)
    hyper:      z = h_a(|y|); lik_z = EB(z); sigma = h_s(z); lik_y = GC(y, sigma)
    factorized: lik_y = EB(y)
    loss_o = sum(ln lik) / (ln 2 * H * W) = -bpp_relaxed(im_in)   (minimised)

The likelihoods are oracle.codec.forward(P, x, model, training=True, noise_y=0, noise_z=0)["likelihoods"]
(tests/test_cpu_rate_attack.py checks that they are); g_s is not run.  ``attack`` is the step loop of
oracle.attack.attack with that expensive branch: same prologue, L-inf box, per-image branch rule, Adam, LR schedule
and eval.

Kernel cases (tests/test_gpu_rate_attack.py): gc_case / eb_case build hand-made tensors with planted values, gc_ref /
eb_ref are autograd of oracle.codec.gc_likelihood / eb_likelihood in a dtype.  Every bound of RATE_TOL is
4 max(e_ref, 2^-24) rounded up to one digit, e_ref being the distance of the fp32 CPU autograd from the float64 one on
the same inputs (rel_err = max |a - b| / max |b|).  The floor 2^-24 is one fp32 rounding: an fp32 number is no closer
to the float64 one than that except by chance, and on the smallest shapes the CPU sums land closer by chance.
tests/test_cpu_rate_attack.py prints the table and checks that the fp32 restatement alone stays inside each bound.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle import attack as oatt
from oracle import codec
from tests import loss_refs as R

MODELS = ("hyper", "factorized")


def to_dtype(P, dtype):
    return {k: v.to(dtype) for k, v in P.items()}


def relaxed_likelihoods(P, x, model):
    """Train-mode likelihoods of the unrounded latents with zero noise; g_s is not run."""
    y = codec.g_a(P, x)
    if model == "factorized":
        _, y_lik = codec.entropy_bottleneck(P, y, True, torch.zeros_like(y))
        return {"y": y_lik}
    if model != "hyper":
        raise NotImplementedError(model)
    z = codec.h_a(P, torch.abs(y))
    z_hat, z_lik = codec.entropy_bottleneck(P, z, True, torch.zeros_like(z))
    scales = codec.h_s(P, z_hat)
    _, y_lik = codec.gaussian_conditional(y, scales, None, True, torch.zeros_like(y))
    return {"y": y_lik, "z": z_lik}


def loss_o(P, x, model):
    """Per-image sum(ln lik) / (ln 2 * H * W) = -bpp_relaxed [B]."""
    H, W = x.shape[2:]
    liks = relaxed_likelihoods(P, x, model)
    return sum(torch.log(l).flatten(1).sum(1) for l in liks.values()) / (math.log(2) * H * W)


def input_grad(P, x, model, dtype=torch.float64):
    """(loss_o [B], d sum_b loss_o / d x) in dtype."""
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    lo = loss_o(to_dtype(P, dtype), xr, model)
    lo.sum().backward()
    return lo.detach(), xr.grad


def attack(P, im_s, steps=1001, epsilon=16.0, noise_thr=1e-4, lr=0.01, clamp=True, model="hyper", init_noise=None,
           eval_msssim=True, record=None, dtype=torch.float32):
    """oracle.attack.attack (per image, att_metric L2) with the rate loss in the expensive branch.
    record: optional list; per step appends dict(loss_i, cheap, lr, loss_o [B] (NaN for cheap images))."""
    if model not in MODELS:
        raise NotImplementedError(model)
    P = to_dtype(P, dtype)
    im_s = im_s.to(dtype)
    B = im_s.shape[0]
    with torch.no_grad():
        H, W = im_s.shape[2:]
        res = codec.forward(P, im_s, model)
        output_s = torch.clamp(res["x_hat"], 0.0, 1.0) if clamp else res["x_hat"]
        bpp_ori = torch.stack([codec.bpp({k: v[b:b + 1] for k, v in res["likelihoods"].items()}, H * W)
                               for b in range(B)])
    noise_range = epsilon / 255.0
    noise = torch.zeros_like(im_s) if init_noise is None else init_noise.to(dtype).clone()
    noise.requires_grad_(True)
    opt = torch.optim.Adam([noise], lr=lr)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, [1, 2, 3], gamma=0.33)
    im_in = None
    for i in range(steps):
        noise_c = codec.UpBound.apply(codec.LowBound.apply(noise, -noise_range), noise_range)
        im_in = codec.UpBound.apply(codec.LowBound.apply(im_s + noise_c, 0.0), 1.0)
        li_b = oatt._per_image_mean((im_s - im_in) ** 2)
        cheap = li_b > noise_thr
        losses = torch.zeros((), dtype=dtype)
        lo_b = torch.full((B,), float("nan"), dtype=dtype)
        if bool(cheap.any()):
            idx = cheap.nonzero().flatten()
            losses = losses + oatt._per_image_mean((im_s[idx] - im_in[idx]) ** 2).sum()
        if bool((~cheap).any()):
            idx = (~cheap).nonzero().flatten()
            lo = loss_o(P, im_in[idx], model)
            lo_b[idx] = lo.detach()
            losses = losses + lo.sum()
        if record is not None:
            record.append({"loss_i": li_b.detach().clone(), "cheap": cheap.clone(), "lr": opt.param_groups[0]["lr"],
                           "loss_o": lo_b})
        opt.zero_grad()
        losses.backward()
        opt.step()
        if i % max(steps // 3, 1) == 0:
            sch.step()
    im_in = im_in.detach()
    ev = oatt.eval_batch(P, im_in, im_s, output_s, model, clamp, adv=False, msssim=eval_msssim)
    return SimpleNamespace(im_adv=ev.im, output_adv=ev.out, output_s=output_s, bpp_ori=bpp_ori, bpp=ev.bpp, eval=ev,
                           noise=noise.detach(), im_in=im_in)


def params(model):
    """The seeded quality-1 parameters of the chain, trajectory and compaction cases."""
    return codec.perturb_params(codec.init_params(model, 1, seed=0), seed=1)


def image(shape, seed):
    return R.rnd(shape, seed)


# Trajectory case.  With these seeded weights |d loss_o / d im_in| is 1e-8 .. 1e-6, near Adam's eps = 1e-8, so a step
# moves the noise by much less than lr and loss_i stays far below 1e-3: on the restatement all 6 * B image-steps take
# the expensive branch (tests/test_cpu_rate_attack.py checks the condition, at least 3 * B).  The branch that mixes
# cheap and expensive images in one step is the compaction case's.
TRAJ = dict(shape=(2, 3, 64, 64), seed=43, steps=6, noise_thr=1e-3)
TRAJ_TOL = dict(noise=2e-3, bpp=1e-3, mse_in=1e-3)


# --------------------------------------------------------------------------- #
# Kernel cases
# --------------------------------------------------------------------------- #
KERNEL_SHAPES = [(3, 8, 1, 1), (3, 8, 7, 9), (2, 6, 5, 3), (2, 192, 4, 6), (2, 320, 4, 6), (1, 8, 33, 47)]
KERNEL_SCALE = 1.0 / (math.log(2) * 64 * 64)   # the attack's scale for a 64 x 64 image

# Non-planted GaussianConditional elements: sigma in [0.15, 2] (above the 0.11 bound by 0.04) and |y| / sigma in
# [0, 3].  Then upper = Phi((.5 - |y|) / sigma) >= Phi(-3 + .5 / 2) = 3e-3 and lower <= Phi(-.25) = 0.40 with
# upper - lower >= 2.4e-3: neither the difference nor 1 / lik amplifies an fp32 rounding of erfc by more than ~400.
GC_SIGMA = (0.15, 2.0)
GC_RATIO = 3.0
# Planted (y, sigma); gy / gsig that must be exactly 0 are marked
GC_PLANTED = [
    (0.0, 0.7),      # y == 0: zero sign, gy == 0
    (0.4, 0.0),      # sigma == 0: the dead ReLU, gsig == 0 (gy through s = 0.11 is not)
    (0.0, 0.05),     # 0 < sigma < 0.11, dL/dsigma < 0: passes the scale bound (and gy == 0)
    (0.05, 0.03),    # the same sign with y != 0
    (0.8, 0.05),     # 0 < sigma < 0.11, dL/dsigma > 0 (zu = -2.7 at s = 0.11): blocked, gsig == 0
    (-0.75, 0.1),    # the same, negative y
    (5.0, 0.5),      # |y| / sigma = 10: lraw = 1e-19 < 1e-9, gy == gsig == 0
    (-9.0, 0.05),    # the same below the scale bound
]
# Non-planted EntropyBottleneck values: |v| <= 30, where the likelihood under loss_refs.eb_params is > 3e-5.
EB_RANGE = 30.0
# Planted v: zero, the far tails (lraw < 1e-9 in fp32 and float64: gv == 0 exactly) and values next to them
EB_PLANTED = [0.0, 600.0, -600.0, 0.5, -0.5, 450.0, -450.0, 12.25]
EB_FAR = 400.0


def _plant(t, values):
    """The first elements of the flattened tensor cycle through `values` (as many as fit, at most 3 rounds); the
    first and last element of plane [0, 0] and the last element of the tensor get values[0] / values[-1]."""
    flat = t.reshape(-1)
    n = min(flat.numel(), 3 * len(values))
    flat[:n] = torch.tensor(values, dtype=t.dtype).repeat(3)[:n]
    return n


def gc_case(shape, seed=301):
    """(y, sigma, planted) NCHW fp32: planted is a bool mask of the planted elements."""
    B, C, H, W = shape
    g = R.gen(seed + C + 7 * H + B)
    sigma = GC_SIGMA[0] + (GC_SIGMA[1] - GC_SIGMA[0]) * torch.rand(shape, generator=g)
    ratio = GC_RATIO * torch.rand(shape, generator=g)
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(1.0), torch.tensor(-1.0))
    y = sign * ratio * sigma
    planted = torch.zeros(shape, dtype=torch.bool)
    n = _plant(y, [p[0] for p in GC_PLANTED])
    _plant(sigma, [p[1] for p in GC_PLANTED])
    planted.reshape(-1)[:n] = True
    # first and last element of a plane, last element of the tensor
    for (b, c, h, w), (yv, sv) in (((B - 1, C - 1, 0, 0), GC_PLANTED[4]), ((B - 1, C - 1, H - 1, W - 1), GC_PLANTED[6])):
        y[b, c, h, w], sigma[b, c, h, w], planted[b, c, h, w] = yv, sv, True
    return y, sigma, planted


def gc_ref(y, sigma, scale=KERNEL_SCALE, dtype=torch.float64):
    """(dL/dy, dL/dpre, sum ln lik [B]) of L = scale * sum ln GC(y, relu(pre)) at pre = sigma (>= 0), in dtype: the
    backward of the ReLU that ends h_s is part of the gradient (relu'(0) = 0)."""
    yr = y.detach().to(dtype).clone().requires_grad_(True)
    pre = sigma.detach().to(dtype).clone().requires_grad_(True)
    ln = torch.log(codec.gc_likelihood(yr, F.relu(pre)))
    (scale * ln.sum()).backward()
    return yr.grad, pre.grad, ln.detach().flatten(1).sum(1)


def eb_case(shape, seed=311):
    """(P, v, planted): loss_refs.eb_params for C channels, v NCHW fp32."""
    B, C, H, W = shape
    P = R.eb_params(C)
    g = R.gen(seed + C + 7 * H + B)
    v = (torch.rand(shape, generator=g) * 2 - 1) * EB_RANGE
    planted = torch.zeros(shape, dtype=torch.bool)
    n = _plant(v, EB_PLANTED)
    planted.reshape(-1)[:n] = True
    for (b, c, h, w), val in (((B - 1, C - 1, 0, 0), EB_PLANTED[1]), ((B - 1, C - 1, H - 1, W - 1), EB_PLANTED[2])):
        v[b, c, h, w], planted[b, c, h, w] = val, True
    return P, v, planted


def eb_ref(P, v, scale=KERNEL_SCALE, dtype=torch.float64):
    """(dL/dv, sum ln lik [B]) of L = scale * sum ln EB(v) through oracle.codec.eb_likelihood, in dtype."""
    vr = v.detach().to(dtype).clone().requires_grad_(True)
    ln = torch.log(R._nchw(codec.eb_likelihood(to_dtype(P, dtype), R._cl(vr, v.shape[1])), v.shape))
    (scale * ln.sum()).backward()
    return vr.grad, ln.detach().flatten(1).sum(1)


def shape_key(shape):
    return "x".join(str(v) for v in shape)


# shape: bounds of (gy, gsig, sumln) for rate_gc and (gv, sumln) for rate_eb        e_ref
RATE_TOL = {
    "3x8x1x1": dict(gy=7e-07, gsig=4e-07, gc_sumln=3e-07, gv=4e-05, eb_sumln=3e-07),
    # e_ref 1.69e-07, 9.48e-08, 1.19e-08, 8.69e-06, 3.41e-08
    "3x8x7x9": dict(gy=7e-07, gsig=8e-07, gc_sumln=5e-07, gv=1e-05, eb_sumln=3e-07),
    # e_ref 1.69e-07, 1.94e-07, 1.01e-07, 2.49e-06, 6.20e-08
    "2x6x5x3": dict(gy=7e-07, gsig=7e-07, gc_sumln=5e-07, gv=1e-05, eb_sumln=5e-07),
    # e_ref 1.69e-07, 1.67e-07, 1.22e-07, 2.37e-06, 1.03e-07
    "2x192x4x6": dict(gy=7e-07, gsig=2e-06, gc_sumln=4e-07, gv=9e-06, eb_sumln=3e-07),
    # e_ref 1.69e-07, 3.06e-07, 9.21e-08, 2.11e-06, 5.25e-08
    "2x320x4x6": dict(gy=7e-07, gsig=2e-06, gc_sumln=3e-07, gv=9e-06, eb_sumln=3e-07),
    # e_ref 1.69e-07, 2.71e-07, 3.54e-08, 2.11e-06, 5.18e-08
    "1x8x33x47": dict(gy=7e-07, gsig=2e-06, gc_sumln=3e-07, gv=2e-05, eb_sumln=3e-07),
    # e_ref 1.69e-07, 2.82e-07, 6.22e-08, 2.54e-06, 3.25e-08
}
