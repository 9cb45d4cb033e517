"""Plain-torch references of the loss side (MS-SSIM, entropy models, weight gradients) that follow the dtype they
are given, and the seeded inputs of the tests that use them: tests/test_cpu_loss_refs.py measures how far the fp32
reference is from the float64 one on these inputs (e_ref), and tests/test_gpu_msssim_edges.py,
test_gpu_entropy_kernels.py and test_gpu_train_kernels.py compare the HIP kernels with the float64 one.

ms_ssim_per_image   oracle.msssim.ms_ssim_per_image (pytorch_msssim variant, mode 0; already follows dtype)
torch_msssim        utils/torch_msssim.py:26-71 (mode 1): the oracle's window (built in fp32 as there), cast to the
                    input dtype, so the fp32 result is the oracle's bit for bit
eb_lik / gc_lik     oracle.codec.eb_likelihood / gc_likelihood (LowBound included) on NCHW tensors, with the
                    per-image sum of log likelihoods
eb_bwd / gc_bwd     autograd of those under an upstream dL/dlik
wgrad               autograd of F.conv2d / F.conv_transpose2d with respect to the weight

The quantised tensors (round(v - med) + med, v + noise) are fp32 statements checked bit for bit; the likelihood
references take the fp32 quantised tensor as their input, so |delta log lik| measures the likelihood alone.
"""
import math

import torch
import torch.nn.functional as F

from oracle import codec
from oracle import msssim as omsssim

LIK_FLOOR = codec.LIKELIHOOD_BOUND   # 1e-9
SCALE_FLOOR = codec.SCALE_BOUND      # 0.11
EB_NAMES = [f"_matrix{i}" for i in range(5)] + [f"_bias{i}" for i in range(5)] + [f"_factor{i}" for i in range(4)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, lo=0.0, hi=1.0):
    return torch.rand(shape, generator=gen(seed)) * (hi - lo) + lo


def rel_err(a, b):
    """tests.conftest.rel_err on torch tensors: max |a - b| / max |b| in float64."""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def log_err(lik, ref):
    """max |log lik - log ref| in float64."""
    return float((lik.detach().double().log() - ref.detach().double().log()).abs().max())


def round_up_1digit(x):
    """x rounded up to one significant digit (the rule of the GPU tolerances: 4 e_ref rounded up)."""
    if x <= 0.0:
        return 0.0
    e = math.floor(math.log10(x))
    m = math.ceil(x / 10.0 ** e - 1e-9)
    return float(f"{m}e{e}") if m < 10 else float(f"1e{e + 1}")


# --------------------------------------------------------------------------- #
# MS-SSIM
# --------------------------------------------------------------------------- #
ms_ssim_per_image = omsssim.ms_ssim_per_image


def _ssim_tm(img1, img2, max_val):
    _, c, h, w = img1.shape
    ws = min(h, w, 11)
    window = omsssim._window_tm(ws, 1.5 * ws / 11, c).to(img1.dtype)
    p = ws // 2
    mu1 = F.conv2d(img1, window, padding=p, groups=c)
    mu2 = F.conv2d(img2, window, padding=p, groups=c)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(img1 * img1, window, padding=p, groups=c) - mu1_sq
    s2 = F.conv2d(img2 * img2, window, padding=p, groups=c) - mu2_sq
    s12 = F.conv2d(img1 * img2, window, padding=p, groups=c) - mu1_mu2
    C1 = (0.01 * max_val) ** 2
    C2 = (0.03 * max_val) ** 2
    V1 = 2.0 * s12 + C2
    V2 = s1 + s2 + C2
    ssim_map = ((2 * mu1_mu2 + C1) * V1) / ((mu1_sq + mu2_sq + C1) * V2)
    return ssim_map.mean(), (V1 / V2).mean()


def torch_msssim(img1, img2, max_val=1.0, levels=5):
    weight = torch.tensor(omsssim.MS_WEIGHTS).to(img1.dtype)
    ms, mcs = [], []
    for _ in range(levels):
        s, c = _ssim_tm(img1, img2, max_val)
        ms.append(s)
        mcs.append(c)
        if len(ms) < levels:   # the reference also pools after the last level, which a 1-row map does not survive
            img1 = F.avg_pool2d(img1, kernel_size=2, stride=2)
            img2 = F.avg_pool2d(img2, kernel_size=2, stride=2)
    ms = torch.stack(ms)
    mcs = torch.stack(mcs)
    return torch.prod(mcs[: levels - 1] ** weight[: levels - 1]) * (ms[levels - 1] ** weight[levels - 1])


def msssim_value_and_grad(X, Y, dval, data_range=1.0, mode=0, dtype=torch.float64):
    """(value[groups], dX, dY) of sum(value * dval) in `dtype`: what msssim.ms_ssim_value_and_grad returns."""
    Xr = X.detach().to(dtype).clone().requires_grad_(True)
    Yr = Y.detach().to(dtype).clone().requires_grad_(True)
    v = ms_ssim_per_image(Xr, Yr, data_range) if mode == 0 else torch_msssim(Xr, Yr, data_range).reshape(1)
    (v * dval.to(dtype)).sum().backward()
    return v.detach(), Xr.grad, Yr.grad


# name: (mode, shape, data_range, dval).  Inputs lie in [0, 1] and are multiplied by data_range.
MSSSIM_CASES = {
    "m0_161x163_dr1": (0, (2, 3, 161, 163), 1.0, (1.0, -0.5)),
    "m0_161x163_dr255": (0, (2, 3, 161, 163), 255.0, (1.0, -0.5)),
    "m0_177x200_dr1": (0, (2, 3, 177, 200), 1.0, (1.0, -0.5)),
    "m0_177x200_dr255": (0, (2, 3, 177, 200), 255.0, (1.0, -0.5)),
    "m0_161x163_dr255_mean": (0, (2, 3, 161, 163), 255.0, (0.5, 0.5)),   # size_average=True under backward()
    "m1_16x48": (1, (2, 3, 16, 48), 1.0, (-0.7,)),
    "m1_50x70": (1, (1, 3, 50, 70), 1.0, (-0.7,)),
}


def msssim_pair(shape, data_range=1.0, seed=51):
    a = rnd(shape, seed)
    b = torch.clamp(a + (rnd(shape, seed + 1) - 0.5) * 0.2, 0, 1)
    return a * data_range, b * data_range


def msssim_case(name):
    mode, shape, dr, dval = MSSSIM_CASES[name]
    X, Y = msssim_pair(shape, dr)
    return mode, X, Y, dr, torch.tensor(dval)


def msssim_relu_pair():
    """(2, 3, 161, 163): image 0 has Y = 1 - X (cs <= 0 at level 0 in every channel: the relu branch, value 0);
    image 1 is a mild perturbation of X."""
    X, Y = msssim_pair((2, 3, 161, 163), 1.0, seed=61)
    Y = Y.clone()
    Y[0] = 1.0 - X[0]
    return X, Y, torch.tensor([1.0, -0.5])


# --------------------------------------------------------------------------- #
# Entropy models
# --------------------------------------------------------------------------- #
def eb_params(C, seed=1):
    """perturb_params-style EntropyBottleneck parameters for C channels; medians are non-zero multiples of 1/16,
    so `median + k + 0.5` is exact in fp32 and the eval-mode rounding ties are really ties."""
    P = {}
    codec._init_eb(P, gen(seed), C)
    P = codec.perturb_params(P, seed=seed + 1)
    q = P["entropy_bottleneck.quantiles"].clone()
    med = torch.round(q[:, 0, 1] * 16) / 16
    med = torch.where(med == 0, torch.full_like(med, 1.0 / 16), med)
    q[:, 0, 1] = med
    P["entropy_bottleneck.quantiles"] = q
    return P


def _to_dtype(P, dtype):
    return {k: v.to(dtype) for k, v in P.items()}


def _cl(x, C):   # NCHW -> [C, 1, L]
    return x.transpose(0, 1).contiguous().reshape(C, 1, -1)


def _nchw(v, shape):   # [C, 1, L] -> NCHW
    N, C = shape[0], shape[1]
    return v.reshape((C, N) + tuple(shape[2:])).transpose(0, 1).contiguous()


def eb_quantise(P, z, training, noise=None):
    """fp32 statement of the quantised tensor (anchors/model.py:86-108 semantics): z + noise, or
    round(z - median) + median with round half to even."""
    med = P["entropy_bottleneck.quantiles"][:, 0, 1].reshape(1, -1, 1, 1)
    return z + noise if training else torch.round(z - med) + med


def eb_raw(P, v, dtype=torch.float64):
    """|sigmoid(s upper) - sigmoid(s lower)| before the 1e-9 floor, NCHW, in dtype."""
    Pd = _to_dtype(P, dtype)
    u = _cl(v.to(dtype), v.shape[1])
    lower = codec.eb_logits_cumulative(Pd, u - 0.5)
    upper = codec.eb_logits_cumulative(Pd, u + 0.5)
    sign = -torch.sign(lower + upper)
    return _nchw(torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower)), v.shape)


def eb_lik(P, v, dtype=torch.float64):
    """(lik NCHW, per-image sum of log lik) of oracle.codec.eb_likelihood at the quantised v, in dtype."""
    lik = _nchw(codec.eb_likelihood(_to_dtype(P, dtype), _cl(v.to(dtype), v.shape[1])), v.shape)
    return lik, lik.log().flatten(1).sum(1)


def eb_bwd(P, v, gl, dtype=torch.float64):
    """(dL/dv NCHW, {name: dL/dparam}) of L = sum(lik * gl) through oracle.codec.eb_likelihood, in dtype."""
    Pd = {k: t.detach().to(dtype).clone().requires_grad_(True) for k, t in P.items() if not k.endswith("quantiles")}
    vr = v.detach().to(dtype).clone().requires_grad_(True)
    lik = _nchw(codec.eb_likelihood(Pd, _cl(vr, v.shape[1])), v.shape)
    (lik * gl.to(dtype)).sum().backward()
    return vr.grad, {n: Pd[f"entropy_bottleneck.{n}"].grad for n in EB_NAMES}


def eb_grad_init(gp64, seed=121):
    """Non-zero gradients for ica_eb_param_scatter to accumulate onto: uniform in +-max |dL/dparam| per tensor."""
    return {n: (rnd(tuple(gp64[n].shape), seed + i, -1, 1) * float(gp64[n].abs().max())).float()
            for i, n in enumerate(EB_NAMES)}


def _clear_band(raw):
    """Elements whose float64 likelihood lies within a factor 100 of the 1e-9 floor."""
    return (raw >= LIK_FLOOR / 100) & (raw <= LIK_FLOOR * 100)


def eb_case(C, N, H, W, training, seed=81):
    """Seeded EntropyBottleneck inputs: values spread +-40 around the (non-zero) medians; under these parameters
    (init_scale 10) the likelihood at +-40 is still > 3e-5 and reaches 1e-11 only past +-160..400, so a fifth of the
    values lie at +-200..640 and sit on the floor.  Eval inputs include exact .5 ties next to even and odd integers.  Elements whose float64 likelihood
    would come within a factor 100 of the floor are moved to the median.  Returns (P, z, noise or None)."""
    P = eb_params(C)
    med = P["entropy_bottleneck.quantiles"][:, 0, 1].reshape(1, C, 1, 1)
    g = gen(seed + C + 7 * H)
    shape = (N, C, H, W)
    k = torch.randint(-40, 41, shape, generator=g).float()
    far = torch.randint(200, 641, shape, generator=g).float() * torch.sign(k)
    k = torch.where(torch.rand(shape, generator=g) < 0.2, far, k)
    off = torch.rand(shape, generator=g) * 0.9 - 0.45
    noise = None
    if training:
        noise = torch.rand(shape, generator=g) - 0.5
    else:
        tie = torch.rand(shape, generator=g) < 0.15
        half = torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(0.5), torch.tensor(-0.5))
        off = torch.where(tie, half, off)
    z = med + (k + off)
    bad = _clear_band(eb_raw(P, eb_quantise(P, z, training, noise)))
    z = torch.where(bad, med + (0.0 * k + off), z)
    return P, z, noise


def _std_cum(x):
    return 0.5 * torch.erfc(-(2 ** -0.5) * x)


def gc_quantise(y, means, training, noise=None):
    if training:
        return y + noise
    return torch.round(y - means) + means if means is not None else torch.round(y)


def gc_raw(y_hat, scales, means=None, dtype=torch.float64):
    """upper - lower before the 1e-9 floor, in dtype."""
    v = y_hat.to(dtype) - means.to(dtype) if means is not None else y_hat.to(dtype)
    s = torch.clamp(scales.to(dtype), min=SCALE_FLOOR)
    v = v.abs()
    return _std_cum((0.5 - v) / s) - _std_cum((-0.5 - v) / s)


def gc_lik(y_hat, scales, means=None, dtype=torch.float64):
    lik = codec.gc_likelihood(y_hat.to(dtype), scales.to(dtype), None if means is None else means.to(dtype))
    return lik, lik.log().flatten(1).sum(1)


def gc_scales(shape, g):
    """Half from [0.01, 0.10], half log-uniform from [0.12, 50]: both sides of the 0.11 clamp, none within 0.01."""
    lo = 0.01 + 0.09 * torch.rand(shape, generator=g)
    hi = torch.exp(math.log(0.12) + (math.log(50.0) - math.log(0.12)) * torch.rand(shape, generator=g))
    return torch.where(torch.rand(shape, generator=g) < 0.5, lo, hi)


def gc_case(C, N, H, W, training, with_means, seed=91):
    """Seeded GaussianConditional inputs (y, scales, means or None, noise or None): |y - mean| / max(s, 0.11) up
    to 9, so some likelihoods sit on the floor; means are multiples of 1/16 and eval inputs include exact .5 ties.
    Elements within a factor 100 of the floor in float64 are moved to the mean."""
    g = gen(seed + C + 7 * H + 2 * int(training) + int(with_means))
    shape = (N, C, H, W)
    s = gc_scales(shape, g)
    means = torch.round((torch.rand(shape, generator=g) * 6 - 3) * 16) / 16 if with_means else None
    t = torch.rand(shape, generator=g) * 9.0
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(1.0), torch.tensor(-1.0))
    v = torch.clamp(sign * t * torch.clamp(s, min=SCALE_FLOOR), -60.0, 60.0)
    noise = None
    if training:
        noise = torch.rand(shape, generator=g) - 0.5
    else:
        tie = torch.rand(shape, generator=g) < 0.15
        v = torch.where(tie, torch.floor(v) + 0.5, v)
    m0 = means if with_means else torch.zeros(shape)
    y = m0 + v
    bad = _clear_band(gc_raw(gc_quantise(y, means, training, noise), s, means))
    y = torch.where(bad, m0, y)
    return y, s, means, noise


def gc_bwd(yt, sigma, gl, dtype=torch.float64):
    """(dL/dy, dL/dsigma, the gradient arriving at the scale bound) of L = sum(lik * gl), means = None."""
    yr = yt.detach().to(dtype).clone().requires_grad_(True)
    sr = sigma.detach().to(dtype).clone().requires_grad_(True)
    (codec.gc_likelihood(yr, sr) * gl.to(dtype)).sum().backward()
    sc = torch.clamp(sigma.detach().to(dtype), min=SCALE_FLOOR).requires_grad_(True)   # no bound active: its input gradient
    (codec.gc_likelihood(yt.to(dtype), sc) * gl.to(dtype)).sum().backward()
    return yr.grad, sr.grad, sc.grad


def bpp_upstream(lik64, g):
    """dL/dlik of a bpp term, c / lik with c of both signs and magnitude in [0.5, 2] (ica_bpp_grad's output under
    scales of either sign), as fp32."""
    c = (0.5 + 1.5 * torch.rand(lik64.shape, generator=g)) * torch.where(
        torch.rand(lik64.shape, generator=g) < 0.5, torch.tensor(1.0), torch.tensor(-1.0))
    return (c.double() / lik64).float()


def gc_bwd_case(C, N, H, W, seed=101):
    """Seeded gc_bwd inputs (yt, sigma, gl).  Besides the gc_case spread: exact zeros in yt, and elements whose
    raw likelihood is 1e-13..5e-12 (floor-active, but their pass-through gradient under gl = c / 1e-9 is far
    above the test's bound)."""
    g = gen(seed + C + 7 * H)
    shape = (N, C, H, W)
    s = gc_scales(shape, g)
    se = torch.clamp(s, min=SCALE_FLOOR)
    t = torch.rand(shape, generator=g) * 9.0
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(1.0), torch.tensor(-1.0))
    v = torch.clamp(sign * t * se, -60.0, 60.0)
    just = (torch.rand(shape, generator=g) < 0.2) & (se < 5.0)
    zt = 6.8 + 0.5 * torch.rand(shape, generator=g)      # Phi(-6.8) = 5e-12, Phi(-7.3) = 1.4e-13
    v = torch.where(just, sign * (0.5 + zt * se), v)
    v = torch.where(torch.rand(shape, generator=g) < 0.05, torch.zeros(shape), v)
    v = torch.where(_clear_band(gc_raw(v, s)), torch.zeros(shape), v)
    lik64, _ = gc_lik(v, s)
    return v, s, bpp_upstream(lik64, g)


def eb_bwd_case(C, N, H, W, seed=111):
    """Seeded eb_bwd inputs (P, v, gl): the train-mode eb_case and a bpp-style upstream of both signs."""
    P, z, noise = eb_case(C, N, H, W, True, seed)
    v = eb_quantise(P, z, True, noise)
    lik64, _ = eb_lik(P, v)
    return P, v, bpp_upstream(lik64, gen(seed + 1))


# --------------------------------------------------------------------------- #
# Weight gradients
# --------------------------------------------------------------------------- #
WGRAD_KINDS = {   # name: (KS, S, role)
    "k5s2": (5, 2, "conv"), "k5s2d": (5, 2, "deconv"), "k3s1": (3, 1, "conv"), "k1s1": (1, 1, "conv"),
    "k3s2": (3, 2, "conv"), "k1s2": (1, 2, "conv"), "k5s1": (5, 1, "conv"),
}
# (A, Bc, small-grid map, big map under S = 2 conv or None for the 2x grid)
WGRAD_SHAPES = {
    "3x33_9x33": (3, 33, (9, 33), None),        # a second 32-pixel segment of one pixel
    "33x3_5x40": (33, 3, (5, 40), None),
    "70x37_1x1": (70, 37, (1, 1), None),
    "70x37_7x7": (70, 37, (7, 7), (13, 13)),    # S = 2 from an odd big map
    "128x128_9x33": (128, 128, (9, 33), None),  # 36 chunks over 32 splits
}


def wgrad_case(kind, shape, N=2):
    """(Sm, Lg, KS, S, role) NCHW operands of K.wgrad: conv role Sm = dL/dy [N, A, small], Lg = x [N, Bc, big];
    deconv role Sm = x [N, A, small], Lg = dL/dy [N, Bc, 2x small]."""
    KS, S, role = WGRAD_KINDS[kind]
    A, Bc, (Hs, Ws), big = WGRAD_SHAPES[shape]
    if S == 1:
        Hb, Wb = Hs, Ws
    elif big is not None and role == "conv":
        Hb, Wb = big
    else:
        Hb, Wb = 2 * Hs, 2 * Ws
    seed = 200 + 10 * list(WGRAD_KINDS).index(kind) + list(WGRAD_SHAPES).index(shape)
    Sm = rnd((N, A, Hs, Ws), seed, -1, 1)
    Lg = rnd((N, Bc, Hb, Wb), seed + 1000, -1, 1)
    return Sm, Lg, KS, S, role


def wgrad(Sm, Lg, KS, S, role, dtype=torch.float64):
    """dL/dW in K.wgrad's [A][Bc][KS][KS] order by autograd: conv W[A = cout][Bc = cin] with dL/dy = Sm, x = Lg;
    deconv (ConvTranspose2d) W[A = cin][Bc = cout] with x = Sm, dL/dy = Lg."""
    A, Bc = Sm.shape[1], Lg.shape[1]
    w = torch.zeros((A, Bc, KS, KS), dtype=dtype, requires_grad=True)
    Sm, Lg = Sm.to(dtype), Lg.to(dtype)
    if role == "conv":
        y = F.conv2d(Lg, w, None, stride=S, padding=KS // 2)
        assert y.shape == Sm.shape, (y.shape, Sm.shape)
        (y * Sm).sum().backward()
    else:
        y = F.conv_transpose2d(Sm, w, None, stride=S, padding=KS // 2, output_padding=S - 1)
        assert y.shape == Lg.shape, (y.shape, Lg.shape)
        (y * Lg).sum().backward()
    return w.grad


# --------------------------------------------------------------------------- #
# Arithmetic elementwise pieces and reductions
# --------------------------------------------------------------------------- #
def gdn_xsq_case():
    """(y, s) nChw4c-shaped [2, 2, 11, 13, 4] (2288 elements: not a multiple of 256): s = n^-1/2 away from 0."""
    shape = (2, 2, 11, 13, 4)
    return rnd(shape, 301, -3, 3), rnd(shape, 302, 0.2, 3.0)


def gdn_xsq(y, s, dtype=torch.float64):
    return (y.to(dtype) / s.to(dtype)) ** 2


def channel_sum_case(C):
    """(x [2, C, 11, 13], out0 [C]): N * HW = 286, a second partial trip of the 256-thread loop."""
    return rnd((2, C, 11, 13), 310 + C, -1, 1), rnd((C,), 320 + C, -50, 50)


def channel_sum(x, out0=None, dtype=torch.float64):
    r = x.to(dtype).sum((0, 2, 3))
    return r if out0 is None else out0.to(dtype) + r


MSE_SCALE = 0.013 * 255.0 ** 2 * 2.0 / (2 * 3 * 11 * 13)   # lambda 255^2 2 / (B 3 H W) of train_engine._loss


def mse_grad_case():
    """(x_hat, x, g0) NCHW [2, 3, 11, 13]: g0 is what g4 holds before the +=."""
    shape = (2, 3, 11, 13)
    return rnd(shape, 331, -0.1, 1.1), rnd(shape, 332), rnd(shape, 333, -1, 1)


def mse_grad(xh, x, g0, dtype=torch.float64):
    return g0.to(dtype) + MSE_SCALE * (xh.to(dtype) - x.to(dtype))
