"""The band study and the band-limited attack step (DESIGN.md "Band VI") restated in torch, float64 by default, with no
engine: what tests/test_gpu_band.py holds the HIP kernels of ica_band.hip to.

Transform.  The orthonormal 8x8 block DCT-II as the explicit matrix D[k][n] = c_k cos((2 n + 1) k pi / 16), c_0 =
sqrt(1 / 8), c_k = 1 / 2: coefficients D X D^T of every 8x8 block of every channel plane, blocks aligned to the image
origin.  The kernels run the even-odd butterfly of ica_dct8.h; the matrix is an independent statement of the same map.
Coefficient (u, v) belongs to band max(u, v); P_S = IDCT . [band in S] . DCT.

Step.  ``step`` builds the forward of the band-limited attack as an autograd graph, Low_bound / Up_bound (utils/ops.py)
as custom functions in the style of oracle/codec.py:

    nc = Up(Low(noise, -eps), eps);  p = P_S(nc);  im_in = Up(Low(im_s + p, 0), 1);  loss_i = mean((im_s - im_in)^2)
    loss[b] = loss_i[b]                    if loss_i[b] > thr    (the cheap branch)
            = <g_net[b], im_in[b]>         otherwise              (any loss whose gradient at im_in is g_net)

and returns im_in, loss_i and d loss / d noise; ``step_closed_form`` is the same gradient written out (the transpose:
bound-backward at im_s + p, P_S again, bound-backward at the noise).

Tolerances.  Every function takes a dtype; the fp32 twin is the same code run in float32 on the CPU.  The guards are
4 x the twin's largest difference from float64 on the cases below (the factor is the kernel's freedom to order its
sums; the convention of tests/jpeg_bpda_restatement.py).  Measured on the CPU; tests/test_cpu_band.py measures them
again and asserts that each constant is 4 x the fresh value within a factor of 2:

    projection   max |P x (fp32) - P x (float64)| / max |x| over the three shapes and the 24 preset masks
                 MEASURED_PROJ 2.2e-07, GUARD_PROJ 8.8e-07
    energies     max over bands |e_k (fp32) - e_k (float64)| / mean(n^2) over the three shapes
                 MEASURED_ENERGY 3.5e-08, GUARD_ENERGY 1.4e-07
    gradient     max |d loss / d noise (fp32) - (float64)| / max |d loss / d noise (float64)| on GRAD_CASES
                 MEASURED_GRAD 2.2e-07, GUARD_GRAD 8.8e-07

The gradient's only discontinuities are the bound masks.  Those at the noise compare fp32 values with +-eps and are
exact in both precisions; those at u = im_s + p are decided alike by fp32 and float64 as long as no u lies within
U_MARGIN of 0 or 1, which tests/test_cpu_band.py asserts for the seeds used (no element is left out of any
comparison).  The images of a gradient case are mid-grey, [0.2, 0.8], except N_SATURATED pixels at exactly 0 or 1,
where the input clamp and its pass-through rule act.
"""
import math

import torch

NB = 8
SHAPES = [(1, 8, 8), (3, 72, 136), (2, 64, 192)]      # (B, H, W): one block; remainders of the 64 x 32 tile on both
#                                                        axes and a batch; several tiles per row
PRESETS = ("only", "lowpass", "without")
EPS = 16.0 / 255.0
U_MARGIN = 1e-4
N_SATURATED = 96
GRAD_CASES = {"72x136": ((2, 72, 136), 0b00000111, 6), "64x192": ((2, 64, 192), 0b10100110, 2)}   # shape, mask, seed

MEASURED_PROJ = 2.2e-07
GUARD_PROJ = 4 * MEASURED_PROJ
MEASURED_ENERGY = 3.5e-08
GUARD_ENERGY = 4 * MEASURED_ENERGY
MEASURED_GRAD = 2.2e-07
GUARD_GRAD = 4 * MEASURED_GRAD


def preset_masks(name):
    return {"only": [1 << k for k in range(NB)], "lowpass": [(2 << k) - 1 for k in range(NB)],
            "without": [0xFF ^ (1 << k) for k in range(NB)]}[name]


def dct_matrix(dtype=torch.float64):
    D = torch.empty((8, 8), dtype=torch.float64)
    for k in range(8):
        for n in range(8):
            D[k, n] = (math.sqrt(1.0 / 8.0) if k == 0 else 0.5) * math.cos((2 * n + 1) * k * math.pi / 16.0)
    return D.to(dtype)


def band_table():
    u = torch.arange(NB)
    return torch.maximum(u[:, None], u[None, :])


def keep_table(mask, dtype=torch.float64):
    return ((mask >> band_table()) & 1).to(dtype)


def blocks(x):
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 8, 8, W // 8, 8).permute(0, 1, 2, 4, 3, 5)


def unblocks(c):
    B, C, hb, wb = c.shape[:4]
    return c.permute(0, 1, 2, 4, 3, 5).reshape(B, C, hb * 8, wb * 8)


def coefs(x):
    """[B, C, H / 8, W / 8, 8, 8]: D X D^T of every block, in x's dtype."""
    D = dct_matrix(x.dtype)
    return D @ blocks(x) @ D.T


def project(x, mask):
    D = dct_matrix(x.dtype)
    return unblocks(D.T @ (coefs(x) * keep_table(mask, x.dtype)) @ D)


def energies(n):
    """[B, 8]: |P_{k} n|^2 / (3 H W), from the coefficients."""
    c2 = coefs(n) ** 2
    tab = band_table()
    return torch.stack([(c2 * (tab == k).to(n.dtype)).sum(dim=(1, 2, 3, 4, 5)) for k in range(NB)], 1) / n[0].numel()


def split(im_s, im_adv, masks, dtype=torch.float64):
    """(x [V, B, 3, H, W], energy [B, 8], mse_in [V, B]) of fp32 images, computed in dtype."""
    s, a = im_s.to(dtype), im_adv.to(dtype)
    n = a - s
    x = torch.stack([torch.clamp(s + project(n, m), 0.0, 1.0) for m in masks])
    return x, energies(n), ((x - s) ** 2).mean(dim=(2, 3, 4))


class LowBound(torch.autograd.Function):
    """utils/ops.py:28-41: fwd clamp(min=b); bwd g * ((x >= b) | (g < 0))."""

    @staticmethod
    def forward(ctx, x, b):
        ctx.save_for_backward(x)
        ctx.b = b
        return torch.clamp(x, min=b)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * ((x >= ctx.b) | (g < 0.0)).to(g.dtype), None


class UpBound(torch.autograd.Function):
    """utils/ops.py:43-56: fwd clamp(max=b); bwd g * ((x <= b) | (g > 0))."""

    @staticmethod
    def forward(ctx, x, b):
        ctx.save_for_backward(x)
        ctx.b = b
        return torch.clamp(x, max=b)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * ((x <= ctx.b) | (g > 0.0)).to(g.dtype), None


def _eps(eps, dtype):
    # the kernels take eps as a float: the bound is the fp32 value in every precision
    return float(torch.tensor(eps, dtype=torch.float32)) if dtype == torch.float64 else eps


def forward(noise, im_s, mask, eps=EPS):
    """(nc, u, im_in, loss_i) in noise's dtype; differentiable."""
    e = _eps(eps, noise.dtype)
    nc = UpBound.apply(LowBound.apply(noise, -e), e)
    u = im_s + project(nc, mask)
    im_in = UpBound.apply(LowBound.apply(u, 0.0), 1.0)
    return nc, u, im_in, ((im_s - im_in) ** 2).mean(dim=(1, 2, 3))


def step(noise, im_s, g_net, mask, thr, eps=EPS, dtype=torch.float64):
    """(im_in, loss_i [B], cheap [B] bool, d loss / d noise) by autograd; noise, im_s, g_net are given fp32 tensors."""
    z = noise.to(dtype).requires_grad_(True)
    s, gn = im_s.to(dtype), g_net.to(dtype)
    _, _, im_in, loss_i = forward(z, s, mask, eps)
    cheap = loss_i.detach() > thr
    loss = torch.where(cheap, loss_i, (gn * im_in).sum(dim=(1, 2, 3)))
    (g,) = torch.autograd.grad(loss.sum(), z)
    return im_in.detach(), loss_i.detach(), cheap, g


def step_closed_form(noise, im_s, g_net, mask, thr, eps=EPS, dtype=torch.float64):
    """d loss / d noise of ``step`` written out: the transpose the Adam kernel applies."""
    z, s, gn = noise.to(dtype), im_s.to(dtype), g_net.to(dtype)
    e = _eps(eps, dtype)
    with torch.no_grad():
        _, u, im_in, loss_i = forward(z, s, mask, eps)
        cheap = (loss_i > thr).view(-1, 1, 1, 1)
        g = torch.where(cheap, -2.0 * ((s - im_in) / s[0].numel()), gn)
        g = g * ((torch.clamp(u, min=0.0) <= 1.0) | (g > 0.0)).to(dtype)
        g = g * ((u >= 0.0) | (g < 0.0)).to(dtype)
        g = project(g, mask)
        g = g * ((torch.clamp(z, min=-e) <= e) | (g > 0.0)).to(dtype)
        g = g * ((z >= -e) | (g < 0.0)).to(dtype)
    return g


def pair(shape, seed):
    """(im_s, im_adv) fp32 in [0, 1]: uniform image, clamped Gaussian perturbation of std 0.02."""
    g = torch.Generator().manual_seed(seed)
    im_s = torch.rand((shape[0], 3, shape[1], shape[2]), generator=g)
    n = 0.02 * torch.randn(im_s.shape, generator=g)
    return im_s, torch.clamp(im_s + n, 0.0, 1.0)


def grad_case(name):
    """(noise, im_s, g_net [B, 3, H, W], mask, thr) fp32: a third of the noise beyond +-eps, image 1's noise at a quarter
    of the scale of image 0's, thr the geometric mean of the two loss_i (one image cheap, one expensive, each at least a
    factor of two from thr)."""
    (B, H, W), mask, seed = GRAD_CASES[name]
    g = torch.Generator().manual_seed(seed)
    im_s = 0.2 + 0.6 * torch.rand((B, 3, H, W), generator=g)
    at = torch.randperm(im_s.numel(), generator=g)[:N_SATURATED]
    im_s.view(-1)[at] = (torch.arange(N_SATURATED) % 2).float()
    noise = EPS * torch.randn(im_s.shape, generator=g)
    noise[1] *= 0.25
    g_net = 1e-3 * torch.randn(im_s.shape, generator=g)
    _, _, _, loss_i = forward(noise.double(), im_s.double(), mask)
    lo, hi = sorted(loss_i.tolist())
    assert hi > 4.0 * lo, (lo, hi)
    return noise, im_s, g_net, mask, math.sqrt(lo * hi)


def rel_err(got, ref, scale=None):
    """max |got - ref| / max |ref| (or / scale) in float64."""
    ref = ref.double()
    s = float(ref.abs().max()) if scale is None else float(scale)
    return float((got.double() - ref).abs().max()) / s


def measure_proj():
    worst = 0.0
    for i, shape in enumerate(SHAPES):
        im_s, im_adv = pair(shape, 100 + i)
        x = im_adv - im_s
        for preset in PRESETS:
            for m in preset_masks(preset):
                worst = max(worst, rel_err(project(x, m), project(x.double(), m), x.abs().max()))
    return worst


def measure_energy():
    worst = 0.0
    for i, shape in enumerate(SHAPES):
        im_s, im_adv = pair(shape, 100 + i)
        e32 = energies(im_adv - im_s)
        n64 = im_adv.double() - im_s.double()
        e64 = energies(n64)
        scale = (n64 ** 2).mean(dim=(1, 2, 3)).view(-1, 1)
        worst = max(worst, float(((e32.double() - e64).abs() / scale).max()))
    return worst


def measure_grad():
    worst = 0.0
    for name in GRAD_CASES:
        noise, im_s, g_net, mask, thr = grad_case(name)
        g64 = step(noise, im_s, g_net, mask, thr)[3]
        g32 = step(noise, im_s, g_net, mask, thr, dtype=torch.float32)[3]
        worst = max(worst, rel_err(g32, g64))
    return worst
