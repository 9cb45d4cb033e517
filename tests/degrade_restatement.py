"""Plain-torch CPU restatement of random_noise.py's degradations (torchvision is not a dependency): the oracle of
tests/test_cpu_degrade.py and tests/test_gpu_degrade.py.

taps / kernel2d / blur   torchvision gaussian_blur: _get_gaussian_kernel1d, torch.mm of the two tap vectors,
                         F.pad(mode="reflect") and a grouped conv2d
schedule / scan          generate_blurimages (random_noise.py:50-65): sigma = sigma - 0.005 until the MSE fits
noise_metrics            test (random_noise.py:68-111) from the two reconstructions
deblur_metrics           test_deblur (random_noise.py:38-48)
"""
import math

import torch
import torch.nn.functional as F

EPS24 = 2.0 ** -24


def taps(k, sigma, dtype=torch.float32):
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=dtype)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def kernel2d(wx, wy):
    """[ky, kx]: torch.mm(wy[:, None], wx[None, :]), one rounded product per tap."""
    return torch.mm(wy[:, None], wx[None, :])


def blur_with_kernel(x, k2):
    ky, kx = k2.shape
    xp = F.pad(x, (kx // 2, kx // 2, ky // 2, ky // 2), mode="reflect")
    w = k2.to(x.dtype).expand(x.shape[1], 1, ky, kx).contiguous()
    return F.conv2d(xp, w, groups=x.shape[1])


def blur(x, ksize, sigma, dtype=torch.float64, taps_dtype=torch.float32, clamp=False):
    """gaussian_blur of x [B, C, H, W] in ``dtype`` with the taps (and their product) computed in ``taps_dtype``.
    ksize = (kx, ky); sigma a float or one per image."""
    kx, ky = ksize
    sig = list(sigma) if isinstance(sigma, (tuple, list)) else [sigma] * x.shape[0]
    out = []
    for b, s in enumerate(sig):
        k2 = kernel2d(taps(kx, s, taps_dtype), taps(ky, s, taps_dtype))
        out.append(blur_with_kernel(x[b:b + 1].to(dtype), k2))
    y = torch.cat(out, 0)
    return y.clamp(0, 1) if clamp else y


def schedule(start=5.0, step=0.005):
    out, s = [], float(start)
    while s > step / 2:
        out.append(s)
        s = s - step
    return out


def sweep_mse(x, sigmas, ksize=(5, 5), dtype=torch.float64):
    """[B, len(sigmas)] float64: mean((clamp(blur_s(x)) - x)^2) of every candidate."""
    xd = x.to(dtype)
    cols = [((blur(x, ksize, s, dtype, clamp=True) - xd) ** 2).mean(dim=(1, 2, 3)).double() for s in sigmas]
    return torch.stack(cols, 1)


def scan(mse_row, budget):
    """The linear scan: the first index whose MSE is <= budget, or -1."""
    for k, v in enumerate(mse_row.tolist()):
        if v <= budget:
            return k
    return -1


def search_delta(ksize, budget):
    """The worst relative MSE error the per-pixel fp32 bound allows: with |err| <= e = (kx ky + 4) 2^-24 per pixel,
    |mse' - mse| <= 2 e sqrt(mse) + e^2, so relative to a budget-sized MSE 2 e / sqrt(T), plus 1e-5 for the sum."""
    kx, ky = ksize
    return 2 * (kx * ky + 4) * EPS24 / math.sqrt(budget) + 1e-5


def check_index(mse_row, k, budget, delta):
    """What the search test asserts of a returned index k against the float64 row."""
    row = mse_row.tolist()
    last = len(row) if k < 0 else k
    early = [j for j in range(last) if not row[j] > budget * (1 - delta)]
    ok_k = k < 0 or row[k] <= budget * (1 + delta)
    return ok_k and not early, early


def has_margin(mse_row, budget, delta):
    """No candidate up to the float64 answer lies within delta of the budget: any scan inside the error bound
    returns the float64 index."""
    k = scan(mse_row, budget)
    row = mse_row.tolist()
    last = len(row) if k < 0 else k + 1
    return all(abs(row[j] - budget) > delta * budget for j in range(last))


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def rand_image(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def smooth_image(H, W, seed, grid=4, amp=1.0):
    """A seeded low-resolution random field, bicubically enlarged and squeezed into [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((1, 3, max(H // grid, 2), max(W // grid, 2)), generator=g)
    x = F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
    return (0.5 + amp * (x - 0.5)).clamp(0, 1)


def checkerboard(H, W, d2=1.05e-4):
    d = math.sqrt(d2)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    sign = (1 - 2 * ((yy + xx) % 2)).double()
    return (0.5 + d * sign).float().expand(1, 3, H, W).contiguous()


def edge_only(B, H, W, kx, ky, seed):
    """Non-zero only in the outermost k // 2 rows and columns: every non-zero output next to an edge got there
    through the reflection (or the first interior taps)."""
    x = rand_image((B, 3, H, W), seed, 0.25, 1.0)
    py, px = max(ky // 2, 1), max(kx // 2, 1)
    x[:, :, py:H - py, px:W - px] = 0
    return x


# the pinned inputs of the search tests: name -> (builder, noise, ksize, start, step)
SEARCH_CASES = {
    "smooth_1e-4": (lambda: torch.cat([smooth_image(32, 48, s) for s in (1, 2)], 0), 1e-4, (5, 5), 5.0, 0.005),
    "smooth_1e-3": (lambda: torch.cat([smooth_image(32, 48, s) for s in (3, 4)], 0), 1e-3, (5, 5), 5.0, 0.005),
    "mixed": (lambda: torch.cat([smooth_image(32, 48, 9), torch.full((1, 3, 32, 48), 0.25),
                                 smooth_image(32, 48, 13, amp=0.5), smooth_image(32, 48, 10)], 0),
              1e-3, (5, 5), 5.0, 0.005),
    "never": (lambda: torch.cat([rand_image((1, 3, 32, 48), 8), torch.full((1, 3, 32, 48), 0.5)], 0),
              1e-4, (5, 5), 5.0, 0.6),
    "checkerboard": (lambda: checkerboard(16, 24), 1e-4, (5, 5), 5.0, 0.005),
}
_CACHE = {}


def search_case(name):
    """(x fp32 [B, 3, H, W], noise, ksize, start, step, sigmas, mse64 [B, S]) of a pinned case, computed once."""
    if name not in _CACHE:
        build, noise, ksize, start, step = SEARCH_CASES[name]
        x = build()
        sig = schedule(start, step)
        _CACHE[name] = (x, noise, ksize, start, step, sig, sweep_mse(x, sig, ksize))
    return _CACHE[name]


# --------------------------------------------------------------------------- #
# metrics
# --------------------------------------------------------------------------- #
def noise_metrics(im, noise, x_hat_ori, x_hat, bpp, num_pixels=None):
    """test's return per image from clamped reconstructions (random_noise.py:102-111); bpp is per padded pixel."""
    im, noise, x_hat_ori, x_hat = (t.double() for t in (im, noise, x_hat_ori, x_hat))
    H, W = im.shape[2:]
    out = []
    for b in range(im.shape[0]):
        err_out = float(((x_hat_ori[b] - x_hat[b]) ** 2).mean())
        power = float((noise[b] ** 2).mean())
        n = H * W if num_pixels is None else num_pixels
        out.append((10.0 * math.log10(err_out / power), float(bpp[b]) * H * W / n,
                    -10.0 * math.log10(float(((x_hat[b] - im[b]) ** 2).mean()))))
    return out


def deblur_metrics(im_blur, im_sharp, x_hat, bpp):
    """test_deblur's return per image (random_noise.py:44-48), x_hat unclamped."""
    im_blur, im_sharp, x_hat = (t.double() for t in (im_blur, im_sharp, x_hat))
    out = []
    for b in range(im_blur.shape[0]):
        psnr_blur = -10.0 * math.log10(float(((im_blur[b] - im_sharp[b]) ** 2).mean()))
        psnr_sharp = -10.0 * math.log10(float(((x_hat[b] - im_sharp[b]) ** 2).mean()))
        out.append((psnr_blur - psnr_sharp, float(bpp[b]), psnr_sharp))
    return out
