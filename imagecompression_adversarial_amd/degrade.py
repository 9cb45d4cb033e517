"""Harmless degradations of random_noise.py on the HIP kernels (ica_degrade.hip): the baselines an adversarial
perturbation is judged against.

gaussian_taps     torchvision _get_gaussian_kernel1d, restated in fp32 torch on the host
gaussian_blur     T.GaussianBlur / gaussian_blur (random_noise.py:31-33): reflect pad, ky x kx correlation
sigma_schedule    the sigma values generate_blurimages visits (random_noise.py:54-63)
blur_to_budget    generate_blurimages: the first sigma of the schedule whose clamped blur fits the MSE budget
apply_noise       random_noise.py:80: clamp(im + noise, 0, 1), mean(noise^2), mean((im_in - im)^2)
evaluate_noise    test (random_noise.py:68-111), per image
evaluate_deblur   test_deblur (random_noise.py:20-48), per image
jpeg_tables       the T.81 Annex K tables scaled by the IJG rule, as integers on the host
jpeg_roundtrip    the baseline-JPEG transform round trip (ica_jpeg.hip; DESIGN.md "JPEG round trip"): what
                  test_commands/jpeg.sh makes with ``cjpeg -q 50``, and the input-transformation defence
jpeg_roundtrip_bwd its input gradient under a surrogate ("ste" or "cubic"): the attack through the JPEG defence
jpeg_to_budget    the first quality from 1 upward whose round trip fits the MSE budget
evaluate_jpeg     test's numbers with the JPEG error in the place of the noise

All image tensors are the planar NCHW fp32 [B, 3, H, W] device tensors attack.evaluate holds.  The sigma scan is a
linear scan on purpose: a normalised 5-tap Gaussian's side tap is not monotone in sigma, so neither is the MSE, and
"the first sigma from the top that fits" is not what a bisection finds (DESIGN.md "Degradations").
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache

import torch

from . import hip_ops as K
from ._lib import call, lib, ptr, stream

KMAX = 9
BLUR_KSIZE, BLUR_SIGMA = (5, 9), 0.5          # random_noise.py:31
SWEEP_KSIZE, SWEEP_FACTOR = (5, 5), 1.01      # random_noise.py:55, :59
SIGMA_START, SIGMA_STEP = 5.0, 0.005          # random_noise.py:54, :60


def gaussian_taps(k, sigma):
    """[k] fp32: linspace(-(k-1)/2, (k-1)/2, k), exp(-0.5 (x / sigma)^2), divided by the sum."""
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def sigma_schedule(start=SIGMA_START, step=SIGMA_STEP):
    """The Python-double sequence of ``sigma = sigma - step`` from ``start``, cut at the last value above step / 2."""
    out, s = [], float(start)
    while s > step / 2:
        out.append(s)
        s = s - step
    return out


def validate(H, W, kernel_size=BLUR_KSIZE, sigma=BLUR_SIGMA, noise=None, factor=SWEEP_FACTOR, start=SIGMA_START,
             step=SIGMA_STEP):
    """ValueError unless the kernels take this problem (include/ica_hip.h, ica_gauss_blur / ica_blur_sweep)."""
    K.positive_int("H", H)
    K.positive_int("W", W)
    if (not isinstance(kernel_size, (tuple, list)) or len(kernel_size) != 2
            or any(not isinstance(k, int) or isinstance(k, bool) for k in kernel_size)):
        raise ValueError(f"kernel_size must be two ints (kx, ky), got {kernel_size!r}")
    kx, ky = kernel_size
    for name, k in (("kx", kx), ("ky", ky)):
        if k < 1 or k > KMAX or k % 2 == 0:
            raise ValueError(f"{name} = {k} is not odd in 1 .. {KMAX}")
    if W % 4:
        raise ValueError(f"W = {W} must be a multiple of 4 (16-byte row loads)")
    if H <= ky // 2 or W <= kx // 2:
        raise ValueError(f"the image {H}x{W} is too small to reflect-pad by ({ky // 2}, {kx // 2})")
    sigmas = sigma if isinstance(sigma, (tuple, list)) else [sigma]
    for s in sigmas:
        if isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) or s <= 0:
            raise ValueError(f"sigma must be a positive finite number, got {s!r}")
    if noise is not None:
        if isinstance(noise, bool) or not isinstance(noise, (int, float)) or not math.isfinite(noise) or noise <= 0:
            raise ValueError(f"noise must be a positive finite number, got {noise!r}")
        if not factor > 0 or not math.isfinite(factor):
            raise ValueError(f"factor must be positive, got {factor!r}")
        if not step > 0 or not start > step / 2 or not math.isfinite(start):
            raise ValueError(f"the schedule start={start!r}, step={step!r} is empty")
        if start / step > 1e6:
            raise ValueError(f"the schedule start={start!r}, step={step!r} has more than 1e6 candidates")


# ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), row-major: row = vertical frequency
JPEG_LUMA = (16, 11, 10, 16, 24, 40, 51, 61,
             12, 12, 14, 19, 26, 58, 60, 55,
             14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77,
             24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101,
             72, 92, 95, 98, 112, 100, 103, 99)
JPEG_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99,
               18, 21, 26, 66, 99, 99, 99, 99,
               24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
JPEG_QUALITY, JPEG_SUBSAMPLING = 50, "420"     # test_commands/jpeg.sh: cjpeg -q 50, cjpeg's default subsampling
JPEG_MCU = {"420": 16, "444": 8}
JPEG_SURROGATES = ("ste", "cubic")             # ICA_JPEG_STE, ICA_JPEG_CUBIC: the index is the C value


def validate_jpeg(H=None, W=None, quality=JPEG_QUALITY, subsampling=JPEG_SUBSAMPLING, noise=None,
                  factor=SWEEP_FACTOR, surrogate=None):
    """ValueError unless ica_jpeg_roundtrip / ica_jpeg_sweep / ica_jpeg_roundtrip_bwd take this problem
    (include/ica_hip.h).  ``quality``: one value or a list; H, W None checks the flags alone; ``surrogate`` None:
    not a backward."""
    if subsampling not in JPEG_MCU:
        raise ValueError(f"subsampling {subsampling!r} is not one of {sorted(JPEG_MCU)}")
    if surrogate is not None and surrogate not in JPEG_SURROGATES:
        raise ValueError(f"surrogate {surrogate!r} is not one of {list(JPEG_SURROGATES)}")
    for q in (quality if isinstance(quality, (tuple, list)) else [quality]):
        if isinstance(q, bool) or not isinstance(q, int) or q < 1 or q > 100:
            raise ValueError(f"a JPEG quality is an integer in 1 .. 100, got {q!r}")
    if H is not None:
        K.positive_int("H", H)
        K.positive_int("W", W)
        mcu = JPEG_MCU[subsampling]
        if H % mcu or W % mcu:
            raise ValueError(f"the image {H}x{W} is not a multiple of the {mcu}x{mcu} MCU of subsampling {subsampling}")
    if noise is not None:
        if isinstance(noise, bool) or not isinstance(noise, (int, float)) or not math.isfinite(noise) or noise <= 0:
            raise ValueError(f"noise must be a positive finite number, got {noise!r}")
        if not factor > 0 or not math.isfinite(factor):
            raise ValueError(f"factor must be positive, got {factor!r}")


def jpeg_tables(q):
    """(luminance [64], chrominance [64]) as lists of ints: the Annex K tables scaled by the IJG rule, s = 5000 // q
    below 50, else 200 - 2 q; each entry clamp((base * s + 50) // 100, 1, 255)."""
    validate_jpeg(quality=q)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((v * s + 50) // 100, 1), 255) for v in base] for base in (JPEG_LUMA, JPEG_CHROMA))


@lru_cache(maxsize=64)
def _jpeg_tabs(qualities, device):
    """[len(qualities), 128] fp32 on ``device``: row i is the table pair of qualities[i] (every entry an exact small
    integer).  Cached per (qualities, device), so a repeated round trip pays no host-to-device copy."""
    return torch.tensor([sum(jpeg_tables(q), []) for q in qualities], dtype=torch.float32).to(device)


def _jpeg_ws(name, B, H, W, sub, dev):
    return torch.empty(getattr(lib(), name)(B, H, W, sub), dtype=torch.float32, device=dev)


def jpeg_roundtrip(x, quality=JPEG_QUALITY, subsampling=JPEG_SUBSAMPLING, ref=None):
    """The JPEG round trip of clamp(x, 0, 1) at ``quality`` (an int, or one per image).  With ``ref`` returns
    (image, mean((image - ref)^2) [B]), else the image."""
    B, H, W = K.check_image(x, "x")
    qs = list(quality) if isinstance(quality, (tuple, list)) else [quality] * B
    validate_jpeg(H, W, qs, subsampling)
    if len(qs) != B:
        raise ValueError(f"{len(qs)} qualities for a batch of {B}")
    if ref is not None:
        if ref.shape != x.shape:
            raise ValueError(f"ref {tuple(ref.shape)} differs from x {tuple(x.shape)}")
        K._dev_check(ref, "ref")
    sub = int(subsampling)
    tabs = _jpeg_tabs(tuple(qs), str(x.device))
    out = torch.empty_like(x)
    mse = torch.empty(B, dtype=torch.float32, device=x.device) if ref is not None else None
    ws = _jpeg_ws("ica_jpeg_roundtrip_ws_size", B, H, W, sub, x.device)
    call("ica_jpeg_roundtrip", ptr(x), ptr(tabs), B, H, W, sub, ptr(ref), ptr(out), ptr(mse), ptr(ws), stream())
    return out if ref is None else (out, mse)


def jpeg_roundtrip_bwd(x, g, quality=JPEG_QUALITY, subsampling=JPEG_SUBSAMPLING, surrogate=None):
    """g_x: the gradient with respect to x of sum(g * jpeg_roundtrip(x, quality, subsampling)) under ``surrogate``
    (DESIGN.md "JPEG round trip", "The attack through it"): "ste", the quantiser has derivative 1, or "cubic",
    3 r^2 with r the coefficient's distance to its rounded value in steps.  No default: the caller names it."""
    B, H, W = K.check_image(x, "x")
    qs = list(quality) if isinstance(quality, (tuple, list)) else [quality] * B
    if surrogate is None:
        raise ValueError(f"name the surrogate: one of {list(JPEG_SURROGATES)}")
    validate_jpeg(H, W, qs, subsampling, surrogate=surrogate)
    if len(qs) != B:
        raise ValueError(f"{len(qs)} qualities for a batch of {B}")
    if g.shape != x.shape:
        raise ValueError(f"g {tuple(g.shape)} differs from x {tuple(x.shape)}")
    K._dev_check(g, "g")
    sub = int(subsampling)
    tabs = _jpeg_tabs(tuple(qs), str(x.device))
    gx = torch.empty_like(x)
    ws = _jpeg_ws("ica_jpeg_roundtrip_bwd_ws_size", B, H, W, sub, x.device)
    call("ica_jpeg_roundtrip_bwd", ptr(x), ptr(tabs), ptr(g), B, H, W, sub, JPEG_SURROGATES.index(surrogate), ptr(gx),
         ptr(ws), stream())
    return gx


def jpeg_sweep(x, noise, factor=SWEEP_FACTOR, subsampling=JPEG_SUBSAMPLING):
    """Scores the qualities 1, 2, .. 100 in that order (the strongest degradation first), a chunk per launch, until
    every image has its first fit: (index [B] int32 on the device, quality index + 1, -1 where none fits; mse
    [B, 100] against x itself, NaN where a candidate was not needed).  A linear scan: JPEG's MSE is not monotone
    in the quality."""
    B, H, W = K.check_image(x, "x")
    validate_jpeg(H, W, JPEG_QUALITY, subsampling, noise, factor)
    dev, sub, n = x.device, int(subsampling), 100
    tabs = _jpeg_tabs(tuple(range(1, n + 1)), str(dev))
    mse = torch.full((B, n), float("nan"), dtype=torch.float32, device=dev)
    idx = torch.full((B,), -1, dtype=torch.int32, device=dev)
    done = torch.zeros(B, dtype=torch.int32, device=dev)
    remaining = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _jpeg_ws("ica_jpeg_sweep_ws_size", B, H, W, sub, dev)
    chunk = lib().ica_jpeg_sweep_chunk()
    for s0 in range(0, n, chunk):
        S = min(chunk, n - s0)
        call("ica_jpeg_sweep", ptr(x), ptr(tabs[s0:]), S, B, H, W, sub, float(factor * noise), s0, ptr(mse), n,
             ptr(idx), ptr(done), ptr(remaining), ptr(ws), stream())
        if int(remaining.item()) == 0:   # the one host read per chunk
            break
    return idx, mse


def jpeg_to_budget(x, noise, factor=SWEEP_FACTOR, subsampling=JPEG_SUBSAMPLING):
    """(round trip at the first quality from 1 upward with mse <= factor * noise, quality [B] int64 (0 where none
    fits), index [B] int32, mse [B]).  An image no quality fits has index -1 and comes back unchanged with mse 0."""
    idx, _ = jpeg_sweep(x, noise, factor, subsampling)
    k = idx.cpu()
    hit = k >= 0
    out, mse = jpeg_roundtrip(x, [i + 1 if i >= 0 else 100 for i in k.tolist()], subsampling, ref=x)
    if not bool(hit.all()):
        miss = (~hit).to(x.device)
        out[miss] = x[miss]
        mse[miss] = 0.0
    return out, (k + 1).to(torch.int64), k, mse


def _ws(name, B, H, W, dev):
    return torch.empty(getattr(lib(), name)(B, H, W), dtype=torch.float32, device=dev)


def gaussian_blur(x, kernel_size=BLUR_KSIZE, sigma=BLUR_SIGMA, clamp=False, ref=None):
    """torchvision's gaussian_blur of x.  ``kernel_size`` is (kx, ky) as in torchvision; ``sigma`` a float or one per
    image.  With ``ref`` returns (blurred, mean((blurred - ref)^2) [B]), else the blurred batch."""
    B, H, W = K.check_image(x, "x")
    sig = [float(s) for s in sigma] if isinstance(sigma, (tuple, list)) else [float(sigma)] * B
    validate(H, W, tuple(kernel_size), sig)
    if len(sig) != B:
        raise ValueError(f"{len(sig)} sigmas for a batch of {B}")
    kx, ky = kernel_size
    if ref is not None:
        if ref.shape != x.shape:
            raise ValueError(f"ref {tuple(ref.shape)} differs from x {tuple(x.shape)}")
        K._dev_check(ref, "ref")
    uniq = {s: (gaussian_taps(kx, s), gaussian_taps(ky, s)) for s in set(sig)}   # one sigma: one pair of host ops
    taps = torch.cat([torch.cat(uniq[s]) for s in sig]).to(x.device).view(B, kx + ky)
    wx, wy = taps[:, :kx].contiguous(), taps[:, kx:].contiguous()
    out = torch.empty_like(x)
    mse = ws = None
    if ref is not None:
        mse = torch.empty(B, dtype=torch.float32, device=x.device)
        ws = _ws("ica_gauss_blur_ws_size", B, H, W, x.device)
    call("ica_gauss_blur", ptr(x), ptr(wx), ptr(wy), B, H, W, kx, ky, int(bool(clamp)), ptr(ref), ptr(out), ptr(mse),
          ptr(ws), stream())
    return out if ref is None else (out, mse)


def blur_sweep(x, sigmas, noise, ksize=SWEEP_KSIZE, factor=SWEEP_FACTOR):
    """Scores the candidates ``sigmas`` in order, a chunk per launch, until every image has its first fit:
    (index [B] int32 on the device, -1 where none fits; mse [B, len(sigmas)], NaN where a candidate was not needed)."""
    B, H, W = K.check_image(x, "x")
    validate(H, W, tuple(ksize), list(sigmas), noise, factor)
    kx, ky = ksize
    dev = x.device
    n = len(sigmas)
    wx = torch.stack([gaussian_taps(kx, s) for s in sigmas]).to(dev)
    wy = torch.stack([gaussian_taps(ky, s) for s in sigmas]).to(dev)
    mse = torch.full((B, n), float("nan"), dtype=torch.float32, device=dev)
    idx = torch.full((B,), -1, dtype=torch.int32, device=dev)
    done = torch.zeros(B, dtype=torch.int32, device=dev)
    remaining = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _ws("ica_blur_sweep_ws_size", B, H, W, dev)
    chunk = lib().ica_blur_sweep_chunk()
    for s0 in range(0, n, chunk):
        S = min(chunk, n - s0)
        call("ica_blur_sweep", ptr(x), ptr(wx[s0:]), ptr(wy[s0:]), S, B, H, W, kx, ky, float(factor * noise), s0,
              ptr(mse), n, ptr(idx), ptr(done), ptr(remaining), ptr(ws), stream())
        if int(remaining.item()) == 0:   # the one host read per chunk
            break
    return idx, mse


def blur_to_budget(x, noise, ksize=SWEEP_KSIZE, factor=SWEEP_FACTOR, start=SIGMA_START, step=SIGMA_STEP):
    """generate_blurimages per image: (clamped blur at the first sigma of the schedule with mse <= factor * noise,
    sigma [B] float64, index [B] int32, mse [B]).  An image no candidate fits has index -1, sigma NaN, and comes back
    unchanged with mse 0."""
    B, H, W = K.check_image(x, "x")
    validate(H, W, tuple(ksize), BLUR_SIGMA, noise, factor, start, step)
    sched = sigma_schedule(start, step)
    idx, _ = blur_sweep(x, sched, noise, ksize, factor)
    k = idx.cpu()
    hit = k >= 0
    sig = [sched[i] if i >= 0 else sched[-1] for i in k.tolist()]
    blurred, mse = gaussian_blur(x, ksize, sig, clamp=True, ref=x)
    if not bool(hit.all()):
        miss = (~hit).to(x.device)
        blurred[miss] = x[miss]
        mse[miss] = 0.0
    sigma = torch.tensor([sched[i] if i >= 0 else float("nan") for i in k.tolist()], dtype=torch.float64)
    return blurred, sigma, k, mse


def apply_noise(im, noise):
    """(clamp(im + noise, 0, 1), mean(noise^2) [B], mean((im_in - im)^2) [B])."""
    B, H, W = K.check_image(im, "im")
    if noise.shape != im.shape:
        raise ValueError(f"noise {tuple(noise.shape)} differs from im {tuple(im.shape)}")
    K._dev_check(noise, "noise")
    if W % 4:
        raise ValueError(f"W = {W} must be a multiple of 4 (16-byte row loads)")
    im_in = torch.empty_like(im)
    power = torch.empty(B, dtype=torch.float32, device=im.device)
    mse_in = torch.empty(B, dtype=torch.float32, device=im.device)
    ws = _ws("ica_noise_apply_ws_size", B, H, W, im.device)
    call("ica_noise_apply", ptr(im), ptr(noise), ptr(im_in), B, H, W, ptr(power), ptr(mse_in), ptr(ws), stream())
    return im_in, power, mse_in


@dataclass
class NoiseResult:
    """test's return (random_noise.py:111) per image, and what its --debug lines print."""
    dpsnr: list          # 10 log10(err_out / mean(noise^2))
    bpp: list            # of the noisy image
    psnr: list           # -10 log10(mean((x_hat - im)^2)) of the noisy image's reconstruction
    bpp_ori: list
    noise_power: list    # mean(noise^2)
    mse_in: list         # mean((im_in - im)^2)
    err_out: list        # mean((x_hat_ori - x_hat)^2)
    x_hat: torch.Tensor  # clamp(x_hat(im_in)) [B, 3, H, W]
    im_in: torch.Tensor


@dataclass
class DeblurResult:
    """test_deblur's return (random_noise.py:48) per image."""
    dpsnr: list          # psnr_blur - psnr_sharp
    bpp: list
    psnr_sharp: list     # -10 log10(mean((x_hat(im_blur) - im_sharp)^2)), x_hat unclamped
    psnr_blur: list      # -10 log10(mean((im_blur - im_sharp)^2))
    x_hat: torch.Tensor


def _db(v):
    return 10.0 * math.log10(v) if v > 0 else float("-inf")


def evaluate_noise(kern, im, noise, num_pixels=None):
    """test (random_noise.py:68-111) per image: one eval forward over [im; im_in].  ``num_pixels`` (an int or one per
    image) is the unpadded H * W that bpp is divided by; the padded size if None."""
    from .attack import eval_forward
    B, H, W = K.check_image(im, "im")
    im_in, power, mse_in = apply_noise(im, noise)
    out, bpp = eval_forward(kern, torch.cat([im, im_in], 0), True)
    x_hat_ori, x_hat = out[:B].contiguous(), out[B:].contiguous()
    err_out = K.sqdiff_mean(x_hat_ori, x_hat).tolist()
    err_im = K.sqdiff_mean(x_hat, im).tolist()
    npx = [H * W] * B if num_pixels is None else ([num_pixels] * B if isinstance(num_pixels, int) else list(num_pixels))
    scale = [H * W / n for n in npx]
    bpp = bpp.tolist()
    power_l = power.tolist()
    return NoiseResult(
        dpsnr=[_db(e / p) if p > 0 else float("nan") for e, p in zip(err_out, power_l)],
        bpp=[bpp[B + b] * scale[b] for b in range(B)],
        psnr=[-_db(e) for e in err_im],
        bpp_ori=[bpp[b] * scale[b] for b in range(B)],
        noise_power=power_l, mse_in=mse_in.tolist(), err_out=err_out, x_hat=x_hat, im_in=im_in)


def evaluate_jpeg(kern, im_jpeg, im, num_pixels=None):
    """test's numbers (random_noise.py:68-111) per image with the JPEG error in the place of the noise:
    noise_power = mse_in = mean((im_jpeg - im)^2), so dpsnr = 10 log10(err_out / mse_in) compares directly with the
    noise baseline and with an attack's VI.  One eval forward over [im; im_jpeg]."""
    from .attack import eval_forward
    B, H, W = K.check_image(im, "im")
    if im_jpeg.shape != im.shape:
        raise ValueError(f"im_jpeg {tuple(im_jpeg.shape)} differs from im {tuple(im.shape)}")
    K._dev_check(im_jpeg, "im_jpeg")
    out, bpp = eval_forward(kern, torch.cat([im, im_jpeg], 0), True)
    x_hat_ori, x_hat = out[:B].contiguous(), out[B:].contiguous()
    mse_in = K.sqdiff_mean(im_jpeg, im).tolist()
    err_out = K.sqdiff_mean(x_hat_ori, x_hat).tolist()
    err_im = K.sqdiff_mean(x_hat, im).tolist()
    npx = [H * W] * B if num_pixels is None else ([num_pixels] * B if isinstance(num_pixels, int) else list(num_pixels))
    scale = [H * W / n for n in npx]
    bpp = bpp.tolist()
    return NoiseResult(
        dpsnr=[_db(e / p) if p > 0 else float("nan") for e, p in zip(err_out, mse_in)],
        bpp=[bpp[B + b] * scale[b] for b in range(B)],
        psnr=[-_db(e) for e in err_im],
        bpp_ori=[bpp[b] * scale[b] for b in range(B)],
        noise_power=mse_in, mse_in=list(mse_in), err_out=err_out, x_hat=x_hat, im_in=im_jpeg)


def evaluate_deblur(kern, im_blur, im_sharp):
    """test_deblur (random_noise.py:38-48) per image, on the unclamped x_hat; bpp over the padded H * W the
    reference divides by (:38)."""
    from .attack import eval_forward
    K.check_image(im_blur, "im_blur")
    if im_sharp.shape != im_blur.shape:
        raise ValueError(f"im_sharp {tuple(im_sharp.shape)} differs from im_blur {tuple(im_blur.shape)}")
    K._dev_check(im_sharp, "im_sharp")
    x_hat, bpp = eval_forward(kern, im_blur, False)
    psnr_blur = [-_db(v) for v in K.sqdiff_mean(im_blur, im_sharp).tolist()]
    psnr_sharp = [-_db(v) for v in K.sqdiff_mean(x_hat, im_sharp).tolist()]
    return DeblurResult(dpsnr=[a - b for a, b in zip(psnr_blur, psnr_sharp)], bpp=bpp.tolist(),
                        psnr_sharp=psnr_sharp, psnr_blur=psnr_blur, x_hat=x_hat)
