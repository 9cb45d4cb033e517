"""Rate-distortion evaluation on clean images (the reference's test.py / batch_test) on the HIP engine.

rd_eval_batch     test.py:51-52   criterion(net(im), im, training=False), per image
rd_eval_defended  test.py:37-49   the same behind --defend (ensemble | bitdepth | resize, and the range clamp)

Per image the numbers are RateDistortionLoss(..., training=False) (train.py:50-70) with N = 1: the likelihoods
clamped at 1/65536, bpp over the padded H * W that coder.read_image produces, mse of the clamped reconstruction, the
pytorch_msssim MS-SSIM, psnr = -10 log10(mse) and msim_dB = -10 log10(1 - msim).  One eval forward, one
``hip_ops.rd_metrics`` launch (ica_rdeval.hip: the clamp, both likelihood sums, the squared error, the clamped NCHW
reconstruction and the census of clamped likelihoods), one row reduction, then the MS-SSIM pyramid.

Defended evaluation follows test.py, not self_ensemble.eval: every method is scored against the ORIGINAL image.
  ensemble : the likelihoods and the back-rotated, clamped reconstruction of the best of the 8 dihedral variants
             (least mean((variant - its unclamped reconstruction)^2), first minimum)
  bitdepth : net(round(x * 63) / 63)           (test.py:46-49 re-runs the net on the rounded image)
  resize   : net(random_resize(x, 243 / 256))  (an image whose size the resize changes raises, as the reference's
             mse would)
  range    : the latent clamp of attack_rd.py:263-268 through forward(latent=...) (an extension, as in self_ensemble)
  jpeg     : net(degrade.jpeg_roundtrip(x, quality, subsampling))  (an extension: the JPEG input transformation)

Deviations from test.py (DESIGN.md "RD evaluation"): images whose smaller side is <= 160 get msim = msim_dB = nan
(pytorch_msssim raises there); msim == 1 gives msim_dB = inf instead of the reference's math domain error; psnr and
msim_dB are float64 of the fp32 mse / msim, as the reference's math.log10 of a Python float.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from . import hip_ops as K
from . import msssim as MS

METHODS = ("ensemble", "bitdepth", "resize", "range", "jpeg")
MSSSIM_MIN_SIDE = 160   # pytorch_msssim: min(H, W) > (11 - 1) * 2 ** 4


@dataclass
class RDResult:
    """Per-image values [B], on the CPU: fp32 as the engine computed them; psnr / msim_dB float64."""
    bpp: torch.Tensor
    bpp_y: torch.Tensor
    bpp_z: torch.Tensor
    mse: torch.Tensor
    psnr: torch.Tensor
    msim: torch.Tensor
    msim_dB: torch.Tensor
    nclamp: torch.Tensor                  # int32: likelihood elements below 2^-16
    x_hat: torch.Tensor | None = None     # clamp(x_hat, 0, 1) [B, 3, H, W], on the device
    real_bpp: torch.Tensor | None = None  # 8 * bytes / (H * W) of net.compress, float64 (--real-bpp)
    best_idx: list | None = None          # ensemble: the chosen variant per image


def neg10log10(v: torch.Tensor) -> torch.Tensor:
    """-10 log10(v) in float64: 0 gives inf (not math.log10's ValueError), a negative value nan."""
    return -10.0 * torch.log10(v.detach().double().cpu())


def compose(sse, lny, lnz, msim, H, W):
    """The per-image metrics from the kernel's sums, in the reference's operations and order (fp32 tensors [B]):
    bpp = 0 + lny / (-ln 2 * H W) + lnz / (-ln 2 * H W), mse = sse / (3 H W).  msim: [B] or None (nan)."""
    den = -math.log(2) * (H * W)
    bpp_y, bpp_z = lny / den, lnz / den
    mse = sse / (3 * H * W)
    if msim is None:
        msim = torch.full_like(mse, float("nan"))
    return {"bpp": bpp_y + bpp_z, "bpp_y": bpp_y, "bpp_z": bpp_z, "mse": mse, "psnr": neg10log10(mse),
            "msim": msim, "msim_dB": neg10log10(1.0 - msim.detach().double().cpu())}


def _check_batch(x):
    B, H, W = K.check_image(x, "x", dev=False)
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError("the RD evaluation runs on HIP fp32 tensors (no CPU fallback)")
    return x.contiguous(), B, H, W


def score(kern, res, target, msssim=True) -> RDResult:
    """RateDistortionLoss(res, target, training=False) per image from an eval forward's result dict."""
    B, _, H, W = target.shape
    lik = res["lik4"]
    lik_z = lik.get("z")
    x_hat4 = K.cast_nc4(res["x_hat4"], torch.float32)   # the bf16 engine's reconstruction
    sse, lny, lnz, nclamp, out = K.rd_metrics(x_hat4, target, lik["y"], kern.M, lik_z,
                                              kern.eb.C if lik_z is not None else 0)
    msim = MS.ms_ssim_per_image(out, target) if msssim and min(H, W) > MSSSIM_MIN_SIDE else None
    m = compose(sse, lny, lnz, msim, H, W)
    cpu = {k: v.detach().cpu() for k, v in m.items()}
    return RDResult(nclamp=nclamp.cpu(), x_hat=out, **cpu)


def real_bpp(net, x) -> torch.Tensor:
    """8 * len(bitstreams) / (H * W) per image from the model's own compress() (float64 [B]).  The context models
    code position by position: slow."""
    if not hasattr(net, "compress"):
        raise NotImplementedError(f"{type(net).__name__} has no compress(): no real bpp for this model")
    B, _, H, W = x.shape
    net.update()
    strings = net.compress(x)["strings"]
    return torch.tensor([8.0 * sum(len(s[b]) for s in strings) / (H * W) for b in range(B)], dtype=torch.float64)


def rd_eval_batch(kern, x, real_bpp_net=None, msssim=True) -> RDResult:
    """test.py's plain evaluation of a batch of same-size images, per image.  real_bpp_net: the model whose
    compress() gives ``real_bpp``; it is reported next to the estimated bpp and never mixed into it."""
    x, B, H, W = _check_batch(x)
    r = score(kern, kern.forward(K.to_nc4(x)), x, msssim)
    if real_bpp_net is not None:
        r.real_bpp = real_bpp(real_bpp_net, x)
    return r


def _cat(results, best_idx=None) -> RDResult:
    def cat(name):
        vals = [getattr(r, name) for r in results]
        return None if vals[0] is None else torch.cat(vals, 0)
    return RDResult(**{f: cat(f) for f in ("bpp", "bpp_y", "bpp_z", "mse", "psnr", "msim", "msim_dB", "nclamp",
                                           "x_hat", "real_bpp")}, best_idx=best_idx)


def _eval_ensemble(kern, x, real_bpp_net, msssim):
    """self_ensemble.self_ensemble in eval mode (self_ensemble.py:85-131) as test.py:41-45 uses it."""
    from . import self_ensemble as SE
    B = x.shape[0]
    xs = SE.rotates(x)
    groups, mses = [], []
    for group in (xs[:4], xs[4:]):
        xcat = torch.cat(group, dim=0)   # variant-major, like the reference's cat(xs[:4])
        res = kern.forward(K.to_nc4(xcat))
        xh = K.from_nc4(K.cast_nc4(res["x_hat4"], torch.float32), 3)
        mses.append(K.sqdiff_mean(xcat, xh).view(4, B))   # mean((x - x_hat)^2), x_hat unclamped
        groups.append((res, xh))
    best = torch.argmin(torch.cat(mses, 0), dim=0).tolist()   # first minimum, like the strict '<' scan
    out = []
    for b, i in enumerate(best):
        res, xh = groups[i // 4]
        row = (i % 4) * B + b
        back = SE.rotates(xh[row:row + 1].contiguous(), reverse=i).contiguous()
        one = {"x_hat4": K.to_nc4(back),
               "lik4": {k: v[row:row + 1].contiguous() for k, v in res["lik4"].items()}}
        r = score(kern, one, x[b:b + 1].contiguous(), msssim)
        if real_bpp_net is not None:
            r.real_bpp = real_bpp(real_bpp_net, xs[i][b:b + 1].contiguous())
        out.append(r)
    return _cat(out, best)


def rd_eval_defended(kern, x, method="ensemble", profile=None, real_bpp_net=None, msssim=True, jpeg=None) -> RDResult:
    """test.py's evaluation with --defend (test.py:37-49), per image, scored against the original ``x``.
    profile: the latent_range.RangeProfile of method 'range'; jpeg: (quality, subsampling) of method 'jpeg'
    (None: what a coder.JpegMethod carries, as batch_test passes it, else (50, "420"))."""
    if method not in METHODS:
        raise ValueError(f"defend method {method!r} not in {METHODS}")
    if method == "jpeg":
        from . import degrade
        jpeg = jpeg or (getattr(method, "quality", degrade.JPEG_QUALITY),
                        getattr(method, "subsampling", degrade.JPEG_SUBSAMPLING))
        degrade.validate_jpeg(quality=jpeg[0], subsampling=jpeg[1])
    x, B, H, W = _check_batch(x)
    if method == "ensemble":
        return _eval_ensemble(kern, x, real_bpp_net, msssim)
    if method == "range":
        from .latent_range import latent_clamp
        if profile is None:
            raise ValueError("method 'range' needs a RangeProfile (profile=...)")
        if real_bpp_net is not None:
            raise NotImplementedError("--real-bpp with the range defence: compress() does not clamp the latent")
        res = kern.forward(K.to_nc4(x), latent=lambda y4: latent_clamp(y4, kern.M, profile))
        return score(kern, res, x, msssim)
    from . import self_ensemble as SE
    xp = SE.defend(kern, x, method, jpeg)
    if xp.shape != x.shape:
        raise RuntimeError(f"defend '{method}' changed the image size {tuple(x.shape)} -> {tuple(xp.shape)} (the "
                           f"reference's mse against the original fails the same way)")
    r = score(kern, kern.forward(K.to_nc4(xp)), x, msssim)
    if real_bpp_net is not None:
        r.real_bpp = real_bpp(real_bpp_net, xp)
    return r
