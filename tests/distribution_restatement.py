"""torch-CPU restatement of the numbers of visual_distribution.py, written fresh from its text, on NCHW tensors
[B][C][H][W] (the script itself works on one image, [C][H][W]; a leading batch axis changes nothing).

histc          :158-159   torch.histc per (image, channel) plane over unit bins
predicted      :85-101    clamp(scales, 0.11), Normal(means, scales).cdf at x -/+ 0.5, clamp(upper - lower, 1/65536),
                          the mean over (H, W); in a chosen dtype (the script's abscissae are float64 numpy values, so
                          its cdf promotes to float64; float32 is the kernel's arithmetic, float64 the truth)
rate           :163-164   sum(hist * -log(pred)) / log(2)
err, ranking   :170-179   rate_adv - rate_ori, argsort(descending)
bits           (not in the script) sum over (H, W) of -log2(likelihood)

nChw4c helpers (to_nc4 / from_nc4) move test tensors into and out of the engine's latent layout."""
import math

import torch

VMIN, NBINS, SCALE_FLOOR, PRED_FLOOR = -5.5, 11, 0.11, 1.0 / 65536.0


def to_nc4(x):
    """[B][C][H][W] (C a multiple of 4) -> [B][C/4][H][W][4]"""
    B, C, H, W = x.shape
    return x.reshape(B, C // 4, 4, H, W).permute(0, 1, 3, 4, 2).contiguous()


def from_nc4(x4):
    B, C4, H, W, _ = x4.shape
    return x4.permute(0, 1, 4, 2, 3).reshape(B, C4 * 4, H, W).contiguous()


def vmax_of(vmin, nbins):
    """vmin + nbins as the float32 the kernel and torch.histc both see"""
    return float(torch.tensor(vmin, dtype=torch.float32) + nbins)


def histc(y, vmin=VMIN, nbins=NBINS):
    """int64 [B][C][nbins]"""
    B, C = y.shape[:2]
    out = torch.empty((B, C, nbins), dtype=torch.int64)
    hi = vmax_of(vmin, nbins)
    for b in range(B):
        for c in range(C):
            out[b, c] = torch.histc(y[b, c].float(), bins=nbins, min=vmin, max=hi).to(torch.int64)
    return out


def centres(vmin=VMIN, nbins=NBINS):
    """:143 np.linspace(v_min + 0.5, v_max - 0.5, bins): unit steps"""
    return [vmin + 0.5 + k for k in range(nbins)]


def predicted(scales, means=None, vmin=VMIN, nbins=NBINS, dtype=torch.float64, scale_floor=SCALE_FLOOR,
              pred_floor=PRED_FLOOR, mean=True):
    """[B][C][nbins] (mean=False: [B][C][H][W][nbins]) in `dtype`"""
    scales = torch.clamp(scales.to(dtype), min=scale_floor)
    means = torch.zeros_like(scales) if means is None else means.to(dtype)
    ax_x = torch.tensor(centres(vmin, nbins), dtype=dtype)
    m1 = torch.distributions.Normal(means[..., None], scales[..., None], validate_args=False)
    lower = m1.cdf(ax_x - 0.5)
    upper = m1.cdf(ax_x + 0.5)
    pred = torch.clamp(upper - lower, min=pred_floor)
    return torch.mean(pred, dim=(2, 3)) if mean else pred


def rate(hist, pred):
    return torch.sum(hist.to(pred.dtype) * -torch.log(pred), dim=-1) / math.log(2)


def rate_gap(hist, pred, hist_adv, pred_adv):
    """(err, channel_index): :170, :179 (stable, so equal gaps keep channel order)"""
    err = rate(hist_adv, pred_adv) - rate(hist, pred)
    return err, torch.argsort(err, dim=-1, descending=True, stable=True)


def bits(lik, dtype=torch.float64):
    return -torch.log2(lik.to(dtype)).sum(dim=(2, 3))
