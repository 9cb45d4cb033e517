"""The latent-distribution study of visual_distribution.py on the HIP kernel (ica_distrib.hip): where, channel by
channel, an adversarial example moves the latent's histogram away from what the entropy model predicts for it.

latent_distrib   torch.histc per channel (:158-159), predicted_distribution (:85-101), sum -log2(lik)   (ica_latent_distrib)
channel_rate     sum_k hist_k * -log(pred_k) / ln 2 (:163-164)
rate_gap         err = rate_adv - rate_ori and the channels ranked by it (:170-179)
study            both eval forwards of a clean / adversarial batch and everything above, per image

y, sigma and mu are the eval forward's own y4 / scales4 / means4 (mu = 0 for the hyperprior model, :136-137), the
tensors the codec codes with; the reference's probe cannot produce them (DESIGN.md "Latent distribution").  For the
bf16 engine everything here runs on the fp32 cast of y4 (the one the forward makes).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from . import hip_ops as K
from ._lib import call, lib, ptr, stream
from .latent_range import _y4_check

VMIN, NBINS = -5.5, 11            # visual_distribution.py:139-141
SCALE_FLOOR = 0.11                # :86
PRED_FLOOR = 1.0 / 65536.0        # :97
MAX_NBINS = 64


@dataclass
class Distrib:
    hist: torch.Tensor            # int32 [B][C][nbins]: torch.histc counts of y
    pred: torch.Tensor            # fp32  [B][C][nbins]: mean over (H, W) of the floored Gaussian bin masses
    bits: torch.Tensor | None     # fp32  [B][C]: sum over (H, W) of -log2(lik); None without lik4
    pixels: int = 0               # H * W of the latent plane
    inputs: tuple = ()            # keep_inputs=True: the (y4, scales4, means4, lik4) the numbers came from


@dataclass
class Study:
    clean: Distrib
    adv: Distrib
    hist_frac: torch.Tensor       # hist / pixels of the clean batch, fp32 [B][C][nbins] (the reference's y_hat)
    hist_frac_adv: torch.Tensor   # the same of the adversarial batch (y_hat_t_hist)
    rate_ori: torch.Tensor        # [B][C]
    rate_adv: torch.Tensor        # [B][C]
    err: torch.Tensor             # [B][C] rate_adv - rate_ori
    channel_index: torch.Tensor   # int64 [B][C]: channels by descending err, ties in channel order
    outside: torch.Tensor         # int64 [B][C]: pixels - sum_k hist, clean
    outside_adv: torch.Tensor
    bits: torch.Tensor            # [B][C], clean
    bits_adv: torch.Tensor


def check_model(model):
    """The study needs a conditional entropy model for y: hyper, context (mbt2018) or cheng2020, as the reference."""
    if model == "factorized":
        raise NotImplementedError("the latent-distribution study needs the conditional entropy model of y (scales, "
                                  "means): -m factorized has none; use hyper, context or cheng2020")


def _bins_check(vmin, nbins):
    if not isinstance(nbins, int) or isinstance(nbins, bool) or not 1 <= nbins <= MAX_NBINS:
        raise ValueError(f"nbins = {nbins!r} must be an int in 1 .. {MAX_NBINS}")
    if not math.isfinite(vmin):
        raise ValueError(f"vmin = {vmin!r} must be finite")


def latent_distrib(y4, C, scales4, means4=None, lik4=None, vmin=VMIN, nbins=NBINS, scale_floor=SCALE_FLOOR,
                   pred_floor=PRED_FLOOR, keep_inputs=False):
    """Distrib(hist, pred, bits) of an nChw4c latent batch: unit bins [vmin + k, vmin + k + 1), the last one closed;
    means4 None is mu = 0, lik4 None gives bits None.  keep_inputs=True keeps references to the four input tensors
    in the result (they stay allocated as long as it lives)."""
    _y4_check(y4, C)
    _bins_check(vmin, nbins)
    for name, t in (("scales4", scales4), ("means4", means4), ("lik4", lik4)):
        if t is None:
            if name == "scales4":
                raise ValueError("scales4 is required")
            continue
        _y4_check(t, C, name)
        if t.shape != y4.shape or t.device != y4.device:
            raise ValueError(f"{name} {tuple(t.shape)} on {t.device} must match y4 {tuple(y4.shape)} on {y4.device}")
    B, _, H, W, _ = y4.shape
    n = lib().ica_latent_distrib_ws_size(B, C, H, W, nbins)
    if n == 0:
        raise ValueError(f"ica_latent_distrib does not take B, C, H, W, nbins = {(B, C, H, W, nbins)}")
    dev = y4.device
    hist = torch.empty((B, C, nbins), dtype=torch.int32, device=dev)
    pred = torch.empty((B, C, nbins), dtype=torch.float32, device=dev)
    bits = torch.empty((B, C), dtype=torch.float32, device=dev) if lik4 is not None else None
    work = torch.empty(n, dtype=torch.float32, device=dev)
    call("ica_latent_distrib", ptr(y4), ptr(scales4), ptr(means4), ptr(lik4), B, C, H, W, float(vmin), nbins,
         float(scale_floor), float(pred_floor), ptr(hist), ptr(pred), ptr(bits), ptr(work), stream())
    return Distrib(hist, pred, bits, H * W, (y4, scales4, means4, lik4) if keep_inputs else ())


def channel_rate(hist, pred):
    """visual_distribution.py:163-164 per (image, channel): sum_k hist_k * -log(pred_k) / ln 2, fp32 torch ops on
    the tensors' own device (B * C * nbins numbers)."""
    return torch.sum(hist.to(torch.float32) * -torch.log(pred.to(torch.float32)), dim=-1) / math.log(2)


def rate_gap(clean, adv, rate_ori=None, rate_adv=None):
    """(err, channel_index) of two Distribs (:170-179): err = rate_adv - rate_ori [B][C]; channel_index the channels
    of each image by descending err, equal values in channel order (a stable sort).  The two rates may be passed
    by a caller that already holds them."""
    rate_ori = channel_rate(clean.hist, clean.pred) if rate_ori is None else rate_ori
    rate_adv = channel_rate(adv.hist, adv.pred) if rate_adv is None else rate_adv
    err = rate_adv - rate_ori
    return err, torch.argsort(err, dim=-1, descending=True, stable=True)


def forward_distrib(kern, x, vmin=VMIN, nbins=NBINS, keep_inputs=False):
    """Distrib of an NCHW image batch: the eval forward, then the kernel on the forward's own tensors."""
    res = kern.forward(K.to_nc4(x))
    y4 = K.cast_nc4(res["y4"], torch.float32)
    return latent_distrib(y4, kern.M, res["scales4"], res.get("means4"), res["lik4"]["y"], vmin, nbins,
                          keep_inputs=keep_inputs)


def study(kern, im, im_adv, vmin=VMIN, nbins=NBINS, keep_inputs=False):
    """The study of a clean batch and its adversarial examples (NCHW on the device, one size) on a CodecKernels or
    ChengKernels of any precision.  keep_inputs: as latent_distrib, for both forwards."""
    check_model(getattr(kern, "model", None))
    _bins_check(vmin, nbins)
    if im.shape != im_adv.shape:
        raise ValueError(f"im {tuple(im.shape)} and im_adv {tuple(im_adv.shape)} must have one shape")
    clean = forward_distrib(kern, im, vmin, nbins, keep_inputs)
    adv = forward_distrib(kern, im_adv, vmin, nbins, keep_inputs)
    rate_ori, rate_adv = channel_rate(clean.hist, clean.pred), channel_rate(adv.hist, adv.pred)
    err, index = rate_gap(clean, adv, rate_ori, rate_adv)
    px = clean.pixels
    return Study(clean, adv, clean.hist / px, adv.hist / px, rate_ori, rate_adv, err, index,
                 px - clean.hist.sum(-1, dtype=torch.int64), px - adv.hist.sum(-1, dtype=torch.int64),
                 clean.bits, adv.bits)
