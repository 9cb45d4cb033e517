"""The per-channel latent range (the paper's "safe zone") on the HIP kernels (ica_latent.hip): the profile over
a dataset, the detector score and the clamp defence, all on the nChw4c latent y4 = g_a(x) the engine holds.

latent_range      feature_range.py:19-21   amax / amin / amax(abs) per (image, channel)   (ica_latent_range)
build_profile     feature_range.py:35-66   the topk-th largest max / smallest min per channel over the images
RangeProfile      feature_range.py:69-72   [channel_max, channel_min], the reference's file format and path
latent_clamp      clamp_value_naive (attack_rd.py:53-73, search.py:25-36)                 (ica_latent_clamp)
latent_clamp_bwd_ the autograd of the clamp's two torch.where with respect to y           (ica_latent_clamp_bwd)
latent_detect     detect (search.py:137-146), one score per image                         (ica_latent_detect)

For the bf16 engine everything here runs on the fp32 cast of y4 (the one CodecKernels.forward makes).
"""
from __future__ import annotations

import os

import torch

from . import hip_ops as K
from ._lib import call, ptr, stream


def _quads_check(C):
    if C < 1 or C % 4:   # the entry points' status -2
        raise ValueError(f"C = {C} channels must be a positive multiple of 4 (whole nChw4c channel quads)")


def _y4_check(y4, C, name="y4"):
    K._dev_check(y4, name)
    if y4.dim() != 5 or y4.shape[4] != 4 or y4.shape[1] != K.c4(C):
        raise ValueError(f"{name} {tuple(y4.shape)} is not an nChw4c tensor of {C} channels")
    _quads_check(C)


class RangeProfile:
    """channel_max / channel_min of a codec's latent: device fp32 [C] for the kernels plus a CPU copy."""

    def __init__(self, channel_max, channel_min, device=None):
        cmax = torch.as_tensor(channel_max).detach().to(torch.float32).flatten()
        cmin = torch.as_tensor(channel_min).detach().to(torch.float32).flatten()
        if cmax.shape != cmin.shape or cmax.numel() == 0:
            raise ValueError(f"profile shapes {tuple(cmax.shape)} / {tuple(cmin.shape)}")
        self.channel_max, self.channel_min = cmax.cpu().contiguous(), cmin.cpu().contiguous()
        self.C = cmax.numel()
        self._dev = {}
        if device is not None:
            self.on(device)

    def on(self, device):
        """(channel_max, channel_min) on `device` (copied once per device)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the latent-range kernels run on the HIP device (no CPU fallback)")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._dev:
            self._dev[key] = (self.channel_max.to(device).contiguous(), self.channel_min.to(device).contiguous())
        return self._dev[key]

    def save(self, path):
        """feature_range.py:72: torch.save([channel_max, channel_min], path), CPU tensors."""
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        torch.save([self.channel_max, self.channel_min], path)

    @classmethod
    def load(cls, path, device=None):
        cmax, cmin = torch.load(path, map_location="cpu", weights_only=True)
        return cls(cmax, cmin, device)

    @staticmethod
    def default_path(args):
        """feature_range.py:69-72 / search.py:26-30: ./attack/data/{model}-{metric}-{quality}[-adv]_range.pt"""
        profile = f"{args.model}-{args.metric}-{args.quality}"
        if args.adv:
            profile += "-adv"
        return f"./attack/data/{profile}_range.pt"


default_path = RangeProfile.default_path


def latent_range(y4, C, absmax=True):
    """(max, min, absmax) [B][C] of each (image, channel) plane of y4: torch.amax / amin / amax(abs) bits."""
    _y4_check(y4, C)
    B, _, H, W, _ = y4.shape
    out = torch.empty((3 if absmax else 2, B, C), dtype=torch.float32, device=y4.device)
    call("ica_latent_range", ptr(y4), B, C, H, W, ptr(out[0]), ptr(out[1]), ptr(out[2]) if absmax else None,
          stream())
    return (out[0], out[1], out[2]) if absmax else (out[0], out[1], None)


def _bounds(profile, C, device):
    if profile.C != C:
        raise ValueError(f"the profile has {profile.C} channels, the latent {C}")
    return profile.on(device)


def latent_clamp(y4, C, profile, out=None, count=False):
    """clamp_value_naive: where(y > cmax, cmax, y) then where(. < cmin, cmin, .).  out may be y4 (in place).
    count=True also returns the per-image number of changed elements (int32 [B], on the device)."""
    _y4_check(y4, C)
    cmax, cmin = _bounds(profile, C, y4.device)
    if out is None:
        out = torch.empty_like(y4)
    else:
        _y4_check(out, C, "out")
        if out.shape != y4.shape:
            raise ValueError("out must have y4's shape")
    B, _, H, W, _ = y4.shape
    n = torch.empty(B, dtype=torch.int32, device=y4.device) if count else None
    call("ica_latent_clamp", ptr(y4), ptr(cmax), ptr(cmin), ptr(out), B, C, H, W, ptr(n), stream())
    return (out, n) if count else out


def latent_clamp_bwd_(g4, y4, C, profile):
    """g4 *= d clamp(y) / d y (1 where both selects took y, else 0), in place; y4 is the clamp's input."""
    _y4_check(y4, C)
    _y4_check(g4, C, "g4")
    if g4.shape != y4.shape:
        raise ValueError("g4 must have y4's shape")
    cmax, cmin = _bounds(profile, C, y4.device)
    B, _, H, W, _ = y4.shape
    call("ica_latent_clamp_bwd", ptr(g4), ptr(y4), ptr(cmax), ptr(cmin), B, C, H, W, stream())
    return g4


def latent_detect(imax, imin, profile):
    """search.detect per image from the per-image channel extremes imax / imin [B][C]: score [B] on the device."""
    K._dev_check(imax, "imax")
    K._dev_check(imin, "imin")
    if imax.dim() != 2 or imax.shape != imin.shape:
        raise ValueError(f"imax {tuple(imax.shape)} / imin {tuple(imin.shape)} must both be [B][C]")
    B, C = imax.shape
    cmax, cmin = _bounds(profile, C, imax.device)
    _quads_check(C)
    score = torch.empty(B, dtype=torch.float32, device=imax.device)
    call("ica_latent_detect", ptr(imax), ptr(imin), ptr(cmax), ptr(cmin), ptr(score), B, C, stream())
    return score


def latent_of(kern, x):
    """y4 = g_a(x) (fp32 nChw4c) of an NCHW image batch on the device."""
    y4, _ = kern.g_a(K.to_nc4(x))
    return K.cast_nc4(y4, torch.float32)


def order_statistic(maxs, mins, topk=100):
    """feature_range.py:65-66 on the collected [N][C] rows: the topk-th largest max and the topk-th smallest min
    per channel."""
    N = maxs.shape[0]
    if N < topk:
        raise ValueError(f"the profile needs at least topk = {topk} images, got N = {N}")
    cmax = maxs.topk(k=topk, dim=0)[0][-1]
    cmin = mins.topk(k=topk, dim=0, largest=False)[0][-1]
    return cmax, cmin


def build_profile(kern, batches, topk=100, device=None):
    """feature_range.py:35-66: per batch of same-size images (NCHW, on the device) g_a then ica_latent_range; the
    per-image rows are collected on the host and reduced by the reference's order statistic (exact O(N C)
    plumbing)."""
    maxs, mins = [], []
    for x in batches:
        mx, mn, _ = latent_range(latent_of(kern, x), kern.M, absmax=False)
        maxs.append(mx.cpu())
        mins.append(mn.cpu())
        device = device or x.device
    if not maxs:
        raise ValueError(f"the profile needs at least topk = {topk} images, got N = 0")
    cmax, cmin = order_statistic(torch.cat(maxs, 0), torch.cat(mins, 0), topk)
    return RangeProfile(cmax, cmin, device)


def score_images(kern, x, profile):
    """search.eval's score of every image of an NCHW batch (clamped to [0, 1] as search.py:157): [B] on the device."""
    mx, mn, _ = latent_range(latent_of(kern, K.clamp01(x.contiguous())), kern.M, absmax=False)
    return latent_detect(mx, mn, profile)
