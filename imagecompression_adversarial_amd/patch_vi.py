"""Patch-wise VI localisation on the HIP kernels (ica_patch.hip): where did an attack's damage land?

local_vi        psnr_partial's maps (attack_patch.py:121-140)   mse_in / mse_out / vi per window, and the argmax
worst_patches   psnr_partial's return (attack_patch.py:141-146) the four win x win patches at the worst window
localize        both, over an attack.AttackResult

The four inputs are the planar NCHW fp32 tensors attack.evaluate / AttackResult hold.  Everything stays on the
device (a batch is cut without a host read); only ``Localized.vi_db`` is a host value.  Differences from the
reference (DESIGN.md "Patch VI"): fp32 instead of its fp16 unfold, any batch size, and windows with
mse_in == 0 are excluded (vi = 0) where the reference would divide by zero.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from . import hip_ops as K
from ._lib import call, lib, ptr, stream

WIN, STRIDE, BORDER = 64, 2, 10   # attack_patch.py:121, :137-140


def map_shape(H, W, win=WIN, stride=STRIDE):
    """(nh, nw): the windows of an H x W image (attack_patch.py:126)."""
    return (H - win) // stride + 1, (W - win) // stride + 1


def validate(H, W, win=WIN, stride=STRIDE, border=BORDER):
    """ValueError unless the kernels take this problem (include/ica_hip.h, ica_patch_vi)."""
    for name, v in (("H", H), ("W", W), ("win", win), ("stride", stride), ("border", border)):
        if not isinstance(v, int) or isinstance(v, bool):
            raise ValueError(f"{name} must be an int, got {v!r}")
    if stride not in (1, 2, 4):
        raise ValueError(f"stride {stride} is not one of 1, 2, 4")
    if win < 1 or win > 128:
        raise ValueError(f"win {win} is outside 1 .. 128")
    if win % stride:
        raise ValueError(f"win {win} is not a multiple of stride {stride}")
    if H < win or W < win:
        raise ValueError(f"the image {H}x{W} is smaller than the window {win}")
    if W % 4:
        raise ValueError(f"W = {W} must be a multiple of 4 (16-byte row loads)")
    if W // stride > 8192:
        raise ValueError(f"W / stride = {W // stride} exceeds 8192 (one cell row is staged in LDS)")
    if border < 0:
        raise ValueError(f"border {border} is negative")


def _check_inputs(im_adv, out_adv, im_s, out_s, win, stride, border):
    B, H, W = K.check_image(im_adv, "im_adv", dev=False)   # validate() runs before the device checks
    for name, t in (("out_adv", out_adv), ("im_s", im_s), ("out_s", out_s)):
        if t.shape != im_adv.shape:
            raise ValueError(f"{name} {tuple(t.shape)} differs from im_adv {tuple(im_adv.shape)}")
    validate(H, W, win, stride, border)
    for name, t in (("im_adv", im_adv), ("out_adv", out_adv), ("im_s", im_s), ("out_s", out_s)):
        K._dev_check(t, name)
    return B, H, W


@dataclass
class LocalVI:
    mse_in: torch.Tensor    # [B, nh, nw]  mean((im_s - im_adv)^2) per window
    mse_out: torch.Tensor   # [B, nh, nw]  mean((out_s - out_adv)^2) per window
    vi: torch.Tensor        # [B, nh, nw]  mse_out / mse_in; 0 on the border and where mse_in == 0
    val: torch.Tensor       # [B]          the largest vi
    pos: torch.Tensor       # [B, 2] int32 its first (row, col) in the map; pixel origin = pos * stride
    win: int
    stride: int
    border: int

    def origin(self):
        """Pixel (y, x) of the worst window's top-left corner, [B, 2] int32 on the device."""
        return self.pos * self.stride


@dataclass
class Localized:
    vi: LocalVI
    patches: torch.Tensor   # [B, 4, 3, win, win]: adv, outadv, s, outs
    vi_db: list             # 10 log10(val) per image (None where val == 0)
    origin: list            # (y, x) pixel origin of the worst window per image


def local_vi(im_adv, out_adv, im_s, out_s, win=WIN, stride=STRIDE, border=BORDER):
    B, H, W = _check_inputs(im_adv, out_adv, im_s, out_s, win, stride, border)
    nh, nw = map_shape(H, W, win, stride)
    dev = im_adv.device
    maps = torch.empty((3, B, nh, nw), dtype=torch.float32, device=dev)
    val = torch.empty(B, dtype=torch.float32, device=dev)
    pos = torch.empty((B, 2), dtype=torch.int32, device=dev)
    ws = torch.empty(lib().ica_patch_vi_ws_size(B, H, W, win, stride), dtype=torch.float32, device=dev)
    key = torch.empty(B, dtype=torch.int64, device=dev)
    call("ica_patch_vi", ptr(im_adv), ptr(out_adv), ptr(im_s), ptr(out_s), B, H, W, win, stride, border, ptr(ws),
          ptr(key), ptr(maps[0]), ptr(maps[1]), ptr(maps[2]), ptr(val), ptr(pos), stream())
    return LocalVI(maps[0], maps[1], maps[2], val, pos, win, stride, border)


def worst_patches(im_adv, out_adv, im_s, out_s, win=WIN, stride=STRIDE, border=BORDER, pos=None):
    """[B, 4, 3, win, win] in psnr_partial's order (adv, outadv, s, outs), cut at the worst window of each image.
    ``pos`` ([B, 2] int32 on the device, e.g. LocalVI.pos) skips the search."""
    B, H, W = _check_inputs(im_adv, out_adv, im_s, out_s, win, stride, border)
    if pos is None:
        pos = local_vi(im_adv, out_adv, im_s, out_s, win, stride, border).pos
    if not pos.is_cuda or pos.dtype != torch.int32 or tuple(pos.shape) != (B, 2) or not pos.is_contiguous():
        raise ValueError("pos must be a contiguous int32 [B, 2] tensor on the device")
    patches = torch.empty((B, 4, 3, win, win), dtype=torch.float32, device=im_adv.device)
    call("ica_patch_gather", ptr(im_adv), ptr(out_adv), ptr(im_s), ptr(out_s), ptr(pos), ptr(patches), B, H, W, win,
          stride, stream())
    return patches


def localize(res, im_s, win=WIN, stride=STRIDE, border=BORDER):
    """The local VI of an attack.AttackResult (its im_adv / output_adv / output_s) against the source im_s."""
    args = (res.im_adv.contiguous(), res.output_adv.contiguous(), im_s.contiguous(), res.output_s.contiguous())
    lv = local_vi(*args, win=win, stride=stride, border=border)
    patches = worst_patches(*args, win=win, stride=stride, border=border, pos=lv.pos)
    vi_db = [10.0 * math.log10(v) if v > 0 else None for v in lv.val.tolist()]
    origin = [tuple(p) for p in lv.origin().tolist()]
    return Localized(lv, patches, vi_db, origin)
