"""Iterated re-compression (generation loss) of recompression.py on the HIP engine: what happens to an image when
the codec's own 8-bit output is coded again and again.

requant8 / quant8_pack / floor_bits   the kernels of ica_recompress.hip
recompress    recompression.py:19-63: G generations of net.eval()(im) -> write_image(clamp(x_hat)) -> read_image,
              for a batch, with every generation's metrics (the reference scores the last one only)
rd_metrics    RateDistortionLoss(training=False) + PSNR of one eval forward (train.py:50-72, utils/metrics.py:7-11):
              test.py's undefended path

The step between two generations is one launch (ica_requant8): it reads the forward's nChw4c reconstruction, writes
the 8-bit codes a PNG would hold (np.round(float32 x * 255), half-to-even), the next generation's nChw4c input
(code / 255, equal to float32(uint8 / 255.0)) and the per-image sums of this generation.  Codes are one int32 per
pixel, r | g << 8 | b << 16 (below 2^24).  Generation 0 consumes ica_quant8_pack(im): for an image read from an 8-bit
file that is the image itself, for any other tensor (synthetic sources, adversarial examples) its 8-bit rounding, so
the chain is defined the same way for every source.

Differences from the reference (DESIGN.md "Re-compression"):
  * every generation is scored, not only the last; bpp uses RateDistortionLoss's likelihood floor 2^-16 over the
    padded H * W, PSNR the unquantised clamp(x_hat), both as the reference's last-generation numbers do;
  * msim >= 1 gives msim_dB = inf (the reference's math.log10(0) raises);
  * a NaN in x_hat codes to 0 (numpy's float -> uint8 cast of a NaN is undefined);
  * defend=True takes the best variant's x_hat and likelihoods from an eval forward of that variant alone, not
    from its slot in the ensemble's batch of four (the engine's numbers do not depend on the batch).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from . import hip_ops as K
from ._lib import call, lib, ptr, stream

LIK_FLOOR = 1.0 / 65536           # train.py:62
MSSSIM_MIN_SIDE = 160             # pytorch_msssim: min(H, W) > (11 - 1) * 2^4


def validate(im, generations=1, check_every=8):
    """ValueError unless ``im`` is a [B, 3, H, W] contiguous fp32 device tensor with H, W multiples of 64 (as
    coder.read_image pads it) and the counts are positive ints.  Runs before anything is launched."""
    B, H, W = K.check_image(im, "im", dev=False)   # the tensor checks below are ValueErrors, the device check last
    if im.dtype != torch.float32:
        raise ValueError(f"im must be float32, got {im.dtype}")
    if not im.is_contiguous():
        raise ValueError("im must be contiguous")
    if H % 64 or W % 64:
        raise ValueError(f"H x W = {H} x {W} must be multiples of 64 (coder.read_image's padding)")
    K.positive_int("generations", generations)
    K.positive_int("check_every", check_every)
    if not im.is_cuda:
        raise ValueError("im must be a HIP device tensor (no CPU fallback)")
    return B, H, W


def quant8_pack(im):
    """Planar [B, 3, H, W] fp32 -> (codes [B, H, W] int32, nChw4c input [B, 1, H, W, 4] = code / 255)."""
    B, _, H, W = im.shape
    K._dev_check(im, "im")
    q = torch.empty((B, H, W), dtype=torch.int32, device=im.device)
    x4 = K.empty_nc4(B, 3, H, W, im.device)
    call("ica_quant8_pack", ptr(im), B, H, W, ptr(x4), ptr(q), stream())
    return q, x4


def requant8(x_hat4, orig, prev_q, next4=None, q=None, out=None, sse_orig=None, sse_gen=None, changed=None,
             moving=None, ws=None):
    """ica_requant8 (include/ica_hip.h).  Outputs that are not passed are allocated; ``out`` is written only when
    passed.  Returns (next4, q, sse_orig [B], sse_gen [B], changed [B] int64)."""
    K._dev_check(x_hat4, "x_hat4")
    B, _, H, W, _ = x_hat4.shape
    dev = x_hat4.device
    next4 = torch.empty_like(x_hat4) if next4 is None else next4
    q = torch.empty((B, H, W), dtype=torch.int32, device=dev) if q is None else q
    sse_orig = torch.empty(B, device=dev) if sse_orig is None else sse_orig
    sse_gen = torch.empty(B, device=dev) if sse_gen is None else sse_gen
    changed = torch.empty(B, dtype=torch.int64, device=dev) if changed is None else changed
    if ws is None:
        ws = torch.empty(lib().ica_requant8_ws_size(B, H, W), device=dev)
    call("ica_requant8", ptr(x_hat4), ptr(orig), ptr(prev_q), B, H, W, ptr(next4), ptr(q), ptr(out), ptr(sse_orig),
          ptr(sse_gen), ptr(changed), ptr(moving), ptr(ws), stream())
    return next4, q, sse_orig, sse_gen, changed


def floor_bits(lik4, C, floor=LIK_FLOOR, out=None):
    """Per image sum log(max(p, floor)) over the C real channels of an nChw4c likelihood tensor."""
    K._dev_check(lik4, "lik4")
    B, _, H, W, _ = lik4.shape
    out = torch.empty(B, device=lik4.device) if out is None else out
    ws = torch.empty(lib().ica_floor_bits_ws_size(B, C, H, W), device=lik4.device)
    call("ica_floor_bits", ptr(lik4), B, C, H, W, float(floor), ptr(out), ptr(ws), stream())
    return out


def _lik_channels(kern, key, lik4):
    return {"y": getattr(kern, "M", None), "z": getattr(kern, "N", None)}.get(key) or 4 * lik4.shape[1]


def _bits_into(kern, res, rows):
    """rows[k] (a [b] view per likelihood tensor of the forward, in its order) <- the floored log sums."""
    for row, (key, lik4) in zip(rows, res["lik4"].items()):
        floor_bits(lik4, _lik_channels(kern, key, lik4), LIK_FLOOR, row)


def _msim(msssim, x_hat, im):
    """(msim [B], msim_dB [B]) lists, or (None, None) where pytorch_msssim refuses the size."""
    H, W = im.shape[2:]
    if min(H, W) <= MSSSIM_MIN_SIDE:
        return None, None
    if msssim is None:
        from . import msssim
    m = msssim.ms_ssim_per_image(x_hat, im).tolist()
    return m, [-10.0 * math.log10(1.0 - v) if v < 1.0 else math.inf for v in m]


@dataclass
class RecompressResult:
    psnr: torch.Tensor        # [G, B] float64: 10 log10(1 / mean((clamp(x_hat_g) - im)^2))
    bpp: torch.Tensor         # [G, B] float64: sum log(max(p, 2^-16)) / (-ln 2 H W)
    changed: torch.Tensor     # [G, B] int64: code values (of 3 H W) generation g changed
    drift: torch.Tensor       # [G, B] float64: mean(((q_out - q_in) / 255)^2) of generation g
    x_hat: torch.Tensor       # [B, 3, H, W]: clamp(x_hat) of the last generation, unquantised
    codes: torch.Tensor       # [B, H, W] int32: the codes the last generation produced (its PNG)
    msim: list | None         # of the last generation against im; None for min(H, W) <= 160
    msim_dB: list | None
    fixed_at: torch.Tensor    # [B] int64: first generation whose output codes equal its input codes, or -1
    generations_run: int      # forwards actually run (< G after an early stop)
    best_idx: torch.Tensor | None = None   # [G, B] int64 with defend=True
    consumed: torch.Tensor | None = None   # [G, B, H, W] int32 with keep_codes: the codes generation g encoded


def _defended_forward(kern, x4):
    """One defended generation's forward: the self-ensemble picks each image's best dihedral variant, that variant
    is coded on its own, and its reconstruction comes back rotated into the image's frame.  Returns (x_hat4,
    floored log sums [K, B] of the best variants' likelihood tensors, best_idx list)."""
    from . import self_ensemble as SE
    x = K.from_nc4(x4, 3)
    _, best_x, best_idx = SE.self_ensemble(kern, x)
    outs, bits = [], []
    for xv, k in zip(best_x, best_idx):
        res = kern.forward(K.to_nc4(xv.contiguous()))
        bits.append(torch.cat([floor_bits(l4, _lik_channels(kern, key, l4)) for key, l4 in res["lik4"].items()]))
        outs.append(SE.rotates(K.from_nc4(res["x_hat4"], 3), reverse=k).contiguous())
    return K.to_nc4(torch.cat(outs, 0)), torch.stack(bits, 1), best_idx


def recompress(kern, im, generations, *, defend=False, stop_at_fixed_point=True, check_every=8, msssim=None,
               keep_codes=False):
    """``generations`` rounds of eval forward -> 8-bit PNG -> read back, for the batch ``im`` ([B, 3, H, W] device
    fp32, zero-padded as coder.read_image pads it), every round scored against ``im``.

    The loop stays on the device: kern.forward(next4) -> ica_requant8 -> next; the tables are device tensors the
    kernels fill in place.  The engine is deterministic, so an image whose codes a generation leaves unchanged stays
    bit-identical from then on: every ``check_every`` generations one 4-byte counter is read (images whose codes
    still move), and when it is 0 the remaining rows are filled from the last computed one with changed = drift = 0.
    stop_at_fixed_point=False runs every generation; both give the same tables.  defend=True codes each
    generation's best self-ensemble variant (self_ensemble.defend's only reachable method here); it reads the
    ensemble's eight errors on the host every generation, as self_ensemble.self_ensemble does."""
    B, H, W = validate(im, generations, check_every)
    G, dev, n = generations, im.device, 3 * H * W
    sse_o = torch.zeros((G, B), device=dev)
    sse_g = torch.zeros((G, B), device=dev)
    changed = torch.zeros((G, B), dtype=torch.int64, device=dev)
    best = torch.zeros((G, B), dtype=torch.int64) if defend else None
    moving = torch.ones(1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib().ica_requant8_ws_size(B, H, W), device=dev)
    x_hat = torch.empty_like(im)
    codes = torch.empty((G + 1 if keep_codes else 2, B, H, W), dtype=torch.int32, device=dev)
    q0, x4 = quant8_pack(im)
    codes[0].copy_(q0)
    bits = None
    ran = 0
    for g in range(G):
        src, dst = (g, g + 1) if keep_codes else (g & 1, (g + 1) & 1)
        if defend:
            xh4, bits_g, best_g = _defended_forward(kern, x4)
            if bits is None:
                bits = torch.zeros((G,) + tuple(bits_g.shape), device=dev)
            bits[g] = bits_g
            best[g] = torch.tensor(best_g, dtype=torch.int64)
        else:
            res = kern.forward(x4)
            if bits is None:
                bits = torch.zeros((G, len(res["lik4"]), B), device=dev)
            _bits_into(kern, res, list(bits[g]))
            xh4 = res["x_hat4"]
        last = g == G - 1
        x4, *_ = requant8(xh4, im, codes[src], None, codes[dst], x_hat, sse_o[g], sse_g[g], changed[g], moving, ws)
        ran = g + 1
        if stop_at_fixed_point and not last and ran % check_every == 0 and int(moving.item()) == 0:
            break
    if ran < G:   # a fixed point: every later generation repeats generation ran - 1 bit for bit
        sse_o[ran:] = sse_o[ran - 1]
        bits[ran:] = bits[ran - 1]
        if defend:
            best[ran:] = best[ran - 1]
        if keep_codes:
            codes[ran + 1:] = codes[ran]
    final = codes[ran if keep_codes else ran & 1]
    still = changed == 0
    first = torch.where(still.any(0), still.to(torch.int64).argmax(0), torch.full((B,), -1, dtype=torch.int64, device=dev))
    msim, msim_dB = _msim(msssim, x_hat, im)
    return RecompressResult(
        psnr=-10.0 * torch.log10(sse_o.double() / n), bpp=bits.double().sum(1) / (-math.log(2) * H * W),
        changed=changed, drift=sse_g.double() / n, x_hat=x_hat, codes=final.clone(), msim=msim, msim_dB=msim_dB,
        fixed_at=first, generations_run=ran, best_idx=best, consumed=codes[:G] if keep_codes else None)


def rd_metrics(kern, im, msssim=None):
    """RateDistortionLoss(training=False) and PSNR of net.eval()(im), per image (test.py's undefended path): a dict
    of bpp_floor, psnr (lists), msim, msim_dB (lists or None) and x_hat.  ``im`` is coded as it is, not rounded to
    8 bits first."""
    B, H, W = validate(im)
    res = kern.forward(K.to_nc4(im))
    bits = torch.zeros((len(res["lik4"]), B), device=im.device)
    _bits_into(kern, res, list(bits))
    x_hat = torch.empty_like(im)
    q0, _ = quant8_pack(im)
    _, _, sse_o, _, _ = requant8(res["x_hat4"], im, q0, out=x_hat)
    msim, msim_dB = _msim(msssim, x_hat, im)
    return {"bpp_floor": (bits.double().sum(0) / (-math.log(2) * H * W)).tolist(),
            "psnr": (-10.0 * torch.log10(sse_o.double() / (3 * H * W))).tolist(),
            "msim": msim, "msim_dB": msim_dB, "x_hat": x_hat}
