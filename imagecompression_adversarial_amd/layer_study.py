"""The layer-wise error-propagation study (layer_store / layer_compare, anchors/utils.py:132-166) on the HIP engine:
where in the codec does an adversarial perturbation grow -- in the analysis transform, at the quantiser, or in the
synthesis transform?

encoder_rows   mean((enc_a[k] - enc_c[k])^2) for the image and every g_a module output (:157-159, without the
               reference's printed factor 0.5)
quant_rows     sqrt(mean((y_a - round(y_c))^2)), sqrt(mean((round(y_a) - round(y_c))^2))   (:160-162, in print order)
decoder_rows   per g_s module sqrt(mean((dec_a - dec_round_c)^2)), sqrt(mean((dec_round_a - dec_round_c)^2))   (:164-166)
layer_compare  the three composed

Every number is per image.  The encoder is ONE g_a forward of the 2B batch [adv; clean] and the decoder ONE g_s
forward of the 3B batch [y_a; round(y_a); round(y_c)] (the reference's dec of the clean image is never read and not
computed); the halves / thirds of every module output go to the reduction as contiguous views, all layers of a side
in one launch (hip_ops.layer_sums, ica_layers.hip).  Launches of the study: 3 reductions (encoder, quant, decoder),
each followed by ica_reduce_rows.

Module granularity: bmshj2018 (factorized / hyper / context) conv, GDN, conv, GDN, conv, GDN, conv on either side (8
encoder rows, 7 decoder rows); cheng2020 the top-level modules of g_a (6 blocks and a conv: 8 rows) and of g_s (7
blocks and the sub-pixel conv: 8 rows).

The engine fuses GDN / IGDN into the conv epilogues and keeps only their outputs, so the conv outputs before the
normalisation are produced by running each of those three convs once more with the bias epilogue, on the same input
and in the same storage layout (3 extra launches a side; the study is one forward, not a step loop).  They are not
reconstructed from the GDN output and its saved s.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import hip_ops as K
from ._lib import call, ptr, stream
from .engine import _lay, _levels

DEBUG_REASON = ("the layer study walks the seven modules of g_a and g_s; the debug model has two, and a path of its "
                "own is not worth having")


@dataclass
class Act:
    """One module output of a batched forward: the tensor, its channels and whether it is stored parity-split."""
    t: torch.Tensor
    C: int
    split: bool = False


@dataclass
class LayerCompare:
    enc_mse: torch.Tensor      # fp32 [B][8]: the image, then every g_a module
    quant_rmse: torch.Tensor   # fp32 [B][2]: (unrounded adv, rounded adv) against the rounded clean latent
    dec_rmse: torch.Tensor     # fp32 [B][rows][2]: the same two columns after every g_s module
    mse_in: torch.Tensor       # fp32 [B]: enc_mse[:, 0]
    enc_shapes: list           # (C, H, W) of every encoder row
    dec_shapes: list           # (C, H, W) of every decoder row
    y_adv4: torch.Tensor = None
    y_clean4: torch.Tensor = None


def check_kern(kern):
    """The engines the study runs on: CodecKernels / ChengKernels with fp32 or x6 operands."""
    model = getattr(kern, "model", None)
    if model == "debug" or not hasattr(kern, "ga") or not hasattr(kern, "gs"):
        raise NotImplementedError(DEBUG_REASON)
    if _is_cheng(kern):
        if kern.ga.blocks[0][1].p6 == K.PREC_B1:
            raise NotImplementedError("the layer study compares fp32 activations: --precision bf16 is not built")
    elif kern.precision == "bf16":
        raise NotImplementedError("the layer study compares fp32 activations: --precision bf16 is not built")


def _is_cheng(kern):
    return getattr(kern, "model", None) == "cheng2020"


def _bias_pack(ga, i):
    """The pack of conv i's bias-epilogue launch: the forward's own, except for the 6-tile packs of the C = 192 GDN
    layers (q6-8), whose conv_down kernels exist for the GDN epilogue only; those are packed once more at the
    library's default tiling, in the forward pack's precision, and kept with the transform."""
    p = ga.convs[i]
    if p.fwd.it != 6:
        return p.fwd
    cache = ga.__dict__.setdefault("_study_packs", {})
    if i not in cache:
        w = ga.weights[i]
        Co, Ci, KK = w.shape[0], w.shape[1], w.shape[-1] ** 2
        cache[i] = K._pack_down(w, Co, Ci, 5, 2, Ci * KK, KK, 0, p.fwd.prec)
    return cache[i]


def _analysis_acts(ga, x4):
    """[x, conv0, gdn1, conv2, gdn3, conv4, gdn5, y] of engine.Analysis: its forward's launches and layouts, plus the
    three bias-epilogue reruns."""
    H, W = x4.shape[2], x4.shape[3]
    lv = _levels(ga.split)
    lv = tuple(f and ((H + (1 << k) - 1) >> k) % 2 == 0 and ((W + (1 << k) - 1) >> k) % 2 == 0
               for k, f in enumerate(lv))
    acts, h, C = [Act(x4, 3)], x4, 3
    for i in range(3):
        p, lay = ga.convs[i], _lay(lv, i, i + 1)
        pre, _, _ = K.conv_down(h, C, _bias_pack(ga, i), p.bias, ga.N, 5, 2, K.EPI_BIAS,
                                tag=f"{ga.tag}.{2 * i}.study", layout=lay)
        h, _, _ = K.conv_down(h, C, p.fwd, p.bias, ga.N, 5, 2, K.EPI_GDN, ga.gdns[i], tag=f"{ga.tag}.{2 * i}.fwd",
                              layout=lay)
        acts += [Act(pre, ga.N, lv[i + 1]), Act(h, ga.N, lv[i + 1])]
        C = ga.N
    p = ga.convs[3]
    y, _, _ = K.conv_down(h, ga.N, p.fwd, p.bias, ga.M, 5, 2, K.EPI_BIAS, tag=f"{ga.tag}.6.fwd", layout=_lay(lv, 3, 4))
    return acts + [Act(y, ga.M)]


def _synthesis_acts(gs, y4):
    """[deconv0, igdn1, deconv2, igdn3, deconv4, igdn5, x_hat] of engine.Synthesis, as _analysis_acts."""
    lv = _levels(gs.split)
    acts, h, C = [], y4, gs.M
    for i in range(3):
        p, lay = gs.convs[i], _lay(lv, 4 - i, 3 - i)
        pre, _, _ = K.conv_up(h, C, p.fwd, p.bias, gs.N, K.EPI_BIAS, tag=f"{gs.tag}.{2 * i}.study", layout=lay)
        h, _, _ = K.conv_up(h, C, p.fwd, p.bias, gs.N, K.EPI_IGDN, gs.gdns[i], tag=f"{gs.tag}.{2 * i}.fwd", layout=lay)
        acts += [Act(pre, gs.N, lv[3 - i]), Act(h, gs.N, lv[3 - i])]
        C = gs.N
    p = gs.convs[3]
    xh, _, _ = K.conv_up(h, gs.N, p.fwd, p.bias, 3, K.EPI_BIAS, tag=f"{gs.tag}.6.fwd", layout=_lay(lv, 1, 0))
    return acts + [Act(xh, 3)]


def _cheng_acts(tr, x4, C_in, C_out):
    """Input and every top-level module output of ChengAnalysis / ChengSynthesis (its forward collects them)."""
    inputs = []
    out, _ = tr.forward(x4, inputs=inputs)
    return [Act(inputs[0], C_in)] + [Act(t, tr.N) for t in inputs[1:]] + [Act(out, C_out)]


def _parts(act, n, B):
    """The n contiguous B-image views of a module output of an n * B batch."""
    if act.t.shape[0] != n * B:
        raise ValueError(f"a module output holds {act.t.shape[0]} images, not {n} x {B}")
    return [act.t[k * B:(k + 1) * B] for k in range(n)]


def _counts(acts, dev):
    return torch.tensor([a.C * a.t.shape[2] * a.t.shape[3] for a in acts], dtype=torch.float32, device=dev)


def _shapes(acts):
    return [(a.C, a.t.shape[2], a.t.shape[3]) for a in acts]


def _check_images(im_adv, im_clean):
    B, H, W = K.check_image(im_adv, "im_adv")
    if K.check_image(im_clean, "im_clean") != (B, H, W) or im_clean.device != im_adv.device:
        raise ValueError(f"im_adv {tuple(im_adv.shape)} and im_clean {tuple(im_clean.shape)} must have one shape "
                         f"and device")
    if H % 64 or W % 64:
        raise ValueError(f"image sides must be multiples of 64 (as the attack pads them), not {H} x {W}")
    return B


def _encoder(kern, im_adv, im_clean):
    check_kern(kern)
    B = _check_images(im_adv, im_clean)
    x4 = K.to_nc4(torch.cat((im_adv, im_clean), 0))
    acts = _cheng_acts(kern.ga, x4, 3, kern.M) if _is_cheng(kern) else _analysis_acts(kern.ga, x4)
    layers = []
    for a in acts:
        adv, clean = _parts(a, 2, B)   # both halves of one launch: one storage layout (a.split) by construction
        layers.append((K.LAYER_PAIR, a.C, adv, clean))
    sums = K.layer_sums(layers, B)                                        # [rows][B][2]
    mse = (sums[:, :, 0] / _counts(acts, sums.device)[:, None]).t().contiguous()
    y_adv4, y_clean4 = _parts(acts[-1], 2, B)
    return mse, y_adv4, y_clean4, _shapes(acts)


def encoder_rows(kern, im_adv, im_clean):
    """(mse [B, 8], y_adv4, y_clean4): mean((enc_a[k] - enc_c[k])^2) per image for the image (row 0) and every g_a
    module output, from one g_a forward of the 2B batch; the unrounded latents are views of its output."""
    return _encoder(kern, im_adv, im_clean)[:3]


def _latent_check(y_adv4, y_clean4, M):
    K.positive_int("M", M)
    for t, nm in ((y_adv4, "y_adv4"), (y_clean4, "y_clean4")):
        K._check_latent(t, M, nm)
    if y_adv4.shape != y_clean4.shape or y_adv4.device != y_clean4.device:
        raise ValueError(f"y_adv4 {tuple(y_adv4.shape)} and y_clean4 {tuple(y_clean4.shape)} must have one shape and "
                         f"device")
    return y_adv4.shape[0]


def quant_rows(y_adv4, y_clean4, M):
    """rmse [B, 2] = sqrt(mean((y_a - round(y_c))^2)), sqrt(mean((round(y_a) - round(y_c))^2)): what the rounding
    leaves of the latent error.  Nothing rounded is stored."""
    B = _latent_check(y_adv4, y_clean4, M)
    sums = K.layer_sums([(K.LAYER_QUANT, M, y_adv4, y_clean4)], B)[0]    # [B][2]
    return torch.sqrt(sums / float(M * y_adv4.shape[2] * y_adv4.shape[3]))


def _decoder(kern, y_adv4, y_clean4):
    check_kern(kern)
    B = _latent_check(y_adv4, y_clean4, kern.M)
    y3 = torch.empty((3 * B,) + tuple(y_adv4.shape[1:]), dtype=torch.float32, device=y_adv4.device)
    y3[:B].copy_(y_adv4)
    n = y_adv4.numel()
    call("ica_round", ptr(y_adv4), ptr(y3[B:2 * B]), n, stream())         # eval_forward's rounding (ica_round)
    call("ica_round", ptr(y_clean4), ptr(y3[2 * B:]), n, stream())
    acts = _cheng_acts(kern.gs, y3, kern.M, 3)[1:] if _is_cheng(kern) else _synthesis_acts(kern.gs, y3)
    layers = []
    for a in acts:
        adv, adv_r, clean_r = _parts(a, 3, B)   # thirds of one launch: one storage layout
        layers.append((K.LAYER_TRIPLE, a.C, adv, adv_r, clean_r))
    sums = K.layer_sums(layers, B)                                        # [rows][B][2]
    rmse = torch.sqrt(sums / _counts(acts, sums.device)[:, None, None])
    return rmse.permute(1, 0, 2).contiguous(), _shapes(acts)


def decoder_rows(kern, y_adv4, y_clean4):
    """rmse [B, rows, 2] after every g_s module: the unrounded and the rounded adversarial latent against the rounded
    clean one, from one g_s forward of the 3B batch [y_a; round(y_a); round(y_c)].  rows = 7 (bmshj2018) or 8
    (cheng2020)."""
    return _decoder(kern, y_adv4, y_clean4)[0]


def layer_compare(kern, im_adv, im_clean):
    """layer_compare (anchors/utils.py:152-166) per image of a batch: encoder_rows, then quant_rows and decoder_rows
    on the latents it returned."""
    mse, y_adv4, y_clean4, enc_shapes = _encoder(kern, im_adv, im_clean)
    quant = quant_rows(y_adv4, y_clean4, kern.M)
    dec, dec_shapes = _decoder(kern, y_adv4, y_clean4)
    return LayerCompare(mse, quant, dec, mse[:, 0].clone(), enc_shapes, dec_shapes, y_adv4, y_clean4)
