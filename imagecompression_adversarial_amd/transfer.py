"""What a perturbation is worth outside the run that made it (transfer_noise.py) on the HIP kernels
(ica_transfer.hip): the N x M study "noise i added to image j" as a batched job with the matrix left on the device.

apply_pairs          transfer_noise.py:88-89 for a block of pairs: clamp(im[j] + noise[i], 0, 1), mean((im_in - im)^2)
score_pairs          transfer_noise.py:96, :133: mean((clamp(x_hat(im_in)) - clamp(x_hat(im)))^2), from nChw4c
pair_chunks          the (noise range, target range) blocks whose forwards see at most ``batch`` images
vi_db                10 log10(mse_out / mse_in) in double; NaN under the guard attack.evaluate uses
transfer_matrix      test + the pair loop (transfer_noise.py:83-96, :130-135) for N noises and M images of one size
size_blocks          the sub-matrices of equal padded size (pairs of different sizes stay NaN)
cross_model_matrix   test_transferability_multiple_models (transfer_noise.py:45-79)

Pairs are ordered i * M + j (noise-major, target-minor), the order transfer_noise.py:134 prints them in.  The clean
forward of a target happens once per call, not once per pair as in the reference (:87): M + N M images go through
the codec instead of 2 N M, and the host reads the two [n][m] blocks once per chunk.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from . import hip_ops as K
from ._lib import call, lib, ptr, stream

GUARD = 1e-20          # attack.evaluate: a ratio is formed only where both means exceed it


def apply_pairs(im, noise):
    """im [M, 3, H, W], noise [N, 3, H, W] -> (im_in [N M, 3, H, W] with pair (i, j) at i M + j,
    mse_in [N, M] = mean((im_in - im[j])^2))."""
    M, H, W = K.check_image(im, "im")
    N, Hn, Wn = K.check_image(noise, "noise")
    if (Hn, Wn) != (H, W):
        raise ValueError(f"noise {tuple(noise.shape)} and im {tuple(im.shape)} differ in size")
    if W % 4:
        raise ValueError(f"W = {W} must be a multiple of 4 (16-byte row loads)")
    n_ws = lib().ica_transfer_apply_ws_size(N, M, H, W)
    if n_ws == 0:
        raise ValueError(f"{N} x {M} pairs of {H}x{W} images exceed the kernel's grid")
    im_in = torch.empty((N * M, 3, H, W), dtype=torch.float32, device=im.device)
    mse_in = torch.empty((N, M), dtype=torch.float32, device=im.device)
    ws = torch.empty(n_ws, dtype=torch.float32, device=im.device)
    call("ica_transfer_apply", ptr(im), ptr(noise), ptr(im_in), N, M, H, W, ptr(mse_in), ptr(ws), stream())
    return im_in, mse_in


def score_pairs(x_hat4, x_s4, N, M, clamp=True):
    """x_hat4 [N M, 1, H, W, 4] (the decoder's output of the pair batch), x_s4 [M, 1, H, W, 4] (of the clean
    targets) -> mse_out [N, M] over the 3 real channels, both operands clamped to [0, 1] if ``clamp``."""
    K.positive_int("N", N)
    K.positive_int("M", M)
    B, H, W = K.check_nc4(x_hat4, "x_hat4")
    Ms, Hs, Ws = K.check_nc4(x_s4, "x_s4")
    if Ms != M or B != N * M:
        raise ValueError(f"x_hat4 holds {B} and x_s4 {Ms} images, not {N} x {M} pairs and {M} targets")
    if (Hs, Ws) != (H, W):
        raise ValueError(f"x_hat4 {tuple(x_hat4.shape)} and x_s4 {tuple(x_s4.shape)} differ in size")
    n_ws = lib().ica_transfer_score_ws_size(N, M, H, W)
    if n_ws == 0:
        raise ValueError(f"{N} x {M} pairs of {H}x{W} images exceed the kernel's grid")
    mse_out = torch.empty((N, M), dtype=torch.float32, device=x_hat4.device)
    ws = torch.empty(n_ws, dtype=torch.float32, device=x_hat4.device)
    call("ica_transfer_score", ptr(x_hat4), ptr(x_s4), N, M, H, W, int(bool(clamp)), ptr(mse_out), ptr(ws), stream())
    return mse_out


def pair_chunks(N, M, batch):
    """[((i0, i1), (j0, j1))]: targets in runs of at most ``batch``; per run max(1, batch // run) noises at a time.
    Every pair lies in exactly one block and no block holds more than ``batch`` pairs."""
    for name, v in (("N", N), ("M", M), ("batch", batch)):
        K.positive_int(name, v)
    out = []
    for j0 in range(0, M, batch):
        j1 = min(j0 + batch, M)
        step = max(1, batch // (j1 - j0))
        out += [((i0, min(i0 + step, N)), (j0, j1)) for i0 in range(0, N, step)]
    return out


def vi_db(mse_in, mse_out):
    """10 log10(mse_out / mse_in) of two Python floats, in double; NaN unless both exceed 1e-20."""
    if mse_in > GUARD and mse_out > GUARD:
        return 10.0 * math.log10(mse_out / mse_in)
    return float("nan")


@dataclass
class TransferResult:
    vi: list                 # [N][M] Python floats: 10 log10(mse_out / mse_in), NaN under the 1e-20 guard
    mse_in: torch.Tensor     # [N, M] mean((im_in - im)^2)
    mse_out: torch.Tensor    # [N, M] mean((x_hat(im_in) - x_hat(im))^2), clamped if ``clamp``


def transfer_matrix(kern, noises, images, batch=32, clamp=True):
    """Noise i on image j for noises [N, 3, H, W] and images [M, 3, H, W] of one padded size.  Each run of targets is
    coded clean once and its x_hat4 kept for every noise chunk; a chunk is one apply_pairs, one forward of at most
    ``batch`` images, one score_pairs and one host read."""
    M, H, W = K.check_image(images, "images")
    N, Hn, Wn = K.check_image(noises, "noises")
    if (Hn, Wn) != (H, W):
        raise ValueError(f"noises {tuple(noises.shape)} and images {tuple(images.shape)} differ in size")
    chunks = pair_chunks(N, M, batch)
    dev = images.device
    mse_in = torch.empty((N, M), dtype=torch.float32, device=dev)
    mse_out = torch.empty((N, M), dtype=torch.float32, device=dev)
    vi = [[float("nan")] * M for _ in range(N)]
    run, im_run, x_s4 = None, None, None
    for (i0, i1), (j0, j1) in chunks:
        if run != (j0, j1):
            run, im_run = (j0, j1), images[j0:j1]
            x_s4 = kern.forward(K.to_nc4(im_run))["x_hat4"]
        n, m = i1 - i0, j1 - j0
        im_in, mi = apply_pairs(im_run, noises[i0:i1])
        mo = score_pairs(kern.forward(K.to_nc4(im_in))["x_hat4"], x_s4, n, m, clamp)
        mse_in[i0:i1, j0:j1] = mi
        mse_out[i0:i1, j0:j1] = mo
        mi_l, mo_l = torch.stack([mi, mo]).tolist()      # the one host read of the chunk
        for a in range(n):
            for b in range(m):
                vi[i0 + a][j0 + b] = vi_db(mi_l[a][b], mo_l[a][b])
    return TransferResult(vi=vi, mse_in=mse_in, mse_out=mse_out)


def size_blocks(src_sizes, dst_sizes):
    """([(rows, cols)], mismatched): per padded size found on both sides the source rows and target columns that
    have it (each in order), and the number of (source, target) pairs whose sizes differ."""
    blocks = []
    for size in dict.fromkeys(src_sizes):
        rows = [i for i, s in enumerate(src_sizes) if s == size]
        cols = [j for j, s in enumerate(dst_sizes) if s == size]
        if cols:
            blocks.append((rows, cols))
    matched = sum(len(r) * len(c) for r, c in blocks)
    return blocks, len(src_sizes) * len(dst_sizes) - matched


def assemble(N, M, blocks, parts):
    """The [N][M] list of Python floats with parts[k], the [len(rows)][len(cols)] list of blocks[k], put at its rows
    and columns; NaN where no block put a value."""
    full = [[float("nan")] * M for _ in range(N)]
    for (rows, cols), part in zip(blocks, parts):
        for a, i in enumerate(rows):
            for b, j in enumerate(cols):
                full[i][j] = part[a][b]
    return full


def cross_model_matrix(kerns, attack_fn, images, batch=32):
    """test_transferability_multiple_models: entry [a][b] is the mean over the images of 10 log10(mse_out / mse_in)
    for adversarial examples made on model a (``attack_fn(kerns[a], im_s) -> im_adv``, once per source model) and
    coded by model b.  ``images``: a [B, 3, H, W] batch or a list of such batches (one per padded size).  A pair
    under the 1e-20 guard is NaN and makes its entry NaN."""
    groups = [images] if torch.is_tensor(images) else list(images)
    chunks = []
    for g in groups:
        B, _, _ = K.check_image(g, "images")
        chunks += [g[b0:b0 + batch] for b0 in range(0, B, batch)]
    nk = len(kerns)
    adv = [[attack_fn(kern, im_s).contiguous() for im_s in chunks] for kern in kerns]
    mse_in = [[K.sqdiff_mean(im_s, im_adv) for im_s, im_adv in zip(chunks, row)] for row in adv]
    out = [[0.0] * nk for _ in range(nk)]
    for b, kern in enumerate(kerns):
        clean = [kern.forward(K.to_nc4(im_s))["x_hat4"] for im_s in chunks]
        for a in range(nk):
            vals = []
            for c, im_adv in enumerate(adv[a]):
                mo = score_pairs(kern.forward(K.to_nc4(im_adv))["x_hat4"], clean[c], 1, im_adv.shape[0])
                mi_l, mo_l = torch.stack([mse_in[a][c], mo[0]]).tolist()
                vals += [vi_db(mi, mo_) for mi, mo_ in zip(mi_l, mo_l)]
            out[a][b] = sum(vals) / len(vals)
    return out
