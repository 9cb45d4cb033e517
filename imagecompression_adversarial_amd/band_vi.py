"""Where in the spectrum an adversarial perturbation does its damage, and an attack confined to chosen bands
(DESIGN.md "Band VI"), on the HIP kernels of ica_band.hip.  The reference points at both and builds neither: its
freq_1/2/3 split (attack_rd.py:427-436) and its low-frequency-only perturbation (attack_rd.py:509-510) are commented
out, so the semantics are this project's.

The transform is the orthonormal 8x8 block DCT-II of every channel plane, blocks aligned to the image origin (H and W
multiples of 8).  Coefficient (u, v) belongs to band max(u, v) = 0..7; band k holds 2 k + 1 coefficients, band 0 is
the block mean, bands 0..k are what an ideal (k + 1) / 8 down- and up-sampling keeps.  A band set is an 8-bit mask,
bit k selecting band k, and P_S = IDCT . [band in S] . DCT is an orthogonal projection.

band_index           the 8x8 table of k
preset_masks         only: 1 << k; lowpass: (2 << k) - 1; without: 0xFF ^ (1 << k), k = 0..7
parse_bands          "0-2,5" -> mask
project              P_S x
split_bands          n = im_adv - im_s: the band energies and, per mask, clamp(im_s + P_S n, 0, 1) with its mse_in
band_study           split_bands, one eval forward over the V B variant images, mse_out / bpp / VI per (variant, image)
BandAttackLoop       the L2 distortion attack with the perturbation p = P_S(clip(noise)) (band_attack_batch runs it)
band_guard           what the band-limited attack does not cover, each with its reason

Two consequences of the attack's definition: the +-eps clip bounds the parameter ``noise``, not p, so a pixel of p may
exceed eps; and ``noise`` itself is not band-limited, p is.  AttackResult.noise stays the parameter: the perturbation
to report is im_adv - im_s.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from .attack import AttackLoop, AttackResult, evaluate
from .transfer import pair_chunks, score_pairs, vi_db

NB = 8                                   # bands
FULL = 0xFF
PRESETS = ("only", "lowpass", "without")


def band_index():
    """The 8x8 table k[u][v] = max(u, v)."""
    u = torch.arange(NB)
    return torch.maximum(u[:, None], u[None, :])


def preset_masks(name):
    if name == "only":
        return [1 << k for k in range(NB)]
    if name == "lowpass":
        return [(2 << k) - 1 for k in range(NB)]
    if name == "without":
        return [FULL ^ (1 << k) for k in range(NB)]
    raise ValueError(f"preset {name!r}: one of {PRESETS}")


def parse_bands(spec):
    """"0-2,5" -> 0b100111.  Items are bands k or inclusive ranges a-b with 0 <= a <= b <= 7."""
    if isinstance(spec, int) and not isinstance(spec, bool):
        return check_mask(spec)
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError(f"bands {spec!r}: a list such as '0-2,5'")
    mask = 0
    for item in spec.split(","):
        ends = item.strip().split("-")
        try:
            lo, hi = (int(ends[0]), int(ends[-1])) if len(ends) in (1, 2) else (None, None)
        except ValueError:
            lo = hi = None
        if lo is None or not 0 <= lo <= hi < NB:
            raise ValueError(f"bands {spec!r}: {item.strip()!r} is not a band 0..7 or a range a-b of them")
        for k in range(lo, hi + 1):
            mask |= 1 << k
    return mask


def check_mask(mask):
    if not isinstance(mask, int) or isinstance(mask, bool) or not 0 <= mask <= FULL:
        raise ValueError(f"band mask {mask!r}: an int 0..255, bit k selecting band k")
    return mask


def mask_label(mask):
    return ",".join(str(k) for k in range(NB) if mask >> k & 1) or "-"


def _masks(masks):
    if isinstance(masks, str):
        return preset_masks(masks)
    out = [check_mask(m) for m in masks]
    if not out:
        raise ValueError("at least one band mask")
    return out


def check_shape(H, W):
    if H < 8 or W < 8 or H % 8 or W % 8:
        raise ValueError(f"{H}x{W}: the band transform takes images whose height and width are multiples of 8")


def _pair(im_s, im_adv):
    from . import hip_ops as K
    K.check_image(im_s, "im_s", dev=False)
    K.check_image(im_adv, "im_adv", dev=False)
    if im_adv.shape != im_s.shape:
        raise ValueError(f"im_adv {tuple(im_adv.shape)} and im_s {tuple(im_s.shape)} differ in shape")
    check_shape(im_s.shape[2], im_s.shape[3])
    K.check_image(im_adv, "im_adv")
    return K.check_image(im_s, "im_s")


def project(x, mask):
    """P_mask x for a planar [B, 3, H, W] batch; mask 0 gives exact zeros."""
    from . import hip_ops as K
    from ._lib import call, ptr, stream
    check_mask(mask)
    K.check_image(x, "x", dev=False)
    check_shape(x.shape[2], x.shape[3])
    B, H, W = K.check_image(x, "x")
    y = torch.empty_like(x)
    call("ica_band_project", ptr(x), mask, B, H, W, ptr(y), stream())
    return y


def split_bands(im_s, im_adv, masks=None, mse=True):
    """n = im_adv - im_s.  -> (x, energy, mse_in): energy [B, 8] = |P_{k} n|^2 / (3 H W) (the eight sum to mean(n^2));
    with ``masks`` (a preset name or a list of V masks) x [V B, 3, H, W], variant v of image b at v B + b, =
    clamp(im_s + P_S n, 0, 1) and mse_in [V, B] = mean((x - im_s)^2) (None with mse=False); without, x and mse_in are
    None."""
    from ._lib import call, lib, ptr, stream
    B, H, W = _pair(im_s, im_adv)
    dev = im_s.device
    ms = _masks(masks) if masks is not None else None
    V = len(ms) if ms else 1
    if V > lib().ica_band_max_variants():
        raise ValueError(f"{V} variants: at most {lib().ica_band_max_variants()} per call")
    n_ws = lib().ica_band_split_ws_size(V, B, H, W)
    if n_ws == 0:
        raise ValueError(f"{B} images of {H}x{W} exceed the kernel's grid")
    energy = torch.empty((B, NB), dtype=torch.float32, device=dev)
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
    x = mse_in = marr = None
    if ms:
        x = torch.empty((V * B, 3, H, W), dtype=torch.float32, device=dev)
        mse_in = torch.empty((V, B), dtype=torch.float32, device=dev) if mse else None
        marr = (C.c_int * V)(*ms)
    call("ica_band_split", ptr(im_s), ptr(im_adv), marr, V, B, H, W, ptr(x), ptr(energy), ptr(mse_in), ptr(ws),
         stream())
    return x, energy, mse_in


@dataclass
class BandStudy:
    masks: list              # the V masks
    energy: torch.Tensor     # [B, 8] band energies of im_adv - im_s
    mse_in: torch.Tensor     # [V, B] mean((x - im_s)^2) of the clamped variant image
    mse_out: torch.Tensor    # [V, B] mean((x_hat(x) - x_hat(im_s))^2)
    bpp: torch.Tensor        # [V, B]
    bpp_ori: torch.Tensor    # [B]
    vi: list                 # [V][B] Python floats: 10 log10(mse_out / mse_in), NaN under the 1e-20 guard


def band_study(kern, im_s, im_adv, masks="only", batch=32, clamp=True):
    """Which band of im_adv - im_s carries the VI: per mask the variant image clamp(im_s + P_S n, 0, 1) is coded and
    scored against the clean reconstruction, which is coded once.  The V B variant images go through the eval forward
    at most ``batch`` at a time."""
    from . import hip_ops as K
    ms = _masks(masks)
    x, energy, mse_in = split_bands(im_s, im_adv, ms)
    B, _, H, W = im_s.shape
    V = len(ms)
    dev = im_s.device
    xv = x.view(V, B, 3, H, W)
    mse_out = torch.empty((V, B), dtype=torch.float32, device=dev)
    bpp = torch.empty((V, B), dtype=torch.float32, device=dev)
    bpp_ori = torch.empty(B, dtype=torch.float32, device=dev)
    run, x_s4 = None, None
    for (v0, v1), (b0, b1) in pair_chunks(V, B, batch):
        if run != (b0, b1):
            run = (b0, b1)
            res = kern.forward(K.to_nc4(im_s[b0:b1]))
            x_s4 = res["x_hat4"]
            bpp_ori[b0:b1] = K.bits_to_bpp(res["sumlog"], H * W)
        n, m = v1 - v0, b1 - b0
        res = kern.forward(K.to_nc4(xv[v0:v1, b0:b1].reshape(n * m, 3, H, W)))
        mse_out[v0:v1, b0:b1] = score_pairs(res["x_hat4"], x_s4, n, m, clamp)
        bpp[v0:v1, b0:b1] = K.bits_to_bpp(res["sumlog"], H * W).view(n, m)
    mi_l, mo_l = torch.stack([mse_in, mse_out]).tolist()      # the one host read
    vi = [[vi_db(mi_l[v][b], mo_l[v][b]) for b in range(B)] for v in range(V)]
    return BandStudy(masks=ms, energy=energy, mse_in=mse_in, mse_out=mse_out, bpp=bpp, bpp_ori=bpp_ori, vi=vi)


def band_guard(model=None, att_metric="L2", rate=False, target=None, roi=None, coupled=False, pad=None, defend=False):
    """What the band-limited attack does not cover, each with its reason (NotImplementedError).  Shared by
    BandAttackLoop and the attack_band CLI, which checks before it loads a model."""
    if rate:
        raise NotImplementedError("the band-limited attack is the distortion attack: -r (the bitrate objective) has "
                                  "its own loop and no projected form is stated")
    if target is not None or roi is not None:
        raise NotImplementedError("the band-limited attack has no target / ROI form (-t as a target, --mask_loc): "
                                  "a box-weighted budget and a block transform do not commute")
    if coupled:
        raise NotImplementedError("the band-limited attack is per-image: the batch-coupled semantics belong to the "
                                  "adversarial fine-tune's attack")
    if pad:
        raise NotImplementedError("the band-limited attack does not take -p: the blocks are aligned to the image "
                                  "origin, which a padded pre-eval would move")
    if defend:
        raise NotImplementedError("the band-limited attack does not run through --defend: the defended loops have "
                                  "their own network step")
    if att_metric != "L2":
        raise NotImplementedError(f"the band-limited attack's budget and cheap branch are the L2 ones (att_metric "
                                  f"{att_metric!r})")
    if model == "debug":
        raise NotImplementedError("the band-limited attack covers the clamped-input models: -m debug attacks an "
                                  "unclamped input")


class BandAttackLoop(AttackLoop):
    """attack_rd.attack_ with the perturbation confined to the bands ``bands`` (a mask or a list such as "0-2,5"):

        nc = Up(Low(noise, -eps), eps);  p = P_S(nc);  im_in = Up(Low(im_s + p, 0), 1);  loss_i = mean((im_s - im_in)^2)

    and in the backward g = P_S(bound-bwd at im_s + p) before the bound-bwd at the noise (the projection is
    symmetric).  The branch rule, Adam, the LR table, the census and the branch compaction are the base class's, and
    so is network_grad: the whole-batch step is replayed as a graph as there."""

    def __init__(self, kern, im_s, bands, steps=1001, epsilon=16.0, noise_thr=1e-4, lr=0.01, att_metric="L2",
                 clamp=True, init_noise=None, coupled=False, group=None, target=None, roi=None, pad=None):
        band_guard(getattr(kern, "model", None), att_metric, False, target, roi, coupled, pad)
        if not getattr(kern, "clamp_input", True):
            band_guard("debug")
        self.mask = parse_bands(bands)
        check_shape(im_s.shape[2], im_s.shape[3])
        super().__init__(kern, im_s, steps, epsilon, noise_thr, lr, "L2", clamp, init_noise)
        from ._lib import lib
        self.band_ws = torch.empty(lib().ica_band_prologue_ws_size(self.B, self.H, self.W), device=im_s.device)

    def step(self, i, record_im_in=False, census=False):
        from ._lib import call, ptr, stream
        B, H, W = self.B, self.H, self.W
        call("ica_band_prologue", ptr(self.noise), ptr(self.im_s), ptr(self.im_in4), ptr(self.loss_i), B, H, W,
             self.eps, self.mask, ptr(self.band_ws), stream())
        E, idx = self._select()
        if E == B and idx is None and self.graph_ok:
            gx4 = self._network_graph()
        else:
            gx4 = self.network_grad(idx, E) if E > 0 else None
        bc2s, neg_step = self._adam_scalars(i)
        call("ica_band_adam", ptr(self.noise), ptr(self.im_s), ptr(gx4), ptr(self.loss_i), ptr(self.m), ptr(self.v),
             ptr(self.im_in if record_im_in else None), B, H, W, self.eps, self.thr, self.gscale, bc2s, neg_step,
             ptr(self.branch), ptr(self.gpos if idx is not None else None), ptr(self.census), self.mask, stream())
        self.steps_done += 1
        if census:
            return self.branch.tolist()
        return None


def band_attack_batch(kern, im_s, bands, steps=1001, epsilon=16.0, noise_thr=1e-4, lr=0.01, clamp=True,
                      init_noise=None, eval_msssim=True, record=False) -> AttackResult:
    """attack_batch with the band-limited perturbation (BandAttackLoop)."""
    loop = BandAttackLoop(kern, im_s, bands, steps, epsilon, noise_thr, lr, "L2", clamp, init_noise)
    branches = loop.run(record=record)
    im_, out, bpp, mse_in, mse_out, msim_in, msim_out, vi, vi_msim = evaluate(
        kern, loop.im_in, loop.im_s, loop.output_s, clamp, adv=False, msssim=eval_msssim)
    return AttackResult(im_adv=im_, output_adv=out, output_s=loop.output_s, bpp_ori=loop.bpp_ori, bpp=bpp,
                        mse_in=mse_in, mse_out=mse_out, msim_in=msim_in, msim_out=msim_out, vi=vi, vi_msim=vi_msim,
                        noise=loop.noise, branches=branches)
