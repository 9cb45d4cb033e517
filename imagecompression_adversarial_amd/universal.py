"""The universal perturbation: ONE additive noise [1, 3, H, W] that breaks the codec on a whole set of images (the
image-agnostic perturbation transfer_noise measures per-image noises against), on the HIP kernels of ica_universal.hip.

The reference has no such experiment; its semantics need no new definition (DESIGN.md §8 "Universal perturbation"):
it is attack_rd.attack_ (attack_rd.py:381-575) with a noise that broadcasts over the batch.  im_s + noise_c broadcasts,
the branch and the losses are the batch means of train.py:342 (``AttackLoop(coupled=True)``), and the input gradient
is summed over the batch where the noise was broadcast, in front of the noise bounds' backward and torch.optim.Adam.

UniversalAttackLoop   the coupled step loop with the shared noise (prologue and update of ica_universal.hip; the
                      network step, its HIP graph and the speculation are AttackLoop's)
universal_batch       the fit and attack.evaluate's per-image post-eval -> AttackResult (noise: [1, 3, H, W])
heldout               the noise on images it was not fitted on (transfer.transfer_matrix with N = 1)
"""
from __future__ import annotations

import torch

from . import dist as D
from . import hip_ops as K
from . import transfer
from ._lib import call, ptr, stream
from .attack import AttackLoop, AttackResult, evaluate


def universal_guard(att_metric="L2", target=None, roi=None, group=None, clamp_input=True):
    """What the universal perturbation does not cover, each with its reason.  Shared by UniversalAttackLoop and the
    universal_noise CLI, which checks before it loads a model."""
    if att_metric != "L2":
        raise NotImplementedError(f"the universal perturbation is fitted on the L2 losses (att_metric {att_metric!r}): "
                                  "the ms-ssim cheap branch has no gradient summed over the batch here")
    if target is not None or roi is not None:
        raise NotImplementedError("the universal perturbation has no target / ROI form: one noise for every image of "
                                  "the set, scored on the whole image")
    if group is not None:
        raise NotImplementedError("the universal perturbation is fitted by one process: several ranks would need an "
                                  "all-reduce of the noise gradient in every step")
    if not clamp_input:
        raise NotImplementedError("the universal perturbation is defined for the clamped-input models (the debug "
                                  "model attacks an unclamped input from a random start)")


def stack_images(im_s):
    """A [B, 3, H, W] batch from a batch or from a list of [1, 3, H, W] / [3, H, W] images of ONE size."""
    if torch.is_tensor(im_s):
        return im_s
    ims = [t if t.dim() == 4 else t.unsqueeze(0) for t in im_s]
    if not ims:
        raise ValueError("no image to fit the perturbation on")
    sizes = {tuple(t.shape[1:]) for t in ims}
    if len(sizes) != 1:
        raise ValueError(f"one perturbation is fitted on images of one size, not {sorted(sizes)}")
    return torch.cat(ims, 0)


class UniversalAttackLoop(AttackLoop):
    """AttackLoop(coupled=True) with noise, m and v of shape [1, 3, H, W]."""

    def __init__(self, kern, im_s, steps=1001, epsilon=16.0, noise_thr=1e-4, lr=0.01, att_metric="L2", clamp=True,
                 group=None, target=None, roi=None):
        universal_guard(att_metric, target, roi, group, bool(getattr(kern, "clamp_input", True)))
        im_s = stack_images(im_s)
        super().__init__(kern, im_s, steps, epsilon, noise_thr, lr, "L2", clamp, coupled=True)
        self.noise = torch.zeros((1, 3, self.H, self.W), device=self.im_s.device)
        self.m = torch.zeros_like(self.noise)
        self.v = torch.zeros_like(self.noise)

    def step(self, i, record_im_in=False, census=False):
        B, H, W = self.B, self.H, self.W
        ev = K._ev_begin("universal.prologue", B)
        call("ica_universal_prologue", ptr(self.noise), ptr(self.im_s), ptr(self.im_in4), ptr(self.part), B, H, W,
             self.eps, stream())
        K._ev_end(ev)
        K.reduce_rows(self.part, B, self.invN, out=self.loss_i)
        D.couple_loss_i(self.loss_i, self.B_global, None)
        E, idx = self._select()   # coupled: the network runs on all images or on none
        if E == B and idx is None and self.graph_ok:
            gx4 = self._network_graph()
        else:
            gx4 = self.network_grad(idx, E) if E > 0 else None
        bc2s, neg_step = self._adam_scalars(i)
        ev = K._ev_begin("universal.adam", B)
        call("ica_universal_adam", ptr(self.noise), ptr(self.im_s), ptr(gx4), ptr(self.loss_i), ptr(self.m),
             ptr(self.v), ptr(self.im_in if record_im_in else None), B, H, W, self.eps, self.thr, self.gscale, bc2s,
             neg_step, ptr(self.branch), ptr(self.census), stream())
        K._ev_end(ev)
        self.steps_done += 1
        if census:
            return self.branch.tolist()
        return None


def universal_batch(kern, im_s, steps=1001, epsilon=16.0, noise_thr=1e-4, lr=0.01, clamp=True, eval_msssim=True,
                    record=False) -> AttackResult:
    """Fit one perturbation on im_s ([B, 3, H, W], or a list of images of one size).  ``noise`` of the result is the
    [1, 3, H, W] perturbation; every other field is per image, as attack_batch gives it."""
    loop = UniversalAttackLoop(kern, im_s, steps, epsilon, noise_thr, lr, "L2", clamp)
    branches = loop.run(record=record)
    im_, out, bpp, mse_in, mse_out, msim_in, msim_out, vi, vi_msim = evaluate(
        kern, loop.im_in, loop.im_s, loop.output_s, clamp, adv=False, msssim=eval_msssim)
    return AttackResult(im_adv=im_, output_adv=out, output_s=loop.output_s, bpp_ori=loop.bpp_ori, bpp=bpp,
                        mse_in=mse_in, mse_out=mse_out, msim_in=msim_in, msim_out=msim_out, vi=vi, vi_msim=vi_msim,
                        noise=loop.noise, branches=branches)


def applied_noise(noise, epsilon):
    """What the loop adds to an image for the raw Adam variable ``noise``: clamp(noise, -eps, eps), eps = epsilon / 255
    (the noise bounds act in the forward; the variable itself may lie outside)."""
    e = float(epsilon) / 255.0
    return noise.clamp(-e, e)


def heldout(kern, noise, images, batch=32):
    """The perturbation ``noise`` ([1, 3, H, W], as it is added: see applied_noise) on ``images`` [M, 3, H, W]:
    transfer.transfer_matrix's TransferResult with one row."""
    return transfer.transfer_matrix(kern, noise, images, batch)
