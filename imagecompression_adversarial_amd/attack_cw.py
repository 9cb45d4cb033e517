"""Drop-in for attack_cw.py / attack_cw_fast.py: the C&W-style binary-search attack on the HIP attack engine.

    python -m imagecompression_adversarial_amd.attack_cw -m hyper -metric mse -q 3 -s 'kodim*.png' -steps 100 -ssteps 10
    python -m imagecompression_adversarial_amd.attack_cw -m hyper -q 3 -s synthetic:4x512x768 --synthetic-weights --fast

attack_cw     attack_cw.py:115-140   step loss loss_i + c * loss_o with the gate c = 0 while mse_o > 1.1 * level
search_noise  attack_cw.py:142-199   one level: noise = 0, fresh Adam, rounds of ``steps`` steps, bisection on c
              attack_cw_fast.py:127-183 (``--fast``): the level ends by the width / residual rule
attack_       attack_cw.py:201-263   the outer bisection on the level, then the eval
batch_attack  attack_cw.py:308-330   output lines :324 and :330

A whole batch runs together with PER-IMAGE semantics: image b follows the trajectory of its own B == 1 reference
run.  Every step runs the network on the whole batch (the HIP-graph network step of AttackLoop); the gate, the
Adam step count, both bisections and the stop tests are per-image scalar work done ON DEVICE (ica_cw.hip).  Rounds
are ``steps`` steps for every image and levels start on round boundaries, so the images stay aligned; an image
that finished stays in the batch, masked (its noise / m / v are not touched).  The host reads one int per round
(the number of active images).

Differences from the reference, deliberate (DESIGN.md "C&W search"):
  * ``--batch B``, torchrun image sharding and ``synthetic:`` sources, as attack_rd.
  * the eval is self_ensemble.eval (attack.evaluate), not attack_cw.eval's extra noise-level clipping.
  * ``-p``, ``-t`` and ``--defend`` raise NotImplementedError; the loss is L2 (no ms-ssim / lpips variants).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import io
import time

import torch

from . import coder
from . import hip_ops as K
from ._lib import call, ptr, stream
from .attack import AttackLoop, AttackResult, evaluate

# rows of the per-image state tensors (include/ica_hip.h)
SD_CL, SD_CR, SD_C, SD_LEVEL, SD_MIN, SD_MAX = range(6)
SI_T, SI_ROUND, SI_LEVELS, SI_ACTIVE, SI_RESET = range(5)


def adam_table(n, lr):
    """(sqrt(bias_correction2), -lr / bias_correction1) of torch.optim.Adam's steps t = 1..n at a constant lr: the
    double arithmetic of AttackLoop._adam_scalars, rounded to fp32 where the kernel reads it."""
    out = []
    for t in range(1, n + 1):
        bc1 = 1 - 0.9 ** t
        bc2 = 1 - 0.999 ** t
        out.append((float(bc2 ** 0.5), float(-(lr / bc1))))
    return out


def max_rounds_per_level(fast, lamb_attack, search_steps):
    """Upper bound on the rounds of one level: ssteps, or (fast) the halvings that bring |c_r - c_l| = la under
    1e-4, plus the first round (c_r = c there, so a move of c_r keeps the width) and one spare for the rounding of
    the midpoints.  It sizes the Adam table."""
    if not fast:
        return int(search_steps)
    w, k = float(lamb_attack), 0
    while w > 1e-4:
        w /= 2
        k += 1
    return max(k, 1) + 2


class CwAttackLoop(AttackLoop):
    """Device state of one batched attack_cw.attack_ run.  Reuses AttackLoop's pre-eval, prologue and network step
    (L2, whole batch, gscale = 1 / numel: ``part`` then holds each image's sum (output_s - o)^2)."""

    def __init__(self, kern, im_s, steps=1001, epsilon=16.0, noise_thr=1e-4, lr=0.01, lamb_attack=0.2,
                 search_steps=20, fast=False, max_level=0.1, clamp=True):
        if steps < 1 or search_steps < 1:
            raise ValueError("the C&W search needs steps >= 1 and search_steps >= 1")
        if lamb_attack < 0:
            raise ValueError("lamb_attack must be >= 0 (c_eff is applied after the network backward)")
        if (im_s.shape[2] * im_s.shape[3]) % 4:
            raise ValueError("H * W must be a multiple of 4 (images are padded to multiples of 64)")
        super().__init__(kern, im_s, steps, epsilon, noise_thr, lr, "L2", clamp)
        B, dev = self.B, self.im_s.device
        self.noise.zero_()   # search_noise starts every level at zero noise, whatever the model
        self.la, self.ssteps, self.fast, self.lr = float(lamb_attack), int(search_steps), bool(fast), float(lr)
        self.max_rounds = max_rounds_per_level(fast, lamb_attack, search_steps)
        self.ntab = steps * self.max_rounds
        self.tab = torch.tensor(adam_table(self.ntab, lr), dtype=torch.float32).to(dev)
        sd = torch.zeros((6, B), dtype=torch.float64)
        sd[SD_CR] = sd[SD_C] = self.la
        sd[SD_LEVEL] = sd[SD_MAX] = float(max_level)
        sd[SD_MIN] = float(noise_thr)
        si = torch.zeros((5, B), dtype=torch.int32)
        si[SI_ACTIVE] = 1
        self.sd, self.si = sd.to(dev), si.to(dev)
        self.lold = torch.zeros(B, device=dev)
        self.mse_o = torch.zeros(B, device=dev)
        self.c_eff = torch.zeros(B, device=dev)
        self.n_active = torch.zeros(1, dtype=torch.int32, device=dev)
        self.n_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._n_ev = torch.cuda.Event()
        self._cfg = (C.c_double * 2)(self.la, float(noise_thr))
        self.host_reads = 0
        self.rounds = 0

    def cw_step(self, record_im_in=False):
        B, H, W = self.B, self.H, self.W
        call("ica_attack_prologue_ex", ptr(self.noise), ptr(self.im_s), ptr(self.im_in4), ptr(self.part), B, H, W,
             self.eps, int(self.clamp_in), stream())
        K.reduce_rows(self.part, B, self.invN, out=self.loss_i)
        gx4 = self._network_graph() if self.graph_ok else self.network_grad(None, B)
        call("ica_cw_gate", ptr(self.part), K.blocks_per_image(), self.invN, ptr(self.sd), ptr(self.si),
             ptr(self.mse_o), ptr(self.c_eff), B, stream())
        call("ica_cw_adam", ptr(self.noise), ptr(self.im_s), ptr(gx4), ptr(self.c_eff), ptr(self.m), ptr(self.v),
             ptr(self.im_in if record_im_in else None), B, H, W, self.eps, self.invN, ptr(self.tab), self.ntab,
             ptr(self.si), int(self.clamp_in), stream())
        self.steps_done += 1

    def round_end(self):
        """Bisection / level / stop logic on the device, the resets of the images that start a level, then the one
        host read of the round: the number of images still active."""
        B = self.B
        call("ica_cw_round", ptr(self.loss_i), ptr(self.mse_o), ptr(self.sd), ptr(self.lold), ptr(self.si),
             ptr(self.n_active), B, int(self.fast), self.ssteps, self.max_rounds, self._cfg, stream())
        call("ica_cw_reset", ptr(self.noise), ptr(self.m), ptr(self.v), ptr(self.si), B, 3 * self.H * self.W,
             stream())
        self.n_host.copy_(self.n_active, non_blocking=True)
        self._n_ev.record()
        self._n_ev.synchronize()
        self.host_reads += 1
        self.rounds += 1
        return int(self.n_host[0])

    def snapshot(self):
        """(c, level, loss_i, mse_o, active) of the round that just ran its steps (before round_end), as lists."""
        sd, si = self.sd.cpu(), self.si.cpu()
        return {"c": sd[SD_C].tolist(), "level": sd[SD_LEVEL].tolist(), "loss_i": self.loss_i.cpu().tolist(),
                "mse_o": self.mse_o.cpu().tolist(), "active": si[SI_ACTIVE].tolist()}

    def run(self, record=False):
        history = []
        cap = self.ssteps * self.max_rounds
        while True:
            for i in range(self.steps):
                self.cw_step(record_im_in=(i == self.steps - 1))
            if record:
                history.append(self.snapshot())
            if self.round_end() == 0:
                return history
            if self.rounds >= cap:
                raise RuntimeError(f"C&W search still active after {cap} rounds")


def cw_attack_batch(kern, im_s, steps=1001, epsilon=16.0, noise_thr=1e-4, lr=0.01, lamb_attack=0.2, search_steps=20,
                    fast=False, max_level=0.1, clamp=True, record=False, eval_msssim=True):
    """attack_cw.attack_ (fast: attack_cw_fast.attack_) for a batch, per image.  Returns an AttackResult; with
    record=True, (AttackResult, history): one dict per round with the per-image lists c, level, loss_i, mse_o
    (the values that round's bisection used) and active (image b's rounds are those with active[b] == 1)."""
    loop = CwAttackLoop(kern, im_s, steps, epsilon, noise_thr, lr, lamb_attack, search_steps, fast, max_level, clamp)
    history = loop.run(record=record)
    im_, out, bpp, mse_in, mse_out, msim_in, msim_out, vi, vi_msim = evaluate(
        kern, loop.im_in, loop.im_s, loop.output_s, clamp, adv=False, msssim=eval_msssim)
    res = AttackResult(im_adv=im_, output_adv=out, output_s=loop.output_s, bpp_ori=loop.bpp_ori, bpp=bpp,
                       mse_in=mse_in, mse_out=mse_out, msim_in=msim_in, msim_out=msim_out, vi=vi, vi_msim=vi_msim,
                       noise=loop.noise)
    res.loop = loop
    return (res, history) if record else res


# --------------------------------------------------------------------------- #
# CLI
# --------------------------------------------------------------------------- #
def _check_args(args):
    if getattr(args, "pad", None):
        raise NotImplementedError("-p is not supported by attack_cw (the C&W search runs unpadded)")
    if getattr(args, "target", None):
        raise NotImplementedError("-t is not supported by attack_cw (the reference only uses it to name output files)")
    if getattr(args, "defend", False):
        raise NotImplementedError("--defend is not supported by attack_cw (the reference's defend() is undefined there)")
    if args.att_metric != "L2":
        raise NotImplementedError("attack_cw implements the L2 loss only")


class attacker:
    def __init__(self, args):
        self.args = args
        print("==================== ATTACK SETTINGS ====================")
        print("[ IMAGE ]:", args.source, "->", args.target)
        print("Attack Loss Metric:", args.att_metric)
        print("Noise Threshold (L2):", args.noise, f"(epsilon={args.epsilon})")
        print(f"{args.steps} Steps")
        print("=========================================================")
        self.net = coder.load_model(args, training=False).to(args.device)
        for p in self.net.parameters():
            p.requires_grad_(False)

    def attack(self, items):
        """items: list of (name, tensor|None, H, W) of one image size; returns one (bpp_ori, bpp, vi) per image."""
        args = self.args
        ims = [t if t is not None else coder.read_image(name)[0] for name, t, _, _ in items]
        im_s = torch.cat(ims, 0).to(args.device).contiguous()
        kern = self.net.kernels(self.net.attack_precision(getattr(args, "precision", None)))
        res = cw_attack_batch(kern, im_s, steps=args.steps, epsilon=args.epsilon, noise_thr=args.noise,
                              lr=args.lr_attack, lamb_attack=args.lamb_attack, search_steps=args.search_steps,
                              fast=args.fast, clamp=args.clamp, eval_msssim=False)
        return [(float(res.bpp_ori[b]), float(res.bpp[b]), res.vi[b]) for b in range(len(items))]


def batch_attack(args):
    """attack_cw.batch_attack (attack_cw.py:308-330) with attack_rd's --batch grouping and torchrun sharding."""
    from . import attack_rd as R
    from . import dist as D
    _check_args(args)
    rank, world, group = R._dist_setup(args)
    if rank == 0:
        myattacker = attacker(args)
    else:
        with contextlib.redirect_stdout(io.StringIO()):
            myattacker = attacker(args)
    items = R._sources(args.source)
    results = []
    for batch in R._groups([items[i] for i in D.shard_range(len(items), rank, world)], args.batch):
        start = time.time()
        out = myattacker.attack(batch)
        per_t = (time.time() - start) / len(batch)
        results += [(it[0], bpp_ori, bpp, vi, per_t) for it, (bpp_ori, bpp, vi) in zip(batch, out)]
    if world > 1:
        import torch.distributed as tdist
        gathered = [None] * world if rank == 0 else None
        tdist.gather_object(results, gathered, dst=0, group=group)
        tdist.barrier(group=group)
        if rank != 0:
            return None
        results = [r for part in gathered for r in part]
    bpp_ori_, bpp_, vi_, t_ = 0.0, 0.0, 0.0, 0.0
    for name, bpp_ori, bpp, vi, per_t in results:
        print(name, bpp_ori, bpp, vi, "Time:", per_t)
        bpp_ori_ += bpp_ori
        bpp_ += bpp
        vi_ += vi if vi is not None else 0.0   # (the reference adds None and crashes)
        t_ += per_t
    n = max(len(results), 1)
    bpp_ori, bpp, vi, t = bpp_ori_ / n, bpp_ / n, vi_ / n, t_ / n
    rel = (bpp - bpp_ori) / bpp_ori if bpp_ori else float("nan")
    print("AVG:", args.quality, bpp_ori, bpp, rel, vi, t)
    return {"bpp_ori": bpp_ori, "bpp": bpp, "vi": vi, "t": t}


def config():
    """coder.config() (the reference's flags, -la and -ssteps among them) plus --fast."""
    p = coder.config()
    p.add_argument("--fast", dest="fast", action="store_true",
                   help="end a level by attack_cw_fast.py's width / residual rule instead of after -ssteps rounds")
    return p


def main(args):
    if args.quality > 0:
        return batch_attack(args)
    q_max = 7 if args.model == "cheng2020" else 9
    out = None
    for q in range(1, q_max):
        args.quality = q
        out = batch_attack(args)
    return out


if __name__ == "__main__":
    main(config().parse_args())
    import torch.distributed as _tdist
    if _tdist.is_initialized():
        _tdist.destroy_process_group()
