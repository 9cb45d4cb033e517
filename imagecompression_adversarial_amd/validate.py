"""The trainer's validation (the reference's test_epoch, train.py:196-242) on the HIP engine.

test_epoch   train.py:196-242   the mean validation loss of the held-out images, the log line, the printed line
  --adv      train.py:210-215   per image: the attack at noise 1e-4, the mean of its VI
  plain      train.py:217-229   per image: criterion(net.eval()(d), d, training=True), the mean of its loss

Per image the plain numbers are RateDistortionLoss(..., training=True) with N = 1 on an EVAL forward: both
likelihood tensors clamped at 2^-16, bpp over the padded H * W, the distortion of the UNCLAMPED x_hat (its mse, or its
pytorch_msssim value), loss = lambda * 255^2 * mse + lamb_r * bpp or lambda * (1 - msim) + lamb_r * bpp, lamb_r = 0 for
lambda == 100 (train.py:77-80).  One eval forward, one ``hip_ops.val_metrics`` launch (ica_rdeval.hip), one row
reduction, and for ms-ssim the MS-SSIM pyramid.  The attack, the eval forward and MS-SSIM are the kernels the attack
engine and the RD evaluation already run; the fused scorer is the only device code that belongs to this module.

Deliberate differences from the reference (DESIGN.md "Validation"):
  * The images are a sorted glob (or synthetic:<B>x<H>x<W>) read with coder.read_image, which zero-pads them to x64;
    the reference's test loader does not pad.  Same-shape images are scored ``--val-batch`` at a time with per-image
    semantics: the result does not depend on the batch.
  * --adv: the noise level 1e-4 is passed to the attack; ``args.noise`` is never touched (the reference overwrites and
    restores it).  An image whose VI is undefined (mse <= 1e-20 on either side, attack.evaluate) is left out of the
    mean and counted; the reference's AverageMeter raises on its None.  If every image is left out, this raises.
  * The means are float64 sums of the per-image values; over ranks, one float64 all-reduce of (sums, count, skipped),
    after which every rank holds the same bits.
  * The log line of --adv, which in the reference holds only zeros, gets `` |\\tVI: {:.4f}`` appended.
  * -metric ms-ssim with an image whose smaller side is <= 160 raises ValueError (pytorch_msssim asserts there).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field

import torch

from . import attack_rd, batch_test, coder
from . import dist as D
from . import hip_ops as K
from . import msssim as MS
from .attack import attack_batch
from .random_noise import _load
from .rd_eval import MSSSIM_MIN_SIDE

VAL_NOISE = 1e-4   # train.py:212 "force input pertubation level to 1e-4"
SUM_KEYS = ("loss", "distortion", "bpp")


@dataclass
class ValResult:
    """The means over the scored images (float64 sums of the per-image fp32 values / count), the same on every rank."""
    loss: float                    # what the scheduler steps on: mean VI (--adv) or mean RD loss (plain)
    count: int                     # images in the mean, over all ranks
    skipped: int = 0               # --adv: images whose VI is undefined
    distortion: float = 0.0        # plain: mean distortion_loss (mse, or the ms-ssim value)
    bpp: float = 0.0               # plain: mean bpp_loss
    aux_loss: float = 0.0          # plain: net.aux_loss()
    adv: bool = False
    rows: list = field(default_factory=list)   # this rank's per-image dicts, in the order of its shard


def val_items(spec):
    """The validation images of ``-val``: a sorted glob or synthetic:<B>x<H>x<W> (the grammar of -s)."""
    if not spec:
        raise ValueError("-val: no validation source")
    items = attack_rd._sources(spec)
    if not items:
        raise FileNotFoundError(spec)
    return items


def check_msssim_sizes(items):
    """pytorch_msssim asserts min(H, W) > 160: name the first file it would refuse, before anything is launched."""
    for it in items:
        _, _, H, W = attack_rd._padded_shape(it)
        if min(H, W) <= MSSSIM_MIN_SIDE:
            raise ValueError(f"-metric ms-ssim: {it[0]} is {H}x{W} after padding; the smaller side must exceed "
                             f"{MSSSIM_MIN_SIDE} (four 2x downsamplings of an 11-tap window)")


def score_plain(kern, x, metric, lmbda):
    """criterion(net.eval()(x), x, training=True) per image (N = 1) for a batch of same-size images: a dict of fp32
    [B] device tensors loss / bpp / distortion, in the reference's operations and order."""
    B, H, W = K.check_image(x, "x", dev=False)
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError("the validation runs on HIP fp32 tensors (no CPU fallback)")
    if metric not in ("mse", "ms-ssim"):
        raise ValueError(f"metric {metric!r} (lpips is out of scope)")
    if metric == "ms-ssim" and min(H, W) <= MSSSIM_MIN_SIDE:
        raise ValueError(f"-metric ms-ssim: a {H}x{W} image; the smaller side must exceed {MSSSIM_MIN_SIDE}")
    x = x.contiguous()
    res = kern.forward(K.to_nc4(x))
    lik = res["lik4"]
    lik_z = lik.get("z")
    x_hat4 = K.cast_nc4(res["x_hat4"], torch.float32)
    sse, lny, lnz, x_hat = K.val_metrics(x_hat4, x, lik["y"], kern.M, lik_z, kern.eb.C if lik_z is not None else 0,
                                         want_x_hat=metric == "ms-ssim")
    den = -math.log(2) * (H * W)
    bpp = lny / den + lnz / den
    lamb_r = 0.0 if lmbda == 100 else 1.0   # train.py:77-80 "Inf Mode"
    if metric == "mse":
        dist = sse / (3 * H * W)
        loss = lmbda * 255 ** 2 * dist + lamb_r * bpp
    else:
        dist = MS.ms_ssim_per_image(x_hat, x)
        loss = lmbda * (1 - dist) + lamb_r * bpp
    return {"loss": loss, "bpp": bpp, "distortion": dist}


def _backend_device(group, device):
    """Where the all-reduced vector lives: the compute device under RCCL, the CPU under gloo."""
    if group is None:
        return torch.device("cpu")
    import torch.distributed as dist
    return torch.device(device) if dist.get_backend(group) == "nccl" else torch.device("cpu")


def sharded_mean(sums, count, skipped=0, group=None, device="cpu"):
    """(means, count, skipped) over all ranks from this rank's float64 sums: one all-reduce of
    [sums..., count, skipped] in float64.  Every rank ends with the same bits; a rank with an empty shard contributes
    zeros.  Raises when no rank scored an image."""
    t = torch.tensor([float(s) for s in sums] + [float(count), float(skipped)], dtype=torch.float64,
                     device=_backend_device(group, device))
    D.allreduce_sum_(t, group, kind="loss")
    t = t.cpu()
    n, sk = int(t[-2]), int(t[-1])
    if n == 0:
        raise RuntimeError(f"validation: no image to average ({sk} skipped: their VI is undefined)")
    return [float(v / n) for v in t[:-2]], n, sk


def _sum64(rows, key):
    return float(sum((torch.tensor(r[key], dtype=torch.float64) for r in rows), torch.zeros((), dtype=torch.float64)))


def validate_plain(kern, items, metric, lmbda, batch=8, device="cuda:0", rank=0, world=1, group=None,
                   aux_loss=0.0) -> ValResult:
    """train.py:217-229 over ``items`` (all ranks pass the same list; each scores its shard)."""
    if metric == "ms-ssim":
        check_msssim_sizes(items)
    sl = D.shard_range(len(items), rank, world)
    mine = items[sl.start:sl.stop]
    rows = [None] * len(mine)
    for idx in batch_test.plan(mine, batch):
        group_items = [mine[i] for i in idx]
        x, _ = _load(group_items, device)
        m = {k: v.detach().cpu() for k, v in score_plain(kern, x, metric, lmbda).items()}
        for b, i in enumerate(idx):
            rows[i] = {"name": group_items[b][0], **{k: float(m[k][b]) for k in SUM_KEYS}}
    means, n, _ = sharded_mean([_sum64(rows, k) for k in SUM_KEYS], len(rows), 0, group, device)
    return ValResult(loss=means[0], distortion=means[1], bpp=means[2], count=n, aux_loss=float(aux_loss), rows=rows)


def validate_adv(kern, items, args, batch=8, device="cuda:0", rank=0, world=1, group=None) -> ValResult:
    """train.py:210-215 over ``items``: per image the attack at noise 1e-4 (per-image semantics, no MS-SSIM in its
    evaluation) and its VI = 10 log10(mse_out / mse_in)."""
    sl = D.shard_range(len(items), rank, world)
    mine = items[sl.start:sl.stop]
    rows = [None] * len(mine)
    for idx in batch_test.plan(mine, batch):
        group_items = [mine[i] for i in idx]
        x, _ = _load(group_items, device)
        res = attack_batch(kern, x, steps=args.steps, epsilon=args.epsilon, noise_thr=VAL_NOISE, lr=args.lr_attack,
                           att_metric=args.att_metric, clamp=args.clamp, eval_msssim=False, coupled=False)
        for b, i in enumerate(idx):
            rows[i] = {"name": group_items[b][0], "vi": res.vi[b]}
    kept = [r for r in rows if r["vi"] is not None]
    means, n, sk = sharded_mean([_sum64(kept, "vi")], len(kept), len(rows) - len(kept), group, device)
    return ValResult(loss=means[0], count=n, skipped=sk, adv=True, rows=rows)


def log_line(epoch, r: ValResult) -> str:
    """train.py:233, character for character; --adv appends the VI (the reference's line holds only zeros there)."""
    loss, d, bpp = (0.0, 0.0, 0.0) if r.adv else (r.loss, r.distortion, r.bpp)
    line = (f"Test epoch {epoch}: Average losses:\tLoss: {loss:.4f} |\tMSE loss: {d:.6f} |\tBpp loss: {bpp:.3f} |"
            f"\tRecomp loss: {0.0:.3f}")
    if r.adv:
        line += f" |\tVI: {r.loss:.4f}"
    return line + "\n"


def test_epoch(epoch, items, net, args, lmbda, log_path=None, rank=0, world=1, group=None) -> ValResult:
    """train.py:196-242.  The parameters are frozen while the kernels run and re-enabled afterwards (as adv_step
    does); the model's train / eval mode on return is what it was on entry.  Rank 0 appends the log line."""
    was_training = net.training
    net.eval()
    for p in net.parameters():
        p.requires_grad_(False)
    try:
        kern = net.kernels(net.attack_precision(getattr(args, "precision", None)))
        batch = max(int(getattr(args, "val_batch", 8)), 1)
        if args.adv:
            r = validate_adv(kern, items, args, batch, args.device, rank, world, group)
        else:
            with torch.no_grad():
                aux = float(net.aux_loss())
            r = validate_plain(kern, items, args.metric, lmbda, batch, args.device, rank, world, group, aux)
    finally:
        for p in net.parameters():
            p.requires_grad_(True)
        net.train(was_training)
    line = log_line(epoch, r)
    if rank == 0:
        if log_path:
            os.makedirs(os.path.dirname(log_path) or ".", exist_ok=True)
            with open(log_path, "a") as f:
                f.write(line)
        if args.adv:
            print(f"Test Loss (VI): {r.loss:.4f}" + (f" ({r.skipped} images skipped: VI undefined)" if r.skipped else ""))
        else:
            print(line)
    return r


test_epoch.__test__ = False   # the reference's name; not a test
