"""Drop-in for attack_rd.py: the distortion attack CLI on the HIP attack engine.

    python -m imagecompression_adversarial_amd.attack_rd -m hyper -metric mse -q 1 -s 'kodim*.png'
    python -m imagecompression_adversarial_amd.attack_rd -m hyper -q 3 -s synthetic:4x512x768 --synthetic-weights

attack_       attack_rd.py:381-575 (+ attack_our :332-379, self_ensemble.eval :173-252)
attacker      attack_rd.py:577-644
batch_attack  attack_rd.py:646-699 (output lines :670 and :688)
main          attack_rd.py:706-715

Differences from the reference, all deliberate and documented:
  * ``--batch B`` attacks B same-size images per launch with per-image semantics
    (bit-identical to B separate runs; tests/test_gpu_attack.py).
  * ``python -m torch.distributed.run --nproc-per-node N -m imagecompression_adversarial_amd.attack_rd ...``
    shards the sorted image list over N ranks (one GPU each, no collective on the attack path); rank 0
    prints the per-image lines in reference order and the AVG line.
  * A ``vi`` of None (mse_out == 0, reference warning at self_ensemble.py:244)
    does not crash the random-restart selection (reference compares None > float).
  * ``--defend`` is not supported (it crashes inside the reference step loop).
  * ``-p P`` pads only the pre-eval, as the reference does (attack_rd.py:389-419); a padded size that is not a
    multiple of 64 raises (the reference's crop would fail on the mismatched reconstruction).
  * ``-t TARGET [--mask_loc x0 x1 y0 y1 -la_tar -la_bkg_in -la_bkg_out]`` runs the targeted / ROI attack
    the README advertises but attack_rd.py never implemented; its loss is defined in
    DESIGN.md ("Targeted / ROI attack").
  * ``-r`` runs the bitrate attack: the reference parses the flag ("rate/distortion attack flag", coder.py:206) and
    never reads it, so there it silently gives the distortion attack.  Here the expensive branch minimises -bpp of
    the relaxed codec (DESIGN.md "Rate attack"); -random keeps the restart with the highest bpp.
"""
from __future__ import annotations

import contextlib
import io
import math
import os
import time
from glob import glob

import torch

from . import coder
from .attack import attack_batch, evaluate, rate_attack_batch, rate_attack_guard, AttackLoop

torch.set_default_dtype(torch.float32)


def _mse_vi(res, b):
    mse = {"mse_in": float(res.mse_in[b]), "mse_out": float(res.mse_out[b])}
    vi = {"vi": res.vi[b], "vi_msim": res.vi_msim[b]}
    return mse, vi


def _rate_guard(args):
    """-r with what the rate attack does not cover raises (attack.rate_attack_guard gives the reasons)."""
    rate_attack_guard(model=args.model, precision=getattr(args, "precision", None), att_metric=args.att_metric,
                      target=getattr(args, "target", None), roi=getattr(args, "mask_loc", None))


def attack_(im_s, net, args):
    """attack_rd.attack_ for a batch: returns (im_adv, output_adv, output_s, bpp_ori, bpp, mse_results, vi_results).
    For B > 1 the metric dicts hold lists (one entry per image)."""
    if getattr(args, "defend", False):
        raise NotImplementedError("--defend is not supported (it crashes inside the reference step loop)")
    kern = net.kernels(net.attack_precision(getattr(args, "precision", None)))
    init_noise = None
    if args.random > 1:
        init_noise = torch.empty_like(im_s).uniform_(-1e-2, 1e-2)
    if getattr(args, "rate", False):
        _rate_guard(args)
        res = rate_attack_batch(kern, im_s, steps=args.steps, epsilon=args.epsilon, noise_thr=args.noise,
                                lr=args.lr_attack, clamp=args.clamp, init_noise=init_noise,
                                eval_msssim=min(im_s.shape[2:]) > 160, pad=args.pad, padding_mode=args.padding_mode)
        return _unpack(res, im_s.shape[0])
    tkw = {}
    if getattr(args, "target", None):
        tkw = dict(target=_target_tensor(args.target, im_s), roi=getattr(args, "mask_loc", None),
                   la_tar=args.lamb_tar, la_bkg_in=args.lamb_bkg_in, la_bkg_out=args.lamb_bkg_out)
    res = attack_batch(kern, im_s, steps=args.steps, epsilon=args.epsilon, noise_thr=args.noise, lr=args.lr_attack,
                       att_metric=args.att_metric, clamp=args.clamp, init_noise=init_noise,
                       eval_msssim=min(im_s.shape[2:]) > 160, pad=args.pad, padding_mode=args.padding_mode, **tkw)
    return _unpack(res, im_s.shape[0])


def _unpack(res, B):
    if B == 1:
        mse, vi = _mse_vi(res, 0)
        return res.im_adv, res.output_adv, res.output_s, res.bpp_ori[0], res.bpp[0], mse, vi
    mses, vis = zip(*[_mse_vi(res, b) for b in range(B)])
    return res.im_adv, res.output_adv, res.output_s, res.bpp_ori, res.bpp, list(mses), list(vis)


def _target_tensor(spec, im_s):
    """Target image for -t (attack_data.py:118-134): zero-padded / cropped into the source's padded frame.
    'synthetic' gives a seeded random target (no files needed)."""
    B, C, H, W = im_s.shape
    if spec == "synthetic":
        g = torch.Generator().manual_seed(1)
        t = torch.rand((1, 3, H, W), generator=g)
    else:
        t, _, _ = coder.read_image(spec)
        pad = torch.zeros((1, 3, H, W))
        h, w = min(H, t.shape[2]), min(W, t.shape[3])
        pad[:, :, :h, :w] = t[:, :, :h, :w]
        t = pad
    return t.to(im_s.device)


def _sources(spec):
    """Glob of image files (sorted, attack_rd.py:648), or synthetic:<B>x<H>x<W> (seeded torch.rand images)."""
    if spec.startswith("synthetic:"):
        B, H, W = (int(v) for v in spec.split(":", 1)[1].split("x"))
        g = torch.Generator().manual_seed(0)
        return [(f"synthetic_{i}", torch.rand((1, 3, H, W), generator=g), H, W) for i in range(B)]
    return [(f, None, None, None) for f in sorted(glob(spec))]


def _padded_shape(item, padding=64):
    """NCHW shape coder.read_image will produce (zero-padded to a multiple of 64), from the PNG header only."""
    name, t, _, _ = item
    if t is not None:
        return tuple(t.shape)
    from PIL import Image
    with Image.open(name) as im:
        W, H = im.size
    return (1, 3, padding * math.ceil(H / padding), padding * math.ceil(W / padding))


def _groups(items, batch):
    """Consecutive runs of same-padded-size images, at most ``batch`` per launch (per-image semantics: the
    grouping changes nothing numerically, only how many images share one set of kernel launches)."""
    groups, cur, cur_shape = [], [], None
    for it in items:
        shape = _padded_shape(it)
        if cur and (len(cur) >= max(batch, 1) or shape != cur_shape):
            groups.append(cur)
            cur = []
        cur.append(it)
        cur_shape = shape
    if cur:
        groups.append(cur)
    return groups


class attacker:
    def __init__(self, args):
        self.args = args
        if getattr(args, "rate", False):
            _rate_guard(args)   # before the model is loaded
        print("==================== ATTACK SETTINGS ====================")
        print("[ IMAGE ]:", args.source, "->", args.target)
        if getattr(args, "rate", False):
            print("Attack Objective: rate")
        print("Attack Loss Metric:", args.att_metric)
        print("Noise Threshold (L2):", args.noise, f"(epsilon={args.epsilon})")
        print(f"{args.steps} Steps")
        print("=========================================================")
        self.net = coder.load_model(args, training=False).to(args.device)
        for p in self.net.parameters():
            p.requires_grad_(False)  # attack: input gradients only (reference computes unused wgrad)
        self.model_config = f"{args.model}_{args.quality}_{args.metric}_"

    def run(self, items):
        """Load ``items`` (list of (name, tensor|None, H, W) of one image size) and attack them as one batch:
        returns (ims, im_s, im_adv, output_adv, output_s, bpp_ori, bpp, mse, vi), the last four per image."""
        ims = []
        for name, t, H, W in items:
            if t is None:
                t, H, W = coder.read_image(name)
            ims.append((t, H, W))
        im_s = torch.cat([t for t, _, _ in ims], 0).to(self.args.device).contiguous()
        im_adv, output_adv, output_s, bpp_ori, bpp, mse, vi = attack_(im_s, self.net, self.args)
        if im_s.shape[0] == 1:
            bpp_ori, bpp, mse, vi = [bpp_ori], [bpp], [mse], [vi]
        return ims, im_s, im_adv, output_adv, output_s, bpp_ori, bpp, mse, vi

    def attack(self, items):
        """items: list of (name, tensor|None, H, W) of one image size; returns per-image results."""
        ims, im_s, im_adv, output_adv, output_s, bpp_ori, bpp, mse, vi = self.run(items)
        out = []
        for b, (name, _, _, _) in enumerate(items):
            v = dict(vi[b])
            mi, mo = mse[b]["mse_in"], mse[b]["mse_out"]
            v["vi_anchor"] = (math.log10(mi) / math.log10(mo)) if (mi > 0 and mo > 0 and mo != 1) else None
            if self.args.target:
                filename = self.model_config + str(name).split("/")[-1].rsplit(".", 1)[0]
                H, W = ims[b][1], ims[b][2]
                coder.write_image(im_adv[b:b + 1], "%s_advin_%s.png" % (filename, self.args.target), H, W)
                coder.write_image(torch.clamp(im_adv[b:b + 1] - im_s[b:b + 1] + 0.5, 0.0, 1.0),
                                  "%s_noise_%s.png" % (filename, self.args.target), H, W)
                coder.write_image(output_adv[b:b + 1], "%s_advout_%s.png" % (filename, self.args.target), H, W)
            out.append((float(bpp_ori[b]), float(bpp[b]), v))
        return out


def _attack_items(myattacker, items, args):
    """Attack ``items`` group by group; returns one (name, bpp_ori, bpp, vi_results, seconds) per image, in
    order.  -random R: R restarts, the best vi kept per image (attack_rd.py:657-664); with -r the highest bpp."""
    if getattr(args, "rate", False):
        score = lambda r: r[1]
    else:
        score = lambda r: r[2]["vi"] if r[2]["vi"] is not None else -float("inf")
    out = []
    for batch in _groups(items, args.batch):
        start = time.time()
        best = [None] * len(batch)
        for _ in range(args.random):
            res = myattacker.attack(batch)
            for b, r in enumerate(res):
                if best[b] is None or score(r) > score(best[b]):
                    best[b] = r
        per_t = (time.time() - start) / len(batch)
        for b, (bpp_ori, bpp, vi_results) in enumerate(best):
            out.append((batch[b][0], bpp_ori, bpp, vi_results, per_t))
    return out


def _dist_setup(args):
    """torchrun launch (WORLD_SIZE > 1): one process per GPU, -device becomes this rank's GPU.  The process
    group carries only the final result gather (no collective on the attack path)."""
    from . import dist as D
    world, _, local = D.env_world()
    if world <= 1:
        return 0, 1, None
    backend = os.environ.get("ICA_DIST_BACKEND")  # default: RCCL on a GPU host, gloo on CPU
    if str(args.device).startswith(("cuda", "hip")):
        ndev = torch.cuda.device_count()
        args.device = f"cuda:{local % max(ndev, 1)}"
        if backend is None and ndev >= world:
            backend = "nccl"
    rank, world, group = D.init_from_env(backend or "gloo")
    return rank, world, group


def collect_results(args, attacker_cls=None):
    """Attack every image of args.source with ``attacker_cls`` (default: this module's attacker): one
    (name, bpp_ori, bpp, vi_results, seconds) per image in reference order.  Under torchrun the sorted image
    list is split into contiguous per-rank shards (dist.shard_range); every rank attacks its shard with no
    collective, the per-image result tuples are gathered to rank 0 once at the end, and every other rank gets
    None.  Shared by the CLIs that print their own lines from these tuples (attack_patch)."""
    from . import dist as D
    attacker_cls = attacker_cls or attacker
    rank, world, group = _dist_setup(args)
    if rank == 0:
        myattacker = attacker_cls(args)
    else:   # settings banners once, from rank 0 (the output matches a one-process run line for line)
        with contextlib.redirect_stdout(io.StringIO()):
            myattacker = attacker_cls(args)
    items = _sources(args.source)
    shard = D.shard_range(len(items), rank, world)
    results = _attack_items(myattacker, [items[i] for i in shard], args)
    if world > 1:
        import torch.distributed as tdist
        gathered = [None] * world if rank == 0 else None
        # names of synthetic items are strings, tensors are not shipped: only the printed numbers travel
        tdist.gather_object(results, gathered, dst=0, group=group)
        if rank != 0:
            tdist.barrier(group=group)
            return None
        results = [r for part in gathered for r in part]
        tdist.barrier(group=group)
    return results


def batch_attack(args):
    """attack_rd.batch_attack (attack_rd.py:646-699): collect_results, then rank 0 prints the reference's
    per-image lines (:670) in reference order and the AVG line (:688)."""
    results = collect_results(args)
    if results is None:
        return None
    bpp_ori_, bpp_, vi_, vi_anchor_, vi_msim_, t_ = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    n_done = 0
    for name, bpp_ori, bpp, vi_results, per_t in results:
        print(name, bpp_ori, bpp, vi_results["vi"], vi_results["vi_msim"], "Time:", per_t)
        bpp_ori_ += bpp_ori
        bpp_ += bpp
        vi_ += vi_results["vi"] if vi_results["vi"] is not None else 0.0
        vi_anchor_ += vi_results["vi_anchor"] if vi_results["vi_anchor"] is not None else 0.0
        # reference quirk kept: vi_msim_ starts at 0.0 (falsy) so the AVG vi_msim is None
        if vi_results["vi_msim"] and vi_msim_:
            vi_msim_ += vi_results["vi_msim"]
        else:
            vi_msim_ = None
        t_ += per_t
        n_done += 1
    num_im = max(n_done, 1)
    vi_msim = vi_msim_ / num_im if vi_msim_ else None
    bpp_ori, bpp, vi, vi_anchor, t = bpp_ori_ / num_im, bpp_ / num_im, vi_ / num_im, vi_anchor_ / num_im, t_ / num_im
    rel = (bpp - bpp_ori) / bpp_ori if bpp_ori else float("nan")
    print(f"AVG: {args.model}-{args.metric}-{args.quality}", bpp_ori, bpp, rel, vi, "vi_anchor:", vi_anchor, vi_msim, t)
    return {"bpp_ori": bpp_ori, "bpp": bpp, "vi": vi, "vi_anchor": vi_anchor, "vi_msim": vi_msim, "t": t}


def main(args):
    if isinstance(args, (list, tuple)):   # an argv list
        args = coder.config().parse_args(list(args))
    if args.quality > 0:
        return batch_attack(args)
    q_max = 7 if args.model == "cheng2020" else 9
    out = None
    for q in range(1, q_max):
        args.quality = q
        out = batch_attack(args)
    return out


if __name__ == "__main__":
    main(coder.config().parse_args())
    import torch.distributed as _tdist
    if _tdist.is_initialized():
        _tdist.destroy_process_group()
