"""Drop-in for visual_distribution.py: in which latent channels does an adversarial example cost its bits?

    python -m imagecompression_adversarial_amd.visual_distribution -m hyper -q 3 -s kodim03.png -t kodim03_advin.png
    python -m imagecompression_adversarial_amd.visual_distribution -m hyper -q 3 -s 'kodim*.png' --attack -steps 200
    python -m imagecompression_adversarial_amd.visual_distribution ... -ckpt at.pth.tar -t2 'adv_at/*.png' --table

predicted_distribution  visual_distribution.py:85-101    latent_distribution.latent_distrib (ica_distrib.hip)
the rate gap, ranking    visual_distribution.py:156-179   latent_distribution.study
print(idx, err[idx])     visual_distribution.py:207-209   the top -k lines of every image

Per pair it prints ``[IMAGE] name`` and the top ``-k`` channels (default 3, the reference's num_plots) as
``idx err[idx]``; at the end ``AVG: mean_err_top1 mean_total_gap_bits mean_outside_frac``: the means over the pairs of
the largest channel gap, of sum_c (bits_adv - bits_ori) by the codec's own likelihoods, and of the share of the
adversarial latent's elements outside the bins.  ``--table`` adds one tab-separated row per (image, channel):
image channel err rate_ori rate_adv bits_ori bits_adv outside_ori outside_adv.  ``--save PATH`` writes the dict of
the reference's commented-out torch.save (:185-190) plus bits / bits_t, CPU tensors with one row per image.

With ``-ckpt`` the study runs twice, on the zoo model (``[MODEL] baseline``) and on the checkpoint (``[MODEL] at``),
the reference's baseline-versus-adversarially-trained comparison; ``-t2`` names the second model's adversarial
images (with ``--attack`` it is attacked itself) and ``--save`` writes its dict next to the first as PATH with
``_at`` before the extension.

Differences from the reference, all deliberate (DESIGN.md "Latent distribution"):
  * y, scales and means are those of the eval forward (the reference's probe feeds h_s(h_a(g_a(x))) without abs or
    rounding and, for the context models, 2M parameter channels that cannot broadcast against y).
  * No figure is drawn: the numbers behind the figures are printed and saved.
  * ``-s`` / ``-t`` are globs paired in sorted order and images of one padded size run ``--batch`` at a time.
  * ``--attack`` makes the adversarial images with the attack_rd distortion attack instead of reading them.
  * Equal gaps are ranked in channel order (a stable sort).
  * One process: the image list is not sharded over torchrun ranks, and a torchrun launch (WORLD_SIZE > 1) is an
    argparse error, so no two ranks print or --save the same study.
  * ``-t`` / ``-t2`` together with ``--attack``, and ``-t2`` without ``-ckpt``, are argparse errors.
"""
from __future__ import annotations

import os

import torch

from . import attack_rd, coder, latent_distribution as LD
from .random_noise import _kern, _load

KEYS = ("y_hat", "y_hat_t_hist", "channel_index", "err", "y_pred", "y_pred_t", "bits", "bits_t")


def config():
    p = coder.config()
    p.add_argument("-t2", dest="at_image", type=str, default=None,
                   help="adversarial images (glob) of the -ckpt model")   # visual_distribution.py:105
    p.add_argument("--attack", action="store_true",
                   help="make the adversarial images with the attack_rd attack (-steps, -e, -noise, ...)")
    p.add_argument("-k", dest="top", type=int, default=3, help="channels printed per image")
    p.add_argument("--table", action="store_true", help="one tab-separated row per (image, channel)")
    p.add_argument("--save", type=str, default=None, help="torch.save the study's tensors here")
    return p


def parse(argv=None):
    p = config()
    args = p.parse_args(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("the study runs in one process: the image list is not sharded over torchrun ranks")
    if not args.target and not args.attack:
        p.error("give the adversarial images with -t <glob>, or --attack to make them")
    if args.attack and (args.target or args.at_image):
        p.error("--attack makes the adversarial images itself: give either it or -t / -t2, not both")
    if args.at_image and not args.checkpoint:
        p.error("-t2 names the adversarial images of the -ckpt model: -ckpt is missing")
    if args.checkpoint and not args.at_image and not args.attack:
        p.error("-ckpt compares a second model: give its adversarial images with -t2 <glob>, or --attack")
    if args.top < 1:
        p.error(f"-k {args.top}: at least one channel")
    return args


def _pairs(source, target, flag):
    items = attack_rd._sources(source)
    if not items:
        raise ValueError(f"no image matches -s {source!r}")
    if target is None:
        return items, None
    advs = attack_rd._sources(target)
    if len(advs) != len(items):
        raise ValueError(f"-s matches {len(items)} images and {flag} {len(advs)}: they are paired in sorted order")
    for a, b in zip(items, advs):
        if attack_rd._padded_shape(a) != attack_rd._padded_shape(b):
            raise ValueError(f"{a[0]} and {b[0]} differ in size")
    return items, advs


def save_path(path, label):
    if label == "baseline":
        return path
    root, ext = os.path.splitext(path)
    return f"{root}_{label}{ext}"


def _attack(kern, im, args):
    from .attack import attack_batch
    return attack_batch(kern, im, steps=args.steps, epsilon=args.epsilon, noise_thr=args.noise, lr=args.lr_attack,
                        att_metric=args.att_metric, clamp=args.clamp, eval_msssim=False, pad=args.pad,
                        padding_mode=args.padding_mode).im_adv


def run(args, label, items, advs):
    """One model over every pair: prints the per-image blocks, the table and the AVG line; returns the tensors."""
    kern = _kern(args)
    rows, saved, table = [], {k: [] for k in KEYS}, []
    pos = 0
    for group in attack_rd._groups(items, args.batch):
        im, _ = _load(group, args.device)
        if advs is None:
            im_adv = _attack(kern, im, args)
        else:
            im_adv, _ = _load(advs[pos:pos + len(group)], args.device)
        pos += len(group)
        st = LD.study(kern, im, im_adv)
        parts = (st.hist_frac, st.hist_frac_adv, st.channel_index, st.err, st.clean.pred, st.adv.pred, st.bits,
                 st.bits_adv)
        cpu = dict(zip(KEYS, (t.cpu() for t in parts)))
        for k in KEYS:
            saved[k].append(cpu[k])
        extra = [t.cpu() for t in (st.rate_ori, st.rate_adv, st.outside, st.outside_adv)]
        C = st.err.shape[1]
        for b, (name, _, _, _) in enumerate(group):
            print("[IMAGE]", name)
            err, index = cpu["err"][b], cpu["channel_index"][b]
            for i in range(min(args.top, C)):
                idx = int(index[i])
                print(idx, float(err[idx]))                      # visual_distribution.py:209
            gap = float((cpu["bits_t"][b].double() - cpu["bits"][b].double()).sum())
            rows.append((float(err[index[0]]), gap, float(extra[3][b].sum()) / (C * st.clean.pixels)))
            for c in range(C):
                table.append((name, c, float(err[c]), float(extra[0][b, c]), float(extra[1][b, c]),
                              float(cpu["bits"][b, c]), float(cpu["bits_t"][b, c]), int(extra[2][b, c]),
                              int(extra[3][b, c])))
    if args.table:
        for r in table:
            print(*r, sep="\t")
    n = len(rows)
    avg = tuple(sum(r[k] for r in rows) / n for k in range(3))
    print("AVG:", *avg)
    saved = {k: torch.cat(v, 0) for k, v in saved.items()}
    if args.save:
        path = save_path(args.save, label)
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        torch.save(saved, path)
    return {"label": label, "err_top1": avg[0], "gap_bits": avg[1], "outside_frac": avg[2], "results": rows,
            "table": table, "saved": saved}


def main(argv=None):
    args = parse(argv)
    LD.check_model(args.model)                 # before any model is built or moved to the device
    items, advs = _pairs(args.source, args.target, "-t")
    ckpt = args.checkpoint
    advs2 = _pairs(args.source, args.at_image, "-t2")[1] if ckpt else None
    args.checkpoint = None                     # visual_distribution.py:114-116: the zoo model first
    if ckpt:
        print("[MODEL] baseline")
    out = [run(args, "baseline", items, advs)]
    if ckpt:
        args.checkpoint = ckpt
        print("[MODEL] at")
        out.append(run(args, "at", items, advs2))
    return out[0] if len(out) == 1 else out


if __name__ == "__main__":
    main()
