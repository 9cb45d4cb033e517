"""The universal-perturbation experiment: fit ONE additive noise on a set of images, then score it on images it has
not seen (universal.py; DESIGN.md §8 "Universal perturbation").  The reference has no such CLI.

    python -m imagecompression_adversarial_amd.universal_noise -m hyper -q 3 -metric mse -s 'fit/*.png' \
        --heldout 'test/*.png' -steps 300 --save universal.pt
    python -m imagecompression_adversarial_amd.universal_noise -m hyper -q 3 --noise-file universal.pt -s 'test/*.png'
    python -m imagecompression_adversarial_amd.universal_noise -m hyper -q 1 --synthetic-weights \
        -s synthetic:4x64x64 --heldout synthetic:2x64x64 -steps 12

  * The -s images are grouped by padded size (one perturbation per size; a group is printed with its size and image
    count) and every group is fitted as ONE batch: the perturbation is defined on the whole set, so a group that does
    not fit in memory is the user's to split.  ``--batch`` bounds the forwards that only score.
  * Per fit image one line in attack_rd's format (name bpp_ori bpp vi vi_msim Time:), then an AVG: line; with
    --heldout the same for every held-out image of a fitted size and a second AVG:.  Held-out images of another size
    are counted and reported in one line, not scored.
  * The perturbation that is saved and scored on other images is the loop's variable clipped to +-epsilon/255, which
    is what the loop adds to an image.  The fit images' own lines come from the loop's last im_in, one Adam step
    earlier, as attack_rd's do.
  * ``--save`` writes {"noise": {(H, W): tensor [1, 3, H, W]}, "model", "quality", "metric", "epsilon", "noise_thr",
    "steps"}; ``--noise-file`` loads such a file (weights_only), skips the fit and scores the -s (and --heldout) images.
  * -r, -t, --mask_loc, --defend, -m debug, an -att_metric other than L2 and a multi-process launch raise before the
    HIP library is loaded.
"""
from __future__ import annotations

import os
import time

import torch

from . import attack_rd, coder

BATCH_HELP = ("images per forward when a perturbation is only scored (--heldout, --noise-file; default 32).  A fit "
              "group always runs as ONE batch, whatever this says: the perturbation is fitted on the whole group, so "
              "a group that does not fit in memory has to be split by the user (fewer -s images)")


def config():
    p = coder.config()
    p.add_argument("--heldout", type=str, default=None,
                   help="images the fitted perturbation is scored on (glob, or synthetic:<B>x<H>x<W>)")
    p.add_argument("--save", type=str, default=None, help="write the fitted perturbations to this file")
    p.add_argument("--noise-file", dest="noise_file", type=str, default=None,
                   help="a file written by --save: skip the fit, score its perturbations on the -s images")
    p.add_argument("--table", action="store_true", help="print one summary row per image size at the end")
    next(a for a in p._actions if a.dest == "batch").help = BATCH_HELP
    p.set_defaults(batch=32)
    return p


def guard(args):
    """What this CLI does not cover; raises before any model or library is loaded."""
    from .universal import universal_guard
    if getattr(args, "rate", False):
        raise NotImplementedError("-r: the universal perturbation is the distortion attack (the rate attack is per image)")
    if getattr(args, "defend", False):
        raise NotImplementedError("--defend is not supported (attack_rd does not support it either)")
    if args.model == "debug":
        raise NotImplementedError("-m debug: the universal perturbation is defined for the clamped-input models")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("the universal perturbation is fitted by one process (WORLD_SIZE > 1): several "
                                  "ranks would need an all-reduce of the noise gradient in every step")
    universal_guard(att_metric=args.att_metric, target=args.target, roi=args.mask_loc)
    if args.save and args.noise_file:
        raise ValueError("--save writes a fitted perturbation and --noise-file skips the fit: give one of them")


def size_groups(sizes):
    """{(H, W): [indexes]} of a list of padded sizes, sizes in order of first appearance, indexes in order."""
    groups = {}
    for i, s in enumerate(sizes):
        groups.setdefault(tuple(int(v) for v in s), []).append(i)
    return groups


def noise_payload(noises, args):
    """The dict --save writes: noises {(H, W): [1, 3, H, W] tensor} and the settings that made them."""
    for (H, W), t in noises.items():
        if tuple(t.shape) != (1, 3, H, W):
            raise ValueError(f"the perturbation for {H}x{W} has shape {tuple(t.shape)}")
    return {"noise": {k: v.detach().cpu().contiguous() for k, v in noises.items()}, "model": args.model,
            "quality": args.quality, "metric": args.metric, "epsilon": args.epsilon, "noise_thr": args.noise,
            "steps": args.steps}


def load_noises(path, sizes):
    """The {(H, W): tensor} of a --save file, restricted to ``sizes`` (the padded sizes of the images to score).
    ValueError for a file of another format and for one none of whose perturbations fits an image."""
    data = torch.load(path, map_location="cpu", weights_only=True)
    noises = data.get("noise") if isinstance(data, dict) else None
    if not isinstance(noises, dict) or not noises:
        raise ValueError(f"{path} is not a file written by --save: no 'noise' dictionary")
    for key, t in noises.items():
        if not (isinstance(key, tuple) and len(key) == 2 and torch.is_tensor(t) and tuple(t.shape) == (1, 3) + key):
            raise ValueError(f"{path}: the entry {key!r} is not a [1, 3, H, W] perturbation stored under (H, W)")
    want = {tuple(int(v) for v in s) for s in sizes}
    found = {k: v.float() for k, v in noises.items() if k in want}
    if not found:
        raise ValueError(f"{path} holds perturbations for {sorted(noises)}, and no image has one of these sizes "
                         f"(images: {sorted(want)})")
    return found


def _load(items, device):
    ims = [t if t is not None else coder.read_image(name)[0] for name, t, _, _ in items]
    return torch.cat(ims, 0).to(device).contiguous()


def _sizes(items):
    return [attack_rd._padded_shape(it)[2:] for it in items]


def _print_rows(rows, args, tag):
    """rows: (name, bpp_ori, bpp, vi, vi_msim, seconds) -> attack_rd's per-image lines and an AVG: line."""
    if not rows:
        return None
    for name, bpp_ori, bpp, vi, vi_msim, t in rows:
        print(name, bpp_ori, bpp, vi, vi_msim, "Time:", t)
    n = len(rows)
    bpp_ori = sum(r[1] for r in rows) / n
    bpp = sum(r[2] for r in rows) / n
    vi = sum(r[3] if r[3] is not None else 0.0 for r in rows) / n
    rel = (bpp - bpp_ori) / bpp_ori if bpp_ori else float("nan")
    print(f"AVG: {args.model}-{args.metric}-{args.quality} [{tag}]", bpp_ori, bpp, rel, vi)
    return {"bpp_ori": bpp_ori, "bpp": bpp, "vi": vi, "n": n}


def _score(kern, noise, items, args):
    """clamp(im + noise, 0, 1) through the codec for ``items`` (one size), --batch images at a time."""
    from .attack import eval_forward, evaluate
    rows = []
    for i0 in range(0, len(items), max(args.batch, 1)):
        chunk = items[i0:i0 + max(args.batch, 1)]
        start = time.time()
        im = _load(chunk, args.device)
        output_s, bpp_ori = eval_forward(kern, im, args.clamp)
        _, _, bpp, _, _, _, _, vi, vi_msim = evaluate(kern, im + noise, im, output_s, args.clamp,
                                                      msssim=min(im.shape[2:]) > 160)
        per_t = (time.time() - start) / len(chunk)
        rows += [(it[0], float(bpp_ori[b]), float(bpp[b]), vi[b], vi_msim[b], per_t) for b, it in enumerate(chunk)]
    return rows


def run(args):
    guard(args)
    fit_items = attack_rd._sources(args.source)
    if not fit_items:
        raise ValueError(f"no image matches -s {args.source!r}")
    held_items = attack_rd._sources(args.heldout) if args.heldout else []
    if args.heldout and not held_items:
        raise ValueError(f"no image matches --heldout {args.heldout!r}")
    fit_groups, held_groups = size_groups(_sizes(fit_items)), size_groups(_sizes(held_items))
    loaded = load_noises(args.noise_file, list(fit_groups) + list(held_groups)) if args.noise_file else None

    from .universal import applied_noise, universal_batch   # the HIP library loads from here on
    net = coder.load_model(args, training=False).to(args.device)
    for p in net.parameters():
        p.requires_grad_(False)
    kern = net.kernels(net.attack_precision(getattr(args, "precision", None)))
    print("==================== UNIVERSAL PERTURBATION ====================")
    print("[ FIT ]:", args.source, "[ HELD OUT ]:", args.heldout)
    print("Noise Threshold (L2):", args.noise, f"(epsilon={args.epsilon})", f"{args.steps} Steps")

    noises, fit_rows = {}, []
    for (H, W), idx in fit_groups.items():
        items = [fit_items[i] for i in idx]
        if loaded is not None:
            if (H, W) not in loaded:
                print(f"[GROUP] {H}x{W}: {len(items)} images, no perturbation of this size in {args.noise_file}")
                continue
            print(f"[GROUP] {H}x{W}: {len(items)} images, perturbation from {args.noise_file}")
            noises[(H, W)] = loaded[(H, W)].to(args.device)
            fit_rows += _score(kern, noises[(H, W)], items, args)
            continue
        print(f"[GROUP] {H}x{W}: {len(items)} images, one perturbation")
        start = time.time()
        res = universal_batch(kern, _load(items, args.device), steps=args.steps, epsilon=args.epsilon,
                              noise_thr=args.noise, lr=args.lr_attack, clamp=args.clamp, eval_msssim=min(H, W) > 160)
        per_t = (time.time() - start) / len(items)
        noises[(H, W)] = applied_noise(res.noise, args.epsilon)
        fit_rows += [(it[0], float(res.bpp_ori[b]), float(res.bpp[b]), res.vi[b], res.vi_msim[b], per_t)
                     for b, it in enumerate(items)]
    if loaded is not None:
        noises.update({k: v.to(args.device) for k, v in loaded.items() if k not in noises})
    out = {"fit": _print_rows(fit_rows, args, "scored" if loaded is not None else "fit"), "noise": noises}

    held_rows, unmatched = [], 0
    for size, idx in held_groups.items():
        if size in noises:
            held_rows += _score(kern, noises[size], [held_items[i] for i in idx], args)
        else:
            unmatched += len(idx)
    if held_items:
        out["heldout"] = _print_rows(held_rows, args, "held out")
        if unmatched:
            print(f"[SIZE] {unmatched} of {len(held_items)} held-out images have a padded size no perturbation was "
                  "fitted for: not scored")
    if args.save:
        torch.save(noise_payload(noises, args), args.save)
        print("[SAVE]", args.save, sorted(noises))
    if args.table:
        print("size images_fit vi_fit images_heldout vi_heldout")
        for size in noises:
            names_f = {fit_items[i][0] for i in fit_groups.get(size, [])}
            names_h = {held_items[i][0] for i in held_groups.get(size, [])}
            f = [r[3] or 0.0 for r in fit_rows if r[0] in names_f]
            h = [r[3] or 0.0 for r in held_rows if r[0] in names_h]
            print(f"{size[0]}x{size[1]}", len(f), sum(f) / len(f) if f else None, len(h), sum(h) / len(h) if h else None)
    return out


def main(argv=None):
    return run(config().parse_args(argv))


if __name__ == "__main__":
    main()
