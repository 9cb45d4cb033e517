"""Which frequency band of an adversarial perturbation carries the VI, and an attack confined to chosen bands
(band_vi.py; DESIGN.md "Band VI").  The reference splits the image into freq_1/2/3 (attack_rd.py:427-436) and has a
low-frequency-only perturbation (attack_rd.py:509-510), both commented out; this tool finishes them.

    python -m imagecompression_adversarial_amd.attack_band -m hyper -q 3 -s kodim03.png -t kodim03_advin.png
    python -m imagecompression_adversarial_amd.attack_band -m hyper -q 3 -s 'kodim*.png' --attack -steps 200 --table
    python -m imagecompression_adversarial_amd.attack_band -m hyper -q 3 -s 'kodim*.png' --attack --bands 3-7

Exactly one of ``-t ADV_GLOB`` (paired with ``-s`` in sorted order) and ``--attack`` names the adversarial images.
``--attack`` alone runs the attack_rd distortion attack (-steps / -e / -noise / ...) and the study dissects it; with
``--bands LIST`` (bands 0..7 and ranges, "0-2,5") it runs the band-limited attack and the study is of its result.
Bands: the orthonormal 8x8 block DCT of each channel plane, coefficient (u, v) in band max(u, v).  ``--preset`` picks
the eight variants of the study: ``only`` (band k alone), ``lowpass`` (bands 0..k), ``without`` (all but band k).

Per image it prints

    [IMAGE] name
    all       share 1 mse_in mse_out VI bpp          the whole perturbation (attack.evaluate)
    <bands>   share mse_in mse_out VI bpp            one line per variant: clamp(im_s + P_S (im_adv - im_s), 0, 1)

where share is the part of mean((im_adv - im_s)^2) that lies in the variant's bands, VI = 10 log10(mse_out / mse_in)
(nan under the 1e-20 guards) and mse_out is taken against the clean reconstruction.  ``AVG:`` lines with the means
over the images follow, one per variant.  ``--table`` adds the eight tab-separated rows of the averages, ``--save
PATH`` writes the numbers as a .pt file.  ``main(argv)`` returns them.  Images whose size is no multiple of 8 are
padded to 64 as everywhere in the CLI; there are no plots.
"""
from __future__ import annotations

import os

import torch

from . import band_vi as BV
from . import coder

COLS = ("share", "mse_in", "mse_out", "vi", "bpp")


def config():
    p = coder.config()
    p.add_argument("--attack", action="store_true",
                   help="make the adversarial images with the attack (-steps, -e, -noise, ...)")
    p.add_argument("--bands", type=str, default=None, metavar="LIST",
                   help="with --attack: confine the perturbation to these bands, e.g. 0-2,5")
    p.add_argument("--preset", type=str, default="only", choices=BV.PRESETS, help="the eight variants of the study")
    p.add_argument("--table", action="store_true", help="the eight tab-separated rows of the averages")
    p.add_argument("--save", type=str, default=None, metavar="PATH", help="write the numbers as a .pt file")
    return p


def parse(argv=None):
    p = config()
    args = p.parse_args(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("the study runs in one process: the image list is not sharded over torchrun ranks")
    if bool(args.target) == bool(args.attack):
        p.error("name the adversarial images with exactly one of -t <glob> and --attack")
    if args.bands is not None:
        if not args.attack:
            p.error("--bands confines the attack: it needs --attack")
        try:
            args.band_mask = BV.parse_bands(args.bands)
        except ValueError as e:
            p.error(str(e))
    return args


def _avg(vals):
    vals = [v for v in vals if v == v]
    return sum(vals) / len(vals) if vals else float("nan")


def run(args, items, advs):
    from . import attack_rd
    from .attack import attack_batch, eval_forward, evaluate
    from .random_noise import _kern, _load
    kern = _kern(args)
    masks = BV.preset_masks(args.preset)
    labels = ["all"] + [BV.mask_label(m) for m in masks]
    rows, energy, pos = [], [], 0
    for group in attack_rd._groups(items, args.batch):
        im, _ = _load(group, args.device)
        if advs is not None:
            im_adv, _ = _load(advs[pos:pos + len(group)], args.device)
        elif args.bands is not None:
            im_adv = BV.band_attack_batch(kern, im, args.band_mask, steps=args.steps, epsilon=args.epsilon,
                                          noise_thr=args.noise, lr=args.lr_attack, clamp=args.clamp,
                                          eval_msssim=False).im_adv
        else:
            im_adv = attack_batch(kern, im, steps=args.steps, epsilon=args.epsilon, noise_thr=args.noise,
                                  lr=args.lr_attack, att_metric=args.att_metric, clamp=args.clamp,
                                  eval_msssim=False).im_adv
        pos += len(group)
        im_adv = im_adv.contiguous()
        out_s, _ = eval_forward(kern, im, args.clamp)
        _, _, bpp_all, mi_all, mo_all, _, _, vi_all, _ = evaluate(kern, im_adv, im, out_s, args.clamp, msssim=False)
        st = BV.band_study(kern, im, im_adv, masks, batch=max(args.batch, 1), clamp=args.clamp)
        en = st.energy.double().cpu()
        tot = en.sum(1)
        mi, mo, bp = st.mse_in.cpu().tolist(), st.mse_out.cpu().tolist(), st.bpp.cpu().tolist()
        mi_a, mo_a, bp_a = mi_all.tolist(), mo_all.tolist(), bpp_all.tolist()
        for b, (name, _, _, _) in enumerate(group):
            print("[IMAGE]", name)
            per = [(1.0, mi_a[b], mo_a[b], float("nan") if vi_all[b] is None else vi_all[b], bp_a[b])]
            for v, m in enumerate(masks):
                inside = sum(float(en[b, k]) for k in range(BV.NB) if m >> k & 1)
                share = inside / float(tot[b]) if float(tot[b]) > 0 else float("nan")
                per.append((share, mi[v][b], mo[v][b], st.vi[v][b], bp[v][b]))
            for label, r in zip(labels, per):
                print(label, *r)
            rows.append({"name": name, "variants": per})
            energy.append(en[b])
    avg = [[_avg([r["variants"][v][c] for r in rows]) for c in range(len(COLS))] for v in range(len(labels))]
    for label, r in zip(labels, avg):
        print("AVG:", label, *r)
    if args.table:
        print("band", *COLS, sep="\t")
        for k in range(BV.NB):
            print(k, *avg[1 + k], sep="\t")
    result = {"preset": args.preset, "masks": masks, "labels": labels, "columns": COLS, "rows": rows, "avg": avg,
              "energy": torch.stack(energy)}
    if args.save:
        torch.save(result, args.save)
    return result


def main(argv=None):
    args = parse(argv)
    if args.bands is not None:                     # before any model is built or moved to the device
        BV.band_guard(model=args.model, att_metric=args.att_metric, rate=args.rate, roi=args.mask_loc, pad=args.pad,
                      defend=args.defend)
    if args.model == "debug":
        raise NotImplementedError("the band study codes its variant images with the clamped-input models: -m debug "
                                  "is not covered")
    from .visual_distribution import _pairs
    items, advs = _pairs(args.source, args.target, "-t")
    return run(args, items, advs)


if __name__ == "__main__":
    main()
