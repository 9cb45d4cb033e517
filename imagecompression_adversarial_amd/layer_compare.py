"""The reference's layer_compare (anchors/utils.py:152-166; its attack scripts call it under --debug) as a tool of its
own: where in the codec does the perturbation of an adversarial example grow?

    python -m imagecompression_adversarial_amd.layer_compare -m hyper -q 3 -s kodim03.png -t kodim03_advin.png
    python -m imagecompression_adversarial_amd.layer_compare -m hyper -q 3 -s 'kodim*.png' --attack -steps 200
    python -m imagecompression_adversarial_amd.layer_compare -m hyper -q 3 -s 'kodim*.png' --gauss 0.01 --table

Exactly one of ``-t ADV_GLOB`` (paired with ``-s`` in sorted order), ``--attack`` (the attack_rd distortion attack
with -steps / -e / -noise / ...) and ``--gauss SIGMA`` (seeded Gaussian noise of that standard deviation on the 0..1
scale, clamped: the harmless control) names the adversarial images.

Per image it prints, with the reference's values and order,

    [IMAGE] name
    Encoder:                 8 lines: 0.5 * mean((enc_adv - enc_clean)^2), the image first, then every g_a module
    Quantization: a b        sqrt(mean((y_adv - round(y_clean))^2)), sqrt(mean((round(y_adv) - round(y_clean))^2))
    Decoder:                 one line per g_s module (7; cheng2020: 8): the same two columns after the module

and at the end ``AVG:`` blocks of the same shape with the means over the images.  ``--table`` adds one tab-separated
row per (image, side, layer): image side layer C H W value value_rounded gain_dB, where value is the row's MSE
(encoder) or RMSE (quant, decoder), value_rounded the rounded column (empty for the encoder) and gain_dB =
10 log10(layer MSE / mse_in) of the value column (empty where mse_in is 0).  ``main(argv)`` returns the numbers.

Differences from the reference (DESIGN.md "Layer compare"): every number is per image; the clean
image's unrounded decode, which the reference computes and never reads, is not computed; ``-s`` / ``-t`` are globs
and images of one padded size run ``--batch`` at a time; ``-m debug`` is not built; one process (a torchrun launch
is an argparse error).  The API (layer_study) returns the plain MSE: the factor 0.5 exists only in these prints.
"""
from __future__ import annotations

import math
import os

import torch

from . import attack_rd, coder, layer_study as LS
from .random_noise import _kern, _load
from .visual_distribution import _attack, _pairs

GAUSS_SEED = 0


def config():
    p = coder.config()
    p.add_argument("--attack", action="store_true",
                   help="make the adversarial images with the attack_rd attack (-steps, -e, -noise, ...)")
    p.add_argument("--gauss", type=float, default=None, metavar="SIGMA",
                   help="adversarial image = clamp(clean + seeded Gaussian noise of this std, 0, 1)")
    p.add_argument("--table", action="store_true", help="one tab-separated row per (image, side, layer)")
    return p


def parse(argv=None):
    p = config()
    args = p.parse_args(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        p.error("the study runs in one process: the image list is not sharded over torchrun ranks")
    given = [f for f, on in (("-t", bool(args.target)), ("--attack", args.attack), ("--gauss", args.gauss is not None))
             if on]
    if len(given) != 1:
        p.error("name the adversarial images with exactly one of -t <glob>, --attack and --gauss SIGMA"
                + (f" (got {', '.join(given)})" if given else ""))
    if args.gauss is not None and not (math.isfinite(args.gauss) and args.gauss >= 0):
        p.error(f"--gauss {args.gauss}: a finite standard deviation >= 0")
    return args


def gauss_adv(im, sigma, first_index=0):
    """clamp(im + sigma * n, 0, 1) with n ~ N(0, 1) seeded per image by its position in the -s list, so an image's
    noise does not depend on --batch."""
    noise = torch.stack([torch.randn(im.shape[1:], generator=torch.Generator().manual_seed(GAUSS_SEED + first_index + b))
                         for b in range(im.shape[0])])
    return torch.clamp(im + float(sigma) * noise.to(im.device), 0.0, 1.0).contiguous()


def _block(enc, quant, dec):
    print("Encoder:")
    for v in enc:
        print(v * 0.5)                                  # anchors/utils.py:159
    print("Quantization:", quant[0], quant[1])          # :162
    print("Decoder:")
    for a, b in dec:
        print(a, b)                                     # :166


def _gain(mse, mse_in):
    if not mse_in > 0:
        return ""
    return 10.0 * math.log10(mse / mse_in) if mse > 0 else float("-inf")


def run(args, items, advs):
    kern = _kern(args)
    LS.check_kern(kern)
    results, table, pos = [], [], 0
    for group in attack_rd._groups(items, args.batch):
        im, _ = _load(group, args.device)
        if advs is not None:
            im_adv, _ = _load(advs[pos:pos + len(group)], args.device)
        elif args.gauss is not None:
            im_adv = gauss_adv(im, args.gauss, pos)
        else:
            im_adv = _attack(kern, im, args).contiguous()
        pos += len(group)
        st = LS.layer_compare(kern, im_adv, im)
        enc, quant, dec = st.enc_mse.cpu().tolist(), st.quant_rmse.cpu().tolist(), st.dec_rmse.cpu().tolist()
        for b, (name, _, _, _) in enumerate(group):
            print("[IMAGE]", name)
            _block(enc[b], quant[b], dec[b])
            results.append({"name": name, "enc": enc[b], "quant": quant[b], "dec": dec[b]})
            mse_in = enc[b][0]
            for k, (shape, v) in enumerate(zip(st.enc_shapes, enc[b])):
                table.append((name, "enc", k, *shape, v, "", _gain(v, mse_in)))
            table.append((name, "quant", 0, *st.enc_shapes[-1], quant[b][0], quant[b][1],
                          _gain(quant[b][0] ** 2, mse_in)))
            for k, (shape, (v, vr)) in enumerate(zip(st.dec_shapes, dec[b])):
                table.append((name, "dec", k, *shape, v, vr, _gain(v ** 2, mse_in)))
    if args.table:
        for r in table:
            print(*r, sep="\t")
    n = len(results)
    avg = {"enc": [sum(r["enc"][k] for r in results) / n for k in range(len(results[0]["enc"]))],
           "quant": [sum(r["quant"][k] for r in results) / n for k in range(2)],
           "dec": [[sum(r["dec"][i][k] for r in results) / n for k in range(2)]
                   for i in range(len(results[0]["dec"]))]}
    print("AVG:")
    _block(avg["enc"], avg["quant"], avg["dec"])
    return {"results": results, "avg": avg, "table": table}


def main(argv=None):
    args = parse(argv)
    if args.model == "debug":                      # before any model is built or moved to the device
        raise NotImplementedError(LS.DEBUG_REASON)
    items, advs = _pairs(args.source, args.target, "-t")
    return run(args, items, advs)


if __name__ == "__main__":
    main()
