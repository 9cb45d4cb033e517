"""Drop-in for recompression.py: generation loss of the codec's own 8-bit output.

    python -m imagecompression_adversarial_amd.recompression -m hyper -q 3 -metric ms-ssim -s 'kodim*.png' -steps 10
    python -m imagecompression_adversarial_amd.recompression ... -steps 50 --defend --table --write-dir out/

test   recompression.py:19-63   recompress.recompress (ica_recompress.hip between the eval forwards)

-steps is the number of generations.  Per image it prints ``[IMAGE] name`` and ``bpp psnr msim Result`` of the last
generation, at the end ``Final: bpp psnr msim msim_dB``, the means over the images.

Differences from the reference, all deliberate (DESIGN.md "Re-compression"):
  * Images of one padded size run ``--batch`` at a time; nothing goes through a file between two generations.
  * The reference's per-generation PNGs (a path built from --log, "./attack/kodak/./logs/log.txt_...", which no
    directory holds) are not written.  ``--write-dir DIR`` writes the last generation's PNG of every image, at the
    padded size as the reference's write_image call does.
  * The reference fills ``bpps[i, j]`` after its loops with the loop variable i, i.e. the last row, and prints the
    mean of that row: the Final line here is that mean.  ``--table`` prints every generation's means as well:
    ``gen <g> mean_bpp mean_psnr mean_changed mean_drift``.
  * msim / msim_dB need min(H, W) > 160 (pytorch_msssim raises below that); smaller images print nan.
  * ``--defend_m`` other than ensemble is refused: the reference calls defend(model, im) without a method.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import attack_rd, coder, recompress
from .random_noise import _kern, _load


def config():
    p = coder.config()
    p.add_argument("--table", action="store_true", help="print the per-generation means")
    p.add_argument("--write-dir", dest="write_dir", type=str, default=None,
                   help="write the last generation's PNG of every image here (padded size)")
    return p


def check_args(args):
    if args.method != "ensemble":
        raise ValueError(f"--defend_m {args.method!r}: recompression's defend() is always 'ensemble'")
    if args.steps < 1:
        raise ValueError(f"-steps {args.steps}: at least one generation")
    items = attack_rd._sources(args.source)
    if not items:
        raise ValueError(f"no image matches -s {args.source!r}")
    return items


def write_codes(codes, filename):
    """[H, W] packed codes -> an RGB PNG."""
    from PIL import Image
    c = codes.cpu().numpy().astype(np.uint32)
    rgb = np.stack([(c >> s) & 255 for s in (0, 8, 16)], -1).astype("uint8")
    Image.fromarray(rgb).save(filename)


def _nan(v):
    return float("nan") if v is None else v


def main(argv=None):
    args = config().parse_args(argv)
    items = check_args(args)
    if args.defend:
        print("Self Ensemble Applied!")
    kern = _kern(args)
    if args.write_dir:
        os.makedirs(args.write_dir, exist_ok=True)
    G = args.steps
    rows, table, written = [], torch.zeros((G, 4), dtype=torch.float64), {}
    for group in attack_rd._groups(items, args.batch):
        im, _ = _load(group, args.device)
        res = recompress.recompress(kern, im, G, defend=args.defend)
        bpp, psnr = res.bpp[-1].tolist(), res.psnr[-1].tolist()
        table += torch.stack([res.bpp.sum(1), res.psnr.sum(1), res.changed.double().sum(1), res.drift.sum(1)], 1).cpu()
        for b, (name, _, _, _) in enumerate(group):
            msim = _nan(res.msim[b] if res.msim else None)
            msim_dB = _nan(res.msim_dB[b] if res.msim_dB else None)
            print("[IMAGE]", name)
            print(bpp[b], psnr[b], msim, "Result")
            rows.append((bpp[b], psnr[b], msim, msim_dB))
            if args.write_dir:
                stem = os.path.splitext(os.path.basename(str(name)))[0]
                written[stem + ".png"] = res.codes[b].cpu()
                write_codes(written[stem + ".png"], os.path.join(args.write_dir, stem + ".png"))
    n = len(rows)
    table /= n
    if args.table:
        for g in range(G):
            print("gen", g, *table[g].tolist())
    final = tuple(sum(r[k] for r in rows) / n for k in range(4))
    print("Final:", *final)
    return {"bpp": final[0], "psnr": final[1], "msim": final[2], "msim_dB": final[3], "results": rows,
            "table": table.tolist(), "written": written}   # written: file name -> the codes [H, W] it holds


if __name__ == "__main__":
    main()
