"""Drop-in for search.py: scan a folder for the image whose latent leaves the range profile the furthest.

    python -m imagecompression_adversarial_amd.search -m hyper -metric mse -q 3 -s 'images/*.png' \\
        [--batch N] [--range-file PATH] [--out-dir DIR] [--synthetic-weights]

detect      search.py:130-146  score of one image against the profile (ica_latent_range + ica_latent_detect)
eval        search.py:150-185  running best (strict >, from 0): print, write the image and its reconstruction
batch_test  search.py:187-192  sorted glob
main        search.py:194-201  -q 0 sweeps the qualities

The scores of a batch of same-size images come from the device in one copy of B floats; the running best is
walked on the host in sorted image order, so the lines printed are those of the reference's one-by-one scan.
"""
from __future__ import annotations

import os

from . import coder
from . import hip_ops as K
from .attack import eval_forward
from .feature_range import image_batches
from .latent_range import RangeProfile, score_images


def config():
    p = coder.config()
    p.add_argument("--range-file", dest="range_file", type=str, default=None,
                   help="the profile to score against; default ./attack/data/{model}-{metric}-{quality}[-adv]_range.pt")
    p.add_argument("--out-dir", dest="out_dir", type=str, default="./attack/search/",
                   help="where each new best image and its reconstruction are written (search.py:152)")
    # feature_range and search take one command line: a script that builds a profile and then scans with it passes
    # both the same argument list, so feature_range's --topk parses here too (the profile file already holds its
    # order statistic; nothing in the scan depends on it)
    p.add_argument("--topk", dest="topk", type=int, default=100,
                   help="accepted so feature_range's argument list can be reused; the scan does not use it")
    return p


def _names(image, score):
    """search.py:154, :166-167: <name> and <name minus extension>_<score:.4f>.png"""
    filename = image.split("/")[-1]
    if "." in filename[-5:]:
        return filename, filename[:-4] + f"_{score:.4f}.png"
    return filename + ".png", filename + f"_{score:.4f}.png"


def batch_test(args):
    net = coder.load_model(args, training=False).to(args.device)
    kern = net.kernels(net.attack_precision(getattr(args, "precision", None)))
    profile = RangeProfile.load(args.range_file or RangeProfile.default_path(args), args.device)
    os.makedirs(args.out_dir, exist_ok=True)
    score_best, found = 0, []
    for names, x in image_batches(args):
        scores = score_images(kern, x, profile).tolist()
        for b, (image, score) in enumerate(zip(names, scores)):
            if score > score_best:
                print("FOUND YOU!", image, score)
                im_s = x[b:b + 1]
                out, _ = eval_forward(kern, K.clamp01(im_s.contiguous()), True)
                f_in, f_out = _names(image, score)
                coder.write_image(im_s, os.path.join(args.out_dir, f_in))
                coder.write_image(out, os.path.join(args.out_dir, f_out))
                score_best = score
                found.append((image, score))
    return found


def main(argv=None):
    args = config().parse_args(argv)
    if args.quality > 0:
        return batch_test(args)
    found = []
    q_max = 7 if args.model == "cheng2020" else 9
    for q in range(1, q_max):
        args.quality = q
        found += batch_test(args)
    return found


if __name__ == "__main__":
    main()
