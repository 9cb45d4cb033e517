"""Drop-in for random_noise.py: how much does the codec amplify a harmless degradation of the same power?

    python -m imagecompression_adversarial_amd.random_noise -m hyper -metric mse -q 3 -noise 1e-4 -s 'kodim*.png'
    python -m imagecompression_adversarial_amd.random_noise -m hyper -q 3 -degrade deblur -s 'blur/*.png' -t 'kodim*.png'
    python -m imagecompression_adversarial_amd.random_noise -s None -t 'kodim*.png' -noise 1e-4
    python -m imagecompression_adversarial_amd.random_noise -m hyper -q 3 -degrade jpeg -s 'kodim*.png' [--jpeg-budget]
    python -m imagecompression_adversarial_amd.random_noise -s None -t 'kodim*.png' -degrade jpeg --jpeg-quality 50

test                 random_noise.py:68-111   degrade.evaluate_noise (ica_degrade.hip + one eval forward)
test_deblur          random_noise.py:20-48    degrade.gaussian_blur + degrade.evaluate_deblur
generate_blurimages  random_noise.py:50-65    degrade.blur_to_budget
main, the -q 0 sweep random_noise.py:113-164  main / sweep_plan

-degrade jpeg (an extension; test_commands/jpeg.sh makes such copies with ``cjpeg -q 50``): degrade.jpeg_roundtrip at
--jpeg-quality, or with --jpeg-budget at the first quality from 1 upward whose MSE meets -noise, then
degrade.evaluate_jpeg.  The lines are the noise mode's with the quality appended; ``-s None -t GLOB -degrade jpeg``
writes the degraded copies as PNG to --jpeg-dir (default ./attack/kodak/jpeg_q{Q}).

Differences from the reference, all deliberate (DESIGN.md "Degradations"):
  * The reference's noise-mode AVG line raises NameError (``images_sharp`` is undefined there) and its deblur AVG
    line prints the last image's dPSNR instead of the mean.  Both AVG lines here print means over len(images).
  * One line per image is printed before the AVG line (the reference prints per-image values only with --debug).
  * Images of one padded size are evaluated ``--batch`` at a time; the noise is still sampled per image on the CPU,
    in file order, from the stream torch.manual_seed(0) starts, so batching changes no value.
  * ``--blur-dir`` (default ./attack/kodak/blur, the reference's constant) is created if absent.
"""
from __future__ import annotations

import os
from glob import glob

import torch

from . import attack_rd, coder, degrade
from . import hip_ops as K

BLUR_DIR = "./attack/kodak/blur"           # random_noise.py:65
SWEEP_NOISES = [1e-5, 1e-4, 1e-3, 1e-2]    # random_noise.py:162


def config():
    p = coder.config()
    p.add_argument("--blur-dir", dest="blur_dir", type=str, default=BLUR_DIR,
                   help="where -s None -t <glob> writes the blurred images")
    p.add_argument("--jpeg-budget", dest="jpeg_budget", action="store_true",
                   help="-degrade jpeg: the first quality from 1 upward whose MSE meets -noise, not --jpeg-quality")
    p.add_argument("--jpeg-dir", dest="jpeg_dir", type=str, default=None,
                   help="where -s None -t <glob> -degrade jpeg writes its copies (default ./attack/kodak/jpeg_q{Q})")
    return p


def mode(args):
    """'generate' (-s None -t <glob>), 'deblur' (-degrade deblur), 'jpeg' (-degrade jpeg), 'generate_jpeg' (both)
    or 'noise'."""
    if args.degrade == "jpeg":
        degrade.validate_jpeg(quality=args.jpeg_quality, subsampling=args.jpeg_subsampling)
    if args.source == "None":
        if not args.target:
            raise ValueError("-s None writes blurred copies of the images -t <glob> names: -t is missing")
        return "generate_jpeg" if args.degrade == "jpeg" else "generate"
    if args.degrade == "jpeg":
        return "jpeg"
    if args.degrade == "deblur":
        if not args.target:
            raise ValueError("-degrade deblur compares against the sharp images -t <glob> names: -t is missing")
        return "deblur"
    if args.degrade is not None:
        raise ValueError(f"-degrade {args.degrade!r} is not one of ['deblur', 'jpeg']")
    return "noise"


def sweep_plan(args):
    """The (quality, noise) runs of one invocation (random_noise.py:150-164); noise is None in deblur mode."""
    m = mode(args)
    if m in ("generate", "generate_jpeg"):
        return []
    qualities = [args.quality] if args.quality > 0 else list(range(1, 7 if args.model == "cheng2020" else 9))
    if m == "deblur":
        return [(q, None) for q in qualities]
    if m == "jpeg":
        return [(q, args.noise) for q in qualities]
    noises = [args.noise] if args.quality > 0 else SWEEP_NOISES
    return [(q, n) for q in qualities for n in noises]


def blur_file_name(image, blur_dir=BLUR_DIR):
    return "%s/%s.png" % (blur_dir.rstrip("/"), str(image).split("/")[-1].split(".")[0])


def _load(items, device):
    ims = [(t, H, W) if t is not None else coder.read_image(name) for name, t, H, W in items]
    return torch.cat([t for t, _, _ in ims], 0).to(device).contiguous(), ims


def _kern(args):
    net = coder.load_model(args, training=False).to(args.device)
    for p in net.parameters():
        p.requires_grad_(False)
    return net.kernels(net.attack_precision(getattr(args, "precision", None)))


def generate_blurimages(args):
    """-s None -t <glob>: a blurred copy of each image whose MSE just meets the -noise budget."""
    items = attack_rd._sources(args.target)
    if not items:
        raise ValueError(f"no image matches -t {args.target!r}")
    os.makedirs(args.blur_dir, exist_ok=True)
    out = []
    for group in attack_rd._groups(items, args.batch):
        x, _ = _load(group, args.device)
        blurred, sigma, index, mse = degrade.blur_to_budget(x, args.noise)
        for b, (name, _, _, _) in enumerate(group):
            print(float(sigma[b]), float(mse[b]))                       # random_noise.py:64
            coder.write_image(blurred[b:b + 1], blur_file_name(name, args.blur_dir))
            out.append((name, float(sigma[b]), int(index[b]), float(mse[b])))
    return out


def jpeg_dir(args):
    """--jpeg-dir, else ./attack/kodak/jpeg_q{Q}; with --jpeg-budget the files are coded at the quality each image's
    budget picks, so the default folder is named after the budget: ./attack/kodak/jpeg_mse{noise}."""
    if args.jpeg_dir:
        return args.jpeg_dir
    return "./attack/kodak/jpeg_mse%g" % args.noise if args.jpeg_budget else "./attack/kodak/jpeg_q%d" % args.jpeg_quality


def _jpeg(args, x):
    """(degraded batch, the quality of each image; 0 where --jpeg-budget found none and the image stays as it is)."""
    if args.jpeg_budget:
        out, quality, _, _ = degrade.jpeg_to_budget(x, args.noise, subsampling=args.jpeg_subsampling)
        return out, quality.tolist()
    return degrade.jpeg_roundtrip(x, args.jpeg_quality, args.jpeg_subsampling), [args.jpeg_quality] * x.shape[0]


def generate_jpegimages(args):
    """-s None -t <glob> -degrade jpeg: a JPEG round trip of each image, as PNG (what jpeg.sh makes with cjpeg)."""
    items = attack_rd._sources(args.target)
    if not items:
        raise ValueError(f"no image matches -t {args.target!r}")
    os.makedirs(jpeg_dir(args), exist_ok=True)
    out = []
    for group in attack_rd._groups(items, args.batch):
        x, ims = _load(group, args.device)
        degraded, quality = _jpeg(args, x)
        mse = K.sqdiff_mean(degraded, x).tolist()
        for b, (name, _, _, _) in enumerate(group):
            print(quality[b], mse[b])
            coder.write_image(degraded[b:b + 1], blur_file_name(name, jpeg_dir(args)), ims[b][1], ims[b][2])
            out.append((name, quality[b], mse[b]))
    return out


def run_jpeg(args, kern, items):
    """-degrade jpeg: one quality's run over ``items``; the noise mode's lines with the JPEG quality appended.  With
    --jpeg-budget an image that no quality fits stays as it is (quality 0, dPSNR nan): it gets its line, is left out
    of the means, and the count of such images is printed before the AVG line."""
    rows = []
    for group in attack_rd._groups(items, args.batch):
        im, ims = _load(group, args.device)
        im_jpeg, quality = _jpeg(args, im)
        res = degrade.evaluate_jpeg(kern, im_jpeg, im, [H * W for _, H, W in ims])
        for b, (name, _, _, _) in enumerate(group):
            if args.debug:
                print("JPEG error (L2):", res.mse_in[b])
                print("MSE (out_adv - out_ori):", res.err_out[b])
            print(name, res.dpsnr[b], res.bpp[b], res.psnr[b], quality[b])
            rows.append((res.dpsnr[b], res.bpp[b], res.psnr[b], quality[b]))
    fitted = [r for r in rows if r[3] > 0]
    if len(fitted) < len(rows):
        print("no quality fits:", len(rows) - len(fitted), "of", len(rows), "images (left out of AVG)")
    n = max(len(fitted), 1)
    avg = tuple(sum(r[i] for r in fitted) / n if fitted else float("nan") for i in range(4))
    print("AVG", args.quality, args.noise, *avg)
    return {"dpsnr": avg[0], "bpp": avg[1], "psnr": avg[2], "jpeg_quality": avg[3], "results": rows,
            "unfitted": len(rows) - len(fitted)}


def run_noise(args, kern, items, noises):
    """One (quality, noise) run over ``items`` with the pre-sampled per-image ``noises``; returns the means."""
    rows = []
    pos = 0
    for group in attack_rd._groups(items, args.batch):
        im, ims = _load(group, args.device)
        nz = torch.cat(noises[pos:pos + len(group)], 0).to(args.device).contiguous()
        pos += len(group)
        res = degrade.evaluate_noise(kern, im, nz, [H * W for _, H, W in ims])
        for b, (name, _, _, _) in enumerate(group):
            if args.debug:
                print("Noise level (L2):", res.noise_power[b])
                print("MSE (out_adv - out_ori):", res.err_out[b])
            if args.target:
                coder.write_image(res.x_hat[b:b + 1], args.target, ims[b][1], ims[b][2])   # random_noise.py:110
            print(name, res.dpsnr[b], res.bpp[b], res.psnr[b])
            rows.append((res.dpsnr[b], res.bpp[b], res.psnr[b]))
    n = len(items)
    avg = tuple(sum(r[i] for r in rows) / n for i in range(3))
    print("AVG", args.quality, args.noise, *avg)
    return {"dpsnr": avg[0], "bpp": avg[1], "psnr": avg[2], "results": rows}


def run_deblur(args, kern):
    """-degrade deblur: blurred files (-s) against sharp files (-t), paired in sorted order as the reference zips
    them; with no blurred file the sharp images are blurred with (5, 9), sigma 0.5, unclamped."""
    images_blur = sorted(glob(args.source))
    sharp = attack_rd._sources(args.target)
    if not sharp:
        raise ValueError(f"no image matches -t {args.target!r}")
    if images_blur:
        sharp = sharp[:len(images_blur)]
    rows, pos = [], 0
    for group in attack_rd._groups(sharp, args.batch):
        im_sharp, _ = _load(group, args.device)
        names_blur = images_blur[pos:pos + len(group)] if images_blur else [None] * len(group)
        pos += len(group)
        if images_blur:
            im_blur, _ = _load([(f, None, None, None) for f in names_blur], args.device)
        else:
            im_blur = degrade.gaussian_blur(im_sharp, degrade.BLUR_KSIZE, degrade.BLUR_SIGMA)
        res = degrade.evaluate_deblur(kern, im_blur, im_sharp)
        for b, it in enumerate(group):
            print(names_blur[b], it[0])                      # random_noise.py:21
            print(res.psnr_blur[b], res.psnr_sharp[b])       # random_noise.py:47
            rows.append((res.dpsnr[b], res.bpp[b], res.psnr_sharp[b]))
    n = len(rows)
    avg = tuple(sum(r[k] for r in rows) / n for k in range(3))
    print("AVG", args.quality, *avg)
    return {"dpsnr": avg[0], "bpp": avg[1], "psnr": avg[2], "results": rows}


def main(argv=None):
    args = config().parse_args(argv)
    print(args.source)
    m = mode(args)
    if m == "generate":
        return generate_blurimages(args)
    if m == "generate_jpeg":
        return generate_jpegimages(args)
    print("[RANDOM NOISE]:", args.source)
    torch.manual_seed(0)                       # random_noise.py:5: the stream the noise is drawn from
    out = []
    for quality, noise in sweep_plan(args):
        args.quality = quality
        kern = _kern(args)
        if m == "deblur":
            out.append(run_deblur(args, kern))
            continue
        args.noise = noise
        items = attack_rd._sources(args.source)
        if not items:
            raise ValueError(f"no image matches -s {args.source!r}")
        if m == "jpeg":
            out.append(run_jpeg(args, kern, items))
            continue
        dist = torch.distributions.normal.Normal(0.0, noise ** 0.5)
        noises = [dist.sample(attack_rd._padded_shape(it)) for it in items]
        out.append(run_noise(args, kern, items, noises))
    return out[0] if len(out) == 1 else out


if __name__ == "__main__":
    main()
