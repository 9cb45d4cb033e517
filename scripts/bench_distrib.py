"""Time of one latent_distribution.latent_distrib call at the shapes the visual_distribution CLI meets, HIP events.

    python scripts/bench_distrib.py [--warmup 20 --calls 200 --out profiles/r07/distrib_time.log]

Per shape: seeded random y / scales / means / likelihoods on the device, --warmup calls, then one pair of events on the
current stream around --calls calls and a synchronise; the figure is the mean per call.  A call is the whole Python
entry: four allocations from torch's caching allocator, the memset of hist, latent_distrib_kernel and the one or
two finish_rows launches.  erff/s counts (nbins + chunks) edge evaluations per element.  Prints one line per shape
and, with --out, writes the same lines there.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

# (B, C, latent H, latent W, nbins, vmin): one / two / 32 images of 768x512 at M = 192, one 2048x2048 image at M = 320
# (the capped split), and 64 bins (four bin chunks)
SHAPES = [(1, 192, 32, 48, 11, -5.5), (2, 192, 32, 48, 11, -5.5), (32, 192, 32, 48, 11, -5.5),
          (1, 320, 128, 128, 11, -5.5), (2, 192, 32, 48, 64, -32.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from imagecompression_adversarial_amd import latent_distribution as LD
    if not torch.cuda.is_available():
        raise RuntimeError("bench_distrib needs a HIP device")
    dev = torch.device("cuda:0")
    lines = []
    for B, C, H, W, nbins, vmin in SHAPES:
        g = torch.Generator().manual_seed(0)
        sh = (B, C // 4, H, W, 4)
        y = (torch.randn(sh, generator=g) * 2).to(dev)
        s = torch.exp(torch.randn(sh, generator=g)).to(dev)
        m = torch.randn(sh, generator=g).to(dev)
        lik = torch.rand(sh, generator=g).clamp(min=1e-9).to(dev)
        for _ in range(args.warmup):
            LD.latent_distrib(y, C, s, m, lik, vmin, nbins)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            LD.latent_distrib(y, C, s, m, lik, vmin, nbins)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.calls
        erf = B * C * H * W * (nbins + (nbins + 15) // 16)
        lines.append(f"B={B} C={C} plane={H}x{W} nbins={nbins}: {us:.1f} us per call, {erf / us * 1e-3:.1f} G erff/s, "
                     f"inputs {16 * B * C * H * W / 1e6:.2f} MB")
        print(lines[-1], flush=True)
    if args.out:
        d = os.path.dirname(args.out)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
