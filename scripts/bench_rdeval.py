"""The loss side of the RD evaluation at the headline shape: the fused ica_rd_metrics launch against the passes it
replaces, HIP events.

    python scripts/bench_rdeval.py [--batch 32 --height 512 --width 768 --warmup 10 --calls 30 --out FILE]

hyper q3 on seeded synthetic weights, one eval forward of --batch images; its x_hat4 and likelihood planes are the
inputs of both sides.  Timed per call with one pair of events on the current stream, the two sides alternating call
by call; the figures are the median and the min-max of --calls calls after --warmup calls of each side.

  fused     hip_ops.rd_metrics: ica_rd_metrics + ica_reduce_rows (the memset of the census included)
  composed  ica_nc4_bound_to_nchw (clamp) + RateDistortionLoss's torch operations per image: for each likelihood
            plane log(clamp(lik, 2^-16)).sum / (-ln 2 H W), then mean((clamp(x_hat, 0, 1) - target)^2)
  forward   the eval forward itself, and rd_eval_batch as a whole (MS-SSIM included), for scale

Bytes: what the fused kernel has to move (x_hat4, target and the planes read once, the clamped image written once),
from the shapes; the rate is those bytes over the fused time.
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def stats(ts):
    return f"median {statistics.median(ts):.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_rdeval needs a HIP device")
    import contextlib
    import io
    from imagecompression_adversarial_amd import coder, hip_ops as K, rd_eval
    from imagecompression_adversarial_amd._lib import call, ptr, stream
    args = coder.config().parse_args(["-m", "hyper", "-q", "3", "-metric", "mse", "--synthetic-weights"])
    with contextlib.redirect_stdout(io.StringIO()):
        net = coder.load_model(args, training=False).to(args.device)
    kern = net.kernels(net.attack_precision(None))
    B, H, W = a.batch, a.height, a.width
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(0)).to(args.device)
    res = kern.forward(K.to_nc4(x))
    xh4, ly, lz = res["x_hat4"], res["lik4"]["y"], res["lik4"]["z"]
    den = -math.log(2) * H * W

    def fused():
        return K.rd_metrics(xh4, x, ly, kern.M, lz, kern.eb.C)

    def composed():
        out = torch.empty_like(x)
        call("ica_nc4_bound_to_nchw", ptr(xh4), ptr(out), B, H, W, 1, stream())
        bpp = 0.0
        for lik in (ly, lz):
            bpp = bpp + torch.log(torch.clamp(lik, min=1.0 / 65536)).flatten(1).sum(1) / den
        mse = ((torch.clamp(out, 0.0, 1.0) - x) ** 2).flatten(1).mean(1)
        return bpp, mse

    for _ in range(a.warmup):
        f, c = fused(), composed()
    torch.cuda.synchronize()
    bpp_f = (f[1] + f[2]) / den
    agree = (float(((bpp_f - c[0]).abs() / c[0].abs()).max()), float(((f[0] / (3 * H * W) - c[1]).abs() / c[1]).max()))
    tf, tc = [], []
    for _ in range(a.calls):
        tf.append(timed(fused)[0])
        tc.append(timed(composed)[0])
    tfw = [timed(lambda: kern.forward(K.to_nc4(x)))[0] for _ in range(max(a.calls // 3, 3))]
    tall = [timed(lambda: rd_eval.rd_eval_batch(kern, x))[0] for _ in range(max(a.calls // 3, 3))]
    nbytes = 4 * (xh4.numel() + 2 * x.numel() + ly.numel() + lz.numel())
    mf, mc = statistics.median(tf), statistics.median(tc)
    lines = [
        f"hyper q3, {B} x {W}x{H}, precision {kern.precision}, {a.calls} calls after {a.warmup} warm-ups, HIP events",
        f"fused    (ica_rd_metrics + ica_reduce_rows, 3 launches with the memset): {stats(tf)}",
        f"composed (layout pass + torch clamp / log / sum / mse): {stats(tc)}",
        f"ratio composed / fused (medians): {mc / mf:.2f}",
        f"fused moves {nbytes / 1e6:.0f} MB (above the 256 MiB Infinity Cache: not resident): "
        f"{nbytes / mf * 1e-9:.2f} TB/s",
        f"largest relative difference fused vs composed: bpp {agree[0]:.1e}, mse {agree[1]:.1e}",
        f"eval forward: {stats(tfw)}",
        f"rd_eval_batch (forward + loss side + MS-SSIM + the copy to the host): {stats(tall)}",
    ]
    print("\n".join(lines), flush=True)
    if a.out:
        d = os.path.dirname(a.out)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
