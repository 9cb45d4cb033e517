"""The validation scorer at the validation shape (24 Kodak-size images, hyper q3): the fused ica_val_metrics launch next
to the eval forward and next to the torch-op composition it replaces, HIP events; then the outer step's share of a
plain training step.

    python scripts/bench_val_metrics.py [--batch 24 --height 512 --width 768 --warmup 10 --calls 30 --out FILE]

  fused     hip_ops.val_metrics (mse metric: no output plane): ica_val_metrics + ica_reduce_rows
  composed  ica_nc4_to_nchw of x_hat + RateDistortionLoss(training=True)'s torch operations per image
  forward   the eval forward itself
  rd_step   one plain training step (8 x 256x256, hyper q3, mse), and within it clip_grad_norm_ + Adam + the aux step
"""
import argparse
import contextlib
import io
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from scripts.bench_rdeval import stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_val_metrics needs a HIP device")
    from imagecompression_adversarial_amd import coder, hip_ops as K, train
    args = train.config().parse_args(["-m", "hyper", "-q", "3", "-metric", "mse", "--synthetic-weights", "--adv"])
    with contextlib.redirect_stdout(io.StringIO()):
        net, _, opt, aux, _ = coder.load_model(args, training=True)
    kern = net.kernels(net.attack_precision(None))
    B, H, W = a.batch, a.height, a.width
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(0)).to(args.device)
    res = kern.forward(K.to_nc4(x))
    xh4, ly, lz = res["x_hat4"], res["lik4"]["y"], res["lik4"]["z"]
    den = -math.log(2) * H * W

    def fused():
        return K.val_metrics(xh4, x, ly, kern.M, lz, kern.eb.C)

    def composed():
        out = K.from_nc4(xh4, 3)
        bpp = 0.0
        for lik in (ly, lz):
            bpp = bpp + torch.log(torch.clamp(lik, min=1.0 / 65536)).flatten(1).sum(1) / den
        return bpp, ((out - x) ** 2).flatten(1).mean(1)

    for _ in range(a.warmup):
        f, c = fused(), composed()
    torch.cuda.synchronize()
    agree = (float((((f[1] + f[2]) / den - c[0]).abs() / c[0].abs()).max()),
             float(((f[0] / (3 * H * W) - c[1]).abs() / c[1]).max()))
    tf, tc = [], []
    for _ in range(a.calls):
        tf.append(timed(fused)[0])
        tc.append(timed(composed)[0])
    tfw = [timed(lambda: kern.forward(K.to_nc4(x)))[0] for _ in range(max(a.calls // 3, 3))]
    lines = [
        f"hyper q3, {B} x {W}x{H}, precision {kern.precision}, {a.calls} calls after {a.warmup} warm-ups, HIP events",
        f"fused    (ica_val_metrics + ica_reduce_rows): {stats(tf)}",
        f"composed (layout pass + torch clamp / log / sum / mse): {stats(tc)}",
        f"eval forward: {stats(tfw)}",
        f"largest relative difference fused vs composed: bpp {agree[0]:.1e}, mse {agree[1]:.1e}",
    ]
    # the outer step's share of a plain training step
    from imagecompression_adversarial_amd.train_engine import RDTrainer
    tr = RDTrainer(net, "mse", train.LAMBS["mse"][2])
    xb = torch.rand((8, 3, 256, 256), generator=torch.Generator().manual_seed(1)).to(args.device)
    for _ in range(3):
        train.rd_step(net, tr, opt, aux, xb)
    t_all = [timed(lambda: train.rd_step(net, tr, opt, aux, xb))[0] for _ in range(10)]

    def outer():
        torch.nn.utils.clip_grad_norm_(train.main_parameters(net), 1.0)
        opt.step()
        al = net.aux_loss()
        al.backward()
        aux.step()

    t_out = []
    for _ in range(10):
        net.train()
        opt.zero_grad(set_to_none=False)
        aux.zero_grad()
        tr.step(xb)
        t_out.append(timed(outer)[0])
    lines += [f"rd_step (8 x 256x256, hyper q3, mse): {stats(t_all)}",
              f"  of which clip_grad_norm_ + Adam + aux step: {stats(t_out)} "
              f"({100 * statistics.median(t_out) / statistics.median(t_all):.0f} % of the step)"]
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
