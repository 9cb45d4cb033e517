"""Time of the perturbation-transfer study against the per-pair loop it replaces, same process, HIP events.

    python scripts/bench_transfer.py [--reps 10 --warmup 2 --n 8 --m 8 --batch 32]

Prints one JSON line, times in ms (median / min / max of --reps single calls), hyper q3 (seeded weights with
g_a.6.weight x 40, so that the rounded latents and with them the reconstructions move), x6 operands, N = M = 8 at
768x512 by default:
  matrix      transfer.transfer_matrix(kern, noises, images, batch): M + N M images through the codec
  per_pair    the same pairs through what existed before: degrade.apply_noise, attack.eval_forward on [im; im_in],
              hip_ops.sqdiff_mean and one .tolist() per pair: 2 N M images through the codec
  apply / score   ica_transfer_apply / ica_transfer_score alone on a block of --batch pairs (4 noises x batch / 4
              targets), outputs and workspace prepared; GBps = the bytes each must move / median
  g_a         the g_a forward of --batch images, the yardstick DESIGN.md records
and checks that both paths give the same dB values to 5e-3.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def per_pair_loop(kern, noises, images):
    from imagecompression_adversarial_amd import degrade, hip_ops as K
    from imagecompression_adversarial_amd.attack import eval_forward
    out = []
    for i in range(noises.shape[0]):
        row = []
        for j in range(images.shape[0]):
            im = images[j:j + 1]
            im_in, _, mse_in = degrade.apply_noise(im, noises[i:i + 1])
            x_hat, _ = eval_forward(kern, torch.cat([im, im_in], 0), True)
            mse_out = K.sqdiff_mean(x_hat[1:].contiguous(), x_hat[:1].contiguous())
            mi, mo = torch.stack([mse_in, mse_out]).flatten().tolist()
            row.append(10.0 * math.log10(mo / mi) if mi > 1e-20 and mo > 1e-20 else float("nan"))
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, nargs=2, default=(512, 768))
    ap.add_argument("--quality", type=int, default=3)
    ap.add_argument("--noise", type=float, default=1e-3)
    args = ap.parse_args()
    from imagecompression_adversarial_amd import coder, hip_ops as K, transfer
    from imagecompression_adversarial_amd._lib import lib, ptr, stream
    dev = torch.device("cuda:0")
    H, W = args.hw
    N, M = args.n, args.m
    cargs = coder.config().parse_args(["-m", "hyper", "-metric", "mse", "-q", str(args.quality),
                                       "--synthetic-weights"])
    net = coder.load_model(cargs, training=False).to(dev)
    with torch.no_grad():   # seeded default-init weights keep |y| small: every pair's reconstruction would coincide
        net.get_parameter("g_a.6.weight").mul_(40.0)
    kern = net.kernels(net.attack_precision(None))
    g = torch.Generator().manual_seed(0)
    images = torch.rand((M, 3, H, W), generator=g).to(dev)
    noises = (torch.randn((N, 3, H, W), generator=g) * args.noise ** 0.5).to(dev)
    out = {"reps": args.reps, "N": N, "M": M, "H": H, "W": W, "batch": args.batch, "quality": args.quality}

    res = transfer.transfer_matrix(kern, noises, images, args.batch)
    ref = per_pair_loop(kern, noises, images)
    diffs = [abs(a - b) for ra, rb in zip(res.vi, ref) for a, b in zip(ra, rb) if not (math.isnan(a) and math.isnan(b))]
    out["max_db_diff"] = max(diffs) if diffs else None
    out["nan_pairs"] = sum(math.isnan(v) for r in res.vi for v in r)
    assert diffs and all(d < 5e-3 for d in diffs), out

    out["matrix_ms"] = timed(lambda: transfer.transfer_matrix(kern, noises, images, args.batch), args.reps, args.warmup)
    out["per_pair_ms"] = timed(lambda: per_pair_loop(kern, noises, images), args.reps, args.warmup)
    out["ratio"] = round(out["per_pair_ms"]["median"] / out["matrix_ms"]["median"], 3)

    # the two kernels alone on one block of `batch` pairs
    n, m = 4, max(args.batch // 4, 1)
    g = torch.Generator(device=dev).manual_seed(1)
    im = torch.rand((m, 3, H, W), generator=g, device=dev)
    nz = torch.randn((n, 3, H, W), generator=g, device=dev) * 0.1
    im_in = torch.empty((n * m, 3, H, W), device=dev)
    mse = torch.empty((n, m), device=dev)
    ws = torch.empty(lib().ica_transfer_apply_ws_size(n, m, H, W), device=dev)
    img = 3 * H * W * 4

    def apply():
        assert lib().ica_transfer_apply(ptr(im), ptr(nz), ptr(im_in), n, m, H, W, ptr(mse), ptr(ws), stream()) == 0
    t = timed(apply, 3 * args.reps, args.warmup)
    nbytes = (n * m + m * ((n + 3) // 4) + n * m) * img          # noise reads, target reads, im_in writes
    t["GBps"] = round(nbytes / (t["median"] * 1e-3) / 1e9, 1)
    out["apply_ms"] = t
    x4 = torch.rand((n * m, 1, H, W, 4), generator=g, device=dev)
    s4 = torch.rand((m, 1, H, W, 4), generator=g, device=dev)
    ws2 = torch.empty(lib().ica_transfer_score_ws_size(n, m, H, W), device=dev)

    def score():
        assert lib().ica_transfer_score(ptr(x4), ptr(s4), n, m, H, W, 1, ptr(mse), ptr(ws2), stream()) == 0
    t = timed(score, 3 * args.reps, args.warmup)
    nbytes = (n * m + m * ((n + 3) // 4)) * H * W * 16
    t["GBps"] = round(nbytes / (t["median"] * 1e-3) / 1e9, 1)
    out["score_ms"] = t
    out["pairs_alone"] = [n, m]
    xb = K.to_nc4(torch.rand((n * m, 3, H, W), generator=g, device=dev))
    out["g_a_ms"] = timed(lambda: kern.g_a(xb), 3 * args.reps, args.warmup)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
