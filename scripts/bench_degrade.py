"""Time of the degradation kernels against their torch baselines, same process, HIP events.

    python scripts/bench_degrade.py [--reps 30 --warmup 3 --loop-reps 3]

Prints one JSON line, times in ms (median / min / max of --reps single calls):
  blur_*          degrade.gaussian_blur, (5, 9), sigma 0.5, clamp, fused MSE against the input, at 32x3x512x768 and
                  4x3x2048x2048; GBps = (one read + one write of the batch) / median; floor_frac against the measured
                  HBM copy rate (6.29 TB/s, MI355X_MICROARCH.md)
  blur_launch_*   the same work without the Python wrapper (taps, output and workspace prepared): per call of the C
                  entry, 10 calls between two events
  blur_torch_*    F.pad(reflect) + grouped conv2d + clamp + per-image mean on the same GPU
  budget          degrade.blur_to_budget at 32x3x512x768 on smooth seeded images, noise 1e-4: chunks of
                  ica_blur_sweep_chunk() candidates; fma_frac = B 3 H W kx ky S_evaluated FMAs / sweep time over the
                  vector fp32 peak (157.3 TFLOPS = 78.65 T FMA/s)
  budget_torch    the reference's loop in torch on the same GPU, one image at a time, the MSE read on the host at
                  every step (--loop-reps runs: one run is tens of thousands of launches)
and checks that both searches return the same indices (or, where they differ, MSEs within 1e-3 of the budget).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_COPY_BPS = 6.29e12
FMA_PEAK = 157.3e12 / 2


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


def torch_kernel(ksize, sigma, dev):
    from imagecompression_adversarial_amd.degrade import gaussian_taps
    kx, ky = ksize
    k2 = torch.mm(gaussian_taps(ky, sigma)[:, None], gaussian_taps(kx, sigma)[None, :])
    return k2.expand(3, 1, ky, kx).contiguous().to(dev)


def torch_blur(x, w, clamp=True):
    ky, kx = w.shape[2:]
    y = F.conv2d(F.pad(x, (kx // 2, kx // 2, ky // 2, ky // 2), mode="reflect"), w, groups=3)
    y = y.clamp(0, 1) if clamp else y
    return y, ((y - x) ** 2).mean(dim=(1, 2, 3))


def torch_budget_loop(x, noise, sched, ksize):
    """generate_blurimages in torch: per image, sigma downwards until the MSE (read on the host) fits."""
    out = []
    for b in range(x.shape[0]):
        im = x[b:b + 1]
        k = 0
        while True:
            y, mse = torch_blur(im, torch_kernel(ksize, sched[k], x.device))
            if not float(mse) > noise * 1.01 or k + 1 == len(sched):
                break
            k += 1
        out.append(k)
    return out


def smooth_batch(B, H, W, dev, grid=4):
    g = torch.Generator().manual_seed(0)
    low = torch.rand((B, 3, H // grid, W // grid), generator=g)
    return F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1).to(dev).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--noise", type=float, default=1e-4)
    ap.add_argument("--skip-loop", action="store_true", help="skip the torch reference loop (minutes of launches)")
    args = ap.parse_args()
    from imagecompression_adversarial_amd import degrade
    from imagecompression_adversarial_amd._lib import lib, ptr, stream
    dev = torch.device("cuda:0")
    out = {"reps": args.reps, "sweep_chunk": lib().ica_blur_sweep_chunk()}
    g = torch.Generator(device=dev).manual_seed(0)
    for tag, shape in (("32x512x768", (32, 3, 512, 768)), ("4x2048x2048", (4, 3, 2048, 2048))):
        x = torch.rand(shape, generator=g, device=dev)
        w = torch_kernel((5, 9), 0.5, dev)
        got, mse = degrade.gaussian_blur(x, (5, 9), 0.5, clamp=True, ref=x)
        ref, mse_t = torch_blur(x, w)
        out[f"blur_{tag}_max_diff_vs_torch"] = float((got - ref).abs().max())
        assert out[f"blur_{tag}_max_diff_vs_torch"] < 1e-4 and float(((mse - mse_t).abs() / mse_t).max()) < 1e-4
        t = timed(lambda: degrade.gaussian_blur(x, (5, 9), 0.5, clamp=True, ref=x), args.reps, args.warmup)
        nbytes = 2 * x.numel() * 4
        t["GBps"] = round(nbytes / (t["median"] * 1e-3) / 1e9, 1)
        t["floor_frac"] = round(nbytes / HBM_COPY_BPS / (t["median"] * 1e-3), 3)
        out[f"blur_{tag}_ms"] = t
        # the launches alone (taps, output and workspace prepared): 10 calls of the C entry between two events
        wx = degrade.gaussian_taps(5, 0.5).repeat(shape[0], 1).to(dev)
        wy = degrade.gaussian_taps(9, 0.5).repeat(shape[0], 1).to(dev)
        B, _, H, W = shape
        ws = torch.empty(lib().ica_gauss_blur_ws_size(B, H, W), device=dev)

        def launches():
            for _ in range(10):
                assert lib().ica_gauss_blur(ptr(x), ptr(wx), ptr(wy), B, H, W, 5, 9, 1, ptr(x), ptr(got), ptr(mse),
                                            ptr(ws), stream()) == 0
        k = timed(launches, args.reps, args.warmup)
        k = {n: round(v / 10, 4) for n, v in k.items()}
        k["GBps"] = round(nbytes / (k["median"] * 1e-3) / 1e9, 1)
        k["floor_frac"] = round(nbytes / HBM_COPY_BPS / (k["median"] * 1e-3), 3)
        out[f"blur_launch_{tag}_ms"] = k
        out[f"blur_torch_{tag}_ms"] = timed(lambda: torch_blur(x, w), args.reps, args.warmup)
        del x, got, ref
    B, H, W = 32, 512, 768
    x = smooth_batch(B, H, W, dev)
    sched = degrade.sigma_schedule()
    blurred, sigma, index, mse = degrade.blur_to_budget(x, args.noise)
    ks = index.tolist()
    out["budget_index_min_max"] = [min(ks), max(ks)]
    out["budget_ms"] = timed(lambda: degrade.blur_to_budget(x, args.noise), args.reps, args.warmup)
    sweep = timed(lambda: degrade.blur_sweep(x, sched, args.noise), args.reps, args.warmup)
    chunk = out["sweep_chunk"]
    evaluated = sum(min((k // chunk + 1) * chunk, len(sched)) for k in ks)      # candidates scored, over the batch
    fmas = 3 * H * W * 25 * evaluated
    sweep["fmas"] = fmas
    sweep["fma_frac"] = round(fmas / FMA_PEAK / (sweep["median"] * 1e-3), 3)
    out["sweep_ms"] = sweep
    if not args.skip_loop:
        ref_ks = torch_budget_loop(x, args.noise, sched, (5, 5))
        out["budget_same_index"] = sum(int(a == b) for a, b in zip(ks, ref_ks))
        for b, (a, r) in enumerate(zip(ks, ref_ks)):
            if a != r:      # fp32 reductions in another order: only a candidate at the budget can differ
                m = float(torch_blur(x[b:b + 1], torch_kernel((5, 5), sched[min(a, r)], dev))[1])
                assert abs(m - 1.01 * args.noise) < 1e-3 * args.noise, (b, a, r, m)
        out["budget_torch_ms"] = timed(lambda: torch_budget_loop(x, args.noise, sched, (5, 5)), args.loop_reps, 0)
        out["budget_torch_ms"]["reps"] = args.loop_reps
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
