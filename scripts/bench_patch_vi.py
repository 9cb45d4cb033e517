"""Time of the patch-wise VI localisation against its two baselines, same process, HIP events.

    python scripts/bench_patch_vi.py [--batch 32 --height 512 --width 768 --reps 30 --warmup 3]

Prints one JSON line with the median (and min / max) of --reps single calls, in ms:
  local_vi / worst_patches   the HIP path (patch_vi.local_vi; worst_patches with its pos, i.e. the gather alone)
  torch                      the torch composition on the GPU: squared differences, channel sum, avg_pool2d(64, 2),
                             divide, border masking, argmax, slicing of the four patches
  eval_forward               the codec's eval forward that precedes the localisation (hyper, --precision)
and checks that both paths picked windows of (nearly) equal vi.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def torch_composition(im_adv, out_adv, im_s, out_s, win, stride, border):
    n = 3 * win * win
    mse_in = F.avg_pool2d(((im_s - im_adv) ** 2).sum(1, keepdim=True), win, stride)[:, 0] * (win * win / n)
    mse_out = F.avg_pool2d(((out_s - out_adv) ** 2).sum(1, keepdim=True), win, stride)[:, 0] * (win * win / n)
    vi = torch.where(mse_in > 0, mse_out / mse_in, torch.zeros_like(mse_out))
    if border > 0:
        vi[:, :border] = 0
        vi[:, -border:] = 0
        vi[:, :, :border] = 0
        vi[:, :, -border:] = 0
    B, nh, nw = vi.shape
    val, idx = vi.reshape(B, -1).max(1)
    pos = torch.stack([idx // nw, idx % nw], 1)
    patches = []
    for b, (r, c) in enumerate(pos.tolist()):      # the slicing needs the position on the host
        y, x = r * stride, c * stride
        patches.append(torch.stack([t[b, :, y:y + win, x:x + win] for t in (im_adv, out_adv, im_s, out_s)]))
    return vi, val, pos, torch.stack(patches)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--quality", type=int, default=3)
    ap.add_argument("--precision", default="x6", choices=("fp32", "x6", "bf16"))
    ap.add_argument("--win", type=int, default=64)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--border", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from imagecompression_adversarial_amd import codec as models
    from imagecompression_adversarial_amd import patch_vi
    from imagecompression_adversarial_amd.attack import eval_forward
    from imagecompression_adversarial_amd.engine import CodecKernels
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = models.bmshj2018_hyperprior(args.quality)
    kern = CodecKernels({k: v.detach().to(dev) for k, v in net.state_dict().items()}, "hyper",
                        precision=args.precision)
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (args.batch, 3, args.height, args.width)
    im_s = torch.rand(shape, generator=g, device=dev)
    im_adv = (im_s + 1e-2 * torch.randn(shape, generator=g, device=dev)).clamp(0, 1)
    out_s = (im_s + 2e-2 * torch.randn(shape, generator=g, device=dev)).clamp(0, 1)
    out_adv = (out_s + 3e-2 * torch.randn(shape, generator=g, device=dev)).clamp(0, 1)
    t = (im_adv, out_adv, im_s, out_s)
    kw = dict(win=args.win, stride=args.stride, border=args.border)
    lv = patch_vi.local_vi(*t, **kw)
    vi, val, pos, patches = torch_composition(*t, **kw)
    # same windows up to fp32 rounding of nearly tied maxima: compare the values the two paths found
    rel = float(((lv.val - val).abs() / val).max())
    assert rel < 1e-4, rel
    out = {"shape": list(shape), "win": args.win, "stride": args.stride, "border": args.border, "reps": args.reps,
           "input_MB": round(4 * im_s.numel() * 4 / 1e6, 1), "argmax_rel_diff": rel,
           "same_pos": bool(torch.equal(lv.pos.long(), pos))}
    out["local_vi_ms"] = timed(lambda: patch_vi.local_vi(*t, **kw), args.reps, args.warmup)
    out["worst_patches_ms"] = timed(lambda: patch_vi.worst_patches(*t, pos=lv.pos, **kw), args.reps, args.warmup)
    out["local_vi_plus_patches_ms"] = timed(
        lambda: patch_vi.worst_patches(*t, pos=patch_vi.local_vi(*t, **kw).pos, **kw), args.reps, args.warmup)
    out["torch_ms"] = timed(lambda: torch_composition(*t, **kw), args.reps, args.warmup)
    out["eval_forward_ms"] = timed(lambda: eval_forward(kern, im_adv), args.reps, args.warmup)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
