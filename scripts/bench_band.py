"""Time of the band kernels (ica_band.hip) and of one band-limited attack step next to one plain attack step, same
process, HIP events.

    python scripts/bench_band.py [--reps 10 --warmup 2 --batch 32 --hw 512 768 --bands 0-2]

Prints one JSON line, times in ms (median / min / max of single calls), hyper q3 (seeded weights), x6 operands, 32
images of 768x512 by default:
  copy         torch's device-to-device copy of the batch, the yardstick of scripts/bw_probe.py: GBps = 2 x bytes / t
  split        ica_band_split alone, 8 `only` variants of the batch, outputs and workspace prepared; GBps = the bytes
               it must move (im_s and im_adv read once, 8 images written) / median
  energies     ica_band_split with out == NULL (two reads, no image written)
  project      ica_band_project alone (one read, one write)
  prologue / adam   the two fused step kernels alone, against ica_attack_prologue_ex / ica_attack_adam_ex on the same
               buffers (plain_prologue / plain_adam)
  band_step / plain_step   BandAttackLoop.step and AttackLoop.step, every image on the expensive branch, after the
               graph of the network step has been captured
Read them with the clock state of the run (`rocm-smi --showclocks`) beside them.
"""
import argparse
import json
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


def with_rate(t, nbytes):
    t["GBps"] = round(nbytes / (t["median"] * 1e-3) / 1e9, 1)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, nargs=2, default=(512, 768))
    ap.add_argument("--quality", type=int, default=3)
    ap.add_argument("--bands", type=str, default="0-2")
    args = ap.parse_args()
    import ctypes as C
    from imagecompression_adversarial_amd import band_vi as BV, coder, hip_ops as K
    from imagecompression_adversarial_amd._lib import lib, ptr, stream
    from imagecompression_adversarial_amd.attack import AttackLoop
    dev = torch.device("cuda:0")
    H, W = args.hw
    B, V = args.batch, 8
    mask = BV.parse_bands(args.bands)
    out = {"reps": args.reps, "B": B, "H": H, "W": W, "quality": args.quality, "bands": args.bands}
    g = torch.Generator(device=dev).manual_seed(0)
    im_s = torch.rand((B, 3, H, W), generator=g, device=dev)
    im_adv = torch.clamp(im_s + 0.02 * torch.randn((B, 3, H, W), generator=g, device=dev), 0.0, 1.0)
    img = B * 3 * H * W * 4
    L, st = lib(), stream()
    reps = 3 * args.reps

    dst = torch.empty_like(im_s)
    out["copy_ms"] = with_rate(timed(lambda: dst.copy_(im_s), reps, args.warmup), 2 * img)

    x = torch.empty((V * B, 3, H, W), device=dev)
    energy, mse = torch.empty((B, 8), device=dev), torch.empty((V, B), device=dev)
    ws = torch.empty(L.ica_band_split_ws_size(V, B, H, W), device=dev)
    masks = (C.c_int * V)(*BV.preset_masks("only"))

    def split(images=True):
        assert L.ica_band_split(ptr(im_s), ptr(im_adv), masks, V, B, H, W, ptr(x) if images else None, ptr(energy),
                                ptr(mse) if images else None, ptr(ws), st) == 0
    out["split_ms"] = with_rate(timed(split, reps, args.warmup), (2 + V) * img)
    out["energies_ms"] = with_rate(timed(lambda: split(False), reps, args.warmup), 2 * img)

    def project():
        assert L.ica_band_project(ptr(im_adv), mask, B, H, W, ptr(dst), st) == 0
    out["project_ms"] = with_rate(timed(project, reps, args.warmup), 2 * img)

    # the step kernels alone, on buffers of their own
    noise = 0.03 * torch.randn((B, 3, H, W), generator=g, device=dev)
    m, v = torch.zeros_like(noise), torch.zeros_like(noise)
    im_in4, g4 = K.empty_nc4(B, 3, H, W, dev), K.empty_nc4(B, 3, H, W, dev).normal_(0.0, 1e-3)
    loss_i = torch.zeros(B, device=dev)            # 0 <= thr: every image reads the network gradient
    part = torch.empty(B * K.blocks_per_image(), device=dev)
    wsp = torch.empty(L.ica_band_prologue_ws_size(B, H, W), device=dev)
    eps, invN = 16.0 / 255.0, 1.0 / (3 * H * W)
    sc = (eps, 1e-4, invN, 0.0316, -0.1)

    def prologue():
        assert L.ica_band_prologue(ptr(noise), ptr(im_s), ptr(im_in4), ptr(loss_i), B, H, W, eps, mask, ptr(wsp),
                                   st) == 0

    def plain_prologue():
        assert L.ica_attack_prologue_ex(ptr(noise), ptr(im_s), ptr(im_in4), ptr(part), B, H, W, eps, 1, st) == 0
    out["prologue_ms"] = with_rate(timed(prologue, reps, args.warmup), (2 + 4 / 3) * img)
    out["plain_prologue_ms"] = with_rate(timed(plain_prologue, reps, args.warmup), (2 + 4 / 3) * img)
    loss_i.zero_()

    def adam():
        assert L.ica_band_adam(ptr(noise), ptr(im_s), ptr(g4), ptr(loss_i), ptr(m), ptr(v), None, B, H, W, *sc, None,
                               None, None, mask, st) == 0

    def plain_adam():
        assert L.ica_attack_adam_ex(ptr(noise), ptr(im_s), ptr(g4), ptr(loss_i), None, ptr(m), ptr(v), None, B, H, W,
                                    *sc, None, None, None, 1, st) == 0
    step_bytes = (4 + 4 / 3 + 3) * img             # noise, im_s, m, v and the gradient read; noise, m, v written
    out["adam_ms"] = with_rate(timed(adam, reps, args.warmup), step_bytes)
    out["plain_adam_ms"] = with_rate(timed(plain_adam, reps, args.warmup), step_bytes)

    # one whole step of each loop (thr = 1: no image ever leaves the expensive branch)
    cargs = coder.config().parse_args(["-m", "hyper", "-metric", "mse", "-q", str(args.quality),
                                       "--synthetic-weights"])
    net = coder.load_model(cargs, training=False).to(dev)
    kern = net.kernels(net.attack_precision(None))
    for name, loop in (("band_step_ms", BV.BandAttackLoop(kern, im_s, mask, steps=1001, noise_thr=1.0)),
                       ("plain_step_ms", AttackLoop(kern, im_s, steps=1001, noise_thr=1.0))):
        it = iter(range(1001))
        out[name] = timed(lambda: loop.step(next(it)), args.reps, max(args.warmup, 3))
        out[name]["graph_replays"] = loop.graph_replays
    out["step_extra_ms"] = round(out["band_step_ms"]["median"] - out["plain_step_ms"]["median"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
