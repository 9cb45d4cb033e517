"""Times ica_jpeg_roundtrip, ica_jpeg_roundtrip_bwd (both surrogates) and one chunk of ica_jpeg_sweep on B x 3 x H x W (default 32 x 768 x 512, Kodak's size) with
device events around ``--reps`` back-to-back calls (default 5000: a timed window of about half a second for the round
trip, two for the sweep chunk) after a warm-up, and prints one JSON line.

    python scripts/bench_jpeg.py [--batch 32] [--height 512] [--width 768] [--reps 5000]

traffic_bytes is what the two passes of a call move by construction (DESIGN.md "JPEG round trip"): the fp32 image in
and out, the fused MSE's read of ref, and the byte planes written once and read once; gbps = traffic / time.  The
sweep chunk reads x twice (once per pass) and moves the byte planes of its 8 candidates.  The backward is three
passes: the forward's block pass (x in, byte planes out), the colour transpose (g and the byte planes in, the fp32
gradient planes out: 4 B/px of Y and 2 B/px (4:2:0) or 8 B/px (4:4:4) of chroma) and the block transpose (x and the
gradient planes in, g_x out).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5000)
    args = ap.parse_args()
    from imagecompression_adversarial_amd import degrade
    from imagecompression_adversarial_amd._lib import call, lib, ptr, stream
    if not torch.cuda.is_available():
        raise RuntimeError("bench_jpeg.py times kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    B, H, W = args.batch, args.height, args.width
    g = torch.Generator().manual_seed(0)
    x = (torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255).to(dev)
    px = B * H * W
    out = {"shape": [B, 3, H, W], "reps": args.reps}
    for sub, plane in (("420", 1.5), ("444", 3.0)):
        s = int(sub)
        tabs = degrade._jpeg_tabs((50,) * B, str(dev))
        o = torch.empty_like(x)
        mse = torch.empty(B, device=dev)
        ws = torch.empty(lib().ica_jpeg_roundtrip_ws_size(B, H, W, s), device=dev)
        t = timed(lambda: call("ica_jpeg_roundtrip", ptr(x), ptr(tabs), B, H, W, s, None, ptr(o), None, ptr(ws),
                               stream()), args.reps)
        traffic = px * (12 + 12 + 2 * plane)
        out["roundtrip_" + sub] = {"ms": t * 1e3, "traffic_bytes": traffic, "gbps": traffic / t / 1e9}
        t = timed(lambda: call("ica_jpeg_roundtrip", ptr(x), ptr(tabs), B, H, W, s, ptr(x), ptr(o), ptr(mse), ptr(ws),
                               stream()), args.reps)
        traffic = px * (12 + 12 + 12 + 2 * plane)
        out["roundtrip_mse_" + sub] = {"ms": t * 1e3, "traffic_bytes": traffic, "gbps": traffic / t / 1e9}
        gout, gx = torch.randn(x.shape, generator=g).to(dev), torch.empty_like(x)
        wsb = torch.empty(lib().ica_jpeg_roundtrip_bwd_ws_size(B, H, W, s), device=dev)
        gplanes = 4 + (2 if sub == "420" else 8)
        traffic = px * ((12 + plane) + (12 + plane + gplanes) + (12 + gplanes + 12))
        for k, name in enumerate(degrade.JPEG_SURROGATES):
            t = timed(lambda: call("ica_jpeg_roundtrip_bwd", ptr(x), ptr(tabs), ptr(gout), B, H, W, s, k, ptr(gx),
                                   ptr(wsb), stream()), args.reps)
            out[f"bwd_{name}_{sub}"] = {"ms": t * 1e3, "traffic_bytes": traffic, "gbps": traffic / t / 1e9}
        S = lib().ica_jpeg_sweep_chunk()
        all_tabs = degrade._jpeg_tabs(tuple(range(1, 101)), str(dev))
        msew = torch.empty((B, 100), device=dev)
        idx = torch.full((B,), -1, dtype=torch.int32, device=dev)
        done = torch.zeros(B, dtype=torch.int32, device=dev)
        rem = torch.empty(1, dtype=torch.int32, device=dev)
        wss = torch.empty(lib().ica_jpeg_sweep_ws_size(B, H, W, s), device=dev)

        def chunk():   # budget 0: nothing fits, so every image stays in the sweep
            call("ica_jpeg_sweep", ptr(x), ptr(all_tabs[40:]), S, B, H, W, s, 0.0, 40, ptr(msew), 100, ptr(idx),
                 ptr(done), ptr(rem), ptr(wss), stream())
        t = timed(chunk, args.reps)
        traffic = px * (12 + 12 + 2 * plane * S)
        out["sweep_chunk_" + sub] = {"candidates": S, "ms": t * 1e3, "traffic_bytes": traffic, "gbps": traffic / t / 1e9}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
