"""Step cost of the C&W search against the distortion attack's all-expensive step, same process, HIP events.

    python scripts/bench_cw.py [--batch 32 --height 512 --width 768 --steps 20 --warmup 3 --reps 3]

Prints one JSON line: ms per step of AttackLoop.step (noise_thr = 1: every image on the network branch) and of
CwAttackLoop.cw_step (level 1e9: no image gated, so the Adam pass reads the network gradient like AttackLoop's),
each the median of --reps timed windows of --steps steps, the two loops interleaved window by window.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--quality", type=int, default=3)
    ap.add_argument("--precision", default="x6", choices=("fp32", "x6", "bf16"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from imagecompression_adversarial_amd import codec as models
    from imagecompression_adversarial_amd.attack import AttackLoop
    from imagecompression_adversarial_amd.attack_cw import CwAttackLoop
    from imagecompression_adversarial_amd.engine import CodecKernels
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = models.bmshj2018_hyperprior(args.quality)
    kern = CodecKernels({k: v.detach().to(dev) for k, v in net.state_dict().items()}, "hyper",
                        precision=args.precision)
    im_s = torch.rand((args.batch, 3, args.height, args.width), generator=torch.Generator(device=dev).manual_seed(0),
                      device=dev)
    rd = AttackLoop(kern, im_s, steps=1001, noise_thr=1.0)
    cw = CwAttackLoop(kern, im_s, steps=1001, search_steps=1, max_level=1e9)
    n = {"rd": 0}

    def rd_step():
        rd.step(n["rd"])
        n["rd"] += 1

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    for _ in range(args.warmup):
        rd_step()
        cw.cw_step()
    torch.cuda.synchronize()
    t_rd, t_cw = [], []
    for _ in range(args.reps):
        t_rd.append(window(rd_step))
        t_cw.append(window(cw.cw_step))
    assert rd.sync_steps <= 1 and rd.expensive_image_steps() == args.batch * rd.steps_done
    assert all(c > 0 for c in cw.c_eff.tolist())   # no image gated: every Adam block read its network gradient
    ms_rd, ms_cw = statistics.median(t_rd), statistics.median(t_cw)
    print(json.dumps({"shape": [args.batch, 3, args.height, args.width], "precision": args.precision,
                      "steps": args.steps, "reps": args.reps, "attack_rd_step_ms": round(ms_rd, 3),
                      "cw_step_ms": round(ms_cw, 3), "cw_over_rd": round(ms_cw / ms_rd, 4),
                      "attack_rd_windows_ms": [round(t, 3) for t in t_rd],
                      "cw_windows_ms": [round(t, 3) for t in t_cw]}), flush=True)


if __name__ == "__main__":
    main()
