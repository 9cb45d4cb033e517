"""The layer study (layer_study.layer_compare) at hyper q3, 8 x 768x512: its three reduction launches next to the same
rows composed from torch ops on the same tensors, and next to the two batched forwards that produce the tensors.
HIP events, warm-ups, median with min-max.

    python scripts/bench_layer_compare.py [--batch 8 --height 512 --width 768 --warmup 5 --calls 20 --out FILE]

  reductions  hip_ops.layer_sums x 3 (encoder pair table, quant, decoder triple table), each + ica_reduce_rows
  composed    ((a - b) ** 2).flatten(1).sum(1) per layer and column, torch.round for the quant row
  forwards    g_a of the 2B batch and g_s of the 3B batch, module outputs kept (with the bias-epilogue reruns)
"""
import argparse
import contextlib
import io
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from scripts.bench_rdeval import stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_layer_compare needs a HIP device")
    from imagecompression_adversarial_amd import coder, hip_ops as K, layer_study as LS
    args = coder.config().parse_args(["-m", "hyper", "-q", "3", "--synthetic-weights", "--precision", "x6"])
    with contextlib.redirect_stdout(io.StringIO()):
        net = coder.load_model(args, training=False).to(args.device)
    kern = net.kernels("x6")
    B, H, W = a.batch, a.height, a.width
    g = torch.Generator().manual_seed(0)
    im = torch.rand((B, 3, H, W), generator=g).to(args.device)
    adv = torch.clamp(im + (torch.rand((B, 3, H, W), generator=g).to(args.device) * 2 - 1) * 4 / 255, 0, 1)

    def forwards():
        enc = LS._analysis_acts(kern.ga, K.to_nc4(torch.cat((adv, im), 0)))
        y = enc[-1].t
        y3 = torch.cat((y[:B], K.round_(y)), 0)
        return enc, LS._synthesis_acts(kern.gs, y3)

    enc, dec = forwards()
    y = enc[-1].t
    enc_l = [(K.LAYER_PAIR, t.C, *LS._parts(t, 2, B)) for t in enc]
    dec_l = [(K.LAYER_TRIPLE, t.C, *LS._parts(t, 3, B)) for t in dec]
    quant_l = [(K.LAYER_QUANT, kern.M, y[:B], y[B:])]

    def reductions():
        return K.layer_sums(enc_l, B), K.layer_sums(quant_l, B), K.layer_sums(dec_l, B)

    def ssd(u, v):
        return ((u - v) ** 2).flatten(1).sum(1)

    def composed():
        e = [ssd(u, v) for _, _, u, v in enc_l]
        ra, rc = torch.round(y[:B]), torch.round(y[B:])
        q = (ssd(y[:B], rc), ssd(ra, rc))
        d = [(ssd(u, w), ssd(v, w)) for _, _, u, v, w in dec_l]
        return e, q, d

    for _ in range(a.warmup):
        r, c = reductions(), composed()
    torch.cuda.synchronize()
    # padding lanes are zero in the engine's tensors, so the torch sums over all four lanes are the same sums
    agree = max(float(((r[0][k, :, 0] - c[0][k]).abs() / c[0][k]).max()) for k in range(len(enc_l)))
    tr, tc = [], []
    for _ in range(a.calls):
        tr.append(timed(reductions)[0])
        tc.append(timed(composed)[0])
    tf = [timed(forwards)[0] for _ in range(max(a.calls // 4, 3))]
    mb = sum(t.t.numel() * 4 for t in enc + dec) / 2 ** 20
    lines = [
        f"hyper q3, {B} x {W}x{H}, precision x6, {a.calls} calls after {a.warmup} warm-ups, HIP events",
        f"reductions (3 x ica_layer_sums + ica_reduce_rows, {len(enc_l)} + 1 + {len(dec_l)} layers): {stats(tr)}",
        f"composed   (torch sub / pow / sum per layer and column, torch.round): {stats(tc)}",
        f"forwards   (g_a of {2 * B} images, g_s of {3 * B}, with the 6 bias-epilogue reruns): {stats(tf)}",
        f"activations read by the reductions: {mb:.0f} MiB",
        f"largest relative difference reductions vs composed, encoder rows: {agree:.1e}",
    ]
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
