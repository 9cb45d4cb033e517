"""CPU restatement of recompression.py's generation step and metrics: the oracle of tests/test_cpu_recompress.py and
tests/test_gpu_recompress.py.

write_array / read_array   coder.py:41-48 and :23-38 on arrays, literally: np.round(float32 x * 255.0).astype(uint8),
                           then uint8 / 255.0 (float64) stored into a float32 array
roundtrip / roundtrip_png  clamp -> write -> read, in memory and through a real PNG (Pillow)
requant                    what ica_requant8 returns, from a planar x_hat: codes, next input, clamp(x_hat), the sums
eval_metrics               RateDistortionLoss(training=False) + PSNR in float64 (train.py:50-72, utils/metrics.py:7-11)
oracle_generation          one generation on the CPU oracle: codec.forward of the decoded codes
"""
import io
import math

import numpy as np
import torch

LIK_FLOOR = 1.0 / 65536


def write_array(x):
    """[3, H, W] float32 in [0, 1] -> [H, W, 3] uint8, as coder.write_image computes it."""
    x = np.round(x.astype(np.float32) * 255.0)
    return x.astype("uint8").transpose(1, 2, 0)


def read_array(u8):
    """[H, W, 3] uint8 -> [3, H, W] float32, as coder.read_image computes it (no padding: sizes are multiples of 64)."""
    img = np.array(u8) / 255.0
    im = np.zeros(img.shape, dtype="float32")
    im[:, :, :3] = img[:, :, :3]
    return im.transpose(2, 0, 1)


def clamp01(x):
    """torch.clamp(x, 0, 1) of a float32 tensor; a NaN becomes 0, the kernel's documented choice."""
    return torch.nan_to_num(x, nan=0.0).clamp(0.0, 1.0)


def roundtrip(x):
    """[B, 3, H, W] float32 (any range) -> (uint8 [B, H, W, 3], float32 [B, 3, H, W]): code()'s clamp, then the
    write and the read."""
    c = clamp01(x).numpy()
    u8 = np.stack([write_array(c[b]) for b in range(c.shape[0])])
    return u8, torch.from_numpy(np.stack([read_array(u) for u in u8]))


def roundtrip_png(x):
    """The same through a real PNG file image, in memory."""
    from PIL import Image
    c = clamp01(x).numpy()
    u8s, ims = [], []
    for b in range(c.shape[0]):
        buf = io.BytesIO()
        Image.fromarray(write_array(c[b])).save(buf, format="PNG")
        buf.seek(0)
        u8 = np.array(Image.open(buf))
        u8s.append(u8)
        ims.append(read_array(u8))
    return np.stack(u8s), torch.from_numpy(np.stack(ims))


def pack(u8):
    """uint8 [B, H, W, 3] -> int32 [B, H, W] codes r | g << 8 | b << 16."""
    u = torch.from_numpy(np.ascontiguousarray(u8)).to(torch.int32)
    return u[..., 0] | (u[..., 1] << 8) | (u[..., 2] << 16)


def unpack(q):
    """int32 [B, H, W] -> int64 [B, 3, H, W] code values."""
    q = q.to(torch.int64)
    return torch.stack([(q >> s) & 255 for s in (0, 8, 16)], 1)


def decode(q):
    """codes -> the float32 image a read of their PNG gives."""
    return (unpack(q).double() / 255.0).float()


def to_nc4(x, dead=0.0):
    """planar [B, 3, H, W] -> nChw4c [B, 1, H, W, 4] with ``dead`` (a number or a [B, H, W] tensor) in lane 3."""
    B, _, H, W = x.shape
    x4 = torch.empty((B, 1, H, W, 4), dtype=torch.float32)
    x4[:, 0, :, :, :3] = x.permute(0, 2, 3, 1)
    x4[:, 0, :, :, 3] = dead
    return x4


def requant(x_hat, orig, prev_q):
    """ica_requant8 restated: dict of q (int32 [B, H, W]), next (planar float32), out (clamp(x_hat)), sse_orig,
    sse_gen (float64 [B]) and changed (int64 [B])."""
    u8, nxt = roundtrip(x_hat)
    q = pack(u8)
    out = clamp01(x_hat)
    dq = unpack(q) - unpack(prev_q)
    return {"q": q, "next": nxt, "out": out,
            "sse_orig": ((out.double() - orig.double()) ** 2).sum(dim=(1, 2, 3)),
            "sse_gen": ((dq.double() / 255.0) ** 2).sum(dim=(1, 2, 3)),
            "changed": (dq != 0).sum(dim=(1, 2, 3))}


def floor_bits(lik, floor=LIK_FLOOR):
    """[B, C, H, W] likelihoods -> float64 [B]: sum log(max(p, floor))."""
    return torch.log(lik.double().clamp(min=floor)).sum(dim=(1, 2, 3))


def eval_metrics(x_hat, likelihoods, im_ori):
    """Per image (bpp, psnr) in float64: bpp = sum log(max(p, 2^-16)) / (-ln 2 H W), psnr = 10 log10(1 / mse) on
    clamp(x_hat)."""
    B, _, H, W = im_ori.shape
    bits = sum(floor_bits(l) for l in likelihoods.values())
    bpp = bits / (-math.log(2) * H * W)
    mse = ((clamp01(x_hat).double() - im_ori.double()) ** 2).mean(dim=(1, 2, 3))
    return [(float(bpp[b]), 10.0 * math.log10(1.0 / float(mse[b]))) for b in range(B)]


def oracle_generation(P, q_in, im_ori, model="hyper"):
    """One generation on the CPU oracle from the codes it consumes: (x_hat, [(bpp, psnr)] per image)."""
    from oracle import codec
    with torch.no_grad():
        res = codec.forward(P, decode(q_in), model)
    return res["x_hat"], eval_metrics(res["x_hat"], res["likelihoods"], im_ori)


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def exact_halfway_values():
    """float32 values v whose float32 product v * 255 is exactly k + 0.5: the ties np.round sends to the even code.
    For every k the floats around (k + 0.5) / 255 are searched."""
    out = []
    for k in range(255):
        v = np.float32((k + 0.5) / 255.0)
        cands = [v]
        for _ in range(3):
            cands = [np.nextafter(cands[0], np.float32(-1)), *cands, np.nextafter(cands[-1], np.float32(2))]
        for c in cands:
            if np.float32(c) * np.float32(255.0) == np.float32(k + 0.5):
                out.append(float(c))
                break
    return out


def kernel_case(B, H, W, seed):
    """(x_hat planar [B, 3, H, W] in [-0.5, 1.5] with pinned rows, orig, prev_q, the number of exact half-way values):
    row 0 of every plane holds 0 and 1, row 1 the codes k / 255, rows 2.. the exact ties, as many as fit."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, 3, H, W), generator=g) * 2.0 - 0.5
    orig = torch.rand((B, 3, H, W), generator=g)
    prev = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.int32).numpy().astype("uint8")
    ties = torch.tensor(exact_halfway_values(), dtype=torch.float32)
    codes = (torch.arange(256).double() / 255.0).float()
    flat = x.view(B, 3, H * W)
    flat[:, :, 0:W:2] = 0.0
    flat[:, :, 1:W:2] = 1.0
    n = min(256, H * W - W)
    flat[:, :, W:W + n] = codes[:n]
    m = min(len(ties), H * W - W - n)
    flat[:, :, W + n:W + n + m] = ties[:m]
    # a third of the pixels keep their previous code in at least one channel: changed is not simply 3 H W
    u8, _ = roundtrip(x)
    keep = torch.rand((B, H, W), generator=g) < 0.33
    prev[keep.numpy()] = u8[keep.numpy()]
    return x, orig, pack(prev), m


def rand_image(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g)
