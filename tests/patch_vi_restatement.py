"""float64 CPU restatement of the patch-wise VI localisation (psnr_partial, attack_patch.py:119-146) and the pinned
inputs of tests/test_gpu_patch_vi.py.

The reference unfolds each of the four images into every 64x64 window at stride 2 (in fp16), takes the mean of
the squared differences per window, divides, blanks a 10-window border and takes the worst window with two
torch.max calls.  Two restatements of that description, both our own text:

  local_vi         squared differences, channel sum, avg_pool2d(win, stride): float64, any batch
  local_vi_unfold  the literal F.unfold form (without the .half()), one image, for tiny shapes only

Windows with mse_in == 0 are excluded (vi = 0) in both; the reference would give inf / NaN there.
"""
import functools

import torch
import torch.nn.functional as F


def map_shape(H, W, win, stride):
    return (H - win) // stride + 1, (W - win) // stride + 1


def blank_border(vi, border):
    """attack_patch.py:137-140 on [..., nh, nw] (a border of 0 blanks nothing)."""
    if border > 0:
        vi[..., :border, :] = 0
        vi[..., -border:, :] = 0
        vi[..., :, :border] = 0
        vi[..., :, -border:] = 0
    return vi


def window_means(a, b, win, stride):
    """mean over the 3 * win^2 window elements of (a - b)^2, float64: [B, nh, nw]."""
    d = (a.double() - b.double()) ** 2
    return F.avg_pool2d(d.sum(1, keepdim=True), win, stride)[:, 0] / 3.0


def first_argmax(vi):
    """(val [B], pos [B, 2]) of the first row-major maximum of [B, nh, nw]: what the reference's max over dim 1
    then dim 0 returns (torch.max returns the first index of a maximum)."""
    B, nh, nw = vi.shape
    vals, poss = [], []
    for b in range(B):
        flat = vi[b].reshape(-1)
        m = flat.max()
        i = int((flat == m).nonzero()[0, 0])
        vals.append(m)
        poss.append((i // nw, i % nw))
    return torch.stack(vals), torch.tensor(poss, dtype=torch.int32)


def local_vi(im_adv, out_adv, im_s, out_s, win=64, stride=2, border=10):
    """dict of float64 mse_in / mse_out / vi [B, nh, nw], val [B], pos [B, 2] and the exclusion mask."""
    mse_in = window_means(im_s, im_adv, win, stride)
    mse_out = window_means(out_s, out_adv, win, stride)
    zero = mse_in == 0
    vi = torch.where(zero, torch.zeros_like(mse_out), mse_out / torch.where(zero, torch.ones_like(mse_in), mse_in))
    vi = blank_border(vi, border)
    excluded = zero | (blank_border(torch.ones_like(vi), border) == 0)
    val, pos = first_argmax(vi)
    return {"mse_in": mse_in, "mse_out": mse_out, "vi": vi, "val": val, "pos": pos, "excluded": excluded}


def local_vi_unfold(im_adv, out_adv, im_s, out_s, win=64, stride=2, border=10):
    """The unfold formulation for one image [1, 3, H, W] in float64: (mse_in, mse_out, vi [nh, nw], (row, col),
    the four patches adv, outadv, s, outs each [1, 3, win, win])."""
    assert im_adv.shape[0] == 1
    H, W = im_adv.shape[2:]
    nh, nw = map_shape(H, W, win, stride)
    cols = [F.unfold(t.double(), win, stride=stride) for t in (im_adv, out_adv, im_s, out_s)]   # [1, 3 win^2, L]
    p_adv, p_outadv, p_s, p_outs = cols
    mse_out = torch.mean((p_outs - p_outadv) ** 2, dim=1).view(nh, nw)
    mse_in = torch.mean((p_s - p_adv) ** 2, dim=1).view(nh, nw)
    zero = mse_in == 0
    vi = torch.where(zero, torch.zeros_like(mse_out), mse_out / torch.where(zero, torch.ones_like(mse_in), mse_in))
    vi = blank_border(vi, border)
    v, index_ = torch.max(vi, dim=1)
    v, index_h = torch.max(v, dim=0)
    row, col = int(index_h), int(index_[index_h])
    patches = [c.view(1, 3, win, win, nh, nw)[:, :, :, :, row, col] for c in cols]
    return mse_in, mse_out, vi, (row, col), patches


def slice_patches(tensors, pos, win, stride):
    """[B, 4, 3, win, win]: the four tensors sliced at pos * stride (same dtype as the inputs)."""
    out = []
    for b in range(tensors[0].shape[0]):
        y, x = int(pos[b][0]) * stride, int(pos[b][1]) * stride
        out.append(torch.stack([t[b, :, y:y + win, x:x + win] for t in tensors]))
    return torch.stack(out)


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def random_case(B, H, W, seed):
    """Unpinned inputs: an image, a ~1e-2 input perturbation, reconstructions with a ~3e-2 error whose amplitude
    varies smoothly over the image.  The worst window's margin over the runner-up can be tiny here."""
    g = torch.Generator().manual_seed(seed)
    im_s = torch.rand((B, 3, H, W), generator=g)
    im_adv = (im_s + 1e-2 * torch.randn((B, 3, H, W), generator=g)).clamp(0, 1)
    out_s = (im_s + 2e-2 * torch.randn((B, 3, H, W), generator=g)).clamp(0, 1)
    yy = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(0, 1, W).view(1, 1, 1, W)
    amp = 1.0 + torch.sin(3.0 * yy + seed) * torch.cos(2.0 * xx)
    out_adv = (out_s + 3e-2 * amp * torch.randn((B, 3, H, W), generator=g)).clamp(0, 1)
    return im_adv, out_adv, im_s, out_s


def planted_case(B, H, W, win, stride, border, seed):
    """Pinned, well-conditioned inputs: on top of random_case, image b gets one win x win block, exactly one
    window of the map (inside the border), where the input perturbation is 16 times smaller and the output error
    3 times larger.  Only that window covers the block fully, so its vi exceeds every other window's by far more
    than the 1e-3 relative that tests/test_cpu_patch_vi.py asks of a pinned case.  Returns the tensors and the
    planted positions [B, 2]."""
    im_adv, out_adv, im_s, out_s = random_case(B, H, W, seed)
    nh, nw = map_shape(H, W, win, stride)
    pos = []
    for b in range(B):
        lo_r, hi_r = min(border, (nh - 1) // 2), max(nh - 1 - border, (nh - 1) // 2)
        lo_c, hi_c = min(border, (nw - 1) // 2), max(nw - 1 - border, (nw - 1) // 2)
        r = lo_r + (7 * b + 3 + seed) % (hi_r - lo_r + 1)
        c = lo_c + (11 * b + 5 + seed) % (hi_c - lo_c + 1)
        y, x = r * stride, c * stride
        sl = (b, slice(None), slice(y, y + win), slice(x, x + win))
        im_adv[sl] = im_s[sl] + (im_adv[sl] - im_s[sl]) / 16.0
        out_adv[sl] = (out_s[sl] + 3.0 * (out_adv[sl] - out_s[sl])).clamp(0, 1)
        pos.append((r, c))
    return (im_adv, out_adv, im_s, out_s), torch.tensor(pos, dtype=torch.int32)


# (name, B, H, W, win, stride, border): the smallest shapes that take every path of the kernels: a map wider than
# one 64-column block and taller than one 32-row block, a second block row, a 1x1 map, every stride, and an H
# whose (H - win) the stride does not divide
PINNED = [
    ("b3_128x160", 3, 128, 160, 64, 2, 10),
    ("b2_192x128", 2, 192, 128, 64, 2, 10),
    ("noborder", 3, 128, 160, 64, 2, 0),
    ("win32_s4", 2, 128, 160, 32, 4, 0),
    ("stride1", 2, 72, 80, 64, 1, 2),
    ("h134_s4", 2, 134, 128, 64, 4, 0),
]


@functools.lru_cache(maxsize=None)
def pinned(name):
    """(tensors, planted pos, float64 oracle) of one PINNED case; computed once and shared (do not modify)."""
    _, B, H, W, win, stride, border = next(c for c in PINNED if c[0] == name)
    tensors, pos = planted_case(B, H, W, win, stride, border, seed=sum(map(ord, name)) % 97)
    return tensors, pos, local_vi(*tensors, win=win, stride=stride, border=border)


def margin(vi_b):
    """(top1 - top2) / top1 of one image's map."""
    top = vi_b.reshape(-1).topk(2)[0]
    return float((top[0] - top[1]) / top[0])
