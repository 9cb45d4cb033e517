"""Restatement of the JPEG round trip's surrogate backward (DESIGN.md "JPEG round trip", "The attack through it") in
torch on the CPU, parametrised by dtype.  The forward is written again from the seven steps with three small
autograd.Functions in the place of the operations that have no gradient, and the vector-Jacobian product is what
autograd makes of it: nothing here is shared with imagecompression_adversarial_amd.degrade or ica_jpeg.hip.  From
tests/jpeg_restatement.py come the tables, the cases, the forward guards and ``fragile``.

    _Round   rint (or the forced decision)                       derivative 1
    _Clamp   clamp(r, lo, hi)                                    passes the gradient iff lo <= r <= hi (inclusive);
                                                                 applied to the rounded value, and to x itself in step 1
    _Quant   q * round-half-away(c / q) (or the forced decision) derivative d(r), r = c / q - round(c / q):
                                                                 1 ("ste") or 3 r^2 ("cubic")

Compared MCUs.  An MCU is left out of a comparison when it is fragile in the forward sense (a rounding decision within
its guard: the kernel may decide otherwise, and then masks and r differ), when a value before the roundings of step 4
or step 7 lies within that stage's guard of -0.5 or 255.5 (the boundaries of the clamp mask on the rounded value,
which the forward restatement treats as boundary-free), and, at 4:2:0, when one of its eight neighbours is left out:
its gradient reads the step-7 masks of pixels two columns or rows into them.  FRAGILE_MAX (10 %) is the ceiling of the
share per case, asserted on the CPU.  Measured shares: 0 everywhere except 48x80-444 3.3 % and 64x64x3-444 1.6 %; no
value of any case lies within its guard of -0.5 or 255.5.  64x64x3-420 is not a case here: counting neighbours takes
it from 6.2 % to 25 %.  batch-420 is two 32 x 48 images (2 x 3 MCUs each, so each has MCUs with a neighbour on every
side along one axis and the tile gather crosses MCU borders) at qualities (40, 70).

Tolerance.  measure_bwd() runs the restatement in fp32 with the float64 run's decisions forced, so that the two differ
by arithmetic alone, and takes |g_x(fp32) - g_x(float64)| / max |g_x(float64)| over the compared MCUs of each case
and surrogate, for the seeded normal field g of ``cotangent``.  MEASURED_BWD is the largest of them and GUARD_BWD is
4 x that (the factor of the forward guards: the kernel's freedom to order its sums).  Measured on the CPU
(tests/test_cpu_jpeg_bpda.py::test_guard_covers_the_measured_error re-measures them):

    ste     1.4e-07 .. 3.1e-07 in every case
    cubic   3.2e-07 .. 1.24e-06, and 2.92e-06 64x64x3-444, 3.74e-06 checker-444, 4.69e-06 checker-420;
            exactly 0 on both sides in the two constant cases
    MEASURED_BWD 4.7e-06, GUARD_BWD 1.88e-05

The DC coefficient.  Every coefficient of a constant block sits on an integer step, so under cubic its gradient is
exactly 0.  D X D^T does not show that: the rounding of its products leaves the DC 5.5e-14 steps off its integer in
float64 (1.5e-05 in fp32) and a residue on every AC coefficient.  _dct_blocks therefore takes the DC from its
definition, (sum - 64 * 128) / 8, and the AC coefficients from the block minus its mean, both exact on integer
samples; the levels stay exactly those of tests/jpeg_restatement.py in every case.
"""
import torch

from tests import jpeg_restatement as R

SURROGATES = ("ste", "cubic")
MEASURED_BWD = 4.7e-06
GUARD_BWD = 4 * MEASURED_BWD

_BATCH = "batch-420"
CASES = [n for n in R.CASES if n != "64x64x3-420"] + [_BATCH]


def case(name):
    """(x fp32 [B, 3, H, W], qualities, subsampling)."""
    if name == _BATCH:
        return R.level_image((2, 3, 32, 48), 11), [40, 70], "420"
    return R.case(name)


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, forced):
        return torch.round(f) if forced is None else forced.to(f.dtype).clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


class _Clamp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, lo, hi):
        ctx.save_for_backward((r >= lo) & (r <= hi))
        return r.clamp(lo, hi)

    @staticmethod
    def backward(ctx, g):
        (m,) = ctx.saved_tensors
        return g * m.to(g.dtype), None, None


class _Quant(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c, Q, forced, cubic):
        r = c / Q
        n = torch.sign(r) * torch.floor(r.abs() + 0.5) if forced is None else forced.to(c.dtype).clone()
        ctx.save_for_backward(3 * (r - n) ** 2 if cubic else torch.ones_like(r))
        ctx.mark_non_differentiable(n)
        return n * Q, n

    @staticmethod
    def backward(ctx, g, _):
        (d,) = ctx.saved_tensors
        return g * d, None, None, None


def _level(f, forced, pre, dec, key):
    r = _Round.apply(f, forced)
    pre[key], dec[key] = f.detach(), r.detach()
    return _Clamp.apply(r, 0.0, 255.0)


def _blocks(p):
    B, h, w = p.shape
    return p.reshape(B, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4)


def _unblocks(b):
    B, nh, nw = b.shape[:3]
    return b.permute(0, 1, 3, 2, 4).reshape(B, nh * 8, nw * 8)


def _dct_blocks(blk, D):
    """The orthonormal 8 x 8 DCT-II of blk - 128 with the DC coefficient taken from its definition, (sum - 64 * 128) / 8,
    and the AC coefficients from the block minus its mean.  A block's samples are integers (or quarters, after the box
    mean), so sum, mean and the differences are exact in fp32 and float64: a constant block has the exact coefficients
    (8 (c - 128), 0, ..., 0), where D X D^T leaves the rounding of its products on every one of them."""
    m = blk.mean(dim=(3, 4), keepdim=True)
    e00 = torch.zeros(8, 8, dtype=blk.dtype)
    e00[0, 0] = 1
    return (D @ (blk - m) @ D.T) * (1 - e00) + 8 * (m - 128) * e00


def _triangle(C, axis):
    """Doubles ``axis``: 3/4 of the nearest sample and 1/4 of the next one, the edge sample replicated."""
    n = C.shape[axis]
    o = torch.arange(2 * n)
    near = o // 2
    nxt = (near + torch.where(o % 2 == 1, 1, -1)).clamp(0, n - 1)
    return 0.75 * C.index_select(axis, near) + 0.25 * C.index_select(axis, nxt)


def forward(x, qualities, subsampling, surrogate, dtype=torch.float64, forced=None):
    """The round trip of x [B, 3, H, W] with the graph of the surrogate attached.  Returns a dict: x (the leaf), out
    (levels / 255 in ``dtype``), levels int64, pre {stage: the values before each rounding}, dec {stage: the rounded
    values, unclamped; coef_*: the rounded quotients}.  forced: the dec of another run, taken in the place of this
    run's own roundings."""
    assert surrogate in SURROGATES
    B, _, H, W = x.shape
    sub = subsampling == "420"
    f = (lambda k: None) if forced is None else (lambda k: forced[k])
    pre, dec = {}, {}
    leaf = x.detach().to(dtype).clone().requires_grad_(True)
    t = _Clamp.apply(leaf, 0.0, 1.0) * 255
    L = _Round.apply(t, f("s1"))
    pre["s1"], dec["s1"] = t.detach(), L.detach()
    Rd, G, Bl = L[:, 0], L[:, 1], L[:, 2]
    ycc = torch.stack([0.299 * Rd + 0.587 * G + 0.114 * Bl,
                       -0.168736 * Rd - 0.331264 * G + 0.5 * Bl + 128,
                       0.5 * Rd - 0.418688 * G - 0.081312 * Bl + 128], 1)
    P = _level(ycc, f("s2"), pre, dec, "s2")
    Y, C = P[:, 0], P[:, 1:]
    if sub:
        C = (C[:, :, 0::2, 0::2] + C[:, :, 0::2, 1::2] + C[:, :, 1::2, 0::2] + C[:, :, 1::2, 1::2]) / 4
    D = R.dct_matrix(dtype)
    tab = torch.tensor([R.tables(q) for q in qualities], dtype=dtype).reshape(B, 2, 1, 1, 8, 8)
    rec = []
    for name, p, Q in (("y", Y, tab[:, 0]), ("cb", C[:, 0], tab[:, 1]), ("cr", C[:, 1], tab[:, 1])):
        coef = _dct_blocks(_blocks(p), D)
        deq, n = _Quant.apply(coef, Q, f("coef_" + name), surrogate == "cubic")
        pre["coef_" + name], dec["coef_" + name] = (coef / Q).detach(), n
        v = _unblocks(D.T @ deq @ D) + 128
        rec.append(_level(v, f("s4_" + name), pre, dec, "s4_" + name))
    Yr, Cr_ = rec[0], torch.stack(rec[1:], 1)
    if sub:
        Cr_ = _triangle(_triangle(Cr_, 2), 3)
    cb, cr = Cr_[:, 0] - 128, Cr_[:, 1] - 128
    rgb = torch.stack([Yr + 1.402 * cr, Yr - 0.344136 * cb - 0.714136 * cr, Yr + 1.772 * cb], 1)
    lv = _level(rgb, f("s7"), pre, dec, "s7")
    return {"x": leaf, "out": lv / 255, "levels": lv.detach().to(torch.int64), "pre": pre, "dec": dec}


def vjp(res, g):
    """g_x [B, 3, H, W] in the run's dtype: autograd's product of g with the surrogate's Jacobian."""
    return torch.autograd.grad(res["out"], res["x"], g.to(res["out"].dtype), retain_graph=True)[0]


def cotangent(shape, seed=7):
    """The seeded normal field g of the comparisons, fp32."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def one_hots(subsampling, H, W):
    """{name: (channel, y, x)} of the one-hot cotangents: a corner pixel, a pixel at the edge of the kernels' 64 x 32
    tile (inside the image where it is larger than a tile, else the last column), an interior MCU-border pixel."""
    m = R.MCU[subsampling]
    return {"corner": (0, 0, 0), "far-corner": (2, H - 1, W - 1),
            "tile-edge": (1, min(32, H) - 1, min(64, W) - 1), "tile-edge+1": (1, min(32, H - 1), min(64, W - 1)),
            "mcu-border": (2, min(m, H - 1) - 1, min(m, W - 1))}


def near_clamp_edge(res, subsampling, guard=R.GUARD):
    """[B, H / mcu, W / mcu] bool: the MCUs with a value before the rounding of step 4 or 7 within that stage's guard of
    -0.5 or 255.5."""
    m = R.MCU[subsampling]
    out = None
    for key, v in res["pre"].items():
        stage = key.split("_")[0]
        if stage not in ("s4", "s7"):
            continue
        near = ((v + 0.5).abs() < guard[stage]) | ((v - 255.5).abs() < guard[stage])
        if near.dim() == 4:
            near = near.any(dim=1)
        cell = m // 2 if (subsampling == "420" and key in ("s4_cb", "s4_cr")) else m
        B, h, w = near.shape
        near = near.reshape(B, h // cell, cell, w // cell, cell).any(dim=4).any(dim=2)
        out = near if out is None else out | near
    return out


def excluded(name):
    """[B, H / mcu, W / mcu] bool: the MCUs of a case left out of the comparisons (the rule of the module docstring),
    and how many of them the clamp-edge rule alone adds."""
    ref = reference(name, "ste")
    x, qs, sub = case(name)
    fwd = R.reference(name) if name in R.CASES else R.roundtrip(x, qs, sub, torch.float64)
    frag = R.fragile(fwd, sub)
    edge = near_clamp_edge(ref, sub)
    out = frag | edge
    if sub == "420":
        out = torch.nn.functional.max_pool2d(out[:, None].float(), 3, 1, 1)[:, 0] > 0
    return out, int((edge & ~frag).sum())


def keep_mask(name):
    """[B, 3, H, W] bool: the pixels of the compared MCUs."""
    x, _, sub = case(name)
    return R.mcu_mask(excluded(name)[0], sub, x.shape[2], x.shape[3]).expand(-1, 3, -1, -1)


def rel_err(got, ref, keep):
    """max |got - ref| / max |ref| over the kept pixels; where the reference is zero there, 0 if got is too, else inf."""
    diff = float(((got.double() - ref.double()).abs() * keep).max())
    top = float((ref.double().abs() * keep).max())
    if top == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / top


_CACHE = {}


def reference(name, surrogate):
    """The float64 run of a case under a surrogate, computed once and shared."""
    if (name, surrogate) not in _CACHE:
        x, qs, sub = case(name)
        _CACHE[(name, surrogate)] = forward(x, qs, sub, surrogate, torch.float64)
    return _CACHE[(name, surrogate)]


def reference_vjp(name, surrogate, g):
    return vjp(reference(name, surrogate), g)


def measure_bwd(cases=None):
    """{(case, surrogate): the fp32 twin's relative difference from float64}, the fp32 run forced onto the float64
    run's decisions, g = cotangent()."""
    out = {}
    for name in (cases or CASES):
        x, qs, sub = case(name)
        g = cotangent(x.shape)
        keep = keep_mask(name)
        for s in SURROGATES:
            a = reference(name, s)
            b = forward(x, qs, sub, s, torch.float32, forced=a["dec"])
            out[(name, s)] = rel_err(vjp(b, g), vjp(a, g), keep)
    return out
