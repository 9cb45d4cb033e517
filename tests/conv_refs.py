"""Plain-torch references of the image-side conv kernels (the Z-gather conv_up to 3 channels and the RGB-input conv
3 -> 128 at k5 s2) that follow the dtype they are given, the comparison rules, and the seeded cases of the tests
that use them: tests/test_cpu_conv_refs.py checks the references and the rules on the CPU (and measures e_ref),
tests/test_gpu_image_ends.py compares the HIP kernels with the float64 references.  Nothing here imports the package
under test.

up3_ref      conv_transpose2d(stride 2, pad 2, output_padding 1): g_s.6 forward, the g_a.0 input gradient
rgb_ref      conv2d(stride 2, pad 2): g_a.0 forward, the g_s.6 input gradient
abs_scale    the same conv of |x|, |w|, |b| in float64: the per-element error scale S
gdn_fwd      (y, s) of oracle.codec.gdn on a conv result: the EPI_GDN launch and the s it saves
igdn_bwd     autograd of oracle.codec.gdn(a, inverse) under an upstream gradient (the conv), with the saved pair
             (y, s = y / a) the kernel reads: the EPI_IGDN_BWD launch
bf           round to bf16 (the bf16 kernels' operands): bf16 references round x and w first, then run in float64

Rule of the plain-bias launches (fp32, x6, bf16 operands with fp32 output), per element:
    |got - ref64| <= (n + 8) 2^-24 S,   n = products summed per output (9 Cin for the Z-gather, 75 for rgb5)
the worst-case bound of an fp32 accumulation of n products (n u sum |x w|, u = 2^-24); an x6 product drops only terms
below 2^-24 of it, and the + 8 covers those, the gather's adds and the bias.  A bf16 output adds 2^-8 |ref64| (its
own rounding).  Rule of the GDN / IGDN_BWD launches: rel_err against float64 <= round_up_1digit(4 e_ref), e_ref the
distance of the fp32 torch run from the float64 one on the same inputs (GDN_TOL, from the table in
tests/test_cpu_conv_refs.py).
"""
import functools

import torch
import torch.nn.functional as F

from oracle import codec
from tests.loss_refs import rel_err, rnd, round_up_1digit   # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24
NOMINAL_CUS = 256        # MI355X; the walk cases take their batch from the device's own count on the GPU

# tile geometry of the kernels (plain integers; the tests never read the sources)
ZP_COLS = 30                     # U3_OW: owned columns of a persistent Z-gather tile
ZP_ROWS = {128: 10, 192: 6}      # u3_rows<CT>() = 4 CT - 2: CT = 3 (Cin 128), CT = 2 (Cin 192)
ZT_ROWS, ZT_COLS = 5, 32         # T3_TH, T3_TW: the tiled Z-gather's block
RGB_COLS = 32                    # rgb5: one wave computes 32 columns of one output row
C_RGB = 128                      # rgb5's output channels


def bf(t):
    return t.bfloat16().float()


def cdiv(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------- #
# layouts (host side): NCHW <-> nChw4c [N, ceil(C / 4), H, W, 4], row-major <-> parity-split
# --------------------------------------------------------------------------- #
def to_nc4(x):
    N, C, H, W = x.shape
    C4 = cdiv(C, 4)
    if C4 * 4 != C:
        x = torch.cat([x, torch.zeros((N, C4 * 4 - C, H, W), dtype=x.dtype)], 1)
    return x.reshape(N, C4, 4, H, W).permute(0, 1, 3, 4, 2).contiguous()


def from_nc4(x4, C):
    N, C4, H, W, _ = x4.shape
    return x4.permute(0, 1, 4, 2, 3).reshape(N, C4 * 4, H, W)[:, :C].contiguous()


def split4(x4):
    """row-major nChw4c -> parity-split: the four (y & 1, x & 1) sub-planes of (H / 2) x (W / 2) pixels in turn"""
    N, C4, H, W, _ = x4.shape
    return x4.view(N, C4, H // 2, 2, W // 2, 2, 4).permute(0, 1, 3, 5, 2, 4, 6).contiguous().view(N, C4, H, W, 4)


def merge4(xs):
    N, C4, H, W, _ = xs.shape
    return xs.view(N, C4, 2, 2, H // 2, W // 2, 4).permute(0, 1, 4, 2, 5, 3, 6).contiguous().view(N, C4, H, W, 4)


# --------------------------------------------------------------------------- #
# references
# --------------------------------------------------------------------------- #
def _b(b, dtype):
    return None if b is None else b.to(dtype)


def up3_ref(x, w, b, dtype=torch.float64):
    """x [N, Cin, H, W], w [Cin, 3, 5, 5] (the ConvTranspose2d weight, or a Conv2d(3, Cin) weight under its input
    gradient), b [3] or None -> [N, 3, 2H, 2W] in dtype."""
    return F.conv_transpose2d(x.to(dtype), w.to(dtype), _b(b, dtype), stride=2, padding=2, output_padding=1)


def rgb_ref(x, w, b, dtype=torch.float64):
    """x [N, 3, H, W], w [Cout, 3, 5, 5] (the Conv2d weight, or a ConvTranspose2d(Cout, 3) weight under its input
    gradient), b [Cout] or None -> [N, Cout, ceil(H / 2), ceil(W / 2)] in dtype."""
    return F.conv2d(x.to(dtype), w.to(dtype), _b(b, dtype), stride=2, padding=2)


def abs_scale(ref_fn, x, w, b):
    """S = ref_fn(|x|, |w|, |b|) in float64: sum of the magnitudes of every term of an output element."""
    return ref_fn(x.abs(), w.abs(), None if b is None else b.abs(), torch.float64)


def gdn_params(C, seed):
    beta = rnd((C,), seed, 0.5, 1.5)
    gamma = 0.1 * torch.eye(C) + 0.02 * rnd((C, C), seed + 1, 0.0, 1.0)
    return beta, gamma


def gdn_fwd(pre, beta, gamma):
    """(y, s) of the GDN of `pre`, in its dtype: y = oracle.codec.gdn(pre), s = norm^-1/2 (y = pre s)."""
    dt = pre.dtype
    C = pre.shape[1]
    beta, gamma = beta.to(dt), gamma.to(dt)
    be, ge = codec.gdn_effective(beta, gamma)
    s = torch.rsqrt(F.conv2d(pre ** 2, ge.reshape(C, C, 1, 1), be))
    return codec.gdn(pre, beta, gamma, False), s


def igdn_bwd(up, a, beta, gamma):
    """(dL/da, y, s) in up's dtype: y = IGDN(a) = oracle.codec.gdn(a, inverse), s = y / a (the saved pair), and the
    gradient of sum(y * up) with respect to a."""
    dt = up.dtype
    ad = a.to(dt).clone().requires_grad_(True)
    y = codec.gdn(ad, beta.to(dt), gamma.to(dt), True)
    y.backward(up)
    return ad.grad, y.detach(), (y / ad).detach()


# --------------------------------------------------------------------------- #
# rules
# --------------------------------------------------------------------------- #
def bias_bound(n, S, ref64=None):
    """The per-element bound; ref64 given: the output is bf16."""
    bound = (n + 8) * U * S
    return bound if ref64 is None else bound + 2.0 ** -8 * ref64.abs()


def bias_rule(got, ref64, S, n, out_bf16=False):
    """(passes, max |got - ref64| / S, max |got - ref64| / bound)."""
    d = (got.double() - ref64).abs()
    bound = bias_bound(n, S, ref64 if out_bf16 else None)
    ok = bool((d <= bound).all())   # False for a NaN, and where S = 0 unless got == ref64
    return ok, float((d / S.clamp_min(1e-300)).max()), float((d / bound.clamp_min(1e-300)).max())


def gdn_rule(got, ref64, tol):
    e = rel_err(got, ref64)
    return e <= tol, e   # False for a NaN


# --------------------------------------------------------------------------- #
# Z-gather cases
# --------------------------------------------------------------------------- #
# name: (Cin, precisions, Hin, Win, N (None: a walk case, N from the CU count), tiles per image, split input)
ZP_CASES = {
    "c128_3x5": (128, ("x6", "bf16"), 3, 5, 1, 1, False),            # one tile: 7 of the 8 XCD groups return at once
    "c128_11x31": (128, ("x6", "bf16"), 11, 31, 1, 4, False),        # 2 x 2 tiles, remainders 1 row / 1 column wide
    "c128_10x30": (128, ("x6",), 10, 30, 3, 1, False),               # exact tiles, total 3 < 8
    "c128_21x61": (128, ("x6", "bf16"), 21, 61, 3, 9, False),        # 27 tiles: r8 = 3, nb = 4, short XCDs' last block returns
    "c128_41x91_walk": (128, ("x6", "bf16"), 41, 91, None, 20, False),
    "c192_7x31": (192, ("x6",), 7, 31, 1, 4, False),                 # R = 6 geometry
    "c192_13x61": (192, ("x6",), 13, 61, 2, 9, False),
    "c192_25x61_walk": (192, ("x6",), 25, 61, None, 15, False),
    "c128_12x62_split": (128, ("x6",), 12, 62, 2, 6, True),          # parity-split input
}
# tiled kernel: name: (Cin, precisions, Hin, Win, N, tiles per image); nch = Cin / 16 = 1, 3 (the pipeline's odd
# tail, and no trip of its loop at all), 4, 12
ZT_CASES = {}
for _c, _p in ((16, ("fp32", "x6")), (48, ("fp32", "x6")), (64, ("fp32", "x6")), (192, ("fp32",))):
    ZT_CASES[f"c{_c}_6x33"] = (_c, _p, 6, 33, 2, 4)     # 2 x 2 blocks of 5 x 32: a 1-row and a 1-column remainder
    ZT_CASES[f"c{_c}_5x32"] = (_c, _p, 5, 32, 1, 1)     # exact


def walk_n(per_image, threshold):
    """Smallest N with N * per_image > threshold."""
    return threshold // per_image + 1


def zp_n(name, cus=NOMINAL_CUS):
    """Batch of a persistent case: walk cases take the smallest N with tiles > 2 * 8 * (CUs // 8), so that every
    block walks at least two tiles and some three."""
    _, _, _, _, N, per, _ = ZP_CASES[name]
    return N if N is not None else walk_n(per, 2 * 8 * (cus // 8))


def zp_blocks(tiles, cus):
    """Blocks of the persistent launch: 8 x nb, nb per XCD, at most one per CU."""
    return 8 * max(1, min(cdiv(tiles, 8), cus // 8))


def _signed(shape, seed, lo, hi):
    """uniform magnitude in [lo, hi] with a random sign: nothing near zero"""
    return rnd(shape, seed, lo, hi) * torch.where(rnd(shape, seed + 500) < 0.5, -1.0, 1.0)


def _zg_inputs(Cin, H, W, N, seed):
    """x in [-1, 1]; w in +-4 / Cin (S ~ 9); bias magnitudes in [0.5, 1.5], far above the bound"""
    return (rnd((N, Cin, H, W), seed, -1, 1), rnd((Cin, 3, 5, 5), seed + 1, -1, 1) * (4.0 / Cin),
            _signed((3,), seed + 2, 0.5, 1.5))


@functools.lru_cache(maxsize=None)
def zg_case(name, N=None):
    """(x, w, b, Cin) of a persistent or tiled case (N: overrides the case's batch)."""
    table = ZP_CASES if name in ZP_CASES else ZT_CASES
    Cin, _, H, W = table[name][:4]
    if N is None:
        N = zp_n(name) if name in ZP_CASES else table[name][4]
    seed = 1000 + 10 * (list(ZP_CASES) + list(ZT_CASES)).index(name)
    return _zg_inputs(Cin, H, W, N, seed) + (Cin,)


@functools.lru_cache(maxsize=None)
def zg_expected(name, N=None, bf16=False):
    """(ref64, S) without the bias, [N, 3, 2H, 2W] float64; bf16: of the bf16-rounded x and w."""
    x, w, _, _ = zg_case(name, N)
    if bf16:
        x, w = bf(x), bf(w)
    return up3_ref(x, w, None), abs_scale(up3_ref, x, w, None)


def with_bias(ref0, S0, b):
    """the bias-free (ref64, S) with a per-channel bias added (b None: as they are)"""
    if b is None:
        return ref0, S0
    v = b.double().reshape(1, -1, 1, 1)
    return ref0 + v, S0 + v.abs()


# --------------------------------------------------------------------------- #
# RGB-input conv cases
# --------------------------------------------------------------------------- #
# name: (H, W, N (None: walk), tiles per image, split output, launch kinds)
RGB_KINDS = ("bias", "bias_bf16", "gdn", "igdn_bwd")
RGB_CASES = {
    "2x2": (2, 2, 1, 1, False, RGB_KINDS),                   # one tile, one valid lane
    "13x67": (13, 67, 1, 14, False, RGB_KINDS),              # odd sides; Wout 34: 2 valid lanes in the second column tile
    "64x64": (64, 64, 3, 32, False, RGB_KINDS),              # exact
    "50x130_walk": (50, 130, None, 75, False, RGB_KINDS),    # runs cross rows and images
    "48x68_split": (48, 68, 2, 48, True, ("gdn", "igdn_bwd")),
}


def rgb_n(name, cus=NOMINAL_CUS):
    """walk: the smallest N with total tiles > 8 * CUs (more than one round of 8 waves per block)."""
    _, _, N, per, _, _ = RGB_CASES[name]
    return N if N is not None else walk_n(per, 8 * cus)


def rgb_blocks(total, cus, waves):
    """Blocks of the persistent rgb5 launch: one per `waves` tiles, at most one per CU."""
    return max(1, min(cus, cdiv(total, waves)))


@functools.lru_cache(maxsize=None)
def rgb_case(name, N=None):
    """dict of the case's inputs: x [N, 3, H, W] in [0, 1] (the image; also the image-side gradient of the input
    -gradient launch, there in [-1, 1]: g), w [128, 3, 5, 5], b [128] (magnitudes 0.05-0.15), (beta, gamma), and a
    [N, 128, Ho, Wo], the IGDN input of the backward launch (magnitudes 0.25-1, so that s = y / a is well defined)."""
    H, W = RGB_CASES[name][:2]
    if N is None:
        N = rgb_n(name)
    seed = 3000 + 10 * list(RGB_CASES).index(name)
    Ho, Wo = cdiv(H, 2), cdiv(W, 2)
    beta, gamma = gdn_params(C_RGB, seed + 5)
    return dict(x=rnd((N, 3, H, W), seed), g=rnd((N, 3, H, W), seed + 1, -1, 1),
                w=rnd((C_RGB, 3, 5, 5), seed + 2, -1, 1) * 0.1, b=_signed((C_RGB,), seed + 3, 0.05, 0.15),
                beta=beta, gamma=gamma, a=_signed((N, C_RGB, Ho, Wo), seed + 4, 0.25, 1.0))


def rgb_compose(c, kind, dtype, pre=None):
    """Outputs of launch `kind` on the inputs c (a dict as rgb_case gives) in dtype.  bias / bias_bf16: (y,);
    gdn: (y, s); igdn_bwd: (dL/da, saved y, saved s).  pre: the conv result to use instead of the reference's (the
    sensitivity tests put their defects there)."""
    if kind in ("bias", "bias_bf16"):
        x, w = (bf(c["x"]), bf(c["w"])) if kind == "bias_bf16" else (c["x"], c["w"])
        return (rgb_ref(x, w, c["b"], dtype) if pre is None else pre,)
    if kind == "gdn":
        return gdn_fwd(rgb_ref(c["x"], c["w"], c["b"], dtype) if pre is None else pre, c["beta"], c["gamma"])
    if kind == "igdn_bwd":
        return igdn_bwd(rgb_ref(c["g"], c["w"], None, dtype) if pre is None else pre, c["a"], c["beta"], c["gamma"])
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def rgb_expected(name, kind, N=None):
    """float64 outputs of rgb_compose, and for the bias kinds S as the last element."""
    c = rgb_case(name, N)
    out = rgb_compose(c, kind, torch.float64)
    if kind == "bias":
        out += (abs_scale(rgb_ref, c["x"], c["w"], c["b"]),)
    elif kind == "bias_bf16":
        out += (abs_scale(rgb_ref, bf(c["x"]), bf(c["w"]), c["b"]),)
    return out


# rel_err tolerances of the GDN launches, round_up_1digit(4 e_ref): (case, kind, output) -> tolerance, from the
# e_ref table of tests/test_cpu_conv_refs.py (which checks that its measurement still gives them)
GDN_OUTPUTS = {"gdn": ("y", "s"), "igdn_bwd": ("dx",)}
GDN_TOL = {
    ("2x2", "gdn", "y"): 3e-07, ("2x2", "gdn", "s"): 3e-07, ("2x2", "igdn_bwd", "dx"): 3e-07,
    ("13x67", "gdn", "y"): 3e-06, ("13x67", "gdn", "s"): 3e-06, ("13x67", "igdn_bwd", "dx"): 2e-06,
    ("64x64", "gdn", "y"): 2e-06, ("64x64", "gdn", "s"): 3e-06, ("64x64", "igdn_bwd", "dx"): 3e-06,
    ("50x130_walk", "gdn", "y"): 2e-06, ("50x130_walk", "gdn", "s"): 3e-06, ("50x130_walk", "igdn_bwd", "dx"): 3e-06,
    ("48x68_split", "gdn", "y"): 2e-06, ("48x68_split", "gdn", "s"): 3e-06, ("48x68_split", "igdn_bwd", "dx"): 2e-06,
}
