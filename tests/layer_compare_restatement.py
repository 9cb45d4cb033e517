"""The layer-wise error-propagation study (layer_store / layer_compare, anchors/utils.py:132-166) restated with
oracle.codec functions, module by module, in the dtype it is given; the seeded cases and the tolerance tables of
tests/test_cpu_layer_compare.py and tests/test_gpu_layer_compare.py.

Per image (the reference's means run over its batch of one image):

    enc        = [x, every g_a module output];  y = enc[-1] (unrounded)
    dec[i]     = g_s modules fed y;  dec_round[i] = g_s modules fed round(y)
    Encoder      mean((enc_a[k] - enc_c[k])^2)                      (the reference prints it times 0.5)
    Quantization sqrt(mean((y_a - round(y_c))^2)), sqrt(mean((round(y_a) - round(y_c))^2))
    Decoder      sqrt(mean((dec_a[i] - dec_round_c[i])^2)), sqrt(mean((dec_round_a[i] - dec_round_c[i])^2))

Modules: bmshj2018 (factorized, hyper, context) conv, GDN, conv, GDN, conv, GDN, conv on both sides; cheng2020 the
top-level modules of g_a (three ResidualBlockWithStride / ResidualBlock pairs and a conv: 7) and of g_s (RB, RBU, RB,
RBU, RB, RBU, RB and the sub-pixel conv: 8).

Bounds.  Every bound is 4 max(e_ref, 2^-24) rounded up to one digit (the rule of tests/rate_attack_restatement.py):
e_ref is the relative distance of the fp32 CPU restatement from the float64 one on the same inputs, the largest over
the rows and images the bound covers; the floor is one fp32 rounding and the factor 4 leaves room for another, fixed,
summation order.  tests/test_cpu_layer_compare.py prints the e_ref tables and checks that fp32 alone stays inside
each bound.  The values below were derived there, on the CPU, and are not tuned to any device output.
"""
import math

import torch

from oracle import codec
from tests import loss_refs as R

BMSHJ = ("factorized", "hyper", "context")


def to_dtype(P, dtype):
    return {k: v.to(dtype) for k, v in P.items()}


def g_a_modules(P, model):
    if model == "cheng2020":
        blocks = [codec.rb_stride, codec.rb] * 3
        mods = [lambda x, f=f, i=i: f(P, f"g_a.{i}", x) for i, f in enumerate(blocks)]
        return mods + [lambda x: codec.conv_k(x, P["g_a.6.weight"], P["g_a.6.bias"], 2)]
    if model not in BMSHJ:
        raise NotImplementedError(model)
    mods = []
    for i in (0, 2, 4):
        mods.append(lambda x, i=i: codec.conv(x, P[f"g_a.{i}.weight"], P[f"g_a.{i}.bias"]))
        mods.append(lambda x, i=i: codec.gdn(x, P[f"g_a.{i + 1}.beta"], P[f"g_a.{i + 1}.gamma"]))
    return mods + [lambda x: codec.conv(x, P["g_a.6.weight"], P["g_a.6.bias"])]


def g_s_modules(P, model):
    if model == "cheng2020":
        blocks = [codec.rb, codec.rb_up] * 3 + [codec.rb]
        mods = [lambda x, f=f, i=i: f(P, f"g_s.{i}", x) for i, f in enumerate(blocks)]
        return mods + [lambda x: codec.subpel(x, P["g_s.7.0.weight"], P["g_s.7.0.bias"])]
    if model not in BMSHJ:
        raise NotImplementedError(model)
    mods = []
    for i in (0, 2, 4):
        mods.append(lambda x, i=i: codec.deconv(x, P[f"g_s.{i}.weight"], P[f"g_s.{i}.bias"]))
        mods.append(lambda x, i=i: codec.gdn(x, P[f"g_s.{i + 1}.beta"], P[f"g_s.{i + 1}.gamma"], inverse=True))
    return mods + [lambda x: codec.deconv(x, P["g_s.6.weight"], P["g_s.6.bias"])]


def walk(mods, x):
    out = []
    for m in mods:
        x = m(x)
        out.append(x)
    return out


def _mean(t):
    return t.flatten(1).mean(1)


def encoder_rows(P, im_adv, im_clean, model, dtype=torch.float64):
    """(mse [B, 8], y_adv, y_clean) in dtype."""
    P = to_dtype(P, dtype)
    mods = g_a_modules(P, model)
    ea = [im_adv.to(dtype)] + walk(mods, im_adv.to(dtype))
    ec = [im_clean.to(dtype)] + walk(mods, im_clean.to(dtype))
    return torch.stack([_mean((a - c) ** 2) for a, c in zip(ea, ec)], 1), ea[-1], ec[-1]


def quant_rows(y_adv, y_clean, dtype=torch.float64):
    """rmse [B, 2]: the rounding acts on the latents as given (their own dtype), the sums run in dtype."""
    ya, ra, rc = y_adv.to(dtype), torch.round(y_adv).to(dtype), torch.round(y_clean).to(dtype)
    return torch.stack([_mean((ya - rc) ** 2), _mean((ra - rc) ** 2)], 1) ** 0.5


def decoder_rows(P, y_adv, y_clean, model, dtype=torch.float64):
    """rmse [B, rows, 2] in dtype.  The clean image's unrounded decode is never read, so it is not computed."""
    P = to_dtype(P, dtype)
    mods = g_s_modules(P, model)
    da = walk(mods, y_adv.to(dtype))
    dra = walk(mods, torch.round(y_adv).to(dtype))
    drc = walk(mods, torch.round(y_clean).to(dtype))
    rows = [torch.stack([_mean((a - rc) ** 2), _mean((ra - rc) ** 2)], 1) ** 0.5 for a, ra, rc in zip(da, dra, drc)]
    return torch.stack(rows, 1)


def study(P, im_adv, im_clean, model, dtype=torch.float64):
    enc, ya, yc = encoder_rows(P, im_adv, im_clean, model, dtype)
    return enc, quant_rows(ya, yc, dtype), decoder_rows(P, ya, yc, model, dtype), ya, yc


def reference_formulas(P, im_adv, im_clean, model, dtype=torch.float64):
    """anchors/utils.py:152-166 written directly: whole-batch means (B = 1 in the reference), dec of the clean image
    included as the reference computes it, and the loop variable `layer` of the encoder loop (the unrounded
    adversarial latent) in the first Quantization number.  Returns (encoder list, (q0, q1), decoder list of pairs)
    of python floats."""
    P = to_dtype(P, dtype)

    def layer_store(x):
        out = {"enc": [x], "dec": [], "dec_round": []}
        for m in g_a_modules(P, model):
            x = m(x)
            out["enc"].append(x)
        x_round = torch.round(x)
        out["dec"] = walk(g_s_modules(P, model), x)
        out["dec_round"] = walk(g_s_modules(P, model), x_round)
        return x_round, out

    x_round, lo = layer_store(im_adv.to(dtype))
    x_s_round, lo_s = layer_store(im_clean.to(dtype))
    enc, layer = [], None
    for layer, layer_s in zip(lo["enc"], lo_s["enc"]):
        enc.append(torch.mean((layer - layer_s) ** 2).item())
    x_error = torch.mean((x_round - x_s_round) ** 2) ** 0.5
    x_err_s = torch.mean((layer - x_s_round) ** 2) ** 0.5
    dec = []
    for layer_r, layer, layer_s_r in zip(lo["dec_round"], lo["dec"], lo_s["dec_round"]):
        dec.append((torch.mean((layer - layer_s_r) ** 2).item() ** 0.5,
                    torch.mean((layer_r - layer_s_r) ** 2).item() ** 0.5))
    return enc, (x_err_s.item(), x_error.item()), dec


# --------------------------------------------------------------------------- #
# Composition cases
# --------------------------------------------------------------------------- #
NOISE_AMP = 4.0 / 255.0
TIE_MARGIN = 0.05
TIE_SHARE_CAP = 0.12

# name: (model, quality, image shape, image seed)
CASES = {
    "hyper-q1-2x64x64": ("hyper", 1, (2, 3, 64, 64), 71),
    "hyper-q1-1x64x128": ("hyper", 1, (1, 3, 64, 128), 72),
    "factorized-q1-1x64x64": ("factorized", 1, (1, 3, 64, 64), 73),
    "hyper-q6-1x64x64": ("hyper", 6, (1, 3, 64, 64), 74),
    "context-q1-1x64x64": ("context", 1, (1, 3, 64, 64), 75),
    "cheng2020-q1-1x64x64": ("cheng2020", 1, (1, 3, 64, 64), 76),
}
# the engine precisions a case runs with on the device
PRECISIONS = {
    "hyper-q1-2x64x64": ("fp32", "x6"), "hyper-q1-1x64x128": ("fp32", "x6"), "factorized-q1-1x64x64": ("fp32",),
    "hyper-q6-1x64x64": ("fp32",), "context-q1-1x64x64": ("fp32",), "cheng2020-q1-1x64x64": ("fp32", "x6"),
}


def params(model, quality):
    return codec.perturb_params(codec.init_params(model, quality, seed=0), seed=1)


def images(shape, seed):
    """(im_adv, im_clean): the clean image plus seeded uniform noise of amplitude 4 / 255, clamped.  No attack."""
    clean = R.rnd(shape, seed)
    noise = (R.rnd(shape, seed + 1000) * 2 - 1) * NOISE_AMP
    return torch.clamp(clean + noise, 0.0, 1.0), clean


def off_ties(y, margin=TIE_MARGIN):
    """(y', share): every element closer than margin to a half-integer moved to exactly margin away (on its own side;
    an exact tie goes up); share = the fraction of elements moved.  fp32 in, fp32 out."""
    y64 = y.double()
    half = torch.floor(y64) + 0.5
    d = y64 - half
    near = d.abs() < margin
    moved = torch.where(near, half + torch.where(d >= 0, margin, -margin), y64)
    return moved.float(), float(near.double().mean())


def spread_gain(y):
    """The power of two that brings the latent's standard deviation to [3, 6): the seeded weights give latents of
    |y| < 0.5, which all round to 0; multiplied by it they spread over many integers."""
    return 2.0 ** math.ceil(math.log2(3.0 / float(y.double().std())))


class Case:
    """The CPU references of one composition case, computed once (float64 and fp32).

    Two pairs of given latents feed the quant / decoder rows.  (y_adv, y_clean) are the case's own latents; with the
    seeded weights every element of them rounds to 0, so their rounded column is exactly 0 on both sides and only
    the unrounded column carries numbers.  (y_adv_s, y_clean_s) are the same latents times spread_gain(y_clean),
    spread over many integers: the rounded paths with numbers in them.  Both are moved off the ties."""

    def __init__(self, name):
        self.name = name
        self.model, self.quality, self.shape, seed = CASES[name]
        self.P = params(self.model, self.quality)
        self.im_adv, self.im_clean = images(self.shape, seed)
        self.enc64, _, _, ya, yc = study(self.P, self.im_adv, self.im_clean, self.model, torch.float64)
        self.enc32 = encoder_rows(self.P, self.im_adv, self.im_clean, self.model, torch.float32)[0]
        # the given latents: float64 latents stored as fp32, moved off the rounding ties
        self.y_adv, self.share_adv = off_ties(ya.float())
        self.y_clean, self.share_clean = off_ties(yc.float())
        self.gain = spread_gain(yc)
        self.y_adv_s, self.share_adv_s = off_ties((ya * self.gain).float())
        self.y_clean_s, self.share_clean_s = off_ties((yc * self.gain).float())
        self.ref = {}
        for tag, a, c in (("", self.y_adv, self.y_clean), ("_s", self.y_adv_s, self.y_clean_s)):
            for dt, nm in ((torch.float64, "64"), (torch.float32, "32")):
                self.ref["quant" + tag + nm] = quant_rows(a, c, dt)
                self.ref["dec" + tag + nm] = decoder_rows(self.P, a, c, self.model, dt)

    def latents(self, tag):
        return (self.y_adv, self.y_clean) if tag == "" else (self.y_adv_s, self.y_clean_s)

    def shares(self):
        return dict(adv=self.share_adv, clean=self.share_clean, adv_s=self.share_adv_s, clean_s=self.share_clean_s)

    def e_ref(self):
        e = dict(enc=row_err(self.enc32, self.enc64))
        for k in ("quant", "dec", "quant_s", "dec_s"):
            e[k] = row_err(self.ref[k + "32"], self.ref[k + "64"])
        return e

    def smallest_mse(self):
        """The smallest mse of any row that is not exactly 0 by construction."""
        vals = [self.enc64] + [self.ref[k + "64"] ** 2 for k in ("quant", "dec", "quant_s", "dec_s")]
        return min(float(v[v > 0].min()) for v in vals)


def row_err(a, b):
    """The largest relative distance of any row: max |a - b| / |b| in float64.  A row that is exactly 0 in b (the
    rounded column of latents that all round to 0) has to be exactly 0 in a: anything else is inf."""
    a, b = a.detach().double(), b.detach().double()
    d = (a - b).abs()
    rel = torch.where(b == 0, torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))),
                      d / b.abs().clamp_min(1e-300))
    return float(rel.max())


FLOOR = 2.0 ** -24


def bound_of(e_ref):
    return R.round_up_1digit(4.0 * max(e_ref, FLOOR))


# case: relative bounds per row of the encoder rows, and of the quant / decoder rows from the case's own latents
# and from the spread ones (_s)                                                                e_ref
STUDY_TOL = {
    "hyper-q1-2x64x64": dict(enc=3e-05, quant=3e-07, dec=3e-06, quant_s=3e-07, dec_s=2e-06),
    # e_ref 5.56e-06, 3.98e-08, 5.78e-07, 4.07e-08, 3.02e-07
    "hyper-q1-1x64x128": dict(enc=2e-05, quant=3e-07, dec=2e-06, quant_s=3e-07, dec_s=7e-07),
    # e_ref 4.62e-06, 4.54e-08, 3.85e-07, 5.09e-08, 1.66e-07
    "factorized-q1-1x64x64": dict(enc=2e-05, quant=3e-07, dec=2e-06, quant_s=3e-07, dec_s=7e-07),
    # e_ref 4.48e-06, 5.03e-08, 4.47e-07, 3.80e-08, 1.67e-07
    "hyper-q6-1x64x64": dict(enc=2e-05, quant=3e-07, dec=2e-06, quant_s=3e-07, dec_s=2e-06),
    # e_ref 3.70e-06, 2.51e-08, 3.24e-07, 3.64e-08, 2.96e-07
    "context-q1-1x64x64": dict(enc=2e-05, quant=3e-07, dec=2e-06, quant_s=3e-07, dec_s=8e-07),
    # e_ref 3.24e-06, 1.75e-08, 4.38e-07, 6.64e-08, 1.91e-07
    "cheng2020-q1-1x64x64": dict(enc=4e-06, quant=3e-07, dec=3e-07, quant_s=3e-07, dec_s=1e-06),
    # e_ref 8.72e-07, 1.37e-09, 5.57e-08, 6.12e-08, 2.27e-07
}
# The smallest mse of any row of any case that is not 0 by construction (float64; the last encoder row of
# hyper-q1-2x64x64): 2^-22 relative to O(1) activations squared is 2e-7 of it, so no row is cancellation noise.
SMALLEST_MSE = 2.449e-07

# --------------------------------------------------------------------------- #
# Kernel cases
# --------------------------------------------------------------------------- #
KERNEL_SHAPES = [(3, 8, 1, 1), (2, 6, 5, 3), (1, 3, 33, 47), (2, 192, 4, 6), (2, 320, 4, 6), (2, 128, 32, 48)]
TIES = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -0.0, 0.0, 4194304.5, -4194304.5, 8388607.5, 0.49999997, 1.0000001, -3.5]


def shape_key(shape):
    return "x".join(str(v) for v in shape)


def kernel_case(shape, seed=401):
    """(a, b, c) NCHW fp32: b and c are a plus differences of order 0.1 (far above an fp32 rounding of values of
    order 3).  The first elements of every image of a hold the rounding ties and those of b the same values plus one
    (ties again, one fp32 addition), so the rounded differences there are small integers: a wrong tie rule moves
    quant1 by at least 1 on sums of that order."""
    B, C, H, W = shape
    g = R.gen(seed + C + 7 * H + B)
    a = torch.randn(shape, generator=g) * 3
    b = a + torch.randn(shape, generator=g) * 0.1
    c = a + torch.randn(shape, generator=g) * 0.1
    ties = torch.tensor(TIES)
    n = min(a[0].numel(), len(TIES))
    a.reshape(B, -1)[:, :n] = ties[:n]
    b.reshape(B, -1)[:, :n] = ties[:n] + 1.0
    return a, b, c


def kernel_ref(a, b, c, dtype=torch.float64):
    """The five sums [B] each in dtype: pair, quant0, quant1, triple0, triple1.  torch.round acts on the fp32 inputs."""
    ra, rb = torch.round(a).to(dtype), torch.round(b).to(dtype)
    a_, b_, c_ = a.to(dtype), b.to(dtype), c.to(dtype)

    def ssd(u, v):
        return ((u - v) ** 2).flatten(1).sum(1)

    return dict(pair=ssd(a_, b_), quant0=ssd(a_, rb), quant1=ssd(ra, rb), triple0=ssd(a_, c_), triple1=ssd(b_, c_))


def kernel_e_ref(shape):
    a, b, c = kernel_case(shape)
    r64, r32 = kernel_ref(a, b, c, torch.float64), kernel_ref(a, b, c, torch.float32)
    return {k: row_err(r32[k], r64[k]) for k in r64}


# shape: bounds of (pair, quant0, quant1, triple0, triple1), relative per image                 e_ref
KERNEL_TOL = {
    "3x8x1x1": dict(pair=3e-07, quant0=3e-07, quant1=3e-07, triple0=3e-07, triple1=7e-07),
    # e_ref 0.00e+00, 0.00e+00, 0.00e+00, 7.19e-08, 1.52e-07
    "2x6x5x3": dict(pair=3e-07, quant0=5e-07, quant1=3e-07, triple0=5e-07, triple1=4e-07),
    # e_ref 2.88e-08, 1.07e-07, 0.00e+00, 1.23e-07, 9.87e-08
    "1x3x33x47": dict(pair=3e-07, quant0=3e-07, quant1=3e-07, triple0=3e-07, triple1=3e-07),
    # e_ref 5.67e-08, 2.83e-08, 0.00e+00, 4.03e-08, 3.92e-08
    "2x192x4x6": dict(pair=3e-07, quant0=3e-07, quant1=3e-07, triple0=3e-07, triple1=3e-07),
    # e_ref 5.60e-08, 6.14e-08, 0.00e+00, 4.43e-08, 6.18e-08
    "2x320x4x6": dict(pair=4e-07, quant0=3e-07, quant1=3e-07, triple0=3e-07, triple1=3e-07),
    # e_ref 8.87e-08, 4.12e-08, 0.00e+00, 7.63e-09, 7.63e-09
    "2x128x32x48": dict(pair=3e-07, quant0=3e-07, quant1=3e-07, triple0=3e-07, triple1=3e-07),
    # e_ref 3.19e-08, 2.60e-08, 0.00e+00, 4.57e-08, 5.14e-08
}
