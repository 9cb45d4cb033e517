"""GPU tests of the latent-distribution study (ica_distrib.hip, latent_distribution, the visual_distribution CLI)
against the restatement tests/distribution_restatement.py.

hist is exact: the kernel restates the CPU torch.histc bin arithmetic in fp32.

pred: erff differs between device and host, and the tails cancel in 1 + erf, so the bound is absolute.  d32 is the
largest |float32 restatement - float64 restatement| of pred over exactly the inputs of this file's kernel cases
(CASES), measured on the CPU when the tests run; the device must stay within 4 * d32 of float64 (the factor covers a
different erff and the mean's different summation order).  Each case is also held to 4 * max(its own d32, one fp32
ulp of the value), so the cases whose arithmetic is nearly exact (mu-50, one-pixel-dominates) are not measured
against the worst case's error.  The model tests measure their own d32 on the engine's
tensors in the same way.  Measured (MI355X; every test prints its figures): d32 = 9.2e-8 over CASES on the test
host's CPU (1.27e-7 on another host: torch's CPU erf differs between vector widths), largest device difference
8.4e-8 (case 2x192x4x6), bound 3.7e-7; context q1 d32 1.1e-7 / device 8.8e-8, cheng2020 q1 1.0e-7 / 7.4e-8, the
scaled hyperprior model 2.3e-7 / 1.0e-7 (clean) and 2.7e-7 / 9.2e-8 (adversarial).

bits against float64: pixels * 2^-24 * sum |terms| (the fp32 chain's own bound) plus the largest difference between
the float32 and the float64 restatement of bits on the same inputs (log2f, measured like d32).

Non-finite values: the installed CPU torch.histc does not raise on NaN or +-inf but converts the bin position of a NaN
to an integer, which C++ leaves undefined; so the reference histogram is taken over the finite values of a plane and
the kernel must count every non-finite value as outside.

err against float64, per channel: sum_k hist_k * delta / (pred_k * ln 2) with delta = 4 * d32, the clean plus the
adversarial side, and nothing else.  What channel_rate's own fp32 evaluation may add ((nbins + 1) * 2^-23 * sum |terms|,
the bound test_channel_rate_on_device_tensors checks on its own) only widens the margin by which the ranking test's
inputs must separate adjacent channels."""
import math

import pytest
import torch

from tests import distribution_restatement as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def LD():
    from imagecompression_adversarial_amd import latent_distribution
    return latent_distribution


# --------------------------------------------------------------------------- #
# the kernel cases: name -> (B, C, H, W, means, lik, vmin, nbins)
# --------------------------------------------------------------------------- #
SHAPES = {
    "1x4x1x1": (1, 4, 1, 1, False, False, -5.5, 11),
    "3x8x4x4": (3, 8, 4, 4, True, True, -5.5, 11),
    "1x4x4x4-16bins": (1, 4, 4, 4, True, True, -8.0, 16),            # exactly one chunk of bins
    "3x8x7x9-64bins": (3, 8, 7, 9, False, True, -32.0, 64),          # four chunks
    "1x4x33x47-1bin": (1, 4, 33, 47, True, False, -0.5, 1),
    "1x4x33x47-17bins": (1, 4, 33, 47, True, True, -8.5, 17),        # a second chunk of one bin
    "3x8x33x47": (3, 8, 33, 47, True, True, -5.5, 11),               # 7 blocks a plane
    "1x4x130x127": (1, 4, 130, 127, True, True, -5.5, 11),           # 65 > 64 blocks: the cap, then the grid stride
    "2x192x4x6": (2, 192, 4, 6, False, True, -5.5, 11),
    "3x8x7x9-vmin0.1": (3, 8, 7, 9, True, True, 0.1, 13),            # vmin + j is not exact in fp32
    "2x320x4x6-64bins": (2, 320, 4, 6, True, True, -32.0, 64),
}
SPECIAL = ("sigma-classes", "mu-50", "mu-half-integers", "one-pixel-dominates")


def random_case(name):
    B, C, H, W, has_m, has_l, vmin, nbins = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    y = torch.randn((B, C, H, W), generator=g) * (0.3 * nbins)         # a share of the values lies outside
    s = torch.exp(torch.randn((B, C, H, W), generator=g)) * 0.5         # some below the 0.11 floor
    m = torch.randn((B, C, H, W), generator=g) * 2 if has_m else None
    lik = torch.rand((B, C, H, W), generator=g).clamp(min=1e-9) if has_l else None
    return y, s, m, lik, vmin, nbins


def special_case(name):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    B, C, H, W = 2, 4, 7, 9
    y = torch.randn((B, C, H, W), generator=g) * 3
    lik = torch.rand((B, C, H, W), generator=g).clamp(min=1e-9)
    m = torch.randn((B, C, H, W), generator=g)
    s = torch.exp(torch.randn((B, C, H, W), generator=g))
    if name == "sigma-classes":       # below the floor, zero, negative, and so wide that every bin is tiny
        s[:, 0], s[:, 1], s[:, 2], s[:, 3] = 0.05, 0.0, -2.0, 1e4
        s[1, 3] = 1e6                  # 1e4 leaves 4e-5 a bin, above the floor; 1e6 is floored everywhere
    elif name == "mu-50":             # upper - lower = 0: the floor applies
        m = torch.where(torch.rand((B, C, H, W), generator=g) < 0.5, -50.0, 50.0)
    elif name == "mu-half-integers":
        m = torch.randint(-6, 6, (B, C, H, W), generator=g).float() + 0.5
    elif name == "one-pixel-dominates":
        H, W = 33, 47
        y = torch.randn((B, C, H, W), generator=g) * 3
        lik = torch.rand((B, C, H, W), generator=g).clamp(min=1e-9)
        s = torch.full((B, C, H, W), 0.11)
        m = torch.full((B, C, H, W), 50.0)       # every pixel on the floor ...
        m[:, :, 17, 23] = 0.0                     # ... but one, whose mass is all in the centre bin
    return y, s, m, lik, -5.5, 11


CASES = tuple(SHAPES) + SPECIAL


class Ref:
    """The CPU reference of one case, computed once."""

    def __init__(self, name):
        self.inputs = random_case(name) if name in SHAPES else special_case(name)
        y, s, m, lik, vmin, nbins = self.inputs
        self.hist = R.histc(y, vmin, nbins)
        self.pred64 = R.predicted(s, m, vmin, nbins, torch.float64)
        self.pred32 = R.predicted(s, m, vmin, nbins, torch.float32)
        self.d32 = float((self.pred32.double() - self.pred64).abs().max())
        self.pixels = y.shape[2] * y.shape[3]
        if lik is not None:
            self.bits64 = R.bits(lik, torch.float64)
            self.dbits = (R.bits(lik, torch.float32).double() - self.bits64).abs()
            self.bits_terms = torch.log2(lik.double()).abs().sum(dim=(2, 3))


@pytest.fixture(scope="module")
def refs():
    out = {name: Ref(name) for name in CASES}
    out["d32"] = max(r.d32 for r in out.values())
    return out


def run(LD, y, s, m=None, lik=None, vmin=-5.5, nbins=11):
    d = LD.latent_distrib(R.to_nc4(y).to(DEV), y.shape[1], R.to_nc4(s).to(DEV),
                          None if m is None else R.to_nc4(m).to(DEV), None if lik is None else R.to_nc4(lik).to(DEV),
                          vmin, nbins)
    return d.hist.cpu(), d.pred.cpu(), None if d.bits is None else d.bits.cpu()


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_restatement(LD, refs, name):
    ref, d32 = refs[name], refs["d32"]
    y, s, m, lik, vmin, nbins = ref.inputs
    hist, pred, bits = run(LD, *ref.inputs)
    assert hist.dtype == torch.int32 and hist.shape == ref.hist.shape
    assert torch.equal(hist.long(), ref.hist)
    lo, hi = torch.tensor(vmin, dtype=torch.float32), torch.tensor(R.vmax_of(vmin, nbins), dtype=torch.float32)
    outside = ((y < lo) | (y > hi)).sum(dim=(2, 3))
    assert torch.equal(ref.pixels - hist.long().sum(-1), outside)
    assert pred.dtype == torch.float32 and bool(torch.isfinite(pred).all())
    dev = float((pred.double() - ref.pred64).abs().max())
    print(f"{name}: d32 (all cases) {d32:.3e}  this case {ref.d32:.3e}  device {dev:.3e}")
    assert dev <= 4 * d32
    # and per case: the case's own d32, but no less than one fp32 ulp of the value (the result is an fp32 number)
    own = 4 * torch.clamp(2.0 ** -23 * ref.pred64, min=ref.d32)
    print(f"{name}: worst share of the per-case bound {float(((pred.double() - ref.pred64).abs() / own).max()):.3f}")
    assert bool(((pred.double() - ref.pred64).abs() <= own).all())
    if lik is None:
        assert bits is None
        return
    diff = (bits.double() - ref.bits64).abs()
    bound = ref.pixels * 2.0 ** -24 * ref.bits_terms + float(ref.dbits.max())
    print(f"{name}: bits device {float(diff.max()):.3e}  float32 restatement {float(ref.dbits.max()):.3e}  "
          f"worst share of the bound {float((diff / bound).max()):.3f}")
    assert bool((diff <= bound).all())


def test_hist_edges_and_non_finite(LD):
    vmin, nbins = -5.5, 11
    f32 = torch.float32
    edges = torch.arange(nbins + 1, dtype=f32) + vmin                  # vmin, every inner edge, vmax: all exact
    inf = torch.tensor(float("inf"))
    below = torch.nextafter(edges[0], -inf)
    above = torch.nextafter(edges[-1], inf)
    y = torch.zeros((1, 4, 4, 5))
    y[0, 0].view(-1)[:12] = edges
    y[0, 0].view(-1)[12:16] = torch.stack([below, above, torch.nextafter(edges[0], inf), torch.nextafter(edges[-1], -inf)])
    y[0, 1] = torch.randn((4, 5), generator=torch.Generator().manual_seed(1)) * 3
    y[0, 1, 0, 0], y[0, 1, 3, 4] = float("nan"), float("inf")           # first and last pixel of the plane
    y[0, 2] = y[0, 1]
    y[0, 2, 0, 0], y[0, 2, 3, 4] = float("-inf"), float("nan")
    y[0, 3] = 100.0                                                       # all outside
    y[0, 3, 1, 1] = -100.0
    s = torch.ones_like(y)
    hist, pred, _ = run(LD, y, s)
    want = torch.stack([torch.histc(p[torch.isfinite(p)], bins=nbins, min=vmin, max=vmin + nbins) for p in y[0]]).long()
    assert torch.equal(hist[0].long(), want)
    assert want[0].tolist() == [2, 1, 1, 1, 1, 5, 1, 1, 1, 1, 3]         # vmax and the float below it close the last bin
    assert int(want[1].sum()) == 18 and int(want[2].sum()) == 18 and not want[3].any()
    assert 20 - int(hist[0, 0].sum()) == 2
    assert bool(torch.isfinite(pred).all())
    # every value outside, NaN scales and means: the kernel returns, pred carries the NaN, hist does not move
    s[0, 0, 0, 0] = float("nan")
    hist2, pred2, _ = run(LD, torch.full_like(y, float("nan")), s, torch.zeros_like(y))
    assert not hist2.any() and bool(torch.isnan(pred2[0, 0]).all()) and bool(torch.isfinite(pred2[0, 1:]).all())


def test_a_row_is_the_same_alone_in_a_batch_and_again(LD):
    g = torch.Generator().manual_seed(7)
    B, C, H, W = 3, 8, 130, 127                                          # the capped split: 64 partials a row
    y = torch.randn((B, C, H, W), generator=g) * 3
    s = torch.exp(torch.randn((B, C, H, W), generator=g))
    m = torch.randn((B, C, H, W), generator=g)
    lik = torch.rand((B, C, H, W), generator=g).clamp(min=1e-9)
    a = run(LD, y, s, m, lik)
    b = run(LD, y, s, m, lik)
    one = run(LD, y[1:2], s[1:2], m[1:2], lik[1:2])
    for ta, tb, to in zip(a, b, one):
        assert torch.equal(ta, tb)
        assert torch.equal(to[0], ta[1])
    small = [t[:, :, :7, :9].contiguous() for t in (y, s, m, lik)]      # one block a plane
    a = run(LD, *small)
    one = run(LD, *[t[1:2] for t in small])
    for ta, to in zip(a, one):
        assert torch.equal(to[0], ta[1])


def test_channel_rate_on_device_tensors(LD, refs):
    for name in ("3x8x33x47", "2x320x4x6-64bins"):
        y, s, m, lik, vmin, nbins = refs[name].inputs
        d = LD.latent_distrib(R.to_nc4(y).to(DEV), y.shape[1], R.to_nc4(s).to(DEV), R.to_nc4(m).to(DEV), None,
                              vmin, nbins)
        rate = LD.channel_rate(d.hist, d.pred)
        assert rate.is_cuda and rate.dtype == torch.float32
        hist, pred = d.hist.cpu().double(), d.pred.cpu().double()
        want = (hist * -torch.log(pred)).sum(-1) / math.log(2)
        terms = (hist * torch.log(pred).abs()).sum(-1) / math.log(2)
        diff = (rate.cpu().double() - want).abs()
        print(name, "channel_rate worst share of (nbins + 1) 2^-23 sum|terms|:",
              float((diff / ((nbins + 1) * 2.0 ** -23 * terms)).max()))
        assert bool((diff <= (nbins + 1) * 2.0 ** -23 * terms).all())


def err_bound(hist, pred64, hist_adv, pred64_adv, d32):
    """The per-channel bound on |err - err64| propagated from the pred tolerance: sum_k hist_k * delta / (pred_k * ln 2)
    with delta = 4 * d32, the clean plus the adversarial side."""
    return sum((h.double() * (4 * d32) / (p * math.log(2))).sum(-1) for h, p in ((hist, pred64), (hist_adv, pred64_adv)))


def rate_eval_bound(hist, pred64, hist_adv, pred64_adv, nbins):
    """What channel_rate's own fp32 evaluation may add to err, (nbins + 1) * 2^-23 * sum |terms| per side and one
    rounding of the difference: used only to widen the margin the ranking must be separated by."""
    total = 0.0
    for h, p in ((hist.double(), pred64), (hist_adv.double(), pred64_adv)):
        terms = (h * torch.log(p).abs()).sum(-1) / math.log(2)
        total = total + ((nbins + 1) * 2.0 ** -23 + 2.0 ** -24) * terms
    return total


def test_rate_gap_and_ranking(LD):
    g = torch.Generator().manual_seed(11)
    B, C, H, W = 2, 8, 33, 47
    y = torch.randn((B, C, H, W), generator=g) * 0.8
    s = torch.ones((B, C, H, W)) + 0.2 * torch.rand((B, C, H, W), generator=g)
    m = 0.1 * torch.randn((B, C, H, W), generator=g)
    shift = 0.5 * torch.arange(C, dtype=torch.float32)                  # grows with the channel number
    y_adv = y + shift.view(1, C, 1, 1)
    hist, hist_adv = R.histc(y), R.histc(y_adv)
    p64, p32 = R.predicted(s, m), R.predicted(s, m, dtype=torch.float32)
    d32 = float((p32.double() - p64).abs().max())
    err64, index64 = R.rate_gap(hist, p64, hist_adv, p64)
    bound = err_bound(hist, p64, hist_adv, p64, d32)
    # the float64 restatement separates every adjacent pair of the ranking by more than twice the bound, here
    # widened by the fp32 evaluation of the rate (a stricter demand on the inputs, not on the device)
    sorted_err = err64.gather(1, index64)
    sorted_bound = (bound + rate_eval_bound(hist, p64, hist_adv, p64, 11)).gather(1, index64)
    gaps = sorted_err[:, :-1] - sorted_err[:, 1:]
    need = 2 * torch.maximum(sorted_bound[:, :-1], sorted_bound[:, 1:])
    print("adjacent gaps", gaps.min().item(), "needed", need.max().item(), "d32", d32)
    assert bool((gaps > need).all())
    to = lambda t: R.to_nc4(t).to(DEV)
    clean = LD.latent_distrib(to(y), C, to(s), to(m))
    adv = LD.latent_distrib(to(y_adv), C, to(s), to(m))
    assert torch.equal(clean.hist.cpu().long(), hist) and torch.equal(adv.hist.cpu().long(), hist_adv)
    err, index = LD.rate_gap(clean, adv)
    diff = (err.cpu().double() - err64).abs()
    print("err share of its bound per channel", (diff / bound.clamp(min=1e-300)).tolist(), "largest |err - err64|",
          float(diff.max()))
    assert bool((diff <= bound).all())
    assert torch.equal(index.cpu(), index64)
    assert index64[0].tolist() == list(range(C - 1, -1, -1))


def test_status_codes(LD):
    from imagecompression_adversarial_amd._lib import lib, ptr, stream
    import ctypes
    L = lib()
    B, C, H, W, nbins = 1, 8, 4, 4, 11
    y4 = torch.zeros((B, 2, H, W, 4), device=DEV)
    s4 = torch.ones((B, 2, H, W, 4), device=DEV)
    hist = torch.full((B, C, nbins), -1, dtype=torch.int32, device=DEV)
    pred = torch.full((B, C, nbins), -1.0, device=DEV)
    bits = torch.full((B, C), -1.0, device=DEV)
    work = torch.full((L.ica_latent_distrib_ws_size(B, C, H, W, nbins) + 64,), -1.0, device=DEV)
    assert L.ica_latent_distrib_ws_size(B, C, H, W, nbins) == B * C * (nbins + 1)

    def status(y=y4, s=s4, m=None, lik=None, C=C, nbins=nbins, hist=hist, pred=pred, bits=bits, work=work, B=B):
        as_ptr = lambda t: t if isinstance(t, ctypes.c_void_p) or t is None else ptr(t)
        return L.ica_latent_distrib(as_ptr(y), as_ptr(s), as_ptr(m), as_ptr(lik), B, C, H, W, -5.5, nbins, 0.11,
                                    1 / 65536, as_ptr(hist), as_ptr(pred), as_ptr(bits), as_ptr(work), stream())

    off = ctypes.c_void_p(s4.data_ptr() + 4)                              # 4-byte aligned only
    assert status(C=6) == -2 and status(C=0) == -2
    assert status(nbins=0) == -5 and status(nbins=65) == -5
    assert status(B=0) == -5 and status(y=None) == -5 and status(hist=None) == -5 and status(work=None) == -5
    assert status(lik=s4, bits=None) == -5
    assert status(s=off) == -5 and status(m=off) == -5
    assert status(pred=s4) == -7 and status(hist=y4) == -7 and status(work=s4) == -7 and status(bits=pred) == -7
    for C_, nb_ in ((6, 11), (8, 0), (8, 65)):
        assert L.ica_latent_distrib_ws_size(B, C_, H, W, nb_) == 0
    torch.cuda.synchronize()
    for t in (hist, pred, bits, work):                                    # nothing was launched or cleared
        assert bool((t == -1).all())
    assert bool((s4 == 1).all())
    with pytest.raises(ValueError, match="multiple of 4|nChw4c"):
        LD.latent_distrib(torch.zeros((1, 2, 4, 4, 4), device=DEV), 6, torch.ones((1, 2, 4, 4, 4), device=DEV))
    for nb_ in (0, 65):
        with pytest.raises(ValueError, match="nbins"):
            LD.latent_distrib(y4, C, s4, nbins=nb_)
    with pytest.raises(ValueError, match="must match"):
        LD.latent_distrib(y4, C, torch.ones((2, 2, H, W, 4), device=DEV))
    assert status() == 0                                                  # and the same call, accepted, runs
    torch.cuda.synchronize()
    assert hist.cpu()[0, :, 5].tolist() == [H * W] * C and int(hist.sum()) == C * H * W


# --------------------------------------------------------------------------- #
# the models
# --------------------------------------------------------------------------- #
def make_kern(model, q, precision=None):
    from imagecompression_adversarial_amd import visual_distribution as V
    from imagecompression_adversarial_amd.random_noise import _kern
    argv = ["-m", model, "-q", str(q), "-metric", "mse", "--synthetic-weights", "--attack"]
    return _kern(V.parse(argv + (["--precision", precision] if precision else [])))


def planar(t4, C):
    return None if t4 is None else R.from_nc4(t4.cpu())[:, :C]


MODELS = [("hyper", 1, 64, 64, None), ("hyper", 1, 128, 192, None), ("context", 1, 64, 64, None),
          ("cheng2020", 1, 64, 64, None), ("hyper", 6, 64, 64, None), ("hyper", 1, 64, 64, "bf16")]


@pytest.mark.parametrize("model,q,H,W,precision", MODELS,
                         ids=["%s-q%d-%dx%d-%s" % (m, q, h, w, p or "default") for m, q, h, w, p in MODELS])
def test_study_against_the_restatement_on_the_engines_own_tensors(LD, model, q, H, W, precision):
    kern = make_kern(model, q, precision)
    assert kern.M == (320 if q == 6 else 128 if model == "cheng2020" else 192)
    check_study(LD, kern, H, W, f"{model} q{q} {H}x{W} {precision}")


def test_study_on_a_model_with_live_latents(LD):
    """Seeded default weights leave y near 0 and the hyperprior's scales on the floor; here the last layers of g_a
    and h_s are scaled up (as tests/test_gpu_recompress.py does for g_a), so y spreads over the bins and past them
    (9 % in the centre bin, 20 % outside on the CPU oracle) and a third of the scales lie above the floor."""
    from oracle import codec
    from imagecompression_adversarial_amd.engine import CodecKernels
    P = codec.perturb_params(codec.init_params("hyper", 1, seed=0), seed=1)
    P["g_a.6.weight"] = P["g_a.6.weight"] * 120.0
    P["h_s.4.weight"] = P["h_s.4.weight"] * 40.0
    kern = CodecKernels({k: v.to(DEV) for k, v in P.items()}, "hyper", "fp32")
    spread = check_study(LD, kern, 128, 192, "hyper q1 128x192 scaled g_a.6")
    assert 0.02 < spread < 0.98           # a real share of the latent lies outside the centre bin


def check_study(LD, kern, H, W, label):
    """study() on a seeded pair against the restatement fed the engine's own tensors; returns the share of the clean
    latent outside the centre bin."""
    model = kern.model
    g = torch.Generator().manual_seed(H + W)
    im = torch.rand((2, 3, H, W), generator=g)
    im_adv = torch.clamp(im + 0.05 * torch.randn((2, 3, H, W), generator=g), 0.0, 1.0)
    st = LD.study(kern, im.to(DEV), im_adv.to(DEV), keep_inputs=True)
    assert LD.study(kern, im.to(DEV), im_adv.to(DEV)).clean.inputs == ()
    C, px = kern.M, (H // 16) * (W // 16)
    assert st.err.shape == (2, C) and st.clean.pixels == px and st.clean.hist.shape == (2, C, 11)
    side = []
    for d in (st.clean, st.adv):
        y, s, m, lik = (planar(t, C) for t in d.inputs)        # kept by keep_inputs=True
        assert y.dtype == torch.float32 and (m is None) == (model == "hyper")
        hist = R.histc(y)
        p64, p32 = R.predicted(s, m), R.predicted(s, m, dtype=torch.float32)
        d32 = float((p32.double() - p64).abs().max())
        dev = float((d.pred.cpu().double() - p64).abs().max())
        assert torch.equal(d.hist.cpu().long(), hist)
        b64 = R.bits(lik)
        dbits = float((R.bits(lik, torch.float32).double() - b64).abs().max())
        bdiff = (d.bits.cpu().double() - b64).abs()
        bbound = px * 2.0 ** -24 * torch.log2(lik.double()).abs().sum(dim=(2, 3)) + dbits
        print(f"{label}: d32 {d32:.3e} device {dev:.3e}; bits device {float(bdiff.max()):.3e} "
              f"float32 restatement {dbits:.3e}; in-range share {float(hist.sum()) / (2 * C * px):.3f}")
        assert dev <= 4 * d32
        assert bool((bdiff <= bbound).all())
        side.append((hist, p64, d32))
    (h0, p0, d0), (h1, p1, d1) = side
    err64, _ = R.rate_gap(h0, p0, h1, p1)
    bound = err_bound(h0, p0, h1, p1, max(d0, d1))
    diff = (st.err.cpu().double() - err64).abs()
    print("  err worst share of its bound", float((diff / bound.clamp(min=1e-300)).max()))
    assert bool((diff <= bound).all())
    assert torch.equal(st.channel_index.cpu(), torch.argsort(st.err.cpu(), dim=-1, descending=True, stable=True))
    assert torch.equal(st.outside.cpu(), px - h0.sum(-1)) and torch.equal(st.outside_adv.cpu(), px - h1.sum(-1))
    for frac, h in ((st.hist_frac, h0), (st.hist_frac_adv, h1)):      # one fp32 division on the device: one ulp
        want = h.double() / px
        assert frac.dtype == torch.float32 and bool(((frac.cpu().double() - want).abs() <= 2.0 ** -23 * want).all())
    assert torch.equal(st.bits, st.clean.bits) and torch.equal(st.bits_adv, st.adv.bits)
    return 1.0 - float(h0[:, :, 5].sum()) / (2 * C * px)


def test_factorized_is_refused(LD):
    kern = make_kern("factorized", 1)
    im = torch.rand((1, 3, 64, 64)).to(DEV)
    with pytest.raises(NotImplementedError, match="factorized"):
        LD.study(kern, im, im)


# --------------------------------------------------------------------------- #
# the CLI
# --------------------------------------------------------------------------- #
def block_lines(lines):
    """{image: its idx / err lines} of a CLI output"""
    out, cur = {}, None
    for ln in lines:
        if ln.startswith("[IMAGE]"):
            cur = out.setdefault(ln.split(None, 1)[1], [])
        elif ln.startswith("AVG:") or "\t" in ln:
            cur = None
        elif cur is not None:
            cur.append(ln.split())
    return out


def test_cli_on_files(tmp_path, capsys):
    from imagecompression_adversarial_amd import coder, visual_distribution as V
    g = torch.Generator().manual_seed(5)
    for i in range(2):
        im = torch.rand((1, 3, 64, 64), generator=g)
        coder.write_image(im, str(tmp_path / f"img{i}.png"))
        coder.write_image(torch.clamp(im + 0.05 * torch.randn(im.shape, generator=g), 0, 1), str(tmp_path / f"adv{i}.png"))
    save = tmp_path / "out" / "distrib.pt"
    out = V.main(["-m", "hyper", "-metric", "mse", "-q", "1", "--synthetic-weights", "--batch", "2", "-k", "2", "--table",
                  "-s", str(tmp_path / "img*.png"), "-t", str(tmp_path / "adv*.png"), "--save", str(save)])
    lines = capsys.readouterr().out.splitlines()
    blocks = block_lines(lines)
    assert sorted(blocks) == [str(tmp_path / "img0.png"), str(tmp_path / "img1.png")]
    C = 192
    saved = torch.load(save, map_location="cpu", weights_only=True)
    assert sorted(saved) == sorted(V.KEYS)
    for k in ("y_hat", "y_hat_t_hist", "y_pred", "y_pred_t"):
        assert saved[k].shape == (2, C, 11) and saved[k].dtype == torch.float32 and not saved[k].is_cuda
    for k in ("err", "bits", "bits_t"):
        assert saved[k].shape == (2, C)
    assert saved["channel_index"].shape == (2, C) and saved["channel_index"].dtype == torch.int64
    for b, name in enumerate(sorted(blocks)):
        rows = blocks[name]
        assert len(rows) == 2 and all(len(r) == 2 for r in rows)
        for i, (idx, err) in enumerate(rows):
            assert int(idx) == int(saved["channel_index"][b, i])
            assert math.isclose(float(err), float(saved["err"][b, int(idx)]), rel_tol=1e-6, abs_tol=1e-9)
    avg = [ln.split() for ln in lines if ln.startswith("AVG:")]
    assert len(avg) == 1 and len(avg[0]) == 4
    top1 = sum(float(saved["err"][b, saved["channel_index"][b, 0]]) for b in range(2)) / 2
    assert math.isclose(float(avg[0][1]), top1, rel_tol=1e-6, abs_tol=1e-9) and math.isclose(float(avg[0][1]), out["err_top1"])
    assert 0.0 <= float(avg[0][3]) <= 1.0
    table = [ln.split("\t") for ln in lines if "\t" in ln]
    assert len(table) == 2 * C and all(len(r) == 9 for r in table)
    assert [int(r[1]) for r in table[:C]] == list(range(C)) and table[C][0] == str(tmp_path / "img1.png")
    assert math.isclose(float(table[C + 3][2]), float(saved["err"][1, 3]), rel_tol=1e-6, abs_tol=1e-9)


def test_cli_attack(capsys):
    from imagecompression_adversarial_amd import visual_distribution as V
    out = V.main(["-m", "hyper", "-metric", "mse", "-q", "1", "--synthetic-weights", "-s", "synthetic:1x64x64",
                  "--attack", "-steps", "3"])
    lines = capsys.readouterr().out.splitlines()
    blocks = block_lines(lines)
    assert list(blocks) == ["synthetic_0"] and len(blocks["synthetic_0"]) == 3
    assert all(len(r) == 2 and 0 <= int(r[0]) < 192 and math.isfinite(float(r[1])) for r in blocks["synthetic_0"])
    avg = [ln.split() for ln in lines if ln.startswith("AVG:")]
    assert len(avg) == 1 and len(avg[0]) == 4 and math.isclose(float(avg[0][2]), out["gap_bits"])
