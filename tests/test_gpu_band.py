"""GPU tests of the band study and the band-limited attack (ica_band.hip, band_vi) against the float64 restatement
tests/band_restatement.py.

Stated tolerances.  Images and projections: max |got - float64| / max |float64| <= GUARD_PROJ; energies: per band
|got - float64| / mean(n^2) <= GUARD_ENERGY; the Adam kernel's gradient: GUARD_GRAD (each 4 x the fp32 twin's largest
difference, tests/band_restatement.py; no element is left out: the clamp is 1-Lipschitz and the gradient cases keep
im_s + p away from 0 and 1, asserted on the CPU by tests/test_cpu_band.py).  The means are sums of non-negative fp32
terms: 1e-5 relative of float64 over the same operands (MEAN_TOL of tests/test_gpu_degrade.py).  Everything is
bit-equal run to run, for an image alone and in a batch, for a variant alone and in a list; the fused step kernels
are bit-equal to the composition of band_vi.project with torch's per-pixel operations."""
import ctypes as C
import math

import pytest
import torch

from tests import band_restatement as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MEAN_TOL = 1e-5
E32 = float(torch.tensor(P.EPS, dtype=torch.float32))
V11 = P.preset_masks("only") + [0xFF, 0, 0b00100101]      # crosses the chunk of 8 variants


@pytest.fixture(scope="module")
def BV():
    from imagecompression_adversarial_amd import band_vi
    return band_vi


def ids(s):
    return "%dx%dx%d" % s


def rel(got, ref):
    return abs(got - ref) / ref


# --------------------------------------------------------------------------- #
# split
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("preset", list(P.PRESETS) + ["v11"])
@pytest.mark.parametrize("shape", P.SHAPES, ids=ids)
def test_split_vs_float64(BV, shape, preset):
    B, H, W = shape
    masks = V11 if preset == "v11" else P.preset_masks(preset)
    V = len(masks)
    im_s, im_adv = P.pair(shape, 100 + P.SHAPES.index(shape))
    sd, ad = im_s.to(DEV), im_adv.to(DEV)
    x, energy, mse_in = BV.split_bands(sd, ad, masks)
    assert x.shape == (V * B, 3, H, W) and energy.shape == (B, 8) and mse_in.shape == (V, B)
    x64, e64, _ = P.split(im_s, im_adv, masks)
    got = x.cpu().view(V, B, 3, H, W)
    err = P.rel_err(got, x64)
    n2 = ((im_adv.double() - im_s.double()) ** 2).mean(dim=(1, 2, 3))
    e_err = float(((energy.cpu().double() - e64).abs() / n2.view(-1, 1)).max())
    s_err = float(((energy.cpu().double().sum(1) - n2).abs() / n2).max())
    print(shape, preset, "image", err, P.GUARD_PROJ, "energy", e_err, "sum", s_err, P.GUARD_ENERGY)
    assert err <= P.GUARD_PROJ
    assert e_err <= P.GUARD_ENERGY and s_err <= P.GUARD_ENERGY
    m64 = ((got.double() - im_s.double()) ** 2).mean(dim=(2, 3, 4))      # over the kernel's own written image
    for v in range(V):
        for b in range(B):
            if float(m64[v, b]) == 0.0:
                assert float(mse_in[v, b]) == 0.0
            else:
                assert rel(float(mse_in[v, b]), float(m64[v, b])) < MEAN_TOL, (v, b)
    # twice; the energies alone; an image alone; a variant alone: the same bits
    again = BV.split_bands(sd, ad, masks)
    assert all(torch.equal(a, g) for a, g in zip(again, (x, energy, mse_in)))
    none = BV.split_bands(sd, ad)
    assert none[0] is None and none[2] is None and torch.equal(none[1], energy)
    xv = x.view(V, B, 3, H, W)
    if preset == "v11":
        for b in range(B if B > 1 else 0):
            x1, e1, m1 = BV.split_bands(sd[b:b + 1].contiguous(), ad[b:b + 1].contiguous(), masks)
            assert torch.equal(x1.view(V, 3, H, W), xv[:, b]) and torch.equal(e1[0], energy[b])
            assert torch.equal(m1[:, 0], mse_in[:, b])
        for v in range(V):
            x1, e1, m1 = BV.split_bands(sd, ad, [masks[v]])
            assert torch.equal(x1, xv[v]) and torch.equal(e1, energy) and torch.equal(m1[0], mse_in[v])


def _levels(shape, seed, lo=64, hi=192):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, (shape[0], 3, shape[1], shape[2]), generator=g).float() / 256.0


def test_split_block_constant_perturbation(BV):
    """A perturbation that is constant on every 8x8 block (exactly: all operands are multiples of 1 / 256) has
    exactly no energy outside band 0, and every `only` k >= 1 image is clamp01(im_s) bit for bit."""
    B, H, W = 3, 72, 136
    im_s = _levels((B, H, W), 7)
    g = torch.Generator().manual_seed(8)
    c = torch.randint(-16, 17, (B, 3, H // 8, W // 8), generator=g).float() / 256.0
    im_adv = im_s + c.repeat_interleave(8, 2).repeat_interleave(8, 3)
    assert torch.equal((im_adv.double() - im_s.double()).float() + im_s, im_adv)
    x, energy, mse_in = BV.split_bands(im_s.to(DEV), im_adv.to(DEV), "only")
    assert float(energy[:, 0].min()) > 0 and float(energy[:, 1:].abs().max()) == 0.0
    xv = x.view(8, B, 3, H, W).cpu()
    for k in range(1, 8):
        assert torch.equal(xv[k], torch.clamp(im_s, 0.0, 1.0)) and float(mse_in[k].abs().max()) == 0.0
    assert P.rel_err(xv[0], im_adv) <= P.GUARD_PROJ


@pytest.mark.parametrize("uv", [(0, 0), (3, 1), (2, 7), (7, 7), (5, 5), (0, 4)])
def test_split_single_basis_function(BV, uv):
    u, v = uv
    D = P.dct_matrix()
    n = 0.05 * torch.outer(D[u], D[v]).repeat(64 // 8, 192 // 8)
    im_s = torch.full((2, 3, 64, 192), 0.5)
    im_adv = (im_s.double() + n).float()
    _, energy, _ = BV.split_bands(im_s.to(DEV), im_adv.to(DEV))
    e = energy.cpu().double()
    share = e[:, max(u, v)] / e.sum(1)
    print(uv, (1 - share).tolist(), P.GUARD_ENERGY)
    assert float(share.min()) >= 1 - P.GUARD_ENERGY


def test_split_zero_perturbation(BV):
    im_s, _ = P.pair((3, 72, 136), 9)
    sd = im_s.to(DEV)
    x, energy, mse_in = BV.split_bands(sd, sd.clone(), V11)
    assert float(energy.abs().max()) == 0.0 and float(mse_in.abs().max()) == 0.0
    assert all(torch.equal(x.view(len(V11), *sd.shape)[v], sd) for v in range(len(V11)))


# --------------------------------------------------------------------------- #
# project
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", P.SHAPES, ids=ids)
def test_project(BV, shape):
    B = shape[0]
    im_s, im_adv = P.pair(shape, 100 + P.SHAPES.index(shape))
    x = im_adv - im_s
    xd = x.to(DEV)
    scale = float(x.abs().max())
    for preset in P.PRESETS:
        for m in P.preset_masks(preset):
            y = BV.project(xd, m)
            err = P.rel_err(y.cpu(), P.project(x.double(), m), scale)
            assert err <= P.GUARD_PROJ, (preset, m, err)
    z = BV.project(xd, 0)
    assert float(z.abs().max()) == 0.0
    m = 0b10100110
    y = BV.project(xd, m)
    assert P.rel_err(BV.project(y, m).cpu(), y.cpu(), scale) <= P.GUARD_PROJ                      # idempotent
    assert P.rel_err((y + BV.project(xd, 0xFF ^ m)).cpu(), x, scale) <= P.GUARD_PROJ              # complements
    assert torch.equal(BV.project(xd, m), y)
    for b in range(B if B > 1 else 0):
        assert torch.equal(BV.project(xd[b:b + 1].contiguous(), m)[0], y[b])


# --------------------------------------------------------------------------- #
# the step kernels
# --------------------------------------------------------------------------- #
def _prologue(noise, im_s, mask):
    from imagecompression_adversarial_amd import hip_ops as K
    from imagecompression_adversarial_amd._lib import call, lib, ptr, stream
    B, _, H, W = im_s.shape
    im_in4 = K.empty_nc4(B, 3, H, W, DEV)
    im_in4.fill_(float("nan"))
    loss_i = torch.empty(B, device=DEV)
    ws = torch.empty(lib().ica_band_prologue_ws_size(B, H, W), device=DEV)
    call("ica_band_prologue", ptr(noise), ptr(im_s), ptr(im_in4), ptr(loss_i), B, H, W, E32, mask, ptr(ws), stream())
    return im_in4, loss_i


@pytest.mark.parametrize("name", list(P.GRAD_CASES))
def test_prologue_is_the_composition(BV, name):
    from imagecompression_adversarial_amd import hip_ops as K
    noise, im_s, _, mask, _ = P.grad_case(name)
    nd, sd = noise.to(DEV), im_s.to(DEV)
    im_in4, loss_i = _prologue(nd, sd, mask)
    im_in = torch.clamp(sd + BV.project(torch.clamp(nd, -E32, E32), mask), 0.0, 1.0)
    want4 = K.to_nc4(im_in)
    print(name, "nan", int(torch.isnan(im_in4).sum()), "differing", int((im_in4 != want4).sum()),
          "max diff", float((im_in4 - want4).abs().nan_to_num(0.0).max()))
    assert torch.equal(im_in4, want4)
    l64 = ((im_s.double() - im_in.cpu().double()) ** 2).mean(dim=(1, 2, 3))
    for b in range(im_s.shape[0]):
        assert rel(float(loss_i[b]), float(l64[b])) < MEAN_TOL
    again = _prologue(nd, sd, mask)
    assert torch.equal(again[0], im_in4) and torch.equal(again[1], loss_i)
    for b in range(im_s.shape[0]):
        one = _prologue(nd[b:b + 1].contiguous(), sd[b:b + 1].contiguous(), mask)
        assert torch.equal(one[0][0], im_in4[b]) and torch.equal(one[1][0], loss_i[b])


def _adam(noise, im_s, g4, loss_i, mask, thr, gpos=None):
    from imagecompression_adversarial_amd._lib import call, ptr, stream
    B, _, H, W = im_s.shape
    nz, m, v = noise.clone(), torch.zeros_like(noise), torch.zeros_like(noise)
    im_in = torch.full_like(noise, float("nan"))
    branch = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    census = torch.zeros(B, dtype=torch.int32, device=DEV)
    call("ica_band_adam", ptr(nz), ptr(im_s), ptr(g4), ptr(loss_i), ptr(m), ptr(v), ptr(im_in), B, H, W, E32,
         float(thr), float(1.0 / (3 * H * W)), float((1 - 0.999) ** 0.5), float(-0.01 / (1 - 0.9)), ptr(branch),
         ptr(gpos), ptr(census), mask, stream())
    return nz, m, v, im_in, branch, census


@pytest.mark.parametrize("name", list(P.GRAD_CASES))
def test_adam_kernel_gradient(BV, name):
    from imagecompression_adversarial_amd import hip_ops as K
    noise, im_s, g_net, mask, thr = P.grad_case(name)
    nd, sd = noise.to(DEV), im_s.to(DEV)
    g4 = K.to_nc4(g_net.to(DEV))
    g4[..., 3] = float("nan")                        # the padding lane must never reach a result
    im_in4, loss_i = _prologue(nd, sd, mask)
    l = loss_i.tolist()
    assert l[0] > 2 * thr and l[1] < thr / 2         # thr a factor of two from both
    nz, m, v, im_in, branch, census = _adam(nd, sd, g4, loss_i, mask, thr)
    _, _, cheap, want = P.step(noise, im_s, g_net, mask, thr)
    assert branch.tolist() == [int(c) for c in cheap.tolist()] == [1, 0] and census.tolist() == [1, 0]
    assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all()) and bool(torch.isfinite(nz).all())
    err = P.rel_err(m.cpu().double() / 0.1, want)
    print(name, "gradient", err, P.GUARD_GRAD)
    assert err <= P.GUARD_GRAD
    assert torch.equal(K.to_nc4(im_in), im_in4)
    again = _adam(nd, sd, g4, loss_i, mask, thr)
    assert all(torch.equal(a, g) for a, g in zip(again, (nz, m, v, im_in, branch, census)))
    # the network gradient as a compacted one-row batch behind gpos
    gpos = torch.tensor([-1, 0], dtype=torch.int32, device=DEV)
    comp = _adam(nd, sd, g4[1:2].contiguous(), loss_i, mask, thr, gpos)
    assert all(torch.equal(a, g) for a, g in zip(comp, (nz, m, v, im_in, branch, census)))
    # an image alone
    for b in range(2):
        one = _adam(nd[b:b + 1].contiguous(), sd[b:b + 1].contiguous(), g4[b:b + 1].contiguous(),
                    loss_i[b:b + 1].contiguous(), mask, thr)
        assert torch.equal(one[0][0], nz[b]) and torch.equal(one[1][0], m[b]) and torch.equal(one[2][0], v[b])


# --------------------------------------------------------------------------- #
# the loop and the study on a small model
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def kern():
    from oracle import codec
    from imagecompression_adversarial_amd.engine import CodecKernels
    P_ = codec.perturb_params(codec.init_params("hyper", 1, seed=0), seed=1)
    return CodecKernels({k: v.to(DEV) for k, v in P_.items()}, "hyper")


def _outside_share(im_adv, im_s, mask):
    e = P.energies(im_adv.cpu().double() - im_s.cpu().double())
    out = sum(e[:, k] for k in range(8) if not mask >> k & 1)
    return (out / e.sum(1)).tolist()


def test_loop_stays_in_its_bands(BV, kern):
    from imagecompression_adversarial_amd.attack import attack_batch
    g = torch.Generator().manual_seed(21)
    im = (0.25 + 0.5 * torch.rand((2, 3, 64, 64), generator=g)).to(DEV)
    mask = BV.parse_bands("0-2")
    res = BV.band_attack_batch(kern, im, "0-2", steps=8, eval_msssim=False)
    assert float(res.im_adv.min()) > 0.0 and float(res.im_adv.max()) < 1.0     # no clamp acts: im_adv - im_s is p
    assert float((res.im_adv - im).abs().max()) > 1e-3
    share = _outside_share(res.im_adv, im, mask)
    print("out-of-band share", share, P.GUARD_ENERGY)
    assert max(share) <= P.GUARD_ENERGY
    again = BV.band_attack_batch(kern, im, "0-2", steps=8, eval_msssim=False)
    assert torch.equal(again.im_adv, res.im_adv) and torch.equal(again.noise, res.noise)
    one = BV.band_attack_batch(kern, im[:1].contiguous(), "0-2", steps=8, eval_msssim=False)
    assert torch.equal(one.im_adv[0], res.im_adv[0]) and torch.equal(one.noise[0], res.noise[0])
    plain = attack_batch(kern, im, steps=8, eval_msssim=False)
    assert min(_outside_share(plain.im_adv, im, mask)) > 0.01                  # the projection is what confines it


@pytest.fixture(scope="module")
def kern_live():
    """The same small model with g_a.6.weight x 40 (as scripts/bench_transfer.py): with the seeded weights every rounded
    latent is 0 (max |y| = 0.12), the reconstruction does not depend on the input and every mse_out would be 0."""
    from oracle import codec
    from imagecompression_adversarial_amd.engine import CodecKernels
    P_ = codec.perturb_params(codec.init_params("hyper", 1, seed=0), seed=1)
    P_["g_a.6.weight"] = P_["g_a.6.weight"] * 40.0
    return CodecKernels({k: v.to(DEV) for k, v in P_.items()}, "hyper")


def test_study_end_to_end(BV, kern_live):
    from imagecompression_adversarial_amd import hip_ops as K
    kern = kern_live
    from imagecompression_adversarial_amd.attack import eval_forward
    im_s, im_adv = P.pair((2, 64, 64), 31)
    sd, ad = im_s.to(DEV), im_adv.to(DEV)
    st = BV.band_study(kern, sd, ad, "only", batch=4)
    x, energy, mse_in = BV.split_bands(sd, ad, "only")
    assert torch.equal(st.energy, energy) and torch.equal(st.mse_in, mse_in) and st.masks == P.preset_masks("only")
    out_s, bpp_s = eval_forward(kern, sd)
    assert torch.equal(st.bpp_ori, bpp_s)
    for v in range(8):
        out, bpp = eval_forward(kern, x[2 * v:2 * v + 2].contiguous())
        mo = K.sqdiff_mean(out, out_s)
        for b in range(2):
            assert rel(float(st.mse_out[v, b]), float(mo[b])) < MEAN_TOL, (v, b)
            mi_, mo_ = float(st.mse_in[v, b]), float(st.mse_out[v, b])
            assert st.vi[v][b] == 10.0 * math.log10(mo_ / mi_)
        assert torch.equal(st.bpp[v], bpp), v


# --------------------------------------------------------------------------- #
# the C ABI's refusals
# --------------------------------------------------------------------------- #
def test_rejected_arguments(BV):
    from imagecompression_adversarial_amd._lib import lib, stream
    L = lib()
    B, H, W = 2, 16, 24
    n = B * 3 * H * W
    buf = torch.zeros(8 * n + 64, device=DEV)
    p = lambda off: C.c_void_p(buf.data_ptr() + 4 * off)      # noqa: E731
    a, b, c, d, e = (p(k * n) for k in range(5))
    wide = p(5 * n)                                           # room for [B][H][W][4] or two variants
    st = stream()
    ok = (C.c_int * 2)(1, 2)
    # project
    for args in ((a, 1, B, 12, W, b), (a, 1, B, H, 20, b), (a, 1, B, 0, W, b), (a, 1, 0, H, W, b), (a, 256, B, H, W, b),
                 (a, -1, B, H, W, b), (None, 1, B, H, W, b), (a, 1, B, H, W, None), (p(1), 1, B, H, W, b),
                 (a, 1, B, H, W, p(n + 1)), (a, 1, 65536, H, W, b)):
        assert L.ica_band_project(*args, st) == -5, args[1:5]
    assert L.ica_band_project(a, 1, B, H, W, a, st) == -7
    assert L.ica_band_project(a, 1, B, H, W, p(n - 4), st) == -7
    # split
    assert L.ica_band_split_ws_size(2, B, H, W) > 0
    for bad in ((0, B, H, W), (L.ica_band_max_variants() + 1, B, H, W), (2, 0, H, W), (2, B, 12, W), (2, B, H, 4)):
        assert L.ica_band_split_ws_size(*bad) == 0
    for V, hh, out, en, mse, ws, mk in ((0, H, wide, c, d, e, ok), (257, H, wide, c, d, e, ok), (2, 12, wide, c, d, e, ok),
                                        (2, H, wide, None, d, e, ok), (2, H, wide, c, d, None, ok),
                                        (2, H, wide, c, d, e, None), (2, H, None, c, d, e, ok),
                                        (2, H, p(5 * n + 1), c, d, e, ok), (2, H, wide, c, d, e, (C.c_int * 2)(1, 256))):
        assert L.ica_band_split(a, b, mk, V, B, hh, W, out, en, mse, ws, st) == -5, (V, hh)
    assert L.ica_band_split(a, b, ok, 2, B, H, W, a, c, d, e, st) == -7
    assert L.ica_band_split(a, b, ok, 2, B, H, W, p(n - 4), c, d, e, st) == -7
    # prologue
    assert L.ica_band_prologue_ws_size(B, H, W) > 0 and L.ica_band_prologue_ws_size(B, 12, W) == 0
    assert L.ica_band_prologue(a, b, wide, c, B, H, 20, 0.1, 7, d, st) == -5
    assert L.ica_band_prologue(a, b, wide, None, B, H, W, 0.1, 7, d, st) == -5
    assert L.ica_band_prologue(a, b, wide, c, B, H, W, 0.1, 300, d, st) == -5
    assert L.ica_band_prologue(a, b, a, c, B, H, W, 0.1, 7, d, st) == -7
    # adam
    s = (0.1, 1e-4, 1e-3, 0.03, -0.1)
    assert L.ica_band_adam(a, b, wide, c, d, e, None, B, 12, W, *s, None, None, None, 7, st) == -5
    assert L.ica_band_adam(a, b, wide, None, d, e, None, B, H, W, *s, None, None, None, 7, st) == -5
    assert L.ica_band_adam(a, b, wide, c, d, d, None, B, H, W, *s, None, None, None, 7, st) == -7
    assert L.ica_band_adam(a, a, wide, c, d, e, None, B, H, W, *s, None, None, None, 7, st) == -7
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                      # nothing was launched
