"""The float64-capable references of tests/loss_refs.py, on the CPU: in fp32 each equals the oracle's fp32 function,
and its distance from the float64 run on the GPU tests' own seeded inputs is e_ref.  The GPU tolerances
(tests/test_gpu_msssim_edges.py, test_gpu_entropy_kernels.py, test_gpu_train_kernels.py) are 4 e_ref rounded up to
one digit; `pytest -s tests/test_cpu_loss_refs.py` prints the table they were taken from.  e_ref: rel_err (max
|a - b| / max |b|) for tensors, max |log lik32 - log lik64| for likelihoods.
"""
import pytest
import torch

from oracle import codec
from oracle import msssim as omsssim
from tests import loss_refs as R

F32, F64 = torch.float32, torch.float64
TABLE = []


def record(name, e):
    TABLE.append((name, e))
    print(f"e_ref {name:44s} {e:9.2e}   4x -> {R.round_up_1digit(4 * e):.0e}")
    assert e == e and e < 1e-3, (name, e)   # finite, and a float32 distance


def test_round_up_rule():
    assert R.round_up_1digit(4 * 2.4e-6) == 1e-5
    assert R.round_up_1digit(4 * 5.0e-7) == 2e-6
    assert R.round_up_1digit(4 * 2.3e-5) == 1e-4
    assert R.round_up_1digit(1.2e-7) == 2e-7


# --------------------------------------------------------------------------- #
# MS-SSIM
# --------------------------------------------------------------------------- #
def test_torch_msssim_fp32_is_the_oracle():
    for shape in ((1, 3, 50, 70), (2, 3, 64, 64), (2, 3, 32, 48)):
        a, b = R.msssim_pair(shape)
        assert torch.equal(R.torch_msssim(a, b), omsssim.torch_msssim(a, b))
        assert R.torch_msssim(a.double(), b.double()).dtype == F64
    # 16x48 ends on a 1x3 map: the oracle (like the reference) pools once more after the last level and raises there
    a, b = R.msssim_pair((2, 3, 16, 48))
    with pytest.raises(RuntimeError):
        omsssim.torch_msssim(a, b)
    assert 0.5 < float(R.torch_msssim(a, b)) < 1.0
    a, b = R.msssim_pair((2, 3, 161, 163))
    assert omsssim.ms_ssim_per_image(a.double(), b.double()).dtype == F64


@pytest.mark.parametrize("name", list(R.MSSSIM_CASES))
def test_msssim_e_ref(name):
    mode, X, Y, dr, dval = R.msssim_case(name)
    v32, gx32, gy32 = R.msssim_value_and_grad(X, Y, dval, dr, mode, F32)
    v64, gx64, gy64 = R.msssim_value_and_grad(X, Y, dval, dr, mode, F64)
    assert v32.dtype == F32 and gx32.dtype == F32 and v64.dtype == F64 and gy64.dtype == F64
    record(f"msssim {name} value", R.rel_err(v32, v64))
    record(f"msssim {name} gX", R.rel_err(gx32, gx64))
    record(f"msssim {name} gY", R.rel_err(gy32, gy64))


def test_msssim_relu_case_reference():
    """Image 0 (Y = 1 - X) takes the relu branch: float64 value exactly 0 with a finite (zero) gradient; image 1 is
    what it would be alone."""
    X, Y, dval = R.msssim_relu_pair()
    v64, gx64, gy64 = R.msssim_value_and_grad(X, Y, dval)
    assert float(v64[0]) == 0.0 and 0.5 < float(v64[1]) < 1.0
    assert torch.isfinite(gx64).all() and torch.isfinite(gy64).all()
    assert float(gx64[0].abs().max()) == 0.0 and float(gy64[0].abs().max()) == 0.0
    v1, gx1, gy1 = R.msssim_value_and_grad(X[1:], Y[1:], dval[1:])
    assert max(R.rel_err(v1[0], v64[1]), R.rel_err(gx1[0], gx64[1]), R.rel_err(gy1[0], gy64[1])) < 1e-12
    v32, gx32, gy32 = R.msssim_value_and_grad(X, Y, dval, dtype=F32)
    record("msssim m0_relu value[1]", R.rel_err(v32[1], v64[1]))
    record("msssim m0_relu gX[1]", R.rel_err(gx32[1], gx64[1]))
    record("msssim m0_relu gY[1]", R.rel_err(gy32[1], gy64[1]))


# --------------------------------------------------------------------------- #
# Entropy models
# --------------------------------------------------------------------------- #
EB_FWD = [(C, hw, tr) for C in (5, 128) for hw in ((3, 5), (23, 23)) for tr in (False, True)]
GC_FWD = [(C, hw, tr, mn) for C in (6, 192) for hw in ((3, 5), (19, 19)) for tr in (False, True)
          for mn in (False, True)]


def both_sides(raw):
    """The float64 raw likelihood has elements on both sides of the floor and none within a factor 100 of it."""
    assert int((raw < R.LIK_FLOOR / 100).sum()) > 0 and int((raw > R.LIK_FLOOR * 100).sum()) > 0
    assert not bool(R._clear_band(raw).any())


@pytest.mark.parametrize("C,hw,training", EB_FWD)
def test_eb_fp32_is_the_oracle_and_e_ref(C, hw, training):
    N = 2
    P, z, noise = R.eb_case(C, N, *hw, training)
    v = R.eb_quantise(P, z, training, noise)
    zo, lo = codec.entropy_bottleneck(P, z, training=training, noise=noise)
    l32, s32 = R.eb_lik(P, v, F32)
    assert torch.equal(v, zo) and torch.equal(l32, lo) and l32.dtype == F32
    l64, s64 = R.eb_lik(P, v, F64)
    both_sides(R.eb_raw(P, v))
    assert float((P["entropy_bottleneck.quantiles"][:, 0, 1] == 0).sum()) == 0
    if not training:
        d = z - P["entropy_bottleneck.quantiles"][:, 0, 1].reshape(1, C, 1, 1)
        tie = (d - torch.floor(d)) == 0.5
        assert int((tie & (torch.floor(d) % 2 == 0)).sum()) > 0 and int((tie & (torch.floor(d) % 2 == 1)).sum()) > 0
    tag = f"eb C{C} {hw[0]}x{hw[1]} {'train' if training else 'eval'}"
    record(f"{tag} log lik", R.log_err(l32, l64))
    record(f"{tag} log-sum", R.rel_err(s32, s64))


@pytest.mark.parametrize("C,hw,training,with_means", GC_FWD)
def test_gc_fp32_is_the_oracle_and_e_ref(C, hw, training, with_means):
    y, s, means, noise = R.gc_case(C, 2, *hw, training, with_means)
    yh = R.gc_quantise(y, means, training, noise)
    yo, lo = codec.gaussian_conditional(y, s, means, training=training, noise=noise)
    l32, s32 = R.gc_lik(yh, s, means, F32)
    assert torch.equal(yh, yo) and torch.equal(l32, lo)
    l64, s64 = R.gc_lik(yh, s, means, F64)
    both_sides(R.gc_raw(yh, s, means))
    assert int((s < 0.10001).sum()) > 0 and int((s > 0.11999).sum()) > 0 and not bool(((s - 0.11).abs() < 0.00999).any())
    tag = f"gc C{C} {hw[0]}x{hw[1]} {'train' if training else 'eval'} {'means' if with_means else 'nomeans'}"
    record(f"{tag} log lik", R.log_err(l32, l64))
    record(f"{tag} log-sum", R.rel_err(s32, s64))


@pytest.mark.parametrize("C", [6, 192])
def test_gc_bwd_e_ref(C):
    yt, s, gl = R.gc_bwd_case(C, 2, 11, 13)
    gy32, gs32, _ = R.gc_bwd(yt, s, gl, F32)
    gy64, gs64, _ = R.gc_bwd(yt, s, gl, F64)
    assert gy32.dtype == F32
    record(f"gc_bwd C{C} gy", R.rel_err(gy32, gy64))
    record(f"gc_bwd C{C} gs", R.rel_err(gs32, gs64))


@pytest.mark.parametrize("C", [5, 128])
def test_eb_bwd_e_ref(C):
    P, v, gl = R.eb_bwd_case(C, 2, 11, 13)
    gv32, gp32 = R.eb_bwd(P, v, gl, F32)
    gv64, gp64 = R.eb_bwd(P, v, gl, F64)
    record(f"eb_bwd C{C} gv", R.rel_err(gv32, gv64))
    g0 = R.eb_grad_init(gp64)   # what the scatter accumulates onto
    for n in R.EB_NAMES:
        record(f"eb_bwd C{C} {n}", R.rel_err(g0[n] + gp32[n], g0[n].double() + gp64[n]))


# --------------------------------------------------------------------------- #
# Weight gradients and the arithmetic pieces
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", list(R.WGRAD_SHAPES))
@pytest.mark.parametrize("kind", list(R.WGRAD_KINDS))
def test_wgrad_e_ref(kind, shape):
    Sm, Lg, KS, S, role = R.wgrad_case(kind, shape)
    g32, g64 = R.wgrad(Sm, Lg, KS, S, role, F32), R.wgrad(Sm, Lg, KS, S, role, F64)
    assert g32.dtype == F32 and tuple(g64.shape) == (Sm.shape[1], Lg.shape[1], KS, KS)
    record(f"wgrad {kind} {shape}", R.rel_err(g32, g64))


def test_wgrad_is_the_conv_weight_gradient():
    """The reference is the plain definition: out[a][b][k] = sum Sm[n][a][p] Lg[n][b][S p + k - KS//2]."""
    Sm, Lg, KS, S, role = R.wgrad_case("k3s2", "70x37_7x7")
    ref = R.wgrad(Sm, Lg, KS, S, role)
    Lp = torch.nn.functional.pad(Lg.double(), (1, 1, 1, 1))
    for ky, kx in ((0, 0), (1, 2), (2, 1)):
        win = Lp[:, :, ky:ky + 2 * 7:2, kx:kx + 2 * 7:2]
        assert R.rel_err(torch.einsum("nahw,nbhw->ab", Sm.double(), win), ref[:, :, ky, kx]) < 1e-12


def test_arithmetic_e_ref():
    y, s = R.gdn_xsq_case()
    record("gdn_xsq", R.rel_err(R.gdn_xsq(y, s, F32), R.gdn_xsq(y, s, F64)))
    for C in (5, 128):
        x, out0 = R.channel_sum_case(C)
        record(f"channel_sum C{C}", R.rel_err(R.channel_sum(x, None, F32), R.channel_sum(x, None, F64)))
        record(f"channel_sum C{C} accumulate", R.rel_err(R.channel_sum(x, out0, F32), R.channel_sum(x, out0, F64)))
    xh, x, g0 = R.mse_grad_case()
    record("mse_grad", R.rel_err(R.mse_grad(xh, x, g0, F32), R.mse_grad(xh, x, g0, F64)))
