"""Training kernels (csrc/ica_train.hip) called directly: wgrad in its six instantiations against float64 autograd of
F.conv2d / F.conv_transpose2d, the one-sided selects bit for bit against fp32 torch, and the arithmetic pieces
against float64.

Every bound is 4 e_ref rounded up to one digit, e_ref being the distance of the fp32 CPU reference from the float64
one on the same seeded inputs (tests/test_cpu_loss_refs.py prints the table); rel_err = max |a - b| / max |b|.
"""
import pytest
import torch

from tests import loss_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (instantiation, channels and map): bound   e_ref
TOL_WGRAD = {
    ("k5s2", "3x33_9x33"): 2e-06,        # e_ref 3.87e-07
    ("k5s2", "33x3_5x40"): 2e-06,        # e_ref 3.24e-07
    ("k5s2", "70x37_1x1"): 3e-07,        # e_ref 5.67e-08
    ("k5s2", "70x37_7x7"): 2e-06,        # e_ref 3.15e-07
    ("k5s2", "128x128_9x33"): 5e-06,     # e_ref 1.00e-06
    ("k5s2d", "3x33_9x33"): 2e-06,       # e_ref 4.44e-07
    ("k5s2d", "33x3_5x40"): 2e-06,       # e_ref 4.80e-07
    ("k5s2d", "70x37_1x1"): 2e-07,       # e_ref 4.85e-08
    ("k5s2d", "70x37_7x7"): 2e-06,       # e_ref 2.98e-07
    ("k5s2d", "128x128_9x33"): 5e-06,    # e_ref 1.02e-06
    ("k3s1", "3x33_9x33"): 3e-06,        # e_ref 6.13e-07
    ("k3s1", "33x3_5x40"): 2e-06,        # e_ref 3.18e-07
    ("k3s1", "70x37_1x1"): 2e-07,        # e_ref 4.45e-08
    ("k3s1", "70x37_7x7"): 2e-06,        # e_ref 3.22e-07
    ("k3s1", "128x128_9x33"): 4e-06,     # e_ref 9.08e-07
    ("k1s1", "3x33_9x33"): 2e-06,        # e_ref 3.43e-07
    ("k1s1", "33x3_5x40"): 2e-06,        # e_ref 3.50e-07
    ("k1s1", "70x37_1x1"): 3e-07,        # e_ref 6.59e-08
    ("k1s1", "70x37_7x7"): 8e-07,        # e_ref 1.92e-07
    ("k1s1", "128x128_9x33"): 3e-06,     # e_ref 5.76e-07
    ("k3s2", "3x33_9x33"): 2e-06,        # e_ref 3.98e-07
    ("k3s2", "33x3_5x40"): 2e-06,        # e_ref 4.06e-07
    ("k3s2", "70x37_1x1"): 2e-07,        # e_ref 4.78e-08
    ("k3s2", "70x37_7x7"): 2e-06,        # e_ref 3.34e-07
    ("k3s2", "128x128_9x33"): 4e-06,     # e_ref 9.71e-07
    ("k1s2", "3x33_9x33"): 2e-06,        # e_ref 3.24e-07
    ("k1s2", "33x3_5x40"): 2e-06,        # e_ref 3.13e-07
    ("k1s2", "70x37_1x1"): 3e-07,        # e_ref 6.50e-08
    ("k1s2", "70x37_7x7"): 2e-06,        # e_ref 2.73e-07
    ("k1s2", "128x128_9x33"): 4e-06,     # e_ref 7.86e-07
    ("k5s1", "3x33_9x33"): 2e-06,        # e_ref 3.02e-07
    ("k5s1", "33x3_5x40"): 2e-06,        # e_ref 3.88e-07
    ("k5s1", "70x37_1x1"): 2e-07,        # e_ref 4.49e-08
    ("k5s1", "70x37_7x7"): 2e-06,        # e_ref 3.68e-07
    ("k5s1", "128x128_9x33"): 5e-06,     # e_ref 1.08e-06
}
TOL_GDN_XSQ = 3e-07                      # e_ref 7.08e-08
TOL_CHANNEL_SUM = {
    (5, False): 4e-07,                   # e_ref 9.24e-08
    (5, True): 2e-07,                    # e_ref 4.71e-08
    (128, False): 5e-07,                 # e_ref 1.23e-07
    (128, True): 2e-07,                  # e_ref 4.88e-08
}
TOL_MSE_GRAD = 4e-07                     # e_ref 7.60e-08


@pytest.fixture(scope="module")
def K():
    from imagecompression_adversarial_amd import hip_ops
    return hip_ops


def chunks(Sm):
    N, _, Hs, Ws = Sm.shape
    return N * Hs * ((Ws + 31) // 32)


def test_wgrad_cases_cover_both_partitions():
    """At least one case has more 32-pixel chunks than splits (the uneven partition: 36 chunks over 32 splits) and
    at least one has as many splits as chunks."""
    from imagecompression_adversarial_amd._lib import lib
    more, equal = 0, 0
    for kind in R.WGRAD_KINDS:
        for shape in R.WGRAD_SHAPES:
            Sm, Lg, KS, S, role = R.wgrad_case(kind, shape)
            n = chunks(Sm)
            ns = int(lib().ica_wgrad_nsplit(Sm.shape[1], Lg.shape[1], n))
            assert 1 <= ns <= n
            more += n > ns
            equal += n == ns
            if shape == "128x128_9x33":
                assert (n, ns) == (36, 32)
    assert more > 0 and equal > 0


@pytest.mark.parametrize("shape", list(R.WGRAD_SHAPES))
@pytest.mark.parametrize("kind", list(R.WGRAD_KINDS))
def test_wgrad_vs_float64(K, kind, shape):
    Sm, Lg, KS, S, role = R.wgrad_case(kind, shape)
    A, Bc = Sm.shape[1], Lg.shape[1]
    g64 = R.wgrad(Sm, Lg, KS, S, role)
    Sm4, Lg4 = K.to_nc4(Sm.to(DEV)), K.to_nc4(Lg.to(DEV))
    tol = TOL_WGRAD[(kind, shape)]
    out = torch.full((A, Bc, KS, KS), float("nan"), device=DEV)     # accumulate=False overwrites
    K.wgrad(Sm4, A, Lg4, Bc, KS, S, out, accumulate=False)
    e = R.rel_err(out.cpu(), g64)
    out0 = R.rnd((A, Bc, KS, KS), 77, -1, 1) * float(g64.abs().max())
    acc = out0.to(DEV).contiguous()
    K.wgrad(Sm4, A, Lg4, Bc, KS, S, acc, accumulate=True)             # accumulate=True: out + grad
    e_acc = R.rel_err(acc.cpu(), out0.double() + g64)
    print(f"wgrad {kind} {shape} {e:.2e} accumulate {e_acc:.2e}")
    assert e <= tol, (kind, shape, e, tol)
    assert e_acc <= tol, (kind, shape, e_acc, tol)


# --------------------------------------------------------------------------- #
# Selects: bit for bit against fp32 torch.  Lengths are no multiple of 256; inputs hold exact zeros, exact bounds
# and both signs of g.
# --------------------------------------------------------------------------- #
N_SEL = 2 * 2 * 11 * 13 * 4   # 2288, an nChw4c tensor [2, 2, 11, 13, 4]


def sel_inputs(seed, special):
    """(x, g): x uniform in [-1, 1] with the first elements cycling through `special`, g of both signs and zero."""
    x = R.rnd((N_SEL,), seed, -1, 1)
    sp = torch.tensor(special, dtype=torch.float32)
    x[: 8 * len(sp)] = sp.repeat(8)
    g = R.rnd((N_SEL,), seed + 1, -2, 2)
    g[::7] = 0.0
    g[: 8 * len(sp)] = torch.tensor([1.5, -1.5, 0.0, -0.0, 0.25, -0.25, 3.0, -3.0]).repeat_interleave(len(sp))
    assert N_SEL % 256 != 0 and int((g > 0).sum()) > 0 and int((g < 0).sum()) > 0
    return x, g


def test_relu_bwd_bit_for_bit(K):
    y, g = sel_inputs(401, [0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5])
    ref = torch.where(y > 0, g, torch.zeros_like(g))
    out = K.relu_bwd_(g.to(DEV).clone(), y.to(DEV))
    assert torch.equal(out.cpu(), ref)


def test_abs_bwd_bit_for_bit(K):
    x, g = sel_inputs(403, [0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5])
    ref = torch.where(x > 0, g, torch.where(x < 0, -g, torch.zeros_like(g)))
    out = K.abs_bwd_(g.to(DEV).clone(), x.to(DEV))
    assert torch.equal(out.cpu(), ref)


def test_lrelu_bwd_bit_for_bit(K):
    a, g = sel_inputs(405, [0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5])
    ref = torch.where(a > 0, g, g * torch.tensor(0.01))
    assert torch.equal(K.lrelu_bwd(g.to(DEV), a.to(DEV)).cpu(), ref)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("bound", [2.0 ** -18, float((1e-6 + 2.0 ** -36) ** 0.5)])
def test_reparam_bwd_bit_for_bit(K, bound, accumulate):
    """dp = dp' 2 max(p, bound) where p >= bound or the result is negative: p below / at / above the bound."""
    b = float(torch.tensor(bound, dtype=torch.float32))   # the bound as the kernel receives it
    bt = torch.tensor(b)
    below, above = float(torch.nextafter(bt, torch.tensor(0.0))), float(torch.nextafter(bt, torch.tensor(1.0)))
    p, gp = sel_inputs(407, [b, below, above, 0.0, -b, 2 * b, 0.5 * b, 1.0])
    assert int((p < b).sum()) > 0 and int((p == b).sum()) > 0 and int((p > b).sum()) > 0
    g = gp * 2.0 * torch.clamp(p, min=b)
    g = torch.where((p >= b) | (g < 0), g, torch.zeros_like(g))
    assert int(((p < b) & (g < 0)).sum()) > 0 and int(((p < b) & (gp > 0)).sum()) > 0
    out0 = R.rnd((N_SEL,), 409, -1, 1)
    ref = out0 + g if accumulate else g
    out = out0.to(DEV).clone() if accumulate else torch.full((N_SEL,), float("nan"), device=DEV)
    K.reparam_bwd(p.to(DEV), gp.to(DEV), out, b, accumulate=accumulate)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("inverse", [False, True])
def test_gdn_t_bit_for_bit(K, inverse):
    """GDN t = -0.5 g y s^2; IGDN t = 0.5 g y / s^2, and 0 where s == 0."""
    s, g = sel_inputs(411, [0.0, -0.0, 0.5, 2.0, 1e-3, 3.0])
    s = s.abs() + torch.where(s == 0, torch.tensor(0.0), torch.tensor(0.05))
    y = R.rnd((N_SEL,), 413, -3, 3)
    assert int((s == 0).sum()) > 0
    gy = g * y
    if inverse:
        ref = torch.where(s != 0, 0.5 * gy / (s * s), torch.zeros_like(gy))
    else:
        ref = -0.5 * gy * (s * s)
    assert bool(torch.isfinite(ref).all())
    shape = (2, 2, 11, 13, 4)
    out = K.gdn_t(g.reshape(shape).to(DEV), y.reshape(shape).to(DEV), s.reshape(shape).to(DEV), inverse)
    assert torch.equal(out.cpu().reshape(-1), ref)


# --------------------------------------------------------------------------- #
# Arithmetic: against float64
# --------------------------------------------------------------------------- #
def test_gdn_xsq_vs_float64(K):
    y, s = R.gdn_xsq_case()
    assert y.numel() % 256 != 0
    e = R.rel_err(K.gdn_xsq(y.to(DEV), s.to(DEV)).cpu(), R.gdn_xsq(y, s))
    print(f"gdn_xsq {e:.2e}")
    assert e <= TOL_GDN_XSQ


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("C", [5, 128])
def test_channel_sum_vs_float64(K, C, accumulate):
    x, out0 = R.channel_sum_case(C)
    assert x.shape[0] * x.shape[2] * x.shape[3] == 286
    out = out0.to(DEV).clone() if accumulate else torch.full((C,), float("nan"), device=DEV)
    K.channel_sum(K.to_nc4(x.to(DEV)), C, out, accumulate=accumulate)
    e = R.rel_err(out.cpu(), R.channel_sum(x, out0 if accumulate else None))
    print(f"channel_sum C{C} accumulate={accumulate} {e:.2e}")
    assert e <= TOL_CHANNEL_SUM[(C, accumulate)]


def test_mse_grad_vs_float64(K):
    xh, x, g0 = R.mse_grad_case()
    g4 = K.to_nc4(g0.to(DEV))
    g4[..., 3] = 7.0                                       # the padding lane is carried through untouched
    K.mse_grad_(K.to_nc4(xh.to(DEV)), x.to(DEV), g4, R.MSE_SCALE)
    e = R.rel_err(K.from_nc4(g4, 3).cpu(), R.mse_grad(xh, x, g0))
    print(f"mse_grad {e:.2e}")
    assert e <= TOL_MSE_GRAD
    assert bool((g4[..., 3] == 7.0).all())
