"""CPU tests of the surrogate backward of the JPEG round trip: the float64 autograd restatement
(tests/jpeg_bpda_restatement.py) against the forward restatement and against what the surrogate must give in the
cases where that is known in closed form, the recorded tolerance, and the argument plumbing of the loop and the CLI."""
import pytest
import torch

from tests import jpeg_bpda_restatement as P
from tests import jpeg_restatement as R


@pytest.mark.parametrize("name", P.CASES)
def test_forward_levels_are_the_forward_restatements(name):
    x, qs, sub = P.case(name)
    fwd = R.reference(name) if name in R.CASES else R.roundtrip(x, qs, sub, torch.float64)
    for s in P.SURROGATES:
        assert torch.equal(P.reference(name, s)["levels"], fwd["levels"])


@pytest.mark.parametrize("name", P.CASES)
def test_excluded_share_is_under_the_ceiling(name):
    ex, by_edge = P.excluded(name)
    share = float(ex.double().mean())
    print(name, "excluded share %.4f, MCUs the clamp-edge rule adds %d" % (share, by_edge))
    assert share <= R.FRAGILE_MAX
    if name == "batch-420":
        x, qs, _ = P.case(name)
        assert x.shape[0] == 2 and len(set(qs)) == 2 and x.shape[2] >= 32 and x.shape[3] >= 48


def test_mask_cases_have_active_clamps():
    """checker and out_of_range are the cases that exercise the masks: hundreds of active step-4 and step-7 clamps, and
    out_of_range's step-1 clamps."""
    for name in ("checker-420", "checker-444", "out_of_range-420", "out_of_range-444"):
        dec = P.reference(name, "ste")["dec"]
        n4 = sum(int(((dec[k] < 0) | (dec[k] > 255)).sum()) for k in ("s4_y", "s4_cb", "s4_cr"))
        n7 = int(((dec["s7"] < 0) | (dec["s7"] > 255)).sum())
        print(name, "active step-4 clamps", n4, "step-7", n7)
        assert (n4 >= 100 and n7 >= 100) if name.startswith("checker") else (n4 > 0 and n7 > 0)
    x = P.case("out_of_range-420")[0]
    assert int(((x < 0) | (x > 1)).sum()) > 100


def test_guard_covers_the_measured_error():
    m = P.measure_bwd()
    for k, v in m.items():
        print(k, "%.3g" % v)
    worst = max(m.values())
    assert worst <= P.MEASURED_BWD and P.MEASURED_BWD <= 1.05 * worst     # the record is the measurement, rounded up
    assert P.GUARD_BWD == 4 * P.MEASURED_BWD


def test_ste_at_444_without_clamps_returns_g():
    """With d = 1, no active clamp and no subsampling the Jacobian is (1 / 255) A^T B^T 255 with A the RGB -> YCbCr and
    B the YCbCr -> RGB matrix of JFIF, and the orthonormal DCT pair in between is the identity: g comes back up to
    how far B A is from the identity, that is within max_i sum_j |(B A - I)_ij| of max |g| per pixel."""
    A = torch.tensor([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]],
                     dtype=torch.float64)
    Bm = torch.tensor([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], dtype=torch.float64)
    E = (Bm @ A - torch.eye(3, dtype=torch.float64)).T          # g_x = (B A)^T g
    bound = float(E.abs().sum(dim=1).max())
    name = "16x16-444"
    ref = P.reference(name, "ste")
    dec = ref["dec"]
    assert all(not bool(((dec[k] < 0) | (dec[k] > 255)).any()) for k in dec if k.startswith("s"))
    x = P.case(name)[0]
    assert bool(((x >= 0) & (x <= 1)).all())
    g = P.cotangent(x.shape)
    gx = P.vjp(ref, g)
    err = float((gx - g.double()).abs().max())
    print("matrix bound %.3g x max|g| %.3g, error %.3g" % (bound, float(g.abs().max()), err))
    # + the float64 rounding of the DCT pair, far below the matrices' six decimals
    assert bound < 1e-5 and err <= bound * float(g.abs().max()) + 1e-12


@pytest.mark.parametrize("name", ["constant-420", "constant-444"])
def test_cubic_on_constant_is_zero(name):
    """Every coefficient of a constant block sits on an integer step, so 3 r^2 = 0 and the cubic gradient is exactly 0:
    in float64 and in the fp32 twin alike (the restatement's DC coefficient is exact: _dct_blocks)."""
    x, _, _ = P.case(name)
    gx = P.reference_vjp(name, "cubic", P.cotangent(x.shape))
    print(name, "max |g_x| per image", gx.abs().amax(dim=(1, 2, 3)).tolist())
    assert float(gx.abs().max()) == 0.0
    x, qs, sub = P.case(name)
    twin = P.forward(x, qs, sub, "cubic", torch.float32, forced=P.reference(name, "cubic")["dec"])
    assert float(P.vjp(twin, P.cotangent(x.shape)).abs().max()) == 0.0


def test_flag_and_argument_checks():
    from imagecompression_adversarial_amd import degrade, self_ensemble as SE
    assert degrade.JPEG_SURROGATES == ("ste", "cubic")
    parse = SE.config().parse_args
    assert parse(["-s", "x.png"]).jpeg_surrogate is None
    for s in degrade.JPEG_SURROGATES:
        assert parse(["-s", "x.png", "--adv", "--defend_m", "jpeg", "--jpeg-surrogate", s]).jpeg_surrogate == s
        degrade.validate_jpeg(quality=50, subsampling="420", surrogate=s)
    with pytest.raises(SystemExit):
        parse(["-s", "x.png", "--jpeg-surrogate", "linear"])
    with pytest.raises(ValueError, match="surrogate"):
        degrade.validate_jpeg(surrogate="linear")
    with pytest.raises(ValueError, match="surrogate"):
        SE.DefendedAttackLoop(None, None, "jpeg", surrogate="linear")
    with pytest.raises(ValueError):
        SE.DefendedAttackLoop(None, None, "jpeg", jpeg=(0, "420"), surrogate="ste")
    with pytest.raises(NotImplementedError, match="gradient"):
        SE.DefendedAttackLoop(None, None, "jpeg")
    with pytest.raises(NotImplementedError, match="gradient"):
        SE.DefendedAttackLoop(None, None, "jpeg", jpeg=(50, "444"), surrogate=None)
    with pytest.raises(NotImplementedError, match="gradient"):
        SE.main(["-s", "synthetic:1x64x64", "--adv", "--defend_m", "jpeg", "--synthetic-weights", "-device", "cpu"])
    with pytest.raises(ValueError, match="surrogate"):
        SE.adv_attack_batch(None, None, "jpeg", surrogate="linear")
