"""CPU checks of the JPEG round trip's definition (tests/jpeg_restatement.py), of the host tables and of the argument
checks of degrade's JPEG entry points.  No device is needed."""
import io
import pickle

import numpy as np
import pytest
import torch

from tests import jpeg_restatement as R


def test_tables_spot_values():
    from imagecompression_adversarial_amd import degrade
    for tables in (R.tables, lambda q: [list(t) for t in degrade.jpeg_tables(q)]):
        luma, chroma = tables(50)
        assert luma == R.LUMA and chroma == R.CHROMA
        assert luma[:8] == [16, 11, 10, 16, 24, 40, 51, 61] and luma[63] == 99 and chroma[:4] == [17, 18, 24, 47]
        assert all(v == 1 for t in tables(100) for v in t)
        assert all(v == 255 for t in tables(1) for v in t)
        assert tables(75)[0][0] == 8 and tables(25)[0][0] == 32
        assert len(luma) == len(chroma) == 64
    for q in range(1, 101):
        assert [list(t) for t in degrade.jpeg_tables(q)] == R.tables(q)


def test_dct_basis_is_orthonormal():
    # an entry of D D^T: 8 products of two entries each rounded once (cos, scale) and 7 additions, every value <= 1,
    # every rounding <= 2^-53: 8 * 3 + 7 = 31 roundings at most, 2^-48 = 32 * 2^-53
    D = R.dct_matrix()
    assert float((D @ D.T - torch.eye(8, dtype=torch.float64)).abs().max()) <= 2.0 ** -48


def test_guards_cover_the_measured_error():
    """GUARD is 4 x the largest fp32 - float64 difference per stage, measured here again over the case table."""
    worst = R.measure_guards()
    for s in R.STAGES:
        print(s, "measured %.3g, table %.3g, guard %.3g" % (worst[s], R.MEASURED[s], R.GUARD[s]))
        assert worst[s] <= R.MEASURED[s] * 1.02 and 4 * R.MEASURED[s] <= R.GUARD[s] <= 4.2 * R.MEASURED[s]


@pytest.mark.parametrize("name", R.CASES)
def test_fragile_share_is_under_the_ceiling(name):
    x, qs, sub = R.case(name)
    share = float(R.fragile(R.reference(name), sub).double().mean())
    print(name, "fragile share %.3f" % share)
    assert share <= R.FRAGILE_MAX


def test_constant_and_clamp_cases_do_what_they_are_for():
    for sub in ("420", "444"):
        x, _, _ = R.case("constant-" + sub)
        assert torch.equal(R.reference("constant-" + sub)["levels"], torch.round(x.double() * 255).long())
        r = R.reference("checker-" + sub)
        assert float(r["pre"]["s7"].max()) > 255 and float(r["pre"]["s7"].min()) < 0            # step 7 clamps
        s4 = torch.cat([r["pre"]["s4_" + p].flatten() for p in ("y", "cb", "cr")])
        assert float(s4.max()) > 255 and float(s4.min()) < 0                                    # step 4 clamps
        x, _, _ = R.case("out_of_range-" + sub)
        assert float(x.min()) < 0 and float(x.max()) > 1


@pytest.mark.parametrize("name", list(R.SWEEP_CASES))
def test_sweep_cases_keep_clear_of_the_budget(name):
    x, noise, sub, mse, frag = R.sweep_case(name)
    T = 1.01 * noise
    ks = [R.first_fit(mse[b], T) for b in range(x.shape[0])]
    print(name, ks)
    assert (ks[1] == -1 and ks[0] >= 0) if name.startswith("never") else (min(ks) >= 0 and ks[0] // 8 != ks[1] // 8)
    clean = 0
    for b, k in enumerate(ks):
        end = k + 1 if k >= 0 else 100
        assert float(((mse[b, :end] - T).abs() / T).min()) > R.BUDGET_GUARD, (b, k)
        assert float(frag[b, k]) <= R.FRAGILE_MAX if k >= 0 else True       # the winner itself is under the ceiling
        clean += int((frag[b, :R.visited(k)] == 0).sum())
    print(name, "visited candidates with no fragile MCU:", clean)
    assert clean >= R.CLEAN_MIN[name]


def test_argument_checks():
    from imagecompression_adversarial_amd import degrade
    for kw in (dict(quality=0), dict(quality=101), dict(quality=50.0), dict(quality=True), dict(quality=[50, 0]),
               dict(subsampling="422"), dict(subsampling=420), dict(H=24, W=32), dict(H=32, W=40),
               dict(H=32, W=32, noise=0.0), dict(H=12, W=16, subsampling="444")):
        with pytest.raises(ValueError):
            degrade.validate_jpeg(**kw)
    degrade.validate_jpeg(24, 40, [1, 100], "444")
    degrade.validate_jpeg(48, 80, 50, "420", noise=1e-4)
    with pytest.raises(ValueError):
        degrade.jpeg_tables(0)


@pytest.mark.parametrize("sub", ["444", "420"])
@pytest.mark.parametrize("q", [50, 75, 90])
def test_mse_agrees_with_pillow(sub, q):
    """mean((out - src)^2) in levels^2 of the restatement against libjpeg's (integer DCT, integer colour tables: a
    sample-wise match is not the claim).  PILLOW_GAP holds the measured relative gaps; each case is bounded by twice
    its gap.  Replicated chroma in the place of the triangle filter is some 7 % off at 4:2:0."""
    from PIL import Image, features
    if not features.check("jpg"):
        pytest.skip("Pillow was built without JPEG support")
    x = R.pillow_image()
    src = torch.round(x.double() * 255)
    ours = float(((R.roundtrip(x, [q], sub)["levels"].double() - src) ** 2).mean())
    buf = io.BytesIO()
    Image.fromarray(src[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(buf, "JPEG", quality=q,
                                                                          subsampling={"444": 0, "420": 2}[sub])
    dec = torch.from_numpy(np.array(Image.open(io.BytesIO(buf.getvalue())))).permute(2, 0, 1)[None].double()
    theirs = float(((dec - src) ** 2).mean())
    from imagecompression_adversarial_amd import degrade
    theirs_q = Image.open(io.BytesIO(buf.getvalue())).quantization
    want = [sorted(t) for t in degrade.jpeg_tables(q)]       # as multisets: Pillow's order (zigzag or not) varies
    assert [sorted(theirs_q[i]) for i in (0, 1)] == want and R.tables(q) == [list(t) for t in degrade.jpeg_tables(q)]
    gap = abs(ours - theirs) / theirs
    print(sub, q, "Pillow %.3f restatement %.3f gap %.3f %% (table %.3f %%)" % (theirs, ours, 100 * gap,
                                                                           100 * R.PILLOW_GAP[(sub, q)]))
    assert gap <= 2 * R.PILLOW_GAP[(sub, q)]


# --------------------------------------------------------------------------- #
# CLI plumbing
# --------------------------------------------------------------------------- #
def test_random_noise_modes_and_flag_defaults():
    from imagecompression_adversarial_amd import random_noise as RN
    parse = RN.config().parse_args
    a = parse(["-degrade", "jpeg", "-s", "x.png"])
    assert RN.mode(a) == "jpeg"
    assert (a.jpeg_quality, a.jpeg_subsampling, a.jpeg_budget, a.jpeg_dir) == (50, "420", False, None)
    assert RN.jpeg_dir(a) == "./attack/kodak/jpeg_q50"
    b = parse(["-degrade", "jpeg", "-s", "None", "-t", "x.png", "--jpeg-budget", "-noise", "1e-3"])
    assert RN.jpeg_dir(b) == "./attack/kodak/jpeg_mse0.001"      # coded at the budget's qualities, not at --jpeg-quality
    assert RN.jpeg_dir(parse(["-degrade", "jpeg", "-s", "x.png", "--jpeg-budget", "--jpeg-dir", "d"])) == "d"
    assert RN.mode(parse(["-degrade", "jpeg", "-s", "None", "-t", "x.png"])) == "generate_jpeg"
    assert RN.mode(parse(["-s", "None", "-t", "x.png"])) == "generate" and RN.mode(parse(["-s", "x.png"])) == "noise"
    assert RN.sweep_plan(parse(["-degrade", "jpeg", "-s", "x.png", "-q", "0", "-noise", "1e-3"])) == [
        (q, 1e-3) for q in range(1, 9)]
    with pytest.raises(ValueError):
        RN.mode(parse(["-degrade", "denoise", "-s", "x.png"]))
    with pytest.raises(ValueError):
        RN.mode(parse(["-degrade", "jpeg", "-s", "x.png", "--jpeg-quality", "0"]))
    with pytest.raises(ValueError):
        RN.mode(parse(["-degrade", "jpeg", "-s", "None"]))
    with pytest.raises(SystemExit):
        parse(["-degrade", "jpeg", "-s", "x.png", "--jpeg-subsampling", "422"])


def test_defend_m_jpeg_is_accepted_and_its_refused_uses_say_why():
    from imagecompression_adversarial_amd import batch_test, rd_eval, recompression, self_ensemble as SE
    assert "jpeg" in rd_eval.METHODS
    a = batch_test.config().parse_args(["-s", "x.png", "--defend", "--defend_m", "jpeg"])
    batch_test.check_args(a)
    assert (a.jpeg_quality, a.jpeg_subsampling) == (50, "420")
    # batch_test hands args.method on: the value carries the two settings, and is the plain string otherwise
    a = batch_test.config().parse_args(["-s", "x.png", "--defend", "--defend_m", "jpeg", "--jpeg-quality", "60",
                                        "--jpeg-subsampling", "444"])
    batch_test.check_args(a)
    assert a.method == "jpeg" and str(a.method) == "jpeg" and (a.method.quality, a.method.subsampling) == (60, "444")
    m = pickle.loads(pickle.dumps(a.method))
    assert m == "jpeg" and (m.quality, m.subsampling) == (60, "444")
    assert type(batch_test.config().parse_args(["--defend_m", "resize"]).method) is str
    a = batch_test.config().parse_args(["-s", "x.png", "--defend", "--defend_m", "jpeg", "--jpeg-quality", "101"])
    with pytest.raises(ValueError, match="1 .. 100"):
        rd_eval.rd_eval_defended(None, torch.zeros(1, 3, 64, 64), a.method)
    with pytest.raises(ValueError):
        rd_eval.rd_eval_defended(None, torch.zeros(1, 3, 64, 64), "jpeg", jpeg=(50, "422"))
    with pytest.raises(ValueError):
        batch_test.check_args(batch_test.config().parse_args(["-s", "x.png", "--defend", "--defend_m", "clip"]))
    with pytest.raises(NotImplementedError, match="gradient"):
        SE.DefendedAttackLoop(None, None, "jpeg")
    with pytest.raises(NotImplementedError, match="gradient"):
        SE.main(["-s", "synthetic:1x64x64", "--adv", "--defend_m", "jpeg", "--synthetic-weights", "-device", "cpu"])
    with pytest.raises(ValueError):
        recompression.check_args(recompression.config().parse_args(["-s", "x.png", "--defend", "--defend_m", "jpeg"]))
