"""CPU side of the latent-range feature (no GPU): the profile's order statistic and file format, the C-ABI
names, the CLI parsers, and the conditioning of the pinned inputs of tests/test_gpu_latent_range.py on the CPU
oracle (tests/latent_range_restatement.py)."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests import latent_range_restatement as R
from tests.conftest import rel_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ica_latent_range", "ica_latent_clamp", "ica_latent_clamp_bwd", "ica_latent_detect")


@pytest.mark.parametrize("N,topk", [(7, 3), (5, 5), (130, 100), (4, 1)])
def test_order_statistic_is_the_references_topk(N, topk):
    from imagecompression_adversarial_amd.latent_range import order_statistic
    g = torch.Generator().manual_seed(N)
    mx, mn = torch.randn((N, 12), generator=g), torch.randn((N, 12), generator=g)
    mx[:, 3] = mx[0, 3]   # ties
    cmax, cmin = order_statistic(mx, mn, topk)
    rmax, rmin = R.channel_profile(mx.view(N, 12, 1, 1), mn.view(N, 12, 1, 1), topk)
    assert torch.equal(cmax, rmax[:, 0, 0]) and torch.equal(cmin, rmin[:, 0, 0])
    # the topk-th largest / smallest value of each column
    assert torch.equal(cmax, mx.sort(0, descending=True)[0][topk - 1])
    assert torch.equal(cmin, mn.sort(0)[0][topk - 1])


def test_order_statistic_needs_topk_images():
    from imagecompression_adversarial_amd.latent_range import order_statistic
    with pytest.raises(ValueError, match=r"100.*7|7.*100"):
        order_statistic(torch.zeros(7, 4), torch.zeros(7, 4), 100)
    with pytest.raises(RuntimeError):   # the reference's own topk raises there too
        R.channel_profile(torch.zeros(7, 4), torch.zeros(7, 4), 100)


def test_profile_file_roundtrip(tmp_path):
    from imagecompression_adversarial_amd.latent_range import RangeProfile, default_path
    g = torch.Generator().manual_seed(0)
    cmax, cmin = torch.rand(16, generator=g), -torch.rand(16, generator=g)
    path = str(tmp_path / "attack" / "data" / "hyper-mse-3_range.pt")   # the directory is created
    RangeProfile(cmax.double(), cmin).save(path)
    raw = torch.load(path, weights_only=True)
    assert isinstance(raw, list) and len(raw) == 2
    assert all(t.dtype == torch.float32 and t.device.type == "cpu" and t.shape == (16,) for t in raw)
    assert torch.equal(raw[0], cmax) and torch.equal(raw[1], cmin)
    back = RangeProfile.load(path)
    assert torch.equal(back.channel_max, cmax) and torch.equal(back.channel_min, cmin) and back.C == 16
    # a file the reference wrote (device-less [C] tensors in a list) loads the same way
    torch.save([cmax, cmin], str(tmp_path / "ref.pt"))
    assert torch.equal(RangeProfile.load(str(tmp_path / "ref.pt")).channel_min, cmin)
    a = SimpleNamespace(model="hyper", metric="mse", quality=3, adv=False)
    assert default_path(a) == "./attack/data/hyper-mse-3_range.pt"
    a.adv = True
    assert default_path(a) == "./attack/data/hyper-mse-3-adv_range.pt"
    with pytest.raises(RuntimeError):
        back.on("cpu")


def test_header_and_bindings_carry_the_entry_points():
    from imagecompression_adversarial_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ica_hip.h")).read()
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % n, hdr, re.M), n
        assert n in _lib._SIGS
        assert hasattr(_lib.lib(), n)
    for cite in ("feature_range.py:19-21", "search.py:137-146", "clamp_value_naive"):
        assert cite in hdr


def test_wrappers_reject_host_tensors():
    from imagecompression_adversarial_amd import latent_range as LR
    prof = LR.RangeProfile(torch.ones(8), -torch.ones(8))
    y4 = torch.zeros(1, 2, 4, 4, 4)
    with pytest.raises(RuntimeError):
        LR.latent_range(y4, 8)
    with pytest.raises(RuntimeError):
        LR.latent_clamp(y4, 8, prof)
    with pytest.raises(RuntimeError):
        LR.latent_clamp_bwd_(y4, y4, 8, prof)
    with pytest.raises(RuntimeError):
        LR.latent_detect(torch.zeros(1, 8), torch.zeros(1, 8), prof)


def _old_flags(parser_fn):
    from imagecompression_adversarial_amd import coder
    argv = ["-m", "factorized", "-metric", "mse", "-q", "2", "-s", "x/*.png", "--batch", "3", "--adv", "--defend",
            "--defend_m", "range", "-steps", "7", "--synthetic-weights"]
    want = vars(coder.config().parse_args(argv))
    got = vars(parser_fn().parse_args(argv))
    assert {k: got[k] for k in want} == want
    assert {k: vars(parser_fn().parse_args([]))[k] for k in want} == vars(coder.config().parse_args([]))
    return set(got) - set(want)


def test_cli_parsers():
    from imagecompression_adversarial_amd import coder, feature_range, search, self_ensemble
    assert _old_flags(self_ensemble.config) == {"range_file"}
    assert _old_flags(feature_range.config) == {"topk", "range_file"}
    assert _old_flags(search.config) == {"topk", "range_file", "out_dir"}
    a = feature_range.config().parse_args(["--topk", "2", "--range-file", "p.pt"])
    assert (a.topk, a.range_file) == (2, "p.pt") and feature_range.config().parse_args([]).topk == 100
    a = search.config().parse_args(["--out-dir", "o", "--range-file", "p.pt"])
    assert (a.out_dir, a.range_file) == ("o", "p.pt") and search.config().parse_args([]).out_dir == "./attack/search/"
    assert self_ensemble.config().parse_args(["--range-file", "p.pt"]).range_file == "p.pt"
    with pytest.raises(SystemExit):   # coder.config() itself stays as it is
        coder.config().parse_args(["--range-file", "p.pt"])
    assert search._names("a/b/kodim01.png", 0.12345) == ("kodim01.png", "kodim01_0.1235.png")
    assert search._names("synthetic_2", 1.5) == ("synthetic_2.png", "synthetic_2_1.5000.png")


def test_attack_rd_defend_still_raises():
    from imagecompression_adversarial_amd import attack_rd
    with pytest.raises(NotImplementedError):
        attack_rd.attack_(torch.zeros(1, 3, 64, 64), None, SimpleNamespace(defend=True))


# --------------------------------------------------------------------------- #
# the pinned inputs of the GPU comparison tests
# --------------------------------------------------------------------------- #
RECON_TOL = 1e-3   # reconstruction tolerance of the defended-eval comparison (tests/test_gpu_defend.py)


@pytest.mark.parametrize("model", ["hyper", "factorized", "context", "cheng2020"])
def test_pinned_eval_inputs_exercise_the_clamp(model):
    """Every pinned input of the GPU defended-eval comparison, on the CPU oracle.  Measured (profile = the clean
    images' own range x R.PROFILE_SCALE[model], seeds 21 / 22): the clamp changes 25.96 % of the latent elements
    for hyper and factorized (they share g_a), 38.4 % for context (1 x 64x128, x 0.5) and 27.7 % for cheng2020
    (1 x 64x128, x 0.7; x 0.5 would be 53.4 %, over the bound); the clamped and unclamped reconstructions differ
    by 0.2096 / 0.2096 / 0.2045 / 0.1701 max abs, 170-210 x the 1e-3 comparison tolerance; and no latent element
    lies within 1e-5 of a bound (the GPU test lets nclamped move by that count, so it must stay far under the
    count itself: at most 1 % of it)."""
    P, im_adv, im_s, output_s, cmax, cmin = R.eval_case(model)
    res, out, y, yc = R.eval_reference(model)
    frac = float((yc != y).float().mean())
    print(model, "clamped fraction", frac)
    assert 0.01 <= frac <= 0.5, frac
    assert sum(r["nclamped"] for r in res) == int((yc != y).sum())
    hi, lo = cmax.view(1, -1, 1, 1), cmin.view(1, -1, 1, 1)
    near = (((y - hi).abs() < 1e-5) | ((y - lo).abs() < 1e-5)).flatten(1).sum(1)
    for b, r in enumerate(res):
        assert int(near[b]) <= r["nclamped"] // 100, (b, int(near[b]), r["nclamped"])
    _, _, _, plain = R.defended_forward(P, im_adv.clamp(0, 1), cmax, cmin, model, clamp_latent=False)
    assert float((out - plain).abs().max()) >= 10 * RECON_TOL
    for r in res:
        assert r["mse_out"] > 1e-6 and r["vi"] is not None
    if model == "factorized":   # the decoded latent is round(y) (attack_rd.py:267), not round(y - median) + median
        from oracle import codec
        with torch.no_grad():
            own = codec.g_s(P, codec.entropy_bottleneck(P, yc)[0]).clamp(0, 1)
        assert float((own - out).abs().max()) >= 10 * RECON_TOL


def test_pinned_attack_trajectory_is_well_conditioned():
    """The attack-through-clamp trajectory (hyper q3 with |y| ~ 1, 2 x 64x64, 8 steps, noise_thr 1e-3, lr 0.01,
    profile = own range x 0.5, seed 70).  Measured: every step takes the expensive branch with loss_i <= 0.32 x
    the threshold; the clamp changes 31.9 % of the latent; a float64 network replay of the restatement moves the
    final noise by rel 2.1e-4 <= 2e-3 / 5 and the eval's mse by < 1e-6 rel <= 1e-3 / 5, with the same branches."""
    ref, rec = R.adv_reference(2)
    ref64, rec64 = R.adv_reference(2, torch.float64)
    assert [r["cheap"].tolist() for r in rec] == [r["cheap"].tolist() for r in rec64]
    assert not any(v for r in rec for v in r["cheap"].tolist())
    assert max(float(r["loss_i"].max()) for r in rec) < 0.5 * R.ADV_THR
    assert rel_err(ref64.noise, ref.noise) <= 2e-3 / 5
    for b in range(2):
        assert float(ref.eval.mse_out[b]) > 1e-6
        for k in ("mse_in", "mse_out"):
            a, c = float(getattr(ref64.eval, k)[b]), float(getattr(ref.eval, k)[b])
            assert abs(a - c) <= 1e-3 / 5 * abs(c)
    from oracle import codec
    P, x, cmax, cmin = R.adv_case()
    with torch.no_grad():
        y = codec.g_a(P, x[:2])
    frac = float((R.clamp_value_naive(y, cmax, cmin) != y).float().mean())
    assert 0.01 <= frac <= 0.5, frac
    # the clamp shapes the trajectory: without it the same attack ends elsewhere by far more than the tolerance
    from oracle import attack as oa
    plain = oa.attack(P, x[:2], steps=R.ADV_STEPS, noise_thr=R.ADV_THR, lr=R.ADV_LR, eval_msssim=False, adv=True)
    assert rel_err(plain.noise, ref.noise) >= 10 * 2e-3
