"""GPU tests of the latent-range kernels (ica_latent.hip), the defended eval, the attack through the clamp and
the feature_range / search CLIs, against torch on the CPU and tests/latent_range_restatement.py.

Stated tolerances: range, clamp, clamp-backward and detect are bit-equal to torch (NaN compared as NaN); the
defended eval and the attack trajectory use the tolerances of tests/test_gpu_defend.py and
tests/test_gpu_defend_adv.py (reconstruction 1e-3, bpp / mse rel 1e-3, vi 5e-3 dB; noise rel 2e-3)."""
import math
import os
import re

import pytest
import torch

from tests import latent_range_restatement as R
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

PLANES = [(1, 1), (4, 4), (7, 9), (12, 20), (33, 47)]
SHAPES = [(3, 8) + hw for hw in PLANES] + [(2, 192, 4, 6), (2, 320, 4, 6)]


@pytest.fixture(scope="module")
def LR():
    from imagecompression_adversarial_amd import latent_range
    return latent_range


def nchw(y4):
    """NCHW copy of a hand-made nChw4c tensor [B][C/4][H][W][4]."""
    B, C4, H, W, _ = y4.shape
    return y4.permute(0, 1, 4, 2, 3).reshape(B, C4 * 4, H, W)


def nc4(x):
    B, C, H, W = x.shape
    return x.reshape(B, C // 4, 4, H, W).permute(0, 1, 3, 4, 2).contiguous()


def randn4(B, C, H, W, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, C // 4, H, W, 4), generator=g) * scale


def same_bits(a, b):
    """Bit equality, every NaN counting as equal to every NaN."""
    a, b = a.cpu(), b.cpu()
    if a.shape != b.shape or not torch.equal(a.isnan(), b.isnan()):
        return False
    z = torch.zeros_like(a)
    return torch.equal(torch.where(a.isnan(), z, a).view(torch.int32), torch.where(b.isnan(), z, b).view(torch.int32))


def check_range(LR, y4):
    C = y4.shape[1] * 4
    got = LR.latent_range(y4.to(DEV), C)
    ref = R.ranges(nchw(y4))
    for g, r, name in zip(got, ref, ("max", "min", "absmax")):
        assert same_bits(g, r), name
    g2 = LR.latent_range(y4.to(DEV), C, absmax=False)
    assert g2[2] is None and same_bits(g2[0], ref[0]) and same_bits(g2[1], ref[1])


# --------------------------------------------------------------------------- #
# ica_latent_range
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", SHAPES)
def test_range_bitexact(LR, shape):
    check_range(LR, randn4(*shape, seed=sum(shape)))


@pytest.mark.parametrize("case", ["first", "last", "negative", "positive", "nan"])
def test_range_edge_cases(LR, case):
    v = nchw(randn4(3, 8, 33, 47, seed=5))   # NCHW (a copy); back to nChw4c below
    if case == "first":
        v[:, :, 0, 0] = 50.0
        v[1, :, 0, 0] = -50.0
    elif case == "last":
        v[:, :, -1, -1] = 50.0
        v[1, :, -1, -1] = -50.0
    elif case == "negative":
        v = -v.abs() - 0.25    # a 0-initialised maximum would answer 0
    elif case == "positive":
        v = v.abs() + 0.25
    else:
        v[1, 5, 17, 3] = float("nan")
        v[2, 0, 32, 46] = float("nan")
    y4 = nc4(v)
    assert torch.equal(nchw(y4).isnan(), v.isnan())
    check_range(LR, y4)
    if case == "nan":
        mx = LR.latent_range(y4.to(DEV), 8)[0].cpu()
        assert mx.isnan().sum() == 2 and mx[1, 5].isnan() and mx[2, 0].isnan()


def test_channels_not_a_multiple_of_four(LR):
    y4 = torch.zeros((1, 2, 4, 4, 4), device=DEV)
    prof = LR.RangeProfile(torch.ones(6), -torch.ones(6), DEV)
    with pytest.raises(ValueError):
        LR.latent_range(y4, 6)
    with pytest.raises(ValueError):
        LR.latent_clamp(y4, 6, prof)
    with pytest.raises(ValueError):
        LR.latent_clamp_bwd_(y4.clone(), y4, 6, prof)
    with pytest.raises(ValueError):
        LR.latent_detect(torch.zeros((1, 6), device=DEV), torch.zeros((1, 6), device=DEV), prof)


# --------------------------------------------------------------------------- #
# ica_latent_clamp / ica_latent_clamp_bwd
# --------------------------------------------------------------------------- #
def clamp_case(shape, seed):
    B, C, H, W = shape
    y4 = randn4(B, C, H, W, seed)
    g = torch.Generator().manual_seed(seed + 1)
    cmax = torch.rand(C, generator=g) * 2.0 + 0.1
    cmin = -torch.rand(C, generator=g) * 2.0 - 0.1
    cmax[2], cmin[2] = -0.3, 0.4            # a channel with cmin > cmax
    v = nchw(y4)                            # NCHW (a copy); back to nChw4c below
    v[0, 0, 0, 0] = cmax[0]                 # values exactly on a bound
    v[B - 1, 1, H - 1, W - 1] = cmin[1]
    v[0, 2, 0, 0] = cmax[2]
    v[0, 2, H - 1, 0] = cmin[2]
    v[B - 1, 3, H // 2, W // 2] = float("nan")
    return nc4(v), cmax, cmin


@pytest.mark.parametrize("shape", SHAPES)
def test_clamp_and_backward_bitexact(LR, shape):
    B, C, H, W = shape
    y4, cmax, cmin = clamp_case(shape, seed=11 + sum(shape))
    prof = LR.RangeProfile(cmax, cmin, DEV)
    y = nchw(y4).clone().requires_grad_(True)
    t = torch.where(y > cmax.view(1, -1, 1, 1), cmax.view(1, -1, 1, 1), y)
    o = torch.where(t < cmin.view(1, -1, 1, 1), cmin.view(1, -1, 1, 1), t)
    gout = nchw(randn4(B, C, H, W, seed=3)).contiguous()
    o.backward(gout)
    o = o.detach()
    count = (o != y.detach()).flatten(1).sum(1).to(torch.int32)
    assert int(count.sum()) > 0 or H * W == 1
    yd = y4.to(DEV)
    got, n = LR.latent_clamp(yd, C, prof, count=True)
    assert same_bits(got, nc4(o))
    assert torch.equal(n.cpu(), count)
    assert same_bits(LR.latent_clamp(yd, C, prof), nc4(o))            # without the count
    assert torch.equal(yd.cpu().isnan(), y4.isnan()) and same_bits(yd, y4)   # the input is left alone
    # backward: g passes where both selects took y (the autograd of the two torch.where)
    g4 = nc4(gout).to(DEV)
    assert LR.latent_clamp_bwd_(g4, yd, C, prof) is g4
    assert torch.equal(g4.cpu(), nc4(y.grad))
    # in place, with the count
    out, n2 = LR.latent_clamp(yd, C, prof, out=yd, count=True)
    assert out is yd and same_bits(yd, nc4(o)) and torch.equal(n2.cpu(), count)


# --------------------------------------------------------------------------- #
# ica_latent_detect
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("B,C", [(1, 8), (5, 8), (5, 192), (1, 320)])
@pytest.mark.parametrize("where", ["inside", "above", "below", "minus_one_inf", "minus_one_nan", "nan_input"])
def test_detect_bitexact(LR, B, C, where):
    g = torch.Generator().manual_seed(B * 1000 + C)
    imax = torch.rand((B, C), generator=g) * 3.0 + 0.5
    imin = -torch.rand((B, C), generator=g) * 3.0 - 0.5
    cmax = torch.rand(C, generator=g) * 1.5 + 1.0     # straddles the images' extremes: some channels leave it
    cmin = -torch.rand(C, generator=g) * 1.5 - 1.0
    if where == "above":        # the whole profile above the images' range
        cmax, cmin = cmax + 10.0, cmin + 10.0
    elif where == "below":
        cmax, cmin = cmax - 10.0, cmin - 10.0
    elif where == "minus_one_inf":   # cmax + 1 == 0 under a positive excess: inf
        cmax[C // 2] = -1.0
    elif where == "minus_one_nan":   # 0 / 0
        cmax[C // 2] = -1.0
        imax[0, C // 2] = -1.0
        cmin[1] = -1.0
        imin[B - 1, 1] = -1.0
    elif where == "nan_input":
        imax[B - 1, C - 1] = float("nan")
    prof = LR.RangeProfile(cmax, cmin, DEV)
    got = LR.latent_detect(imax.to(DEV), imin.to(DEV), prof).cpu()
    ref = torch.stack([R.detect_from_ranges(imax[b], imin[b], cmax, cmin) for b in range(B)])
    assert same_bits(got, ref), (got, ref)
    if where == "minus_one_inf":
        assert bool(torch.isinf(got).all())
    if where in ("minus_one_nan", "nan_input"):
        assert bool(got.isnan().any())
    if where == "inside":
        assert bool((got > 0).all())


def test_detect_of_a_latent_equals_search_detect(LR):
    y4 = randn4(2, 8, 7, 9, seed=9)
    cmax, cmin = torch.full((8,), 1.5), torch.full((8,), -1.25)
    prof = LR.RangeProfile(cmax, cmin, DEV)
    mx, mn, _ = LR.latent_range(y4.to(DEV), 8)
    got = LR.latent_detect(mx, mn, prof).cpu()
    ref = torch.stack([R.detect(nchw(y4)[b:b + 1], cmax, cmin) for b in range(2)])
    assert same_bits(got, ref)


# --------------------------------------------------------------------------- #
# defended eval (attack_rd.py:263-268) vs the oracle composition
# --------------------------------------------------------------------------- #
def kernels_for(P, model, precision="fp32"):
    sd = {k: v.to(DEV) for k, v in P.items()}
    if model == "cheng2020":
        from imagecompression_adversarial_amd.engine_cheng import ChengKernels
        return ChengKernels(sd, precision=precision)
    from imagecompression_adversarial_amd.engine import CodecKernels
    return CodecKernels(sd, model, precision)


@pytest.mark.parametrize("model", ["hyper", "factorized", "context", "cheng2020"])
def test_evaluate_defend_range_vs_oracle(LR, model):
    from imagecompression_adversarial_amd import hip_ops as K
    from imagecompression_adversarial_amd import self_ensemble as SE
    P, im_adv, im_s, output_s, cmax, cmin = R.eval_case(model)
    kern = kernels_for(P, model)
    prof = LR.RangeProfile(cmax, cmin, DEV)
    x4 = K.to_nc4(im_adv.to(DEV))
    before = kern.forward(x4)                  # the transform-free forward, saved
    got, out = SE.evaluate_defend(kern, im_adv.to(DEV), im_s.to(DEV), output_s.to(DEV), "range", profile=prof,
                                  msssim=False)
    ref, rout, y, yc = R.eval_reference(model)
    print(model, "max |out - ref|", float((out.cpu() - rout).abs().max()))
    assert float((out.cpu() - rout).abs().max()) < 1e-3
    hi, lo = cmax.view(1, -1, 1, 1), cmin.view(1, -1, 1, 1)
    near = (((y - hi).abs() < 1e-5) | ((y - lo).abs() < 1e-5)).flatten(1).sum(1)
    for b, (g, r) in enumerate(zip(got, ref)):
        print(model, b, g, r)
        assert "mse_pre" not in g and "vi_pre" not in g and "best_idx" not in g
        assert math.isclose(g["bpp"], r["bpp"], rel_tol=1e-3)
        assert math.isclose(g["mse_in"], r["mse_in"], rel_tol=1e-5)
        assert r["mse_out"] > 1e-6
        assert math.isclose(g["mse_out"], r["mse_out"], rel_tol=1e-3)
        assert abs(g["vi"] - r["vi"]) < 5e-3
        assert abs(g["nclamped"] - r["nclamped"]) <= int(near[b])
        assert g["nclamped"] > 0
    # forward() without a transform is what it was: same bits before and after the defended call
    after = kern.forward(x4)
    for k in ("x_hat4", "y4", "y_hat4", "sumlog"):
        assert torch.equal(before[k], after[k]), k
    if model != "factorized":   # an identity transform changes nothing where g_s decodes round(y) anyway
        ident = kern.forward(x4, latent=lambda y4: y4)
        assert torch.equal(ident["x_hat4"], before["x_hat4"]) and torch.equal(ident["sumlog"], before["sumlog"])
    with pytest.raises(ValueError):
        SE.evaluate_defend(kern, im_adv.to(DEV), im_s.to(DEV), output_s.to(DEV), "range")   # no profile


@pytest.mark.parametrize("model", ["hyper", "cheng2020"])
def test_defended_eval_on_the_bf16_engine(LR, model):
    """--precision bf16: the clamp runs on the fp32 latent (the cast of the bf16 g_a output for bmshj2018; cheng2020
    keeps fp32 activations), and the defended eval decodes exactly clamp(that latent)."""
    from imagecompression_adversarial_amd import hip_ops as K
    from imagecompression_adversarial_amd import self_ensemble as SE
    P, im_adv, im_s, output_s, cmax, cmin = R.eval_case(model)
    kern = kernels_for(P, model, "bf16")
    prof = LR.RangeProfile(cmax, cmin, DEV)
    x4 = K.to_nc4(im_adv.to(DEV))
    y4 = K.cast_nc4(kern.g_a(x4)[0], torch.float32)
    want, n = LR.latent_clamp(y4, kern.M, prof, count=True)
    res = kern.forward(x4, latent=lambda t: LR.latent_clamp(t, kern.M, prof))
    assert res["y4"].dtype == torch.float32 and torch.equal(res["y4"], want)
    got, out = SE.evaluate_defend(kern, im_adv.to(DEV), im_s.to(DEV), output_s.to(DEV), "range", profile=prof,
                                  msssim=False)
    assert [g["nclamped"] for g in got] == n.tolist() and min(n.tolist()) > 0
    assert bool(torch.isfinite(out).all()) and all(math.isfinite(g["bpp"]) and g["bpp"] > 0 for g in got)


def test_debug_model_has_no_latent_transform():
    from oracle import codec
    from imagecompression_adversarial_amd import hip_ops as K
    from imagecompression_adversarial_amd.engine_debug import DebugKernels
    P = codec.init_params("debug", 3, seed=0)
    kern = DebugKernels({k: v.to(DEV) for k, v in P.items()})
    with pytest.raises(NotImplementedError):
        kern.forward(K.to_nc4(R.rnd((1, 3, 32, 32), 1).to(DEV)), latent=lambda y4: y4)


# --------------------------------------------------------------------------- #
# the attack through the clamp
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def adv_runs(LR):
    """x6 and fp32 runs of the pinned trajectory (2 images), plus fp32 runs of image 1 in a batch of 3 and alone."""
    from imagecompression_adversarial_amd import self_ensemble as SE
    P, x, cmax, cmin = R.adv_case()
    prof = LR.RangeProfile(cmax, cmin, DEV)
    kw = dict(steps=R.ADV_STEPS, noise_thr=R.ADV_THR, lr=R.ADV_LR, eval_msssim=False, record=True, profile=prof)
    runs = {}
    for precision in ("x6", "fp32"):
        kern = kernels_for(P, "hyper", precision)
        runs[precision] = SE.adv_attack_batch(kern, x[:2].to(DEV), "range", **kw)
        if precision == "fp32":
            runs["three"] = SE.adv_attack_batch(kern, x.to(DEV), "range", **kw)
            runs["alone"] = SE.adv_attack_batch(kern, x[1:2].to(DEV), "range", **kw)
    return runs


@pytest.mark.parametrize("precision", ["x6", "fp32"])
def test_attack_through_clamp_vs_restatement(adv_runs, precision):
    res, out, loop, branches = adv_runs[precision]
    ref, rec = R.adv_reference(2)
    assert len(branches) == R.ADV_STEPS
    for i, br in enumerate(branches):
        assert [bool(v) for v in br] == [bool(v) for v in rec[i]["cheap"]], i
    print(precision, "noise rel", rel_err(loop.noise.cpu(), ref.noise))
    assert rel_err(loop.noise.cpu(), ref.noise) < 2e-3
    for b, r in enumerate(res):
        print(precision, b, r, float(ref.eval.mse_in[b]), float(ref.eval.mse_out[b]))
        assert math.isclose(r["mse_in"], float(ref.eval.mse_in[b]), rel_tol=1e-3)
        assert math.isclose(r["mse_out"], float(ref.eval.mse_out[b]), rel_tol=1e-3)
        assert r["vi_msim"] is None


def test_attack_through_clamp_is_per_image(adv_runs):
    three, alone = adv_runs["three"][2], adv_runs["alone"][2]
    assert torch.equal(three.noise[1], alone.noise[0])
    assert torch.equal(three.im_in[1], alone.im_in[0])
    assert torch.equal(adv_runs["fp32"][2].noise[1], alone.noise[0])


def test_attack_through_clamp_rejects_bf16_and_missing_profile(LR):
    from imagecompression_adversarial_amd import self_ensemble as SE
    P, x, cmax, cmin = R.adv_case()
    prof = LR.RangeProfile(cmax, cmin, DEV)
    with pytest.raises(NotImplementedError):
        SE.DefendedAttackLoop(kernels_for(P, "hyper", "bf16"), x[:1].to(DEV), "range", profile=prof)
    with pytest.raises(ValueError):
        SE.DefendedAttackLoop(kernels_for(P, "hyper", "fp32"), x[:1].to(DEV), "range")


# --------------------------------------------------------------------------- #
# CLIs
# --------------------------------------------------------------------------- #
BASE = ["-m", "hyper", "-metric", "mse", "-q", "3", "--synthetic-weights", "-s", "synthetic:4x64x64"]


@pytest.fixture(scope="module")
def cli_profile(tmp_path_factory):
    """feature_range's file for the synthetic images, and the engine / images it was made from."""
    from imagecompression_adversarial_amd import coder, feature_range
    from imagecompression_adversarial_amd.attack_rd import _sources
    path = str(tmp_path_factory.mktemp("range") / "data" / "hyper-mse-3_range.pt")
    argv = BASE + ["--topk", "2", "--batch", "2", "--range-file", path]
    profile, wrote = feature_range.main(argv)
    assert wrote == path and os.path.exists(path)
    args = feature_range.config().parse_args(argv)
    net = coder.load_model(args, training=False).to(args.device)
    kern = net.kernels(net.attack_precision(None))
    x = torch.cat([t for _, t, _, _ in _sources(args.source)], 0).to(DEV)
    return path, profile, kern, x


def test_feature_range_cli(LR, cli_profile, capsys):
    path, profile, kern, x = cli_profile
    raw = torch.load(path, weights_only=True)
    want = LR.build_profile(kern, [x], topk=2)
    assert torch.equal(raw[0], want.channel_max) and torch.equal(raw[1], want.channel_min)
    assert torch.equal(profile.channel_max, raw[0])
    # the order statistic of the per-image rows: with topk = 2 of 4 images, one image per channel lies outside
    mx, mn, _ = LR.latent_range(LR.latent_of(kern, x), kern.M)
    assert torch.equal(raw[0], mx.cpu().sort(0, descending=True)[0][1])
    assert torch.equal(raw[1], mn.cpu().sort(0)[0][1])
    with pytest.raises(ValueError, match="100"):
        LR.build_profile(kern, [x])   # 4 images < topk = 100
    from imagecompression_adversarial_amd import feature_range
    capsys.readouterr()
    feature_range.main(BASE + ["--topk", "4", "--range-file", path + ".4"])
    txt = capsys.readouterr().out
    assert "[Activation Range Evaluator]: synthetic:4x64x64" in txt and "tensor(" in txt


def test_search_cli(LR, cli_profile, tmp_path, capsys):
    from imagecompression_adversarial_amd import search
    path, profile, kern, x = cli_profile
    capsys.readouterr()
    found = search.main(BASE + ["--batch", "4", "--range-file", path, "--out-dir", str(tmp_path / "found")])
    lines = re.findall(r"^FOUND YOU! (\S+) (\S+)$", capsys.readouterr().out, re.M)
    assert lines and len(lines) == len(found)
    scores = [float(s) for _, s in lines]
    assert all(b > a for a, b in zip(scores, scores[1:])) and scores[0] > 0
    prof = LR.RangeProfile.load(path, DEV)
    every = LR.score_images(kern, x, prof).tolist()
    best = 0
    want = []
    for b, s in enumerate(every):   # search.py:161-168: strict >, from 0, in image order
        if s > best:
            want.append((f"synthetic_{b}", s))
            best = s
    assert [(n, float(s)) for n, s in lines] == want
    for (name, s) in want:
        b = int(name.rsplit("_", 1)[1])
        assert s == float(LR.score_images(kern, x[b:b + 1], prof)[0])
        assert os.path.exists(tmp_path / "found" / f"{name}.png")
        assert os.path.exists(tmp_path / "found" / f"{name}_{s:.4f}.png")


@pytest.mark.parametrize("adv", [False, True])
def test_self_ensemble_range_cli(cli_profile, capsys, adv):
    from imagecompression_adversarial_amd import self_ensemble
    path = cli_profile[0]
    capsys.readouterr()
    out = self_ensemble.main(["-m", "hyper", "-metric", "mse", "-q", "3", "--synthetic-weights", "-s",
                              "synthetic:1x64x64", "-steps", "3", "--defend", "--defend_m", "range", "--range-file",
                              path] + (["--adv"] if adv else []))
    txt = capsys.readouterr().out
    assert "Defense Method: range" in txt and "AVG: 3" in txt and "synthetic_0" in txt
    assert out["bpp"] > 0
