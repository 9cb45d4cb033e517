"""GPU tests of the patch-wise VI localisation (ica_patch.hip, patch_vi, the attack_patch CLI) against the float64
restatement tests/patch_vi_restatement.py.

Stated tolerances.  A window mean is a sum of non-negative fp32 terms in chains of at most 48 + 128 + 128
additions on top of a correctly rounded difference, a fused square-accumulate and one division, so its relative
error is below about 3e2 * 2^-24 = 1.8e-5 in the worst case: mse_in / mse_out are held to 2e-5 relative of float64
everywhere, vi (one more division of two such means) to 4e-5 where no exclusion applies, and exactly 0 where one
does.  val / pos are bit-exact against the kernel's own map; gather and determinism are bit-exact."""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import patch_vi_restatement as R
from tests.conftest import REPO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MEAN_TOL, VI_TOL = 2e-5, 4e-5


@pytest.fixture(scope="module")
def PV():
    from imagecompression_adversarial_amd import patch_vi
    return patch_vi


def dev(tensors):
    return [t.to(DEV).contiguous() for t in tensors]


def max_rel(got, ref, mask=None):
    got, ref = got.cpu().double(), ref.double()
    if mask is not None:
        got, ref = got[mask], ref[mask]
    zero = ref == 0
    if bool(zero.any()):        # a sum of exact zeros is exactly zero in any precision
        assert float(got[zero].abs().max()) == 0
    got, ref = got[~zero], ref[~zero]
    if ref.numel() == 0:
        return 0.0
    assert bool((ref > 0).all())
    return float(((got - ref).abs() / ref).max())


def check_against_oracle(PV, tensors, ref, win, stride, border, tag):
    """The maps, the exclusions and the argmax of one call; returns the LocalVI."""
    lv = PV.local_vi(*dev(tensors), win=win, stride=stride, border=border)
    B, _, H, W = tensors[0].shape
    nh, nw = R.map_shape(H, W, win, stride)
    assert lv.mse_in.shape == lv.mse_out.shape == lv.vi.shape == (B, nh, nw)
    assert lv.val.shape == (B,) and lv.pos.shape == (B, 2) and lv.pos.dtype == torch.int32
    nz = ref["mse_in"] > 0
    e_in, e_out = max_rel(lv.mse_in, ref["mse_in"]), max_rel(lv.mse_out, ref["mse_out"])
    keep = ~ref["excluded"]
    e_vi = max_rel(lv.vi, ref["vi"], keep)
    print(tag, "rel err mse_in %.3g mse_out %.3g vi %.3g" % (e_in, e_out, e_vi))
    assert e_in < MEAN_TOL and e_out < MEAN_TOL
    if bool((~nz).any()):
        assert float(lv.mse_in.cpu()[~nz].abs().max()) == 0
    assert e_vi < VI_TOL
    if bool(ref["excluded"].any()):
        assert float(lv.vi.cpu()[ref["excluded"]].abs().max()) == 0
    # val / pos: the first row-major maximum of the kernel's own map, bit-exact
    val, pos = R.first_argmax(lv.vi.cpu())
    assert torch.equal(lv.val.cpu(), val) and torch.equal(lv.pos.cpu(), pos), (lv.val, val, lv.pos, pos)
    assert torch.equal(lv.origin().cpu(), pos * stride)
    return lv


# --------------------------------------------------------------------------- #
# maps, exclusions, argmax
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", R.PINNED, ids=[c[0] for c in R.PINNED])
def test_pinned_cases_vs_oracle(PV, case):
    name, B, H, W, win, stride, border = case
    tensors, planted, ref = R.pinned(name)
    lv = check_against_oracle(PV, tensors, ref, win, stride, border, name)
    assert torch.equal(lv.pos.cpu(), ref["pos"]) and torch.equal(lv.pos.cpu(), planted)
    assert max_rel(lv.val, ref["val"]) < VI_TOL


@pytest.mark.parametrize("shape,win,stride,border", [
    ((3, 128, 160), 64, 2, 10), ((2, 192, 128), 64, 2, 0), ((2, 128, 160), 32, 4, 0), ((1, 72, 80), 64, 1, 2),
    ((2, 134, 128), 64, 4, 0), ((1, 64, 64), 64, 2, 0), ((2, 128, 128), 128, 1, 0), ((1, 136, 128), 128, 4, 0)])
def test_random_inputs_vs_oracle(PV, shape, win, stride, border):
    """Unpinned inputs (no planted window, margins of the order of the tolerance): the oracle's vi at the returned
    position is within 4e-5 relative of the oracle's maximum."""
    B, H, W = shape
    tensors = R.random_case(B, H, W, seed=H + W + win + stride)
    ref = R.local_vi(*tensors, win=win, stride=stride, border=border)
    lv = check_against_oracle(PV, tensors, ref, win, stride, border, f"random{shape}")
    for b, (r, c) in enumerate(lv.pos.cpu().tolist()):
        best = float(ref["val"][b])
        assert best > 0 and (best - float(ref["vi"][b, r, c])) / best < VI_TOL


def test_zero_mse_in_block_and_border_are_exactly_zero(PV):
    im_adv, out_adv, im_s, out_s = R.random_case(2, 128, 160, seed=5)
    im_adv[1, :, 20:92, 10:84] = im_s[1, :, 20:92, 10:84]
    for border in (0, 10):
        ref = R.local_vi(im_adv, out_adv, im_s, out_s, border=border)
        assert int((ref["mse_in"][1] == 0).sum()) == 30 and int((ref["mse_in"][0] == 0).sum()) == 0
        lv = check_against_oracle(PV, (im_adv, out_adv, im_s, out_s), ref, 64, 2, border, f"zero-block b{border}")
        zero = ref["mse_in"] == 0
        assert float(lv.mse_in.cpu()[zero].abs().max()) == 0 and float(lv.vi.cpu()[zero].abs().max()) == 0
        assert bool(torch.isfinite(lv.vi).all()) and bool(torch.isfinite(lv.val).all())


@pytest.mark.parametrize("shape,border", [((2, 64, 64), 10), ((1, 72, 80), 10), ((2, 128, 160), 17), ((1, 64, 64), 1)])
def test_all_border_map(PV, shape, border):
    tensors = R.random_case(*shape, seed=6)
    lv = PV.local_vi(*dev(tensors), border=border)
    assert float(lv.vi.abs().max()) == 0
    assert lv.val.cpu().tolist() == [0.0] * shape[0] and lv.pos.cpu().tolist() == [[0, 0]] * shape[0]
    assert bool((lv.mse_in > 0).all())
    patches = PV.worst_patches(*dev(tensors), border=border)
    assert torch.equal(patches.cpu(), R.slice_patches(tensors, [(0, 0)] * shape[0], 64, 2))


def test_ties_take_the_first_row_major_window(PV):
    """Identical windows: a perturbation and an error that are 8-periodic in both directions make every window's
    sums the same bits, so the whole interior ties and the first interior window wins."""
    B, H, W = 2, 128, 160
    g = torch.Generator().manual_seed(7)
    tile_in = 1e-2 * torch.randn((B, 3, 8, 8), generator=g)
    tile_out = 3e-2 * torch.randn((B, 3, 8, 8), generator=g)
    im_s = torch.full((B, 3, H, W), 0.5)
    out_s = torch.full((B, 3, H, W), 0.25)
    im_adv = im_s + tile_in.repeat(1, 1, H // 8, W // 8)
    out_adv = out_s + tile_out.repeat(1, 1, H // 8, W // 8)
    for stride, border in ((4, 3), (2, 10)):
        lv = PV.local_vi(*dev((im_adv, out_adv, im_s, out_s)), stride=stride, border=border)
        vi = lv.vi.cpu()
        step = 8 // stride                      # windows a multiple of 8 pixels apart are identical
        r0 = -(-border // step) * step
        for b in range(B):
            same = vi[b, r0::step, r0::step]
            same = same[: (vi.shape[1] - border - r0 + step - 1) // step, : (vi.shape[2] - border - r0 + step - 1) // step]
            assert same.numel() > 1 and bool((same == same[0, 0]).all())
        val, pos = R.first_argmax(vi)
        assert torch.equal(lv.pos.cpu(), pos) and torch.equal(lv.val.cpu(), val)
        for b in range(B):                      # the winner has equals later in the map
            assert int((vi[b] == val[b]).sum()) > 1


# --------------------------------------------------------------------------- #
# gather, determinism
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", R.PINNED, ids=[c[0] for c in R.PINNED])
def test_gather_is_bit_equal_to_slicing(PV, case):
    name, B, H, W, win, stride, border = case
    tensors, planted, ref = R.pinned(name)
    d = dev(tensors)
    patches = PV.worst_patches(*d, win=win, stride=stride, border=border)
    assert patches.shape == (B, 4, 3, win, win)
    assert torch.equal(patches.cpu(), R.slice_patches(tensors, planted, win, stride))
    # a caller-given pos: the last window of the map, whose patch ends at the last used pixel
    nh, nw = R.map_shape(H, W, win, stride)
    last = torch.tensor([[nh - 1, nw - 1]] * B, dtype=torch.int32)
    got = PV.worst_patches(*d, win=win, stride=stride, border=border, pos=last.to(DEV))
    assert torch.equal(got.cpu(), R.slice_patches(tensors, last, win, stride))


def test_deterministic_and_batch_independent(PV):
    for name in ("b3_128x160", "h134_s4", "stride1"):
        _, B, H, W, win, stride, border = next(c for c in R.PINNED if c[0] == name)
        tensors = R.pinned(name)[0]
        d = dev(tensors)
        a = PV.local_vi(*d, win=win, stride=stride, border=border)
        b = PV.local_vi(*d, win=win, stride=stride, border=border)
        pa = PV.worst_patches(*d, win=win, stride=stride, border=border)
        for f in ("mse_in", "mse_out", "vi", "val", "pos"):
            assert torch.equal(getattr(a, f), getattr(b, f)), f
        for i in range(B):
            one = [t[i:i + 1].contiguous() for t in d]
            s = PV.local_vi(*one, win=win, stride=stride, border=border)
            for f in ("mse_in", "mse_out", "vi", "val", "pos"):
                assert torch.equal(getattr(s, f)[0], getattr(a, f)[i]), (name, i, f)
            assert torch.equal(PV.worst_patches(*one, win=win, stride=stride, border=border)[0], pa[i])


def test_rejected_arguments_raise_before_launch(PV):
    t = torch.zeros((1, 3, 128, 128), device=DEV)
    for kw in (dict(stride=3), dict(win=66, stride=4), dict(win=132, stride=4), dict(border=-1)):
        with pytest.raises(ValueError):
            PV.local_vi(t, t, t, t, **kw)
    with pytest.raises(ValueError):
        PV.local_vi(t[:, :, :, :126].contiguous(), t, t, t)
    # the C entry point refuses the same problems with a non-zero status and launches nothing
    from imagecompression_adversarial_amd._lib import lib, ptr, stream
    for (H, W, win, stride, border) in [(128, 128, 64, 3, 10), (128, 128, 66, 4, 0), (256, 256, 132, 4, 0),
                                        (60, 128, 64, 2, 0), (128, 130, 64, 2, 0), (128, 128, 64, 2, -1)]:
        assert lib().ica_patch_vi_ws_size(1, H, W, win, stride) == 0 or border < 0
        rc = lib().ica_patch_vi(ptr(t), ptr(t), ptr(t), ptr(t), 1, H, W, win, stride, border, None, None, None, None,
                                None, None, None, stream())
        assert rc != 0
        if border >= 0:
            assert lib().ica_patch_gather(ptr(t), ptr(t), ptr(t), ptr(t), None, None, 1, H, W, win, stride,
                                          stream()) != 0
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- #
# end to end
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def short_attack():
    """hyper q1, B = 2 at 128x128, 4 steps."""
    from oracle import codec
    from imagecompression_adversarial_amd.attack import attack_batch
    from imagecompression_adversarial_amd.engine import CodecKernels
    P = codec.perturb_params(codec.init_params("hyper", 1, seed=0), seed=1)
    P["g_a.6.weight"] = P["g_a.6.weight"] * 40.0     # |y| ~ 1 and more: the rounded-latent reconstructions move
    kern = CodecKernels({k: v.to(DEV) for k, v in P.items()}, "hyper", "fp32")
    g = torch.Generator().manual_seed(11)
    im_s = torch.rand((2, 3, 128, 128), generator=g).to(DEV)
    res = attack_batch(kern, im_s, steps=4, noise_thr=1e-4, lr=0.01, eval_msssim=False)
    return res, im_s


def test_localize_an_attack_result(PV, short_attack):
    res, im_s = short_attack
    loc = PV.localize(res, im_s, border=2)
    tensors = [t.cpu() for t in (res.im_adv, res.output_adv, im_s, res.output_s)]
    ref = R.local_vi(*tensors, border=2)
    check_against_oracle(PV, tensors, ref, 64, 2, 2, "attack")
    assert loc.vi.vi.shape == (2, 33, 33) and loc.patches.shape == (2, 4, 3, 64, 64)
    pos = loc.vi.pos.cpu()
    assert torch.equal(loc.patches.cpu(), R.slice_patches(tensors, pos, 64, 2))
    for b in range(2):
        assert loc.origin[b] == (int(pos[b, 0]) * 2, int(pos[b, 1]) * 2)
        assert float(loc.vi.val[b]) > 0 and loc.vi_db[b] == 10.0 * math.log10(float(loc.vi.val[b]))
        r, c = pos[b].tolist()
        best = float(ref["val"][b])
        assert (best - float(ref["vi"][b, r, c])) / best < VI_TOL


def test_global_vi_lies_between_the_window_ratios(PV, short_attack):
    """The four windows at map positions (0, 0), (0, 32), (32, 0), (32, 32) tile a 128x128 image exactly, so the
    image's mse_out / mse_in is the mediant of their four ratios and lies between the smallest and the largest
    window ratio of the map (border = 0): exact in exact arithmetic, checked with the 4e-5 of the window ratios."""
    res, im_s = short_attack
    lv = PV.local_vi(res.im_adv, res.output_adv, im_s, res.output_s.contiguous(), border=0)
    for b in range(2):
        ratios = lv.vi[b][lv.mse_in[b] > 0].double()
        g = float(res.mse_out[b]) / float(res.mse_in[b])
        print(b, "global", g, "windows", float(ratios.min()), float(ratios.max()))
        assert float(ratios.min()) * (1 - VI_TOL) <= g <= float(ratios.max()) * (1 + VI_TOL)


def test_attack_patch_cli(tmp_path):
    from PIL import Image
    cli = ["-m", "imagecompression_adversarial_amd.attack_patch", "-m", "hyper", "-metric", "mse", "-q", "1", "-s",
           "synthetic:2x128x128", "--synthetic-weights", "-steps", "3", "--batch", "2", "--border", "2", "-t", "1"]
    r = subprocess.run([sys.executable] + cli, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=REPO),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    per_image = [ln for ln in lines if ln.startswith("synthetic_") and "Time:" in ln]
    worst = [ln for ln in lines if " worst 64x64 window at (y=" in ln]
    assert len(per_image) == 2 and len(worst) == 2 and len(per_image[0].split()) == 6
    avg = [ln for ln in lines if ln.startswith("AVG: 1 ")]
    assert len(avg) == 1 and len(avg[0].split()) == 6
    root = tmp_path / "attack" / "patch"
    for i in range(2):
        for f in (f"hyper_1_mse_synthetic_{i}_advin_1.png", f"hyper_1_mse_synthetic_{i}_advout_1.png"):
            assert Image.open(root / f).size == (128, 128), f
        for sub, f in (("adv", "advin"), ("adv", "advout"), ("ori", "oriin"), ("ori", "oriout")):
            p = root / "hyper_1_mse_" / sub / f"synthetic_{i}_{f}_patch_1.png"
            assert Image.open(p).size == (64, 64), p
    assert sorted(os.listdir(tmp_path)) == ["attack"]       # attack_rd's own -t files are not written
