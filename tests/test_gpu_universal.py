"""The universal perturbation (one noise for B images) on the GPU.

Kernels, bit for bit (torch.equal): ica_universal_prologue against the per-image prologue on the expanded noise;
ica_universal_adam against the project's pinned per-image Adam kernel fed the batch reduction restated in torch
(tests/universal_restatement.masked_sum), which pins the new sum over the images and leaves the Adam tail to the
kernel that already has it.  Loop: the branch sequence, noise and im_adv of the CPU oracle run with a [1, 3, H, W]
noise (the reference's attack_ verbatim), at the tolerances of test_coupled_attack_vs_oracle: noise rel < 2e-3,
im_adv rel < 1e-5 (the oracle's own fp32 run stays within 7.3e-4 / 1.2e-6 of its float64 run in these settings).
"""
import numpy as np
import pytest
import torch

from oracle import attack as oatt
from oracle import codec
from tests.conftest import rel_err
from tests.universal_restatement import im_in_of, masked_sum

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = float(np.float32(16.0 / 255.0))
THR = 1e-4
GSCALE = float(np.float32(1.0 / 4096.0))
BC2S, NEG_STEP = float(np.float32(0.0774)), float(np.float32(-0.0365))   # the Adam scalars of some step t


def rnd(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


@pytest.fixture(scope="module")
def hyper3():
    from imagecompression_adversarial_amd.engine import CodecKernels
    P = codec.perturb_params(codec.init_params("hyper", 3, seed=0), seed=1)
    return P, CodecKernels({k: v.to(DEV) for k, v in P.items()}, "hyper")


def _inputs(B, H, W, seed):
    """im_s in [0, 1] with about 5 % of its elements exactly 0 or 1, noise in +-1.5 eps (both noise bounds and both
    image bounds are hit), a signed network gradient and a non-zero Adam state."""
    im_s = rnd((B, 3, H, W), seed)
    pick = rnd((B, 3, H, W), seed + 1)
    im_s = torch.where(pick < 0.025, torch.zeros(()), torch.where(pick > 0.975, torch.ones(()), im_s))
    noise = rnd((1, 3, H, W), seed + 2, -1.5 * EPS, 1.5 * EPS)
    gnet = rnd((B, 3, H, W), seed + 3, -1e-3, 1e-3)
    # two pixels where every image's gradient is stopped: above 1 with a gradient pushing up, below 0 pushing down
    im_s[:, :, 0, 0], noise[:, :, 0, 0], gnet[:, :, 0, 0] = 1.0, 0.5 * EPS, -1e-3
    im_s[:, :, 0, 1], noise[:, :, 0, 1], gnet[:, :, 0, 1] = 0.0, -0.5 * EPS, 1e-3
    m = rnd((1, 3, H, W), seed + 4, -1e-4, 1e-4)
    v = rnd((1, 3, H, W), seed + 5, 0.0, 1e-7)
    return im_s, noise, gnet, m, v


SHAPES = [(B, H, W) for (H, W) in ((5, 7), (8, 12)) for B in (1, 2, 5)] + [(2, 512, 768)]
# 5x7: the scalar form (H W % 4 != 0); 8x12: the 16-byte form; 512x768: 98304 quads > 256 blocks x 256 threads, so the
# grid-stride loop wraps


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_prologue_equals_per_image_prologue(B, H, W):
    from imagecompression_adversarial_amd import hip_ops as K
    from imagecompression_adversarial_amd._lib import call, ptr, stream
    im_s, noise, _, _, _ = _inputs(B, H, W, 100 + B)
    im_s, noise = im_s.to(DEV), noise.to(DEV)
    nb = K.blocks_per_image()
    out, part = K.empty_nc4(B, 3, H, W, DEV), torch.empty(B * nb, device=DEV)
    ref, rpart = K.empty_nc4(B, 3, H, W, DEV), torch.empty(B * nb, device=DEV)
    call("ica_universal_prologue", ptr(noise), ptr(im_s), ptr(out), ptr(part), B, H, W, EPS, stream())
    call("ica_attack_prologue_ex", ptr(noise.expand(B, -1, -1, -1).contiguous()), ptr(im_s), ptr(ref), ptr(rpart),
         B, H, W, EPS, 1, stream())
    assert torch.equal(out, ref)
    assert torch.equal(part, rpart)
    assert float(part.sum()) > 0.0


def _universal_adam(im_s, noise, gnet4, m, v, loss, B, H, W, census):
    from imagecompression_adversarial_amd._lib import call, ptr, stream
    nz, mm, vv = noise.clone(), m.clone(), v.clone()
    loss_i = torch.full((B,), loss, device=DEV)
    im_in = torch.full_like(im_s, -7.0)
    branch = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    call("ica_universal_adam", ptr(nz), ptr(im_s), ptr(gnet4), ptr(loss_i), ptr(mm), ptr(vv), ptr(im_in), B, H, W,
         EPS, THR, GSCALE, BC2S, NEG_STEP, ptr(branch), ptr(census), stream())
    return nz, mm, vv, im_in, branch


def _per_image_adam(im_s, noise, gnet4, m, v, loss, H, W, clamp_in):
    """The existing kernel on ONE image (ica_attack_adam_ex)."""
    from imagecompression_adversarial_amd._lib import call, ptr, stream
    nz, mm, vv = noise.clone(), m.clone(), v.clone()
    loss_i = torch.full((1,), loss, device=DEV)
    call("ica_attack_adam_ex", ptr(nz), ptr(im_s), ptr(gnet4), ptr(loss_i), None, ptr(mm), ptr(vv), None, 1, H, W,
         EPS, THR, GSCALE, BC2S, NEG_STEP, None, None, None, clamp_in, stream())
    return nz, mm, vv


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_adam_equals_pinned_adam_on_restated_sum(B, H, W):
    from imagecompression_adversarial_amd import hip_ops as K
    im_s, noise, gnet, m, v = _inputs(B, H, W, 200 + B)
    d = [t.to(DEV) for t in (im_s, noise, gnet, m, v)]
    gnet4 = K.to_nc4(d[2])
    census = torch.zeros(B, dtype=torch.int32, device=DEV)
    im_in_ref = im_in_of(noise, im_s, EPS)
    for cheap, loss in ((False, 0.0), (True, 2 * THR)):
        nz, mm, vv, im_in, branch = _universal_adam(d[0], d[1], gnet4, d[3], d[4], loss, B, H, W, census)
        G = masked_sum(noise, im_s, gnet, cheap, EPS, GSCALE)
        assert float(G.abs().max()) > 0.0 and bool((G[0, :, 0, :2] == 0).all())     # gradients pass, masks bite
        rn, rm, rv = _per_image_adam(d[0][:1].contiguous(), d[1], K.to_nc4(G.to(DEV)), d[3], d[4], 0.0, H, W, 0)
        assert torch.equal(nz, rn), cheap
        assert torch.equal(mm, rm), cheap
        assert torch.equal(vv, rv), cheap
        assert not torch.equal(nz, d[1])
        assert torch.equal(im_in.cpu(), im_in_ref), cheap
        assert branch.tolist() == [int(cheap)] * B
        assert census.tolist() == [int(cheap)] * B      # incremented on the cheap call only


@pytest.mark.parametrize("H,W", [(5, 7), (8, 12)])
def test_adam_one_image_equals_per_image_kernel(H, W):
    from imagecompression_adversarial_amd import hip_ops as K
    d = [t.to(DEV) for t in _inputs(1, H, W, 300)]
    gnet4 = K.to_nc4(d[2])
    for loss in (0.0, 2 * THR):
        nz, mm, vv, _, _ = _universal_adam(d[0], d[1], gnet4, d[3], d[4], loss, 1, H, W, None)
        rn, rm, rv = _per_image_adam(d[0], d[1], gnet4, d[3], d[4], loss, H, W, 1)
        assert torch.equal(nz, rn) and torch.equal(mm, rm) and torch.equal(vv, rv), loss


X = rnd((3, 3, 64, 128), 51)
# (noise_thr, epsilon, steps, the oracle's branch sequence): chosen on the CPU so that the oracle's fp32 and float64
# runs take the same branches; nearest loss_i 15 % (a) and 4.6 % (c) from the threshold, (b) all expensive with 44 % of
# the noise on the epsilon bound
SETTINGS = {"a": (4e-6, 16.0, 8, [0, 0, 0, 1, 0, 0, 0, 0]),
            "b": (4e-6, 0.5, 8, [0] * 8),
            "c": (2e-6, 0.5, 12, [0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0])}


@pytest.mark.parametrize("name", list(SETTINGS))
def test_universal_attack_vs_oracle(hyper3, name):
    from imagecompression_adversarial_amd.universal import applied_noise, universal_batch
    P, kern = hyper3
    thr, epsilon, steps, expect = SETTINGS[name]
    rec = []
    ref = oatt.attack(P, X, steps=steps, epsilon=epsilon, noise_thr=thr, coupled=True, eval_msssim=False, record=rec,
                      init_noise=torch.zeros(1, 3, 64, 128))
    assert tuple(ref.noise.shape) == (1, 3, 64, 128)
    assert [int(r["cheap"][0]) for r in rec] == expect
    res = universal_batch(kern, X.to(DEV), steps=steps, epsilon=epsilon, noise_thr=thr, eval_msssim=False, record=True)
    print(name, "oracle loss_i / thr:", [round(float(r["loss_i"][0]) / thr, 4) for r in rec])
    print(name, "gpu branches:", [br[0] for br in res.branches])
    for i, br in enumerate(res.branches):
        assert len(br) == 3 and len(set(br)) == 1, (i, br)
        assert bool(br[0]) == bool(rec[i]["cheap"][0]), i
    e_noise, e_adv = rel_err(res.noise.cpu(), ref.noise), rel_err(res.im_adv.cpu(), ref.im_adv)
    print(name, "rel_err noise", e_noise, "im_adv", e_adv)
    assert tuple(res.noise.shape) == (1, 3, 64, 128)
    assert e_noise < 2e-3
    assert e_adv < 1e-5
    # |noise| <= eps after clipping; im_adv = fl(im_s + noise_c) adds one rounding at magnitude <= 1 (2^-24)
    eps = float(np.float32(epsilon / 255.0))
    assert float(applied_noise(res.noise, epsilon).abs().max()) <= eps
    assert float((res.im_adv - X.to(DEV)).abs().max()) <= eps + 2.0 ** -23
    assert float(res.im_adv.min()) >= 0.0 and float(res.im_adv.max()) <= 1.0


def test_one_image_equals_coupled_attack(hyper3):
    from imagecompression_adversarial_amd.attack import attack_batch
    from imagecompression_adversarial_amd.universal import universal_batch
    _, kern = hyper3
    x = X[:1].to(DEV).contiguous()
    kw = dict(steps=8, noise_thr=4e-6, eval_msssim=False, record=True)
    res = universal_batch(kern, x, **kw)
    ref = attack_batch(kern, x, coupled=True, **kw)
    assert res.branches == ref.branches
    assert torch.equal(res.noise, ref.noise)
    assert torch.equal(res.im_adv, ref.im_adv)


def test_graph_and_eager_same_bits(hyper3):
    from imagecompression_adversarial_amd.universal import UniversalAttackLoop
    _, kern = hyper3
    thr, epsilon, steps, _ = SETTINGS["b"]
    out = []
    for graph in (True, False):
        loop = UniversalAttackLoop(kern, X.to(DEV), steps=steps, epsilon=epsilon, noise_thr=thr)
        assert loop.graph_ok
        loop.graph_ok = graph
        loop.run()
        assert (loop.graph_replays > 0) == graph
        out.append(loop.noise.clone())
    assert torch.equal(out[0], out[1])


def test_heldout(hyper3):
    """The library's held-out score on the fit images is the fit's own mse_in.  The noise that made the fit's last
    im_in is the loop's variable BEFORE the last Adam update, clipped to +-eps (AttackResult.noise is the variable after
    it, as the oracle's is), so the loop is stepped here and that noise is taken in front of the last step."""
    from imagecompression_adversarial_amd import transfer
    from imagecompression_adversarial_amd.attack import evaluate
    from imagecompression_adversarial_amd.universal import UniversalAttackLoop, applied_noise, heldout
    _, kern = hyper3
    thr, epsilon, steps, _ = SETTINGS["b"]
    x = X.to(DEV)
    loop = UniversalAttackLoop(kern, x, steps=steps, epsilon=epsilon, noise_thr=thr)
    for i in range(steps - 1):
        loop.step(i)
    noise = applied_noise(loop.noise, epsilon)
    loop.step(steps - 1, record_im_in=True)
    mse_in = evaluate(kern, loop.im_in, loop.im_s, loop.output_s, msssim=False)[3]
    assert float(mse_in.min()) > 0.0
    got = heldout(kern, noise, x)
    assert tuple(got.mse_in.shape) == (1, 3)
    assert torch.allclose(got.mse_in[0], mse_in, rtol=1e-5, atol=0.0)
    y = rnd((4, 3, 64, 128), 52).to(DEV)
    a, b = heldout(kern, noise, y, 2), transfer.transfer_matrix(kern, noise, y, 2)
    assert torch.equal(a.mse_in, b.mse_in) and torch.equal(a.mse_out, b.mse_out)
    assert np.array_equal(np.array(a.vi), np.array(b.vi), equal_nan=True)     # (NaN under the 1e-20 guard: the
    assert float(a.mse_in.min()) > 0.0                                        # perturbed synthetic codec's rounded
    assert tuple(a.mse_in.shape) == (1, 4)                                    # latents do not move at eps 0.5 / 255)


def test_x6_executor(hyper3):
    """One other executor: shape, invariants and the fp32 run's branch record."""
    from imagecompression_adversarial_amd.engine import CodecKernels
    from imagecompression_adversarial_amd.universal import universal_batch
    P, kern = hyper3
    k6 = CodecKernels({k: v.to(DEV) for k, v in P.items()}, "hyper", precision="x6")
    x = X.to(DEV)
    kw = dict(steps=3, epsilon=0.5, noise_thr=4e-6, eval_msssim=False, record=True)
    r6, r32 = universal_batch(k6, x, **kw), universal_batch(kern, x, **kw)
    assert tuple(r6.noise.shape) == (1, 3, 64, 128)
    assert r6.branches == r32.branches
    assert float((r6.im_adv - x).abs().max()) <= float(np.float32(0.5 / 255.0)) + 2.0 ** -23
    assert float(r6.im_adv.min()) >= 0.0 and float(r6.im_adv.max()) <= 1.0
    assert float(r6.noise.abs().max()) > 0.0
