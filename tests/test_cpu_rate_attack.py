"""The bitrate attack's restatement (tests/rate_attack_restatement.py) on the CPU: its loss is the codec's zero-noise
train-mode likelihoods, its gradient matches a central finite difference in float64, its step bookkeeping is
oracle.attack.attack's, the CLI refuses what the attack does not cover, and the table of the kernel tests' bounds."""
import math

import pytest
import torch

from oracle import attack as oatt
from oracle import codec
from tests import loss_refs as R
from tests import rate_attack_restatement as RA

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("model", RA.MODELS)
def test_likelihoods_are_the_codec_forward_at_zero_noise(model):
    P = RA.params(model)
    x = RA.image((2, 3, 64, 64), 11)
    with torch.no_grad():
        y = codec.g_a(P, x)
        z0 = torch.zeros((2, P["entropy_bottleneck._bias0"].shape[0], 1, 1))
        ref = codec.forward(P, x, model, training=True, noise_y=torch.zeros_like(y), noise_z=z0)["likelihoods"]
        got = RA.relaxed_likelihoods(P, x, model)
    assert set(got) == set(ref)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    lo = RA.loss_o(P, x, model)
    bpp = torch.stack([codec.bpp({k: v[b:b + 1] for k, v in ref.items()}, 64 * 64) for b in range(2)])
    assert torch.allclose(-lo, bpp, rtol=1e-6, atol=0)


@pytest.mark.parametrize("model", RA.MODELS)
def test_gradient_vs_central_difference_float64(model):
    """<grad, d> against (L(x + h d) - L(x - h d)) / 2h, float64, 64 x 64, h = 1e-4, along one direction that
    follows the gradient's signs and two seeded normal ones.

    A LowerBound passes a gradient that its forward (a clamp) does not have, so where 0 < sigma < 0.11 autograd and
    a finite difference differ by design (1e-4 of the directional derivative with the seeded hyper weights).  The
    comparison therefore runs with h_s's last bias raised by 0.5, which puts every sigma above the bound (asserted),
    and every likelihood is far above 1e-9 (asserted): then the loss is piecewise smooth and the two must agree.
    Tolerance: 1e-5 relative (truncation, kinks of ReLU / |y| between the probes) + 50 eps |L| / h (rounding of the
    two float64 losses, sums of a few thousand logarithms)."""
    P = dict(RA.params(model))
    if model == "hyper":
        P["h_s.4.bias"] = P["h_s.4.bias"] + 0.5
    P64 = RA.to_dtype(P, F64)
    x = RA.image((1, 3, 64, 64), 13).to(F64) * 0.8 + 0.1
    with torch.no_grad():
        liks = RA.relaxed_likelihoods(P64, x, model)
        assert min(float(l.min()) for l in liks.values()) > 1e-6
        if model == "hyper":
            y = codec.g_a(P64, x)
            assert float(codec.h_s(P64, codec.h_a(P64, y.abs())).min()) > 0.12
    lo, g = RA.input_grad(P, x, model, F64)
    assert float(g.abs().max()) > 0
    h = 1e-4
    floor = 50 * 2.0 ** -52 * abs(float(lo.sum())) / h
    dirs = [torch.sign(g) * (0.5 + 0.5 * torch.rand(x.shape, generator=R.gen(5), dtype=F64))]
    dirs += [torch.randn(x.shape, generator=R.gen(seed), dtype=F64) for seed in (1, 2)]
    for k, d in enumerate(dirs):
        with torch.no_grad():
            fd = (RA.loss_o(P64, x + h * d, model).sum() - RA.loss_o(P64, x - h * d, model).sum()) / (2 * h)
        an = (g * d).sum()
        print(f"fd {model} dir {k}: autograd {float(an):.6e} fd {float(fd):.6e} floor {floor:.1e}")
        assert abs(float(fd - an)) <= 1e-5 * abs(float(an)) + floor, (model, k, float(fd), float(an))
    assert abs(float((g * dirs[0]).sum())) > 100 * floor   # the aligned direction is far above the rounding floor


def test_bookkeeping_is_the_oracles_on_cheap_steps():
    """Every step cheap (a start above the threshold): the rate loop and oracle.attack.attack run the same
    prologue, branch rule, Adam steps and LR schedule, so noise, records and eval agree bit for bit."""
    P = RA.params("hyper")
    x = RA.image((2, 3, 64, 64), 17)
    n0 = R.rnd(x.shape, 19, -1e-2, 1e-2)
    kw = dict(steps=7, noise_thr=1e-6, init_noise=n0, eval_msssim=False)
    ra, ro = [], []
    a = RA.attack(P, x, model="hyper", record=ra, **kw)
    o = oatt.attack(P, x, model="hyper", record=ro, **kw)
    assert all(bool(r["cheap"].all()) for r in ra) and all(bool(r["cheap"].all()) for r in ro)
    assert [r["lr"] for r in ra] == [r["lr"] for r in ro]
    assert len({r["lr"] for r in ra}) > 1   # the schedule moved
    for p, q in zip(ra, ro):
        assert torch.equal(p["loss_i"], q["loss_i"])
    assert torch.equal(a.noise, o.noise) and torch.equal(a.im_adv, o.im_adv)
    assert torch.equal(a.bpp, o.bpp) and torch.equal(a.bpp_ori, o.bpp_ori)
    from imagecompression_adversarial_amd.attack import _lr_table
    assert _lr_table(7, 0.01) == pytest.approx([r["lr"] for r in ra], rel=1e-12)


@pytest.mark.parametrize("model", RA.MODELS)
def test_trajectory_case_condition(model):
    """The GPU trajectory case needs at least 3 * B expensive image-steps: confirmed here on the restatement."""
    T = RA.TRAJ
    rec = []
    r = RA.attack(RA.params(model), RA.image(T["shape"], T["seed"]), steps=T["steps"], noise_thr=T["noise_thr"],
                  model=model, eval_msssim=False, record=rec)
    B = T["shape"][0]
    exp = sum(int((~q["cheap"]).sum()) for q in rec)
    print(f"trajectory {model}: expensive image-steps {exp} of {B * T['steps']}; bpp_ori {r.bpp_ori.tolist()} "
          f"bpp {r.bpp.tolist()}")
    assert exp >= 3 * B
    assert all(math.isfinite(v) for q in rec for v, c in zip(q["loss_o"].tolist(), q["cheap"].tolist()) if not c)


# --------------------------------------------------------------------------- #
# CLI guards
# --------------------------------------------------------------------------- #
BASE = ["-r", "-steps", "3", "-s", "synthetic:1x128x128", "--synthetic-weights", "-q", "1"]


@pytest.mark.parametrize("extra", [
    ["-t", "synthetic"],
    ["--mask_loc", "8", "40", "16", "48"],
    ["-att_metric", "ms-ssim"],
    ["--precision", "bf16"],
    ["-m", "context"],
    ["-m", "cheng2020"],
    ["-m", "debug"],
], ids=lambda e: " ".join(e))
def test_cli_guards_raise(extra):
    """-r with what the rate attack does not cover raises before a model is built (no device needed)."""
    from imagecompression_adversarial_amd import attack_rd
    with pytest.raises(NotImplementedError):
        attack_rd.main(BASE + extra)


def test_loop_guards_raise():
    from imagecompression_adversarial_amd.attack import rate_attack_guard
    rate_attack_guard(model="hyper", precision="x6")
    rate_attack_guard(model="factorized", precision="fp32")
    for kw in (dict(coupled=True), dict(target=object()), dict(roi=(0, 8, 0, 8)), dict(att_metric="ms-ssim"),
               dict(precision="bf16"), dict(model="context"), dict(model="cheng2020"), dict(model="debug")):
        with pytest.raises(NotImplementedError):
            rate_attack_guard(**kw)


# --------------------------------------------------------------------------- #
# The kernel cases: planted selects, and the table of bounds (tests/test_gpu_rate_attack.py)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", RA.KERNEL_SHAPES, ids=RA.shape_key)
def test_kernel_case_bounds(shape):
    tol = RA.RATE_TOL[RA.shape_key(shape)]
    y, s, planted = RA.gc_case(shape)
    assert float(s.min()) >= 0.0
    free = ~planted
    if bool(free.any()):   # the stated range of the non-planted elements
        assert float(s[free].min()) >= RA.GC_SIGMA[0] and float(s[free].max()) <= RA.GC_SIGMA[1]
        assert float((y[free].abs() / s[free]).max()) <= RA.GC_RATIO * (1 + 1e-6)
    raw = R.gc_raw(y, s)
    assert not bool(R._clear_band(raw).any())                  # every likelihood select is the same in both dtypes
    assert not bool(((s > 0.10) & (s < 0.12)).any())           # and every scale select
    refs = {dt: RA.gc_ref(y, s, dtype=dt) for dt in (F32, F64)}
    for dt in (F32, F64):
        gy, gs, _ = refs[dt]
        assert bool((gy[y == 0] == 0).all()) and bool((gs[s == 0] == 0).all())
        assert bool((gy[raw < 1e-11] == 0).all()) and bool((gs[raw < 1e-11] == 0).all())
        assert bool((gs[(s > 0) & (s < 0.11) & (y.abs() >= 0.75)] == 0).all())        # blocked by the scale bound
        assert bool((gs[(s > 0) & (s < 0.11) & (y.abs() <= 0.05)] < 0).all())         # passed by it
    P, v, _ = RA.eb_case(shape)
    eraw = R.eb_raw(P, v)
    assert not bool(R._clear_band(eraw).any())
    far = v.abs() >= RA.EB_FAR
    assert bool((eraw[far] < 1e-11).all()) and bool((eraw[~far] > 1e-7).all())
    erefs = {dt: RA.eb_ref(P, v, dtype=dt) for dt in (F32, F64)}
    for dt in (F32, F64):
        assert bool((erefs[dt][0][far] == 0).all())
    e = dict(gy=R.rel_err(refs[F32][0], refs[F64][0]), gsig=R.rel_err(refs[F32][1], refs[F64][1]),
             gc_sumln=R.rel_err(refs[F32][2], refs[F64][2]), gv=R.rel_err(erefs[F32][0], erefs[F64][0]),
             eb_sumln=R.rel_err(erefs[F32][1], erefs[F64][1]))
    for k, ev in e.items():
        rule = R.round_up_1digit(4 * max(ev, 2.0 ** -24))
        print(f"e_ref rate {RA.shape_key(shape):10s} {k:9s} {ev:9.2e}   rule -> {rule:.0e}   bound {tol[k]:.0e}")
        assert ev == ev and ev <= tol[k], (shape, k, ev, tol[k])
