"""GPU parity of the C&W-style binary-search attack (imagecompression_adversarial_amd.attack_cw, ica_cw.hip)
against its B = 1 CPU restatement (tests/cw_restatement.py).

Tolerances (the project's): one / two steps noise, m, v rel <= 2e-3, im_in rel <= 1e-5; the state machine
EXACT; trajectories: identical per-round decision histories, final noise max rel < 1e-2 with 99.9 % of the
elements < 1e-3, im_adv rel < 1e-4, bpp / mse_in as test_attack_vs_oracle_256; batch independence BIT-EXACT.
The trajectory inputs are the ones tests/test_cpu_cw.py pins (every decision >= 1e-2 from its threshold).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cw_restatement as R
from tests.conftest import REPO, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KW = dict(epsilon=R.SETTINGS["epsilon"], noise_thr=R.SETTINGS["noise_thr"], lr=R.SETTINGS["lr"],
          lamb_attack=R.SETTINGS["la"], max_level=R.SETTINGS["max_level"])


@pytest.fixture(scope="module")
def hyper3():
    from imagecompression_adversarial_amd.engine import CodecKernels
    P = R.hyper3_params()
    return P, CodecKernels({k: v.to(DEV) for k, v in P.items()}, "hyper")


@pytest.fixture(scope="module")
def pinned(hyper3):
    """The pinned B = 3 batches on the device, both modes: (result, history), computed once."""
    from imagecompression_adversarial_amd.attack_cw import cw_attack_batch
    _, kern = hyper3
    return {fast: cw_attack_batch(kern, R.images(fast).to(DEV), R.STEPS, search_steps=R.SSTEPS, fast=fast,
                                  record=True, eval_msssim=False, **KW) for fast in (False, True)}


def test_single_steps_vs_restatement(hyper3):
    """B = 2 with the level between the two images' mse_o: image 0 is gated (c_eff = 0), image 1 is not."""
    from imagecompression_adversarial_amd.attack_cw import CwAttackLoop
    P, kern = hyper3
    x = torch.cat([R.rnd(R.SHAPE, 12), R.rnd(R.SHAPE, 11) * 0.5], 0)
    level, la, lr = 1.8e-6, 1.0, 0.01
    loop = CwAttackLoop(kern, x.to(DEV), steps=2, lr=lr, lamb_attack=la, search_steps=2, max_level=level)
    refs = []
    for b in range(2):
        out_s, _ = R.pre_eval(P, x[b:b + 1])
        refs.append((R.Level(P, x[b:b + 1], out_s, 16.0, lr), R.new_state(1e-4, la, 2, level)))
    for step in range(2):
        loop.cw_step(record_im_in=True)
        ref = [lv.step(st) for lv, st in refs]
        mse_ref = [float(r[2]) for r in ref]
        assert mse_ref[0] > 1.1 * level * 1.01 and mse_ref[1] < 1.1 * level * 0.99
        assert loop.c_eff.tolist() == [0.0, 1.0] == [r[3] for r in ref]
        assert np.allclose(loop.mse_o.cpu().numpy(), mse_ref, rtol=1e-3, atol=0)
        assert np.allclose(loop.loss_i.cpu().numpy(), [float(r[1]) for r in ref], rtol=1e-3, atol=1e-12)
        assert loop.si[0].tolist() == [step + 1] * 2
        for b, (lv, _) in enumerate(refs):
            m, v = lv.adam_state()
            assert rel_err(loop.noise[b].cpu(), lv.noise.detach()[0]) < 2e-3, (step, b)
            assert rel_err(loop.m[b].cpu(), m[0]) < 2e-3, (step, b)
            assert rel_err(loop.v[b].cpu(), v[0]) < 2e-3, (step, b)
            assert rel_err(loop.im_in[b].cpu(), ref[b][0][0]) < 1e-5, (step, b)
    assert float(loop.noise[0].abs().max()) == 0.0 and float(loop.noise[1].abs().max()) > 0.0


def _device_state(states):
    sd = torch.tensor([[s[k] for s in states] for k in ("c_l", "c_r", "c", "level", "min", "max")],
                      dtype=torch.float64)
    si = torch.tensor([[s[k] for s in states] for k in ("t", "round", "levels", "active", "reset")],
                      dtype=torch.int32)
    lold = torch.stack([s["loss_i_old"].float() for s in states])
    return sd, lold, si


def drive_round_update(fast, on_round, B=256, ssteps=4, la=0.2, thr=1e-4, steps=5):
    """B random (loss_i, mse_o) sequences through round_update; on_round(states, loss_i, mse_o, cap) after every
    round.  loss_i hovers around noise_thr (a third of the sequences within the break window), mse_o around the
    level (a third within the fast rule's 1 % residual window).  Returns (states, rounds per finished level)."""
    from imagecompression_adversarial_amd.attack_cw import max_rounds_per_level
    cap = max_rounds_per_level(fast, la, ssteps)
    g = torch.Generator().manual_seed(5 + fast)
    states = [R.new_state(thr, la, ssteps, 0.1, max_rounds=cap) for _ in range(B)]
    li_base = torch.where(torch.rand(B, generator=g) < 0.35, thr * (1 + 0.16 * (torch.rand(B, generator=g) - 0.5)),
                          thr * (0.2 + 2.0 * torch.rand(B, generator=g)))
    li_jit = torch.where(torch.rand(B, generator=g) < 0.5, torch.tensor(2e-3), torch.tensor(0.3))
    tight = torch.rand(B, generator=g) < 0.35
    rounds_per_level, rounds = [], 0
    while any(s["active"] for s in states):
        rounds += 1
        assert rounds <= ssteps * cap
        loss_i = (li_base * (1 + li_jit * (torch.rand(B, generator=g) - 0.5))).float()
        u = torch.where(tight, 0.99 * (1 + 0.03 * (torch.rand(B, generator=g) - 0.5)),
                        0.7 + 0.6 * torch.rand(B, generator=g))
        mse_o = (torch.tensor([s["level"] for s in states], dtype=torch.float64) * u.double()).float()
        for b, s in enumerate(states):
            if not s["active"]:
                continue
            s["t"] += steps
            r0 = s["round"]
            R.round_update(s, loss_i[b], mse_o[b], fast)
            if s["active"] == 0 or s["reset"]:
                rounds_per_level.append(r0 + 1)
        on_round(states, loss_i, mse_o, cap)
    return states, rounds_per_level, cap


@pytest.mark.parametrize("fast", [False, True])
def test_round_kernel_vs_round_update(fast):
    """ica_cw_round == round_update in every state field after every round, for 256 random (loss_i, mse_o)
    sequences: ones that stop by the break test, by the level count, and whose levels end at the round cap."""
    from imagecompression_adversarial_amd._lib import call, ptr, stream
    B, ssteps, la, thr, steps = 256, 4, 0.2, 1e-4, 5
    sd, lold, si = (t.to(DEV) for t in _device_state([R.new_state(thr, la, ssteps, 0.1) for _ in range(B)]))
    n_act = torch.zeros(1, dtype=torch.int32, device=DEV)
    cfg = (ctypes.c_double * 2)(la, thr)

    def on_round(states, loss_i, mse_o, cap):
        si[0] += steps * si[3]
        li_d, mo_d = loss_i.to(DEV), mse_o.to(DEV)   # (named: ptr() does not keep a temporary alive)
        call("ica_cw_round", ptr(li_d), ptr(mo_d), ptr(sd), ptr(lold), ptr(si), ptr(n_act), B, int(fast), ssteps,
             cap, cfg, stream())
        want_sd, want_lold, want_si = _device_state(states)
        assert torch.equal(sd.cpu(), want_sd)
        assert torch.equal(lold.cpu(), want_lold)
        assert torch.equal(si.cpu(), want_si)
        assert int(n_act) == sum(s["active"] for s in states)

    states, rounds_per_level, cap = drive_round_update(fast, on_round, B, ssteps, la, thr, steps)
    ends = [s["ended_by"] for s in states]
    assert ends.count("break") >= 10 and ends.count("levels") >= 10, (ends.count("break"), ends.count("levels"))
    if fast:
        # a level's natural round cap: the first round keeps the width when c_r moves, then 11 halvings bring
        # 0.2 under 1e-4; the safety cap of the Adam table (13) is never the reason
        assert max(rounds_per_level) == 12 and min(rounds_per_level) == 1 and cap == 13
    else:
        assert set(rounds_per_level) == {ssteps}


@pytest.mark.parametrize("fast", [False, True])
def test_trajectory_vs_restatement(hyper3, pinned, fast):
    """steps = 6, ssteps = 3, B = 3 against three B = 1 restatement runs: identical decision histories and final
    search state; final noise max rel < 1e-2 with 99.9 % of the elements < 1e-3; im_adv rel < 1e-4; bpp, mse_in.
    (tests/test_cpu_cw.py checks that the restatement's own rounding error on these inputs is a fifth of that.)"""
    res, hist = pinned[fast]
    refs = R.reference(fast)
    noise_stat, missed = {}, []
    for b, ref in enumerate(refs):
        mine = [(h["c"][b], h["level"][b], h["loss_i"][b], h["mse_o"][b]) for h in hist if h["active"][b]]
        want = [(h["c"], h["level"], h["loss_i"], h["mse_o"]) for h in ref["history"]]
        # c and level are doubles produced by the same decisions: identical, round for round
        assert [m[:2] for m in mine] == [w[:2] for w in want], (fast, b)
        assert np.allclose([m[2:] for m in mine], [w[2:] for w in want], rtol=1e-3, atol=1e-15), (fast, b)
        st = ref["state"]
        assert int(res.loop.si[2, b]) == st["levels"] and int(res.loop.si[3, b]) == 0
        assert [float(res.loop.sd[k, b]) for k in range(6)] == [st[k] for k in ("c_l", "c_r", "c", "level", "min",
                                                                                 "max")]
        nz, nr = res.noise[b].cpu(), ref["noise"][0]
        if float(nr.abs().max()) == 0.0:     # gated through its last level: the noise never left zero
            assert float(nz.abs().max()) == 0.0
        else:
            d = (nz - nr).abs() / nr.abs().max()
            noise_stat[b] = (float(d.max()), float((d < 1e-3).float().mean()))
            print("noise statistic", fast, b, noise_stat[b])
        e_adv = rel_err(res.im_adv[b].cpu(), ref["eval"].im[0])
        print("im_adv rel", fast, b, e_adv)
        if not e_adv < 1e-4:
            missed.append(("im_adv rel", fast, b, e_adv))
        assert rel_err(res.output_s[b].cpu(), ref["output_s"][0]) < 1e-4
        assert torch.allclose(res.bpp_ori[b].cpu(), ref["bpp_ori"], rtol=1e-4, atol=1e-5)
        assert torch.allclose(res.bpp[b].cpu(), ref["eval"].bpp[0], rtol=1e-4, atol=1e-5)
        assert torch.allclose(res.mse_in[b].cpu(), ref["eval"].mse_in[0], rtol=1e-3, atol=1e-12)
    assert noise_stat
    for b, (dmax, frac) in noise_stat.items():
        if not (dmax < 1e-2 and frac > 0.999):
            missed.append(("noise max rel, fraction < 1e-3", fast, b, dmax, frac))
    assert not missed, missed


def test_batch_independence_bitexact(hyper3, pinned):
    """Image 1 of the B = 3 run == its B = 1 run, while image 0 stops earlier (break after its second level)."""
    from imagecompression_adversarial_amd.attack_cw import cw_attack_batch
    _, kern = hyper3
    rb, hist = pinned[False]
    assert rb.loop.si[2].tolist()[0] != rb.loop.si[2].tolist()[1]
    assert sum(h["active"][0] for h in hist) < sum(h["active"][1] for h in hist)
    x1 = R.images(False)[1:2].to(DEV).contiguous()
    r1 = cw_attack_batch(kern, x1, R.STEPS, search_steps=R.SSTEPS, eval_msssim=False, **KW)
    assert torch.equal(rb.noise[1:2], r1.noise)
    assert torch.equal(rb.output_adv[1:2], r1.output_adv)
    assert torch.equal(rb.bpp[1:2], r1.bpp)


@pytest.mark.parametrize("fast", [False, True])
def test_no_host_in_the_loop(pinned, fast):
    res, hist = pinned[fast]
    loop = res.loop
    assert loop.rounds == len(hist) == max(len(r["history"]) for r in R.reference(fast))
    assert loop.host_reads == loop.rounds
    assert loop.graph_replays == loop.rounds * R.STEPS == loop.steps_done
    assert loop.sync_steps == 0


def test_invariants(hyper3):
    from imagecompression_adversarial_amd.attack_cw import CwAttackLoop, cw_attack_batch
    _, kern = hyper3
    # the box binds: a large step and loss weight against a small epsilon
    x = torch.cat([R.rnd(R.SHAPE, 41), R.rnd(R.SHAPE, 42) * 0.5], 0).to(DEV)
    res = cw_attack_batch(kern, x, steps=3, epsilon=2.0, lr=0.2, lamb_attack=1000.0, search_steps=2,
                          eval_msssim=False)
    eps = np.float32(2 / 255.0)
    assert float(res.noise.abs().max()) > eps
    # im_in = fl(im_s + noise_c): half an ulp of a value in [0.5, 1] (2^-24) over the box at most
    assert float((res.im_adv - x).abs().max()) <= float(eps) + 2.0 ** -24 * (1 + 2.0 ** -6)
    assert float(res.im_adv.min()) >= 0.0 and float(res.im_adv.max()) <= 1.0
    # a finished image's noise / m / v / im_in do not change while the others continue
    loop = CwAttackLoop(kern, R.images(False).to(DEV), R.STEPS, search_steps=R.SSTEPS, **KW)
    frozen, n = None, 3
    while n:
        for i in range(R.STEPS):
            loop.cw_step(record_im_in=(i == R.STEPS - 1))
        n = loop.round_end()
        if frozen is None and int(loop.si[3, 0]) == 0 and n:
            frozen = [t[0].clone() for t in (loop.noise, loop.m, loop.v, loop.im_in)]
    assert frozen is not None
    for a, t in zip(frozen, (loop.noise, loop.m, loop.v, loop.im_in)):
        assert torch.equal(a, t[0])


@pytest.mark.parametrize("model", ["hyper", "cheng2020"])
def test_cli_end_to_end(tmp_path, model):
    cmd = [sys.executable, "-m", "imagecompression_adversarial_amd.attack_cw", "-m", model, "-q", "3", "-s",
           "synthetic:2x64x64", "--synthetic-weights", "-steps", "2", "-ssteps", "2", "--batch", "2"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("synthetic_", "AVG:"))]
    assert len(lines) == 3 and lines[0].startswith("synthetic_0 ") and lines[1].startswith("synthetic_1 ")
    assert all("Time:" in ln for ln in lines[:2]) and lines[2].startswith("AVG: 3 "), r.stdout[-2000:]
    assert len(lines[2].split()) == 7
