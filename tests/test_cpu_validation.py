"""The trainer's validation without a device: the new train flags, ValidationPolicy against the reference's rule and
a hand-stepped ReduceLROnPlateau, the restatement's plain loss against this package's RateDistortionLoss, the sharded
float64 mean over gloo at world 2, and the log line's format (tests/validation_restatement.py)."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import codec
from tests import rd_eval_restatement as RD
from tests import validation_restatement as VR

F32, F64 = torch.float32, torch.float64


# --------------------------------------------------------------------------- #
# CLI
# --------------------------------------------------------------------------- #
def test_config_parses_the_validation_flags():
    from imagecompression_adversarial_amd import train
    d = train.config().parse_args([])
    assert d.val is None and d.val_every is None and d.val_batch == 8 and d.ckpt_dir is None
    a = train.config().parse_args(["-val", "synthetic:2x64x64", "--val-every", "5", "--val-batch", "3",
                                   "--ckpt-dir", "somewhere"])
    assert (a.val, a.val_every, a.val_batch, a.ckpt_dir) == ("synthetic:2x64x64", 5, 3, "somewhere")


def test_recompress_is_refused_with_its_reason():
    from imagecompression_adversarial_amd import train
    for extra in ([], ["--adv"]):
        with pytest.raises(NotImplementedError, match="re-compression"):
            train.train(train.config().parse_args(["-re", "1", "--synthetic-weights", "-device", "cpu"] + extra))


def test_checkpoint_dir_follows_the_reference():
    from imagecompression_adversarial_amd import train
    a = train.config().parse_args(["-m", "hyper", "-metric", "mse", "-noise", "0.001", "-steps", "7"])
    assert train.checkpoint_dir(a, 0.0067) == "./ckpts/anchor/hyper-0.0067-mse"
    assert train.checkpoint_dir(a, 100) == "./ckpts/anchor/hyper-Inf-mse"
    assert train.checkpoint_dir(a, 1) == "./ckpts/anchor/hyper-Inf-mse"
    a.adv = True
    assert train.checkpoint_dir(a, 0.0067) == "./ckpts/adv/hyper-0.0067-mse-0.001-7"
    a.ckpt_dir = "elsewhere"
    assert train.checkpoint_dir(a, 0.0067) == "elsewhere"


def test_empty_validation_glob_raises(tmp_path):
    from imagecompression_adversarial_amd import validate
    with pytest.raises(FileNotFoundError):
        validate.val_items(str(tmp_path / "none*.png"))
    assert [it[0] for it in validate.val_items("synthetic:3x64x64")] == [f"synthetic_{i}" for i in range(3)]


def test_msssim_refuses_a_small_image_by_name(tmp_path):
    from imagecompression_adversarial_amd import coder, validate
    coder.write_image(RD.image((1, 3, 176, 192), 3), str(tmp_path / "a_big.png"))
    coder.write_image(RD.image((1, 3, 100, 192), 4), str(tmp_path / "b_small.png"))
    items = validate.val_items(str(tmp_path / "*.png"))
    with pytest.raises(ValueError, match="b_small.png"):
        validate.check_msssim_sizes(items)
    validate.check_msssim_sizes(items[:1])


# --------------------------------------------------------------------------- #
# ValidationPolicy
# --------------------------------------------------------------------------- #
def _scheduler(lr=1e-4):
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    return opt, torch.optim.lr_scheduler.ReduceLROnPlateau(opt, "min", factor=0.5)


def test_policy_fires_at_the_reference_steps():
    from imagecompression_adversarial_amd.train import ValidationPolicy
    adv = ValidationPolicy(True, 2001)
    fired = [s for s in range(2001) if adv.due(s)]
    assert fired == list(range(10, 2001, 10))                       # train.py:432: step % 10 == 0 and step > 0
    assert adv.finished(2000) and not adv.finished(1999)            # train.py:455
    plain = ValidationPolicy(False, 25001)
    assert [s for s in range(25001) if plain.due(s)] == [10000, 20000, 25000]    # :458, and once after the last step
    plain = ValidationPolicy(False, 20001)
    assert [s for s in range(20001) if plain.due(s)] == [10000, 20000]           # the last step is due already
    assert not any(plain.finished(s) for s in (2000, 20000))
    every = ValidationPolicy(True, 21, period=7)
    assert [s for s in range(21) if every.due(s)] == [7, 14]
    off = ValidationPolicy(True, 301, enabled=False, save_every=100)
    assert not any(off.due(s) for s in range(301))
    assert [s for s in range(301) if off.save_due(s)] == [100, 200, 300]
    assert not any(adv.save_due(s) for s in range(301))
    assert not ValidationPolicy(True, 3001, enabled=False).finished(2000)   # without -val the loop is today's


def test_policy_best_save_and_lr_follow_the_rule():
    from imagecompression_adversarial_amd.train import ValidationPolicy
    # a scripted loss per validation: improves, then stalls for longer than torch's patience (10)
    losses = [5.0, 4.0, 4.5, 3.0] + [3.5] * 12 + [2.0, 2.5]
    policy = ValidationPolicy(True, 2001)
    opt, sch = _scheduler()
    ref_opt, ref_sch = _scheduler()
    best, lrs, ref_lrs = float("inf"), [], []
    for k, loss in enumerate(losses):
        step = 10 * (k + 1)
        assert policy.due(step)
        is_best, save = policy.update(loss, step, sch)
        ref_sch.step(loss)                                          # the scheduler stepped by hand
        want_best = loss < best
        best = min(best, loss)
        assert is_best == want_best and policy.best == best, (step, loss)
        assert save == (want_best or step % 100 == 0), (step, loss)   # train.py:442
        lrs.append(opt.param_groups[0]["lr"])
        ref_lrs.append(ref_opt.param_groups[0]["lr"])
    assert lrs == ref_lrs
    assert lrs[3] == 1e-4 and lrs[3 + 11] == 5e-5 and lrs[-1] == 5e-5    # halves on the 11th validation without a best
    assert sch.state_dict()["last_epoch"] == len(losses)
    assert [k for k, l in enumerate(losses) if l == best] == [16]


def test_policy_best_survives_a_checkpoint_round_trip(tmp_path):
    from imagecompression_adversarial_amd.train import ValidationPolicy, save_checkpoint
    policy = ValidationPolicy(False, 100, period=10)
    _, sch = _scheduler()
    for step, loss in ((10, 3.0), (20, 1.5), (30, 2.0)):
        policy.update(loss, step, sch)
    path = str(tmp_path / "sub" / "ckpt.pth.tar")
    save_checkpoint({"epoch": 0, "step": 30, "loss": 2.0, "lr_scheduler": sch.state_dict(), "best": policy.best}, path)
    loaded = torch.load(path, weights_only=True)
    resumed = ValidationPolicy(False, 100, period=10, best=ValidationPolicy.best_of(loaded))
    assert resumed.best == 1.5
    _, sch2 = _scheduler()
    sch2.load_state_dict(loaded["lr_scheduler"])
    assert sch2.state_dict()["last_epoch"] == 3
    assert resumed.update(1.7, 40, sch2) == (False, False)          # worse than the stored best: no overwrite
    assert resumed.update(1.2, 50, sch2) == (True, True)
    del loaded["best"]                                              # a checkpoint from before the key existed
    assert ValidationPolicy.best_of(loaded) == float("inf") and ValidationPolicy.best_of(None) == float("inf")


# --------------------------------------------------------------------------- #
# The restatement against this package's RateDistortionLoss
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("model,metric,shape,lmbda", [
    ("hyper", "mse", (2, 3, 64, 64), 0.0018), ("factorized", "mse", (2, 3, 64, 64), 0.0018),
    ("hyper", "mse", (1, 3, 64, 64), 100.0),                        # the Inf mode: no rate term
    # 176 rows: y has 11, h_s(h_a(y)) 12, so the hyperprior is undefined there (the reference's fails too); the
    # factorized model takes every multiple of 16
    ("factorized", "ms-ssim", (1, 3, 176, 192), 2.40)])
def test_restatement_is_the_packages_rd_loss(monkeypatch, model, metric, shape, lmbda):
    """train.RateDistortionLoss(training=True), its MS-SSIM (HIP kernels) replaced by the oracle's pytorch_msssim
    restatement, on oracle codec.forward(training=False) outputs with N = 1: the same numbers."""
    from imagecompression_adversarial_amd import train
    from imagecompression_adversarial_amd.train import RateDistortionLoss
    from oracle import msssim as omsssim
    monkeypatch.setattr(train.MS, "ms_ssim", lambda X, Y, data_range=1.0: omsssim.ms_ssim(X, Y, data_range))
    P = RD.params(model)                                            # latents that do not all round to 0
    x = RD.image(shape, 31)
    got = VR.plain(P, x, model, metric, lmbda, F64)
    crit = RateDistortionLoss(metric, lmbda)
    with torch.no_grad():
        for b in range(shape[0]):
            xb = x[b:b + 1].double()
            out = codec.forward(RD.to_dtype(P, F64), xb, model, training=False)
            assert float(out["x_hat"].min()) < 0.0 or float(out["x_hat"].max()) > 1.0 or metric == "ms-ssim"
            want = crit(out, xb, training=True)
            for k, kk in (("loss", "loss"), ("bpp", "bpp_loss"), ("distortion", "distortion_loss")):
                assert float(got[k][b]) == pytest.approx(float(want[kk]), rel=1e-12, abs=0), (k, b)
    if lmbda == 100.0:
        assert float(got["loss"][0]) == pytest.approx(100.0 * 255 ** 2 * float(got["distortion"][0]), rel=1e-12)


def test_adv_case_has_a_defined_vi_on_the_oracle():
    """The committed seed: the float64 oracle's VI is defined for both images, and the fp32 oracle settles it to a
    tenth of the bound the GPU test uses."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    P, x = VR.adv_params(1), RD.image(VR.ADV_SHAPE, VR.ADV_SEED)
    v64 = VR.adv_vi(P, x, VR.ADV_STEPS, dtype=F64)
    v32 = VR.adv_vi(P, x, VR.ADV_STEPS, dtype=F32)
    assert all(v is not None for v in v64 + v32)
    assert max(abs(a - b) for a, b in zip(v32, v64)) <= VR.VI_TOL / 10
    assert VR.VI_TOL == pytest.approx(8.69e-3, rel=1e-3)


# --------------------------------------------------------------------------- #
# The sharded mean (gloo, world 2)
# --------------------------------------------------------------------------- #
VALUES = [3.2146811, 3.4179743, 0.0123457, 17.25, 2.5e-3]
VALUES = [float(torch.tensor(v, dtype=F32)) for v in VALUES]         # fp32 values, as the engine produces them


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q, splits):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    try:
        from imagecompression_adversarial_amd import dist as D
        from imagecompression_adversarial_amd import validate as V
        r, w, group = D.init_from_env("gloo")
        out = {}
        # the shards dist.shard_range gives: 5 values as 2 + 3, 1 value as 0 + 1 (rank 0's shard is empty)
        for name, vals in splits.items():
            sl = D.shard_range(len(vals), r, w)
            mine = vals[sl.start:sl.stop]
            rows = [{"v": v} for v in mine]
            means, n, sk = V.sharded_mean([V._sum64(rows, "v")], len(rows), 1 if name == "five" and r == 0 else 0,
                                          group)
            out[name] = (means[0].hex(), n, sk, len(mine))
        q.put((rank, out))
    except Exception as e:  # surface failures to the parent
        q.put((rank, {"error": repr(e)}))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_sharded_mean_world2_is_bit_identical_and_survives_an_empty_rank():
    from imagecompression_adversarial_amd import validate as V
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    splits = {"five": VALUES, "one": VALUES[:1]}
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, splits)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=120) for _ in procs)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    for r in (0, 1):
        assert "error" not in res[r], res[r]
    single, n, sk = V.sharded_mean([V._sum64([{"v": v} for v in VALUES], "v")], 5)
    assert (n, sk) == (5, 0) and single[0] == VR.mean64(VALUES)
    assert {res[0]["five"][3], res[1]["five"][3]} == {2, 3}
    for r in (0, 1):
        assert res[r]["five"][:3] == (single[0].hex(), 5, 1)       # the same bits on both ranks, and the skipped count
    assert {res[0]["one"][3], res[1]["one"][3]} == {0, 1}          # one rank's shard is empty
    for r in (0, 1):
        assert res[r]["one"][:3] == (VALUES[0].hex(), 1, 0)


def test_sharded_mean_raises_when_every_image_is_skipped():
    from imagecompression_adversarial_amd import validate as V
    with pytest.raises(RuntimeError, match="2 skipped"):
        V.sharded_mean([0.0], 0, 2)


# --------------------------------------------------------------------------- #
# The log line
# --------------------------------------------------------------------------- #
def test_log_line_is_the_references_format():
    from imagecompression_adversarial_amd.validate import ValResult, log_line
    plain = ValResult(loss=1.23456789, count=3, distortion=0.00123456789, bpp=0.456789)
    assert log_line(7, plain) == VR.log_line(7, 1.23456789, 0.00123456789, 0.456789)
    assert log_line(7, plain) == ("Test epoch 7: Average losses:\tLoss: 1.2346 |\tMSE loss: 0.001235 |\t"
                                  "Bpp loss: 0.457 |\tRecomp loss: 0.000\n")
    adv = ValResult(loss=3.31632, count=2, adv=True)
    assert log_line(0, adv) == VR.log_line(0, 0, 0, 0)[:-1] + " |\tVI: 3.3163\n"
