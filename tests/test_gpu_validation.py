"""The trainer's validation on the GPU: the ica_val_metrics kernel against float64, plain and --adv test_epoch against
the oracle restatement, rd_step against adv_step's second half and the oracle's train step, and the train CLI end to
end (validation steps, scheduler, best model, resume).

Bounds: tests/validation_restatement.py.  Kernel: 4 max(e_ref, 2^-24) rounded up to one digit, e_ref measured here as
the fp32 CPU restatement's distance from float64 on the same inputs.  Plain: FORWARD_TOL of
tests/rd_eval_restatement.py (bpp, mse relative 1e-3; msim absolute 1e-5) and the loss bounds that follow.  VI:
8.69e-3 dB.  rd_step: the tolerances of tests/test_gpu_train.py::test_adv_train_step_vs_oracle.
"""
import contextlib
import io
import os
from types import SimpleNamespace

import pytest
import torch

from oracle import attack as oa
from oracle import codec as oc
from tests import loss_refs as R
from tests import rd_eval_restatement as RD
from tests import validation_restatement as VR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def K():
    from imagecompression_adversarial_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def V():
    from imagecompression_adversarial_amd import validate
    return validate


def nc4_dirty(K, x):
    """to_nc4 with the padding lanes (c >= C) filled with 1e-30: a kernel that reads them shows it in a sum."""
    x4 = K.to_nc4(x.to(DEV))
    C = x.shape[1]
    if C % 4:
        x4[:, -1, :, :, C % 4:] = 1e-30
    return x4


def launch(K, c, want):
    ys, zs = c["lik_y"], c["lik_z"]
    return K.val_metrics(nc4_dirty(K, c["x_hat"]), c["target"].to(DEV), nc4_dirty(K, ys), ys.shape[1],
                         None if zs is None else nc4_dirty(K, zs), 0 if zs is None else zs.shape[1], want_x_hat=want)


# --------------------------------------------------------------------------- #
# Kernel
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", VR.KERNEL_CASES, ids=RD.case_key)
def test_val_metrics_vs_float64(K, case):
    c = RD.kernel_case(case)
    args = (c["x_hat"], c["target"], c["lik_y"], c["lik_z"])
    # the inputs hold what the issue asks for: reconstructions outside [0, 1], likelihoods at and below 2^-16
    assert float(c["x_hat"].min()) < 0.0 and float(c["x_hat"].max()) > 1.0
    for lik in (c["lik_y"], c["lik_z"]):
        if lik is not None:
            assert bool((lik == VR.LIK_MIN).any()) and bool((lik < VR.LIK_MIN).any())
    ref64 = VR.kernel_ref(*args, F64)
    e_ref = RD.kernel_errors(VR.kernel_ref(*args, F32), ref64)
    tol = VR.kernel_tol(e_ref)
    clamped = RD.kernel_ref(*args, F64)[0]
    got = launch(K, c, True)
    sse, lny, lnz, out = got
    e = RD.kernel_errors((sse.cpu(), lny.cpu(), lnz.cpu()), ref64)
    for k, v in e.items():
        print(f"val_metrics {RD.case_key(case)} {k} {v:.2e} e_ref {e_ref[k]:.2e} bound {tol[k]:.0e}")
    for k, v in e.items():
        assert v <= tol[k], (case, k, v, tol[k])
    # a clamped implementation is far outside the bound
    assert R.rel_err(clamped, ref64[0]) > 100 * tol["sse"]
    if c["lik_z"] is None:
        assert not bool(lnz.any())
    # the NCHW plane is the layout conversion of the input, bit for bit
    assert torch.equal(out.cpu(), c["x_hat"])
    # a null output pointer skips the store and changes no sum
    none = launch(K, c, False)
    assert none[3] is None and all(torch.equal(a, b) for a, b in zip(none[:3], got[:3]))
    # an image's numbers are the same bits alone and in the batch
    for b in range(case[0][0]):
        one = launch(K, {k: (v if v is None else v[b:b + 1]) for k, v in c.items()}, True)
        for a, full in zip(one, got):
            assert torch.equal(a, full[b:b + 1]), b


def test_val_metrics_refuses_bad_arguments(K):
    from imagecompression_adversarial_amd._lib import lib, ptr, stream
    c = RD.kernel_case(VR.KERNEL_CASES[1])
    xh4, tg = K.to_nc4(c["x_hat"].to(DEV)), c["target"].to(DEV)
    y4, z4 = K.to_nc4(c["lik_y"].to(DEV)), K.to_nc4(c["lik_z"].to(DEV))
    Cy, Cz = c["lik_y"].shape[1], c["lik_z"].shape[1]
    K.val_metrics(xh4, tg, y4, Cy, z4, Cz)
    for f in (lambda: K.val_metrics(xh4, tg, y4, 12, z4, Cz), lambda: K.val_metrics(xh4, tg, y4, Cy, None, Cz),
              lambda: K.val_metrics(xh4, tg, y4[:1].contiguous(), Cy, z4, Cz),
              lambda: K.val_metrics(None, tg, y4, Cy, z4, Cz), lambda: K.val_metrics(xh4, tg.cpu(), y4, Cy, z4, Cz)):
        with pytest.raises(ValueError):
            f()
    # the C entry: the file's status codes, nothing launched
    B, _, H, W = tg.shape
    part = torch.full((B * 3 * int(lib().ica_rd_metrics_blocks()),), -7.0, device=DEV)
    out = torch.empty_like(tg)
    f = lib().ica_val_metrics
    ok = (ptr(xh4), ptr(tg), ptr(y4), ptr(z4), ptr(out), ptr(part), B, H, W, Cy, 4, 4, Cz, 1, 1)
    for i in (0, 1, 2, 5):
        a = list(ok)
        a[i] = None
        assert f(*a, stream()) == -5, i
    for i, v in ((6, 0), (6, 70000), (7, 0), (9, 0)):
        a = list(ok)
        a[i] = v
        assert f(*a, stream()) == -5, i
    a = list(ok)
    a[3] = None                                                               # a z shape without a z plane
    assert f(*a, stream()) == -5
    a = list(ok)
    a[4] = ptr(tg)                                                             # the output on top of an input
    assert f(*a, stream()) == -7
    torch.cuda.synchronize()
    assert bool((part == -7.0).all())                                          # nothing ran
    a = list(ok)
    a[4] = None                                                                # no output plane: accepted
    assert f(*a, stream()) == 0 and f(*ok, stream()) == 0


# --------------------------------------------------------------------------- #
# Plain test_epoch against the restatement
# --------------------------------------------------------------------------- #
_KERN = {}


def kernels(model, precision="x6"):
    from imagecompression_adversarial_amd.engine import CodecKernels
    if (model, precision) not in _KERN:
        P = VR.plain_params(model)
        _KERN[(model, precision)] = (P, CodecKernels({k: v.to(DEV) for k, v in P.items()}, model, precision))
    return _KERN[(model, precision)]


# three images of two padded shapes: (file height, width) -> padded to x64 by coder.read_image
PLAIN_SIZES = {"mse": [(64, 64), (50, 120), (64, 64)], "ms-ssim": [(176, 192), (176, 250), (176, 192)]}
PLAIN_LAMBDA = {"mse": 0.0018, "ms-ssim": 2.40}


def write_images(tmp_path, sizes, seed=300):
    from imagecompression_adversarial_amd import coder
    for i, (h, w) in enumerate(sizes):
        coder.write_image(RD.image((1, 3, h, w), seed + i), str(tmp_path / f"im{i}.png"))
    return str(tmp_path / "im*.png")


@pytest.mark.parametrize("model,metric", [("hyper", "mse"), ("factorized", "mse"), ("hyper", "ms-ssim"),
                                          ("factorized", "ms-ssim")])
def test_plain_test_epoch_vs_restatement(V, tmp_path, model, metric):
    from imagecompression_adversarial_amd import coder
    P, kern = kernels(model)
    lmbda = PLAIN_LAMBDA[metric]
    items = V.val_items(write_images(tmp_path, PLAIN_SIZES[metric]))
    r2 = V.validate_plain(kern, items, metric, lmbda, batch=2, device=DEV)
    r1 = V.validate_plain(kern, items, metric, lmbda, batch=1, device=DEV)
    assert r2.count == 3 and [row["name"] for row in r2.rows] == [it[0] for it in items]
    assert (r1.loss, r1.bpp, r1.distortion) == (r2.loss, r2.bpp, r2.distortion)     # --val-batch changes no bit
    assert r1.rows == r2.rows
    refs = []
    for it in items:
        x, _, _ = coder.read_image(it[0])
        refs.append({k: float(v[0]) for k, v in VR.plain(P, x, model, metric, lmbda, F64).items()})
    tol = RD.FORWARD_TOL
    for row, ref in zip(r2.rows, refs):
        print(f"{model} {metric} {os.path.basename(row['name'])}: loss {row['loss']:.6f} ({ref['loss']:.6f}) bpp "
              f"{row['bpp']:.6f} ({ref['bpp']:.6f}) distortion {row['distortion']:.3e} ({ref['distortion']:.3e})")
    for row, ref in zip(r2.rows, refs):
        assert abs(row["bpp"] - ref["bpp"]) <= tol["bpp"] * abs(ref["bpp"])
        if metric == "mse":
            assert abs(row["distortion"] - ref["distortion"]) <= tol["mse"] * ref["distortion"]
            assert abs(row["loss"] - ref["loss"]) <= 1e-3 * ref["loss"]
        else:
            assert abs(row["distortion"] - ref["distortion"]) <= tol["msim"]
            assert abs(row["loss"] - ref["loss"]) <= lmbda * tol["msim"] + 1e-3 * ref["bpp"]
    # the means are float64 sums of the per-image fp32 values
    for k in ("loss", "bpp", "distortion"):
        assert getattr(r2, k) == VR.mean64([row[k] for row in r2.rows]), k
    assert len({row["distortion"] for row in r2.rows}) == 3


def test_plain_msssim_refuses_a_small_image(V, tmp_path):
    _, kern = kernels("hyper")
    items = V.val_items(write_images(tmp_path, [(176, 192), (64, 64)]))
    with pytest.raises(ValueError, match="im1.png"):
        V.validate_plain(kern, items, "ms-ssim", 2.40, batch=2, device=DEV)


# --------------------------------------------------------------------------- #
# --adv test_epoch against the oracle's attack
# --------------------------------------------------------------------------- #
def _net(model, P, quality=1):
    from imagecompression_adversarial_amd import codec
    net = codec.bmshj2018_hyperprior(quality) if model == "hyper" else codec.bmshj2018_factorized(quality)
    sd = net.state_dict()
    sd.update({k: v.reshape(sd[k].shape) for k, v in P.items() if k in sd})
    net.load_state_dict(sd)
    return net.to(DEV)


_ADV_REF = {}


def adv_ref():
    if not _ADV_REF:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        P, x = VR.adv_params(1), RD.image(VR.ADV_SHAPE, VR.ADV_SEED)
        _ADV_REF.update(P=P, x=x, vi=VR.adv_vi(P, x, VR.ADV_STEPS, dtype=F64))
    return _ADV_REF


def adv_args(precision, **kw):
    return SimpleNamespace(adv=True, steps=VR.ADV_STEPS, epsilon=16.0, noise=0.0123, lr_attack=0.01, att_metric="L2",
                           clamp=True, precision=precision, device="cuda:0", val_batch=2, metric="mse", **kw)


@pytest.mark.parametrize("precision", ["x6", "fp32"])
@pytest.mark.parametrize("training", [True, False])
def test_adv_test_epoch_vs_oracle(V, tmp_path, capsys, precision, training):
    ref = adv_ref()
    net = _net("hyper", ref["P"]).train(training)
    items = [(f"image_{b}", ref["x"][b:b + 1], 64, 64) for b in range(2)]
    args = adv_args(precision)
    log = str(tmp_path / "ckpt" / "log.txt")
    r = V.test_epoch(4, items, net, args, 0.0018, log)
    vis = [row["vi"] for row in r.rows]
    print(f"vi {vis} oracle {ref['vi']} bound {VR.VI_TOL:.2e}")
    assert all(v is not None for v in ref["vi"])
    for v, w in zip(vis, ref["vi"]):
        assert abs(v - w) <= VR.VI_TOL, (v, w)
    assert r.loss == VR.mean64(vis) and (r.count, r.skipped, r.adv) == (2, 0, True)
    assert args.noise == 0.0123                                               # never touched
    assert all(p.requires_grad for p in net.parameters())
    assert net.training is training
    assert open(log).read() == VR.log_line(4, 0, 0, 0)[:-1] + f" |\tVI: {r.loss:.4f}\n"
    assert f"Test Loss (VI): {r.loss:.4f}" in capsys.readouterr().out


def test_adv_test_epoch_skips_an_undefined_vi(V, tmp_path, monkeypatch):
    """An image that comes back from the attack equal to its own target has mse_in = 0 and no VI: it is left out and
    counted, and the mean is that of the others.  The stub hands image 1 back unchanged through the real evaluation."""
    from imagecompression_adversarial_amd import attack as A
    ref = adv_ref()
    net = _net("hyper", ref["P"]).eval()
    x3 = torch.cat([ref["x"][:1], ref["x"][:1], ref["x"][1:]], 0)
    items = [(f"image_{b}", x3[b:b + 1], 64, 64) for b in range(3)]
    real = A.attack_batch

    def stub(kern, im_s, **kw):
        res = real(kern, im_s, **kw)
        if im_s.shape[0] == 3:
            loop = A.AttackLoop(kern, im_s, steps=0, noise_thr=kw["noise_thr"])
            im_in = res.im_adv.clone()
            im_in[1] = im_s[1]                                                 # the planted image: its own target
            ev = A.evaluate(kern, im_in, loop.im_s, loop.output_s, True, msssim=False)
            res.vi = ev[7]
        return res

    monkeypatch.setattr(V, "attack_batch", stub)
    args = adv_args("x6")
    args.val_batch = 3
    r = V.test_epoch(0, items, net, args, 0.0018, str(tmp_path / "log.txt"))
    vis = [row["vi"] for row in r.rows]
    assert vis[1] is None and vis[0] is not None and vis[2] is not None
    assert (r.count, r.skipped) == (2, 1) and r.loss == VR.mean64([vis[0], vis[2]])
    monkeypatch.setattr(V, "attack_batch", real)
    plain = V.test_epoch(0, [items[0], items[2]], net, args, 0.0018, None)
    assert plain.loss == r.loss and plain.skipped == 0                         # the skipped image changed nothing
    # every image undefined: raises
    monkeypatch.setattr(V, "attack_batch", lambda kern, im_s, **kw: SimpleNamespace(vi=[None] * im_s.shape[0]))
    with pytest.raises(RuntimeError, match="skipped"):
        V.test_epoch(0, items, net, args, 0.0018, None)
    assert all(p.requires_grad for p in net.parameters()) and not net.training


# --------------------------------------------------------------------------- #
# rd_step
# --------------------------------------------------------------------------- #
def test_rd_step_is_adv_steps_second_half_and_the_oracles_train_step():
    from imagecompression_adversarial_amd import coder
    from imagecompression_adversarial_amd.train import adv_step, rd_step
    from imagecompression_adversarial_amd.train_engine import RDTrainer
    q, B, H, W, lr_train, lmbda = 1, 2, 64, 64, 1e-4, 0.0018
    P = VR.plain_params("hyper", q)
    N, M = oc.model_channels("hyper", q)
    x = R.rnd((B, 3, H, W), 41)
    ny = R.rnd((B, M, H // 16, W // 16), 42) - 0.5
    nz = R.rnd((B, N, H // 64, W // 64), 43) - 0.5
    qn = (ny.to(DEV), nz.to(DEV))

    def fresh():
        net = _net("hyper", P, q).train()
        opt, aux = coder.configure_optimizers(net, SimpleNamespace(adv=True, lr_train=lr_train))
        return net, RDTrainer(net, "mse", lmbda), opt, aux

    # adv_step after a 1-step inner attack, and rd_step on the batch that attack produced
    net_a, tr_a, opt_a, aux_a = fresh()
    args = SimpleNamespace(steps=1, epsilon=16.0, noise=1e-4, lr_attack=0.01, att_metric="L2", clamp=True,
                           round_adv=False)
    out_a, batch = adv_step(net_a, tr_a, opt_a, aux_a, x.to(DEV), args, qnoise=qn)
    net_r, tr_r, opt_r, aux_r = fresh()
    out_r = rd_step(net_r, tr_r, opt_r, aux_r, batch, None, 1, qn)
    for k in ("loss", "bpp_loss", "distortion_loss", "grad_norm", "aux_loss"):
        assert torch.equal(torch.as_tensor(out_a[k]), torch.as_tensor(out_r[k])), k
    for (k, a), (_, b) in zip(net_a.named_parameters(), net_r.named_parameters()):
        assert torch.equal(a, b), k
    assert net_r.training
    # one plain step on the clean batch against the oracle's train step: with epsilon 0 its inner attack returns
    # clamp(x + 0, 0, 1) = x, and what remains is train.py:367-400
    net_p, tr_p, opt_p, aux_p = fresh()
    out = rd_step(net_p, tr_p, opt_p, aux_p, x.to(DEV), None, 1, qn)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    Pn, ref_out, ref_aux, ref_adv = oa.adv_train_step(P, x, steps=1, epsilon=0.0, metric="mse", lmbda=lmbda, lr_train=lr_train,
                                                      noise_y=ny, noise_z=nz)
    assert torch.equal(ref_adv, x)
    for k in ("loss", "bpp_loss", "distortion_loss"):
        assert abs(float(out[k]) - ref_out[k]) <= 1e-4 * max(abs(ref_out[k]), 1.0), k
    assert abs(float(out["aux_loss"]) - ref_aux) <= 1e-4 * max(abs(ref_aux), 1.0)
    named = dict(net_p.named_parameters())
    worst = []
    for k, v in Pn.items():
        step = lr_train if not k.endswith(".quantiles") else 1e-3
        d = (named[k].detach().cpu().reshape(v.shape) - v).abs() / step
        worst.append((float(d.max()), float(torch.quantile(d.flatten().double(), 0.999)) if d.numel() > 1 else 0.0, k))
    worst.sort(reverse=True)
    assert worst[0][0] <= 2.0, worst[:3]
    assert max(w[1] for w in worst) <= 1e-2, sorted(worst, key=lambda w: -w[1])[:3]


# --------------------------------------------------------------------------- #
# The CLI end to end
# --------------------------------------------------------------------------- #
def run_train(argv):
    from imagecompression_adversarial_amd import train
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = train.train(train.config().parse_args(list(argv)))
    return out, buf.getvalue()


@pytest.fixture
def moving_latents(monkeypatch):
    """The plain synthetic weights round every latent to 0 (|y| < 0.2), so the reconstruction does not move under an
    attack and every VI is undefined, which validation refuses.  g_a's last layer is scaled by 40, as
    tests/test_gpu_rd_eval.py scales it, inside --synthetic-weights."""
    from imagecompression_adversarial_amd import coder
    real = coder._synthetic_init

    def init(net, seed=0):
        real(net, seed)
        with torch.no_grad():
            for k in ("g_a.6.weight", "g_a.6.bias"):
                net.get_parameter(k).mul_(RD.LATENT_GAIN)

    monkeypatch.setattr(coder, "_synthetic_init", init)


CLI = ["-m", "hyper", "-q", "1", "-metric", "mse", "-steps", "2", "-train_steps", "21", "-s", "synthetic:2x64x64",
       "-val", "synthetic:2x64x64", "--val-every", "10", "--synthetic-weights"]


def test_cli_adv_validates_steps_the_scheduler_and_resumes(tmp_path, moving_latents):
    d = str(tmp_path / "tmp")
    out, text = run_train(["--adv"] + CLI + ["--ckpt-dir", d])
    assert [s for s, _ in out["validations"]] == [10, 20]
    losses = [v for _, v in out["validations"]]
    assert out["best"] == min(losses)
    assert text.count("Test Loss (VI):") == 2 and text.count("New Best:") == 2
    lines = open(os.path.join(d, "log.txt")).read().splitlines()
    assert len(lines) == 2 and all(ln.startswith("Test epoch 0: Average losses:\tLoss: 0.0000 |") for ln in lines)
    assert [ln.rsplit("VI: ", 1)[1] for ln in lines] == [f"{v:.4f}" for v in losses]
    best = torch.load(os.path.join(d, "best_loss.pth.tar"), weights_only=True)
    assert set(best) == {"epoch", "step", "state_dict", "loss", "optimizer", "aux_optimizer", "lr_scheduler", "best"}
    k_best = losses.index(min(losses))
    assert best["step"] == (10, 20)[k_best] and best["loss"] == best["best"] == min(losses)
    assert os.path.exists(os.path.join(d, "ckpt-0-10.pth.tar"))               # the first validation is always a best
    last = torch.load(os.path.join(d, f"ckpt-0-{best['step']}.pth.tar"), weights_only=True)
    assert last["lr_scheduler"]["last_epoch"] == k_best + 1
    if os.path.exists(os.path.join(d, "ckpt-0-20.pth.tar")):
        assert torch.load(os.path.join(d, "ckpt-0-20.pth.tar"), weights_only=True)["lr_scheduler"]["last_epoch"] == 2
    # resume: the same best, epoch + 1, no validation in a 1-step run
    d2 = str(tmp_path / "resumed")
    argv = ["--adv"] + CLI + ["--ckpt-dir", d2, "-ckpt", os.path.join(d, "best_loss.pth.tar")]
    argv[argv.index("-train_steps") + 1] = "1"
    out2, _ = run_train(argv)
    assert out2["best"] == best["best"] and out2["validations"] == []


def test_cli_plain_training_validates_and_completes(tmp_path):
    d = str(tmp_path / "tmp")
    out, text = run_train(CLI + ["--ckpt-dir", d])
    assert [s for s, _ in out["validations"]] == [10, 20]                     # step 20 is also the last step
    lines = open(os.path.join(d, "log.txt")).read().splitlines()
    assert len(lines) == 2 and "VI:" not in lines[0] and lines[0].endswith("Recomp loss: 0.000")
    assert text.count("Test epoch 0: Average losses:") == 2
    best = torch.load(os.path.join(d, "best_loss.pth.tar"), weights_only=True)
    assert best["best"] == out["best"] == min(v for _, v in out["validations"])
    assert torch.isfinite(torch.as_tensor(out["loss"]))
