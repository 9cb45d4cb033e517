"""The RD evaluation (batch_test, the reference's test.py) on the GPU: the ica_rd_metrics kernel against float64,
rd_eval_batch / rd_eval_defended against the oracle composition, --real-bpp against net.compress(), and the CLI.

Kernel bounds: tests/rd_eval_restatement.py KERNEL_TOL (4 max(e_ref, 2^-24) rounded up, e_ref the fp32 CPU
restatement's own distance from float64; tests/test_cpu_rd_eval.py prints the table), rel_err = max |a - b| / max |b|;
nclamp and the clamped image are compared bit for bit.  Composition: FORWARD_TOL of the same file (the eval forward's
bpp / mse bounds of tests/test_gpu_defend.py and what follows from them through the logarithms, derived there); the
seeds are ones for which the fp32 CPU oracle itself agrees with float64 (checked in tests/test_cpu_rd_eval.py).
"""
import contextlib
import io

import pytest
import torch

from tests import loss_refs as R
from tests import rd_eval_restatement as RD

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def K():
    from imagecompression_adversarial_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def RE():
    from imagecompression_adversarial_amd import rd_eval
    return rd_eval


_KERN = {}


def kernels(model, precision="fp32"):
    """One executor per (model, precision), and the CPU parameters it was built from."""
    from imagecompression_adversarial_amd.engine import CodecKernels
    from imagecompression_adversarial_amd.engine_cheng import ChengKernels
    if (model, precision) not in _KERN:
        P = RD.params(model)
        sd = {k: v.to(DEV) for k, v in P.items()}
        kern = ChengKernels(sd, precision=precision) if model == "cheng2020" else CodecKernels(sd, model, precision)
        _KERN[(model, precision)] = (P, kern)
    return _KERN[(model, precision)]


def nc4_dirty(K, x):
    """to_nc4 with the padding lanes (c >= C) filled with 1e-30: a kernel that reads them shows it in a sum, in the
    census (a likelihood below 2^-16) and in the squared error."""
    x4 = K.to_nc4(x.to(DEV))
    C = x.shape[1]
    if C % 4:
        x4[:, -1, :, :, C % 4:] = 1e-30
    return x4


def launch(K, c):
    ys, zs = c["lik_y"], c["lik_z"]
    return K.rd_metrics(nc4_dirty(K, c["x_hat"]), c["target"].to(DEV), nc4_dirty(K, ys), ys.shape[1],
                        None if zs is None else nc4_dirty(K, zs), 0 if zs is None else zs.shape[1])


# --------------------------------------------------------------------------- #
# Kernel
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", RD.KERNEL_CASES, ids=RD.case_key)
def test_rd_metrics_vs_float64(K, case):
    c = RD.kernel_case(case)
    tol = RD.KERNEL_TOL[RD.case_key(case)]
    sse64, lny64, lnz64, n64, out64 = RD.kernel_ref(c["x_hat"], c["target"], c["lik_y"], c["lik_z"], F64)
    got = launch(K, c)
    again = launch(K, c)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                  # two launches, identical bits
    sse, lny, lnz, nclamp, out = (t.cpu() for t in got)
    assert nclamp.dtype == torch.int32 and torch.equal(nclamp.long(), n64)     # the census, exactly
    assert torch.equal(out.double(), out64)                                    # clamp is exact
    if c["lik_z"] is None:
        assert not bool(lnz.any())
    e = RD.kernel_errors((sse, lny, lnz), (sse64, lny64, lnz64))
    for k, v in e.items():
        print(f"rd_metrics {RD.case_key(case)} {k} {v:.2e} bound {tol[k]:.0e}")
    for k, v in e.items():
        assert v <= tol[k], (case, k, v, tol[k])
    # an image's numbers are the same bits alone and in the batch
    b = case[0][0] - 1
    one = launch(K, {k: (v if v is None else v[b:b + 1]) for k, v in c.items()})
    for a, full in zip(one, got):
        assert torch.equal(a, full[b:b + 1])


def test_rd_metrics_refuses_bad_arguments(K):
    c = RD.kernel_case(RD.KERNEL_CASES[1])
    xh4, tg = K.to_nc4(c["x_hat"].to(DEV)), c["target"].to(DEV)
    y4, z4 = K.to_nc4(c["lik_y"].to(DEV)), K.to_nc4(c["lik_z"].to(DEV))
    Cy, Cz = c["lik_y"].shape[1], c["lik_z"].shape[1]
    K.rd_metrics(xh4, tg, y4, Cy, z4, Cz)                                      # the arguments as they should be
    bad = [
        lambda: K.rd_metrics(xh4, tg, y4, 12, z4, Cz),                         # channel count and tensor disagree
        lambda: K.rd_metrics(xh4, tg, y4, Cy, z4, Cz + 8),
        lambda: K.rd_metrics(xh4, tg, y4[:1].contiguous(), Cy, z4, Cz),        # batch mismatch
        lambda: K.rd_metrics(xh4, tg, y4, Cy, z4[:1].contiguous(), Cz),
        lambda: K.rd_metrics(xh4[:1].contiguous(), tg, y4, Cy, z4, Cz),
        lambda: K.rd_metrics(xh4, tg, None, Cy, z4, Cz),                       # missing required tensors
        lambda: K.rd_metrics(None, tg, y4, Cy, z4, Cz),
        lambda: K.rd_metrics(xh4, None, y4, Cy, z4, Cz),
        lambda: K.rd_metrics(xh4, tg, y4, Cy, None, Cz),                       # z channels without a z plane
        lambda: K.rd_metrics(xh4, tg.double(), y4, Cy, z4, Cz),
        lambda: K.rd_metrics(xh4, tg.cpu(), y4, Cy, z4, Cz),
        lambda: K.rd_metrics(xh4[..., :3], tg, y4, Cy, z4, Cz),                # not an nChw4c reconstruction
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()


def test_rd_metrics_c_entry_returns_a_status(K):
    """The C entry itself refuses null required pointers and shapes it does not take: a status, no launch."""
    from imagecompression_adversarial_amd._lib import lib, ptr, stream
    c = RD.kernel_case(RD.KERNEL_CASES[1])
    xh4, tg = K.to_nc4(c["x_hat"].to(DEV)), c["target"].to(DEV)
    y4 = K.to_nc4(c["lik_y"].to(DEV))
    out, part = torch.empty_like(tg), torch.empty(2 * 3 * int(lib().ica_rd_metrics_blocks()), device=DEV)
    n = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    f = lib().ica_rd_metrics
    ok = (ptr(xh4), ptr(tg), ptr(y4), None, ptr(out), ptr(part), ptr(n), 2, 16, 16, 6, 5, 3, 0, 0, 0)
    for i in (0, 1, 2, 4, 5, 6):
        a = list(ok)
        a[i] = None
        assert f(*a, stream()) == -5, i
    for i, v in ((7, 0), (7, 70000), (8, 0), (10, 0), (13, 8)):
        a = list(ok)
        a[i] = v
        assert f(*a, stream()) == -5, i
    a = list(ok)
    a[4] = ptr(tg)                                                             # the output on top of an input
    assert f(*a, stream()) == -7
    torch.cuda.synchronize()
    assert n.tolist() == [-7, -7]                                              # nothing ran
    assert f(*ok, stream()) == 0


# --------------------------------------------------------------------------- #
# rd_eval_batch against the oracle composition
# --------------------------------------------------------------------------- #
_REF = {}


def plain_ref(model, shape, seed):
    if (model, shape, seed) not in _REF:
        _REF[(model, shape, seed)] = RD.plain(RD.params(model), RD.image(shape, seed), model, F64)
    return _REF[(model, shape, seed)]


def check_forward(res, ref, what):
    e = RD.forward_errors(res, ref)
    print(f"{what}: " + " ".join(f"{k} {v:.2e} (bound {RD.FORWARD_TOL[k]:.1e})" for k, v in e.items())
          + f"; bpp {res.bpp.tolist()} psnr {res.psnr.tolist()} nclamp {res.nclamp.tolist()}")
    for k, v in e.items():
        assert v <= RD.FORWARD_TOL[k], (what, k, v)
    assert float((res.x_hat.cpu().double() - ref["x_hat"]).abs().max()) < 1e-3
    assert torch.allclose(res.bpp, res.bpp_y + res.bpp_z, rtol=1e-6, atol=0)
    # the census counts likelihoods below 2^-16; one within fp32 rounding of the bound may fall on the other side
    n_ref = ref["nclamp"]
    assert bool(((res.nclamp.long() - n_ref).abs() <= 1 + n_ref // 100).all()), (res.nclamp, n_ref)


# hyper and factorized on fp32 and x6 operands; the context models once, on x6 (the CLI's default engine)
FORWARD_RUNS = [(m, s, seed, p) for m, s, seed in RD.FORWARD_CASES
                for p in (("fp32", "x6") if m in ("hyper", "factorized") else ("x6",))]


@pytest.mark.parametrize("model,shape,seed,precision", FORWARD_RUNS,
                         ids=lambda v: RD.case_key((v,)) if isinstance(v, tuple) else str(v))
def test_rd_eval_batch_vs_oracle(RE, model, shape, seed, precision):
    _, kern = kernels(model, precision)
    ref = plain_ref(model, shape, seed)
    x = RD.image(shape, seed).to(DEV)
    res = RE.rd_eval_batch(kern, x)
    check_forward(res, ref, f"rd_eval_batch {model} {RD.case_key((shape,))} {precision}")
    assert bool(res.msim.isnan().all()) and bool(res.msim_dB.isnan().all())   # min(H, W) <= 160
    assert res.psnr.dtype == F64 and res.real_bpp is None
    if model == "factorized":
        assert not bool(res.bpp_z.any())
    # an image alone gives the bits it has in the batch
    one = RE.rd_eval_batch(kern, x[-1:].contiguous())
    for k in ("bpp", "mse", "psnr"):
        assert torch.equal(getattr(one, k), getattr(res, k)[-1:]), k


def test_rd_eval_batch_msssim(RE):
    """The smallest size pytorch_msssim takes: msim within 1e-5, msim_dB within the bound derived from it."""
    model, shape, seed = RD.MSIM_CASE
    _, kern = kernels(model, "x6")
    ref = plain_ref(model, shape, seed)
    res = RE.rd_eval_batch(kern, RD.image(shape, seed).to(DEV))
    check_forward(res, ref, "rd_eval_batch msssim")
    d = float((res.msim.double() - ref["msim"]).abs().max())
    d_db = float((res.msim_dB - ref["msim_dB"]).abs().max())
    bound = RD.msim_db_bound(float(ref["msim"].max()))
    print(f"msim {res.msim.tolist()} d {d:.2e} msim_dB {res.msim_dB.tolist()} d {d_db:.2e} bound {bound:.2e}")
    assert d <= RD.FORWARD_TOL["msim"] and d_db <= bound


def test_rd_eval_batch_bf16_engine(RE):
    """The bf16 engine: x_hat goes through cast_nc4; the loss side is the fp32 kernel on whatever the forward gave, so
    the result equals the restatement applied to this engine's own tensors."""
    _, kern = kernels("hyper", "bf16")
    from imagecompression_adversarial_amd import hip_ops as K
    x = RD.image((2, 3, 64, 64), 71).to(DEV)
    res = RE.rd_eval_batch(kern, x)
    fw = kern.forward(K.to_nc4(x))
    out = {"x_hat": K.from_nc4(K.cast_nc4(fw["x_hat4"], F32), 3).cpu().double(),
           "likelihoods": {"y": K.from_nc4(fw["lik4"]["y"], kern.M).cpu().double(),
                           "z": K.from_nc4(fw["lik4"]["z"], kern.N).cpu().double()}}
    ref = RD.metrics(out, x.cpu().double())
    assert torch.equal(res.nclamp.long(), ref["nclamp"])
    assert torch.allclose(res.bpp.double(), ref["bpp"], rtol=1e-6, atol=0)
    assert torch.allclose(res.mse.double(), ref["mse"], rtol=1e-6, atol=0)


def test_rd_eval_batch_debug_model(RE):
    from oracle import codec
    from imagecompression_adversarial_amd.engine_debug import DebugKernels
    P = codec.perturb_params(codec.init_params("debug", 1, seed=0), seed=1)
    kern = DebugKernels({k: v.to(DEV) for k, v in P.items()})
    x = RD.image((2, 3, 64, 64), 81)
    ref, m32 = RD.plain(P, x, "debug", F64), RD.plain(P, x, "debug", F32)
    for k, v in RD.forward_errors(m32, ref).items():
        assert v <= RD.FORWARD_TOL[k]                                          # the case's condition, on the CPU
    check_forward(RE.rd_eval_batch(kern, x.to(DEV)), ref, "rd_eval_batch debug")


# --------------------------------------------------------------------------- #
# Defended evaluation (test.py:37-49)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("method", ["ensemble", "bitdepth", "resize", "range"])
def test_rd_eval_defended_vs_oracle(RE, method):
    from imagecompression_adversarial_amd import self_ensemble as SE
    from imagecompression_adversarial_amd.latent_range import RangeProfile
    shape, seed = RD.DEFEND_CASES[method]
    P, kern = kernels("hyper", "fp32")
    x = RD.image(shape, seed)
    pre = prof = gprof = None
    if method in ("bitdepth", "resize"):
        # resize: its ~1e-7 differences from torch's (checked to 2e-6, tests/test_gpu_defend.py) would flip isolated
        # round(y), so the codec part is compared on the GPU's preprocessed image
        pre = SE.defend(kern, x.to(DEV), method).cpu()
        cpu = RD.odef.bitdepth_reduction(x) if method == "bitdepth" else RD.odef.random_resize(x, 243 / 256)
        assert float((pre - cpu).abs().max()) < 2e-6
    if method == "range":
        prof = RD.range_profile(P, x)
        gprof = RangeProfile(*prof, device=DEV)
    ref = RD.defended(P, x, method, "hyper", F64, pre=pre, profile=prof)
    res = RE.rd_eval_defended(kern, x.to(DEV), method, profile=gprof)
    check_forward(res, ref, f"rd_eval_defended {method}")
    if method == "ensemble":
        assert res.best_idx == ref["best_idx"]
    # scored against the ORIGINAL image: the clamped reconstruction's mse against x is the reported one
    direct = ((res.x_hat.cpu().double() - x.double()) ** 2).flatten(1).mean(1)
    assert torch.allclose(res.mse.double(), direct, rtol=1e-5, atol=0)
    plain = RE.rd_eval_batch(kern, x.to(DEV))
    assert not torch.equal(plain.bpp, res.bpp) or method == "ensemble" and res.best_idx == [0]


def test_rd_eval_defended_refusals(RE):
    _, kern = kernels("hyper", "fp32")
    x = RD.image((1, 3, 64, 64), 5).to(DEV)
    with pytest.raises(RuntimeError):
        RE.rd_eval_defended(kern, x, "resize")         # 64 -> 60 -> 63: the reference's mse fails the same way
    with pytest.raises(ValueError):
        RE.rd_eval_defended(kern, x, "range")          # no profile
    with pytest.raises(ValueError):
        RE.rd_eval_defended(kern, x, "clip")


# --------------------------------------------------------------------------- #
# --real-bpp and the CLI
# --------------------------------------------------------------------------- #
def run_cli(argv):
    from imagecompression_adversarial_amd import batch_test
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = batch_test.main(list(argv))
    return out, buf.getvalue()


def test_real_bpp_is_the_models_compress(RE):
    from imagecompression_adversarial_amd import batch_test, coder
    args = batch_test.config().parse_args(["-m", "hyper", "-q", "1", "-metric", "mse", "--synthetic-weights"])
    with contextlib.redirect_stdout(io.StringIO()):
        net = coder.load_model(args, training=False).to(DEV)
    with torch.no_grad():
        for k in ("g_a.6.weight", "g_a.6.bias"):
            net.get_parameter(k).mul_(RD.LATENT_GAIN)
    x = RD.image((2, 3, 64, 128), 91).to(DEV)
    res = RE.rd_eval_batch(net.kernels("x6"), x, real_bpp_net=net)
    net.update()
    strings = net.compress(x)["strings"]
    want = [8.0 * sum(len(s[b]) for s in strings) / (64 * 128) for b in range(2)]
    assert res.real_bpp.tolist() == want and min(want) > 0
    no = RE.rd_eval_batch(net.kernels("x6"), x)
    assert no.real_bpp is None and torch.equal(no.bpp, res.bpp)               # never mixed into the estimate
    print(f"real bpp {want} estimated {res.bpp.tolist()}")


def test_cli_avg_line_is_the_mean_of_the_per_image_values():
    out, text = run_cli(["-m", "hyper", "-q", "1", "-s", "synthetic:3x64x64", "--synthetic-weights", "--table"])
    lines = text.splitlines()
    assert "[Evaluate RD]: synthetic:3x64x64" in lines
    avg = [ln for ln in lines if ln.startswith("AVG:")]
    assert len(avg) == 1
    nums = [float(v) for v in avg[0].split()[1:]]
    rows = out["results"]
    assert len(nums) == 4 and len(rows) == 3 and [r["name"] for r in rows] == [f"synthetic_{i}" for i in range(3)]
    for v, k in zip(nums, ("bpp", "psnr", "msim", "msim_dB")):
        mean = sum(r[k] for r in rows) / 3
        assert v == mean or (v != v and mean != mean), (k, v, mean)           # nan msim at 64 x 64
        assert out[k] == mean or (out[k] != out[k] and mean != mean)
    assert nums[0] > 0 and nums[1] > 0
    table = [ln for ln in lines if ln.startswith("synthetic_")]
    assert len(table) == 3 and all(len(ln.split()) == 6 for ln in table)       # name, 4 metrics, nclamp
    assert [int(ln.split()[5]) for ln in table] == [r["nclamp"] for r in rows]


def test_cli_two_sizes_come_back_in_input_order(tmp_path):
    from imagecompression_adversarial_amd import batch_test, coder
    sizes = [(64, 64), (50, 120), (64, 64), (64, 100)]                         # padded: 64x64, 64x128, 64x64, 64x128
    for i, (h, w) in enumerate(sizes):
        coder.write_image(RD.image((1, 3, h, w), 100 + i), str(tmp_path / f"im{i}.png"))
    argv = ["-m", "hyper", "-q", "1", "-metric", "mse", "--synthetic-weights", "-s", str(tmp_path / "im*.png")]
    out, text = run_cli(argv + ["--batch", "2", "--debug"])
    names = [r["name"] for r in out["results"]]
    assert names == [str(tmp_path / f"im{i}.png") for i in range(4)]
    printed = [ln.split()[0] for ln in text.splitlines() if ln.startswith(str(tmp_path))]
    assert printed == names
    one, _ = run_cli(argv)                                                     # one image per launch: the same bits
    for a, b in zip(out["results"], one["results"]):
        assert a["name"] == b["name"] and a["bpp"] == b["bpp"] and a["psnr"] == b["psnr"]
    # (with the plain synthetic weights every latent rounds to 0 and the bpp is a constant of the weights: the
    # distortion is what tells two images of one size apart)
    assert out["results"][0]["psnr"] != out["results"][2]["psnr"]
    assert len({r["psnr"] for r in out["results"]}) == 4
