"""GPU tests of the perturbation-transfer study (ica_transfer.hip, transfer, the transfer_noise CLI) against the
restatement tests/transfer_restatement.py.

Stated tolerances.  im_in is one correctly rounded add and a clamp per element: bit-equal to torch's.  The two means
are sums of non-negative fp32 terms: 1e-5 relative of float64 over the same operands (MEAN_TOL of
tests/test_gpu_degrade.py).  A pair's numbers are bit-equal run to run, alone (N = 1 or M = 1) and inside a block of
pairs.  transfer_matrix against the per-pair path of the same engine (degrade.apply_noise, eval_forward on
[im; im_in], hip_ops.sqdiff_mean) with the restatement's float64 metrics: 5e-3 dB, the eval-metric tolerance of
tests/test_gpu_degrade.py, for pairs with mse_out > 1e-7."""
import math

import pytest
import torch

from tests import transfer_restatement as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(1, 1, 8, 8), (3, 2, 72, 136), (5, 3, 64, 192)]   # one block; tile remainders 3 and 5 = 4 + 1; > 1 block
MEAN_TOL = 1e-5


@pytest.fixture(scope="module")
def T():
    from imagecompression_adversarial_amd import transfer
    return transfer


def rel(got, ref):
    return abs(got - ref) / ref


def ids(s):
    return "%dx%dx%dx%d" % s


# --------------------------------------------------------------------------- #
# apply_pairs
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_apply_pairs(T, shape):
    N, M, H, W = shape
    im = R.rand_image((M, 3, H, W), 50 + H)
    g = torch.Generator().manual_seed(51 + W)
    noise = torch.randn((N, 3, H, W), generator=g) * 0.2           # large enough to clamp on both sides
    imd, nd = im.to(DEV), noise.to(DEV)
    im_in, mse_in = T.apply_pairs(imd, nd)
    want, m64 = R.pair_inputs(im, noise)
    assert float(want.min()) == 0 and float(want.max()) == 1       # the clamp acts on both sides
    assert im_in.shape == (N * M, 3, H, W) and mse_in.shape == (N, M)
    got = im_in.cpu()
    for i in range(N):
        for j in range(M):
            assert torch.equal(got[i * M + j], want[i * M + j]), (i, j)
            print(shape, i, j, float(mse_in[i, j]), m64[i][j])
            assert rel(float(mse_in[i, j]), m64[i][j]) < MEAN_TOL
    again = T.apply_pairs(imd, nd)
    assert torch.equal(again[0], im_in) and torch.equal(again[1], mse_in)
    for i in range(N):                                             # a row alone
        one_in, one = T.apply_pairs(imd, nd[i:i + 1])
        assert torch.equal(one[0], mse_in[i]) and torch.equal(one_in, im_in[i * M:(i + 1) * M]), i
    for j in range(M):                                             # a column alone
        one_in, one = T.apply_pairs(imd[j:j + 1], nd)
        assert torch.equal(one[:, 0], mse_in[:, j]) and torch.equal(one_in, im_in[j::M]), j
    # the same chain as the per-image kernel: a pair alone is ica_noise_apply's number
    from imagecompression_adversarial_amd import degrade
    _, _, single = degrade.apply_noise(imd[:1], nd[:1])
    assert torch.equal(single[0], mse_in[0, 0])
    nz = nd.clone()
    nz[N - 1] = 0
    zin, zero = T.apply_pairs(imd, nz)
    assert bool((zero[N - 1] == 0).all()) and torch.equal(zin[(N - 1) * M:], imd)
    assert torch.equal(zero[:N - 1], mse_in[:N - 1])


# --------------------------------------------------------------------------- #
# score_pairs
# --------------------------------------------------------------------------- #
def nc4_rand(B, H, W, seed):
    x = R.rand_image((B, 1, H, W, 4), seed, -0.5, 1.5)
    x[..., 3] = float("nan")                                        # the padding lane must never enter a sum
    return x


def score64(x_hat4, x_s4, N, M, clamp):
    nchw = lambda t: t[:, 0, :, :, :3].permute(0, 3, 1, 2)
    return R.pair_outputs(nchw(x_hat4), nchw(x_s4), N, M, clamp)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_score_pairs(T, shape):
    N, M, H, W = shape
    x_hat4, x_s4 = nc4_rand(N * M, H, W, 60 + H), nc4_rand(M, H, W, 61 + W)
    xd, sd = x_hat4.to(DEV), x_s4.to(DEV)
    got = {c: T.score_pairs(xd, sd, N, M, clamp=c) for c in (True, False)}
    assert torch.equal(T.score_pairs(xd, sd, N, M), got[True])      # clamp is on by default
    for c in (True, False):
        ref = score64(x_hat4, x_s4, N, M, c)
        assert got[c].shape == (N, M) and bool(torch.isfinite(got[c]).all())
        for i in range(N):
            for j in range(M):
                print(shape, "clamp" if c else "plain", i, j, float(got[c][i, j]), ref[i][j])
                assert rel(float(got[c][i, j]), ref[i][j]) < MEAN_TOL
    assert bool((got[False] > got[True] * 1.05).all())              # uniform on [-0.5, 1.5]: clamping removes > 5 %
    for c in (True, False):
        assert torch.equal(T.score_pairs(xd, sd, N, M, clamp=c), got[c])
        for i in range(N):
            one = T.score_pairs(xd[i * M:(i + 1) * M], sd, 1, M, clamp=c)
            assert torch.equal(one[0], got[c][i]), (c, i)
        for j in range(M):
            one = T.score_pairs(xd[j::M].contiguous(), sd[j:j + 1], N, 1, clamp=c)
            assert torch.equal(one[:, 0], got[c][:, j]), (c, j)
        same = T.score_pairs(sd.repeat(N, 1, 1, 1, 1), sd, N, M, clamp=c)
        assert bool((same == 0).all())


# --------------------------------------------------------------------------- #
# rejections
# --------------------------------------------------------------------------- #
def test_rejected_arguments(T):
    import ctypes as C
    from imagecompression_adversarial_amd._lib import lib, ptr, stream
    z = lambda *s: torch.zeros(s, device=DEV)
    with pytest.raises(ValueError):
        T.apply_pairs(z(1, 3, 8, 6), z(1, 3, 8, 6))                 # W % 4
    with pytest.raises(ValueError):
        T.apply_pairs(z(1, 3, 8, 8), z(1, 3, 8, 12))                # sizes differ
    with pytest.raises(ValueError):
        T.apply_pairs(z(1, 3, 8, 8), z(1, 4, 8, 8))
    with pytest.raises(ValueError):
        T.score_pairs(z(3, 1, 8, 8, 4), z(2, 1, 8, 8, 4), 2, 2)     # 3 images are not 2 x 2 pairs
    with pytest.raises(ValueError):
        T.score_pairs(z(4, 1, 8, 8, 4), z(2, 1, 8, 4, 4), 2, 2)
    with pytest.raises(ValueError):
        T.score_pairs(z(4, 1, 8, 8, 4), z(2, 1, 8, 8, 4), 4, 1)     # M is not the number of targets
    with pytest.raises(ValueError):
        T.transfer_matrix(None, z(1, 3, 64, 64), z(1, 3, 64, 128))

    L = lib()
    im, noise, out = z(2, 3, 8, 8), z(2, 3, 8, 8), z(4, 3, 8, 8)
    mse, ws = z(2, 2), z(64)
    off = lambda t: C.c_void_p(t.data_ptr() + 4)
    apply = lambda a, b, o, N=2, M=2, H=8, W=8, m=mse, w=ws: L.ica_transfer_apply(
        a if isinstance(a, C.c_void_p) or a is None else ptr(a), b if isinstance(b, C.c_void_p) or b is None else ptr(b),
        o if isinstance(o, C.c_void_p) or o is None else ptr(o), N, M, H, W, ptr(m), ptr(w), stream())
    assert apply(im, noise, out) == 0
    assert apply(im, noise, im, N=1, M=1) == -7 and apply(im, noise, noise, N=1, M=1) == -7     # in place
    big = z(5, 3, 8, 8)
    assert apply(big[3:], noise, big[:4]) == -7 and apply(im, big[3:], big[:4]) == -7          # partial overlap
    assert apply(big[4:], noise, big[:4], M=1) == 0                                             # adjacent is fine
    assert apply(None, noise, out) == -5 and apply(im, None, out) == -5 and apply(im, noise, None) == -5
    assert apply(im, noise, out, m=None) == -5 and apply(im, noise, out, w=None) == -5
    assert apply(off(im), noise, out, M=1) == -5 and apply(im, off(noise), out, N=1) == -5
    assert apply(im, noise, off(out), N=1) == -5
    for kw in (dict(W=6), dict(N=0), dict(M=0), dict(M=65536), dict(N=4 * 65535 + 1, M=1), dict(H=0),
               dict(N=1 << 11, M=1 << 10), dict(H=1 << 15, W=1 << 14)):
        assert apply(im, noise, out, **kw) == -5, kw
    assert L.ica_transfer_apply_ws_size(1, 1, 8, 6) == 0 and L.ica_transfer_apply_ws_size(2, 65536, 8, 8) == 0
    assert L.ica_transfer_apply_ws_size(2, 2, 8, 8) == 4

    x4, s4 = z(4, 1, 8, 8, 4), z(2, 1, 8, 8, 4)
    score = lambda a, b, N=2, M=2, H=8, W=8, m=mse, w=ws: L.ica_transfer_score(
        a if isinstance(a, C.c_void_p) or a is None else ptr(a), b if isinstance(b, C.c_void_p) or b is None else ptr(b),
        N, M, H, W, 1, ptr(m), ptr(w), stream())
    assert score(x4, s4) == 0
    assert score(None, s4) == -5 and score(x4, None) == -5 and score(x4, s4, m=None) == -5
    assert score(x4, s4, w=None) == -5 and score(off(x4), s4, N=1) == -5 and score(x4, off(s4), M=1) == -5
    for kw in (dict(N=0), dict(M=65536), dict(W=0), dict(N=1 << 11, M=1 << 10)):
        assert score(x4, s4, **kw) == -5, kw
    assert L.ica_transfer_score_ws_size(0, 1, 8, 8) == 0 and L.ica_transfer_score_ws_size(2, 2, 8, 8) == 4
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- #
# transfer_matrix end to end
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def kern():
    from oracle import codec
    from imagecompression_adversarial_amd.engine import CodecKernels
    P = codec.perturb_params(codec.init_params("hyper", 1, seed=0), seed=1)
    P["g_a.6.weight"] = P["g_a.6.weight"] * 40.0     # |y| ~ 1 and more: the rounded-latent reconstructions move
    return CodecKernels({k: v.to(DEV) for k, v in P.items()}, "hyper", "fp32")


@pytest.mark.parametrize("hw", [(64, 64), (64, 128)])
def test_transfer_matrix_vs_per_pair_path(T, kern, hw, monkeypatch):
    from imagecompression_adversarial_amd import degrade, hip_ops as K
    from imagecompression_adversarial_amd.attack import eval_forward
    H, W = hw
    N, M = 3, 2
    im = R.rand_image((M, 3, H, W), 60 + W)
    torch.manual_seed(0)
    noise = torch.distributions.normal.Normal(0.0, 1e-3 ** 0.5).sample((N, 3, H, W))
    imd, nd = im.to(DEV), noise.to(DEV)

    # the per-pair path that exists without the study: one clean and one noisy forward per pair
    pairs, clean, mse_dev = [], [None] * M, [[0.0] * M for _ in range(N)]
    for i in range(N):
        for j in range(M):
            im_in, _, mi = degrade.apply_noise(imd[j:j + 1], nd[i:i + 1])
            out, _ = eval_forward(kern, torch.cat([imd[j:j + 1], im_in], 0), True)
            mo = K.sqdiff_mean(out[1:].contiguous(), out[:1].contiguous())
            mse_dev[i][j] = (mi.tolist()[0], mo.tolist()[0])
            pairs.append(out[1].cpu())
            clean[j] = out[0].cpu()
    want = R.pair_matrix(im, noise, torch.stack(pairs), torch.stack(clean))

    seen = []
    forward = kern.forward
    monkeypatch.setattr(kern, "forward", lambda x4, *a, **k: (seen.append(x4.shape[0]), forward(x4, *a, **k))[1])
    res = T.transfer_matrix(kern, nd, imd, batch=4)
    monkeypatch.undo()
    assert seen == [2, 4, 2] and sum(seen) == M + N * M            # the targets once, then the noises in two chunks
    assert res.mse_in.shape == (N, M) and res.mse_out.shape == (N, M)
    mo_l = res.mse_out.tolist()
    for i in range(N):
        for j in range(M):
            mi, mo = mse_dev[i][j]
            print(hw, i, j, res.vi[i][j], want[i][j], 10 * math.log10(mo / mi), mo_l[i][j])
            assert mo_l[i][j] > 1e-7
            assert abs(res.vi[i][j] - want[i][j]) < 5e-3
            assert abs(res.vi[i][j] - 10 * math.log10(mo / mi)) < 5e-3
    whole = T.transfer_matrix(kern, nd, imd, batch=32)             # one chunk of 6 pairs
    assert torch.equal(whole.mse_in, res.mse_in)
    assert all(abs(a - b) < 5e-3 for ra, rb in zip(whole.vi, res.vi) for a, b in zip(ra, rb))
    # clamping both operands moves them no further apart, element by element, and every rounding is monotone
    plain = T.transfer_matrix(kern, nd, imd, batch=32, clamp=False)
    assert bool((plain.mse_out >= whole.mse_out).all()) and torch.equal(plain.mse_in, res.mse_in)


# --------------------------------------------------------------------------- #
# the CLI
# --------------------------------------------------------------------------- #
def float_lines(txt):
    out = []
    for ln in txt.splitlines():
        try:
            out.append(float(ln))
        except ValueError:
            pass
    return out


def test_transfer_noise_cli(tmp_path, capsys, monkeypatch):
    from imagecompression_adversarial_amd import transfer_noise
    monkeypatch.chdir(tmp_path)
    argv = ["-s2", "synthetic:2x64x64", "-s", "synthetic:3x64x64", "-m", "hyper", "-q", "1", "--synthetic-weights",
            "-steps", "3", "--batch", "4"]
    vis = transfer_noise.main(argv)
    lines = float_lines(capsys.readouterr().out)
    assert tuple(vis.shape) == (2, 3) and len(lines) == 6
    saved = torch.load(tmp_path / "hyper_1_ms-ssim_transfer.pkl")
    assert torch.equal(saved.isnan(), vis.isnan()) and torch.equal(saved.nan_to_num(0.0), vis.nan_to_num(0.0))
    print("transfer matrix", vis)
    for v, cell in zip(lines, vis.flatten().tolist()):              # source-major, target-minor
        assert not math.isinf(v) and (math.isnan(v) and math.isnan(cell) or abs(v - cell) <= 1e-5 * abs(v))
    transfer_noise.main(argv)
    again = float_lines(capsys.readouterr().out)
    assert [repr(v) for v in again] == [repr(v) for v in lines]


def test_transfer_noise_cli_cross_model(tmp_path, capsys, monkeypatch):
    import numpy as np
    from imagecompression_adversarial_amd import transfer_noise
    monkeypatch.chdir(tmp_path)
    m = transfer_noise.main(["--cross-model", "--models", "factorized,hyper", "-q", "1", "--synthetic-weights",
                             "-steps", "3", "-s", "synthetic:2x64x64", "--batch", "4"])
    capsys.readouterr()
    assert m.shape == (2, 2) and not np.isinf(m).any()
    saved = np.load(tmp_path / "transfer_methods.npy")
    assert np.array_equal(saved, m, equal_nan=True)
