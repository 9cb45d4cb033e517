"""The image-side conv kernels, each launch against the float64 references of tests/conv_refs.py, at the shapes where
a persistent tile walk or a tile edge can go wrong.

Z-gather (conv_up to 3 channels: the g_s.6 forward on the deconv pack, the g_a.0 input gradient on the conv's .bwd
pack), with and without a bias:
  conv_up3_x6p_kernel<8, 3>        x6, Cin 128     cases c128_*
  conv_up3_x6p_kernel<12, 2>       x6, Cin 192     cases c192_*
  conv_up3_x6p_kernel<8, 3, true>  bf16, Cin 128   cases c128_* (their bf16 column)
  conv_up3_kernel<false, true>     x6, tiled       cases c16_*, c48_*, c64_*
  conv_up3_kernel<false>           fp32, tiled     cases c16_*, c48_*, c64_*, c192_* of ZT_CASES
RGB-input conv (3 -> 128, k5 s2: the g_a.0 forward on the conv pack, the g_s.6 input gradient on the deconv's .bwd
pack):
  conv_rgb5_x6_kernel<EPI_BIAS>, <EPI_GDN> (y and the saved s), conv_rgb5_bwd_x6_kernel<EPI_IGDN_BWD>,
  conv_rgb5_bf16_kernel<EPI_BIAS>  every case of RGB_CASES (the split-output case: GDN and IGDN_BWD)

Every launch writes into out = images [1 : N + 1] of a NaN-filled buffer of N + 2 images: afterwards the two outer
images are still NaN (nothing written outside), no NaN is left inside (every tile written by this launch, not
inherited from an earlier one through the allocator), and the padding lane of the 3-channel quad is exactly 0.
K.last_launch() names the kernel and grid, so a dispatch change cannot move a case off the kernel it was written for.
The walk cases take their batch from the device's CU count, so that every persistent block walks two or more tiles
(Z-gather: runs of 2 and 3 tiles across image boundaries, ending on the prefetch of a tile that does not exist;
rgb5: runs of >= 9 row tiles across rows and images), and check three images alone against their slice of the batch,
bit for bit.

Rules (tests/conv_refs.py): plain-bias launches |got - ref64| <= (n + 8) 2^-24 S per element (+ 2^-8 |ref64| for a
bf16 output); GDN / IGDN_BWD launches rel_err <= 4 e_ref rounded up (GDN_TOL).  `pytest -s` prints each case's
margin."""
import pytest
import torch

from tests import conv_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

ZP_KERNEL = {(128, "x6"): "conv_up3_x6p_kernel<8, 3, false>", (192, "x6"): "conv_up3_x6p_kernel<12, 2, false>",
             (128, "bf16"): "conv_up3_x6p_kernel<8, 3, true>"}
ZT_KERNEL = {"fp32": "conv_up3_kernel<false, false>", "x6": "conv_up3_kernel<false, true>"}
# kind: (kernel, threads per block, waves per block = tiles per round)
RGB_KERNEL = {"bias": ("conv_rgb5_x6_kernel<0>", 512, 8), "gdn": ("conv_rgb5_x6_kernel<2>", 512, 8),
              "igdn_bwd": ("conv_rgb5_bwd_x6_kernel<5>", 256, 4), "bias_bf16": ("conv_rgb5_bf16_kernel<0>", 512, 8)}


@pytest.fixture(scope="module")
def K():
    from imagecompression_adversarial_amd import hip_ops
    assert (hip_ops.EPI_BIAS, hip_ops.EPI_GDN, hip_ops.EPI_IGDN_BWD) == (0, 2, 5)   # the kernel names above
    return hip_ops


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _prec(K, name):
    return {"fp32": K.PREC_FP32, "x6": K.PREC_X6, "bf16": K.PREC_BF16}[name]


def _nan_out(N, C4, H, W, dtype=torch.float32):
    """(buffer of N + 2 NaN images, its images [1 : N + 1])"""
    buf = torch.full((N + 2, C4, H, W, 4), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[1:N + 1]


def _guards(buf, what):
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), f"{what}: wrote outside its output"
    assert not bool(torch.isnan(buf[1:-1]).any()), f"{what}: left output unwritten (or wrote a NaN)"


# --------------------------------------------------------------------------- #
# Z-gather
# --------------------------------------------------------------------------- #
def _zg_launch(K, x4, Cin, pack, bias, layout, kernel, threads):
    N, _, H, W, _ = x4.shape
    buf, out = _nan_out(N, 1, 2 * H, 2 * W)
    K.last_launch()
    y, _, _ = K.conv_up(x4, Cin, pack, bias, 3, out=out, layout=layout)
    name, thr = K.last_launch()
    assert y is out
    assert kernel in name and thr == threads, (name, thr, kernel, threads)
    _guards(buf, kernel)
    assert float(out[..., 3].abs().max()) == 0.0, "padding lane of the RGB quad"
    return out


def _zg_input(x, prec, split):
    x4 = R.to_nc4(R.bf(x)).bfloat16() if prec == "bf16" else R.to_nc4(x)
    return (R.split4(x4) if split else x4).to(DEV)


def _zg_check(got4, ref0, S0, bias, n, tag):
    ref, S = R.with_bias(ref0, S0, bias)
    ok, ratio, worst = R.bias_rule(R.from_nc4(got4.cpu(), 3), ref, S, n)
    print(f"{tag}: max |d|/S {ratio:.2e} = {worst:.3f} of the bound")
    assert ok, (tag, ratio, worst)
    return ratio, worst


@pytest.mark.parametrize("name,prec", [(n, p) for n, c in R.ZP_CASES.items() for p in c[1]])
def test_zgather_persistent(K, cus, name, prec):
    Cin, _, H, W, n_fixed, per, split = R.ZP_CASES[name]
    N = R.zp_n(name, cus)
    tiles = N * per
    if n_fixed is None:
        assert tiles > 2 * 8 * (cus // 8)   # every block walks at least two tiles
    x, w, b, _ = R.zg_case(name, N)
    ref0, S0 = R.zg_expected(name, N, prec == "bf16")
    wd, bd = w.to(DEV), b.to(DEV)
    fwd = K.PackedConv(wd, bd, "deconv", 2, _prec(K, prec))     # g_s.6 forward
    bwd = K.PackedConv(wd, None, "conv", 2, _prec(K, prec))     # g_a.0 input gradient: the same [Cin][3][5][5] view
    views = {"fwd": fwd.fwd, "dgrad": bwd.bwd}
    for p in views.values():
        assert p.order == K.ORDER_UP3 and p.prec == _prec(K, prec)
    x4 = _zg_input(x, prec, split)
    layout = K.LAYOUT_IN if split else 0
    kernel = ZP_KERNEL[(Cin, prec)]
    worst = 0.0
    for view, pack in views.items():
        for bias in (b, None):
            bdev = None if bias is None else bd
            out = _zg_launch(K, x4, Cin, pack, bdev, layout, kernel, 256 * R.zp_blocks(tiles, cus))
            tag = f"zgather {name} {prec} {view} bias={bias is not None:d} N={N}"
            worst = max(worst, _zg_check(out, ref0, S0, bias, 9 * Cin, tag)[1])
            if n_fixed is None:   # batch independence: an image alone gives the bits of its slice of the batch
                for i in (0, N // 2, N - 1):
                    alone = _zg_launch(K, x4[i:i + 1], Cin, pack, bdev, layout, kernel, 256 * R.zp_blocks(per, cus))
                    assert torch.equal(alone[0], out[i]), (tag, i, float((alone[0] - out[i]).abs().max()))
    print(f"TABLE zgather {kernel} {name} N={N} tiles={tiles}: worst {worst:.3f} of the bound")


@pytest.mark.parametrize("name,prec", [(n, p) for n, c in R.ZT_CASES.items() for p in c[1]])
def test_zgather_tiled(K, name, prec):
    Cin, _, H, W, N, per = R.ZT_CASES[name]
    x, w, b, _ = R.zg_case(name)
    ref0, S0 = R.zg_expected(name)
    pack = K.pack_up3(w.to(DEV), _prec(K, prec))
    assert pack.order == K.ORDER_UP3 and pack.prec == _prec(K, prec)
    x4 = _zg_input(x, prec, False)
    worst = 0.0
    for bias in (b, None):
        out = _zg_launch(K, x4, Cin, pack, None if bias is None else b.to(DEV), 0, ZT_KERNEL[prec], 256 * N * per)
        worst = max(worst, _zg_check(out, ref0, S0, bias, 9 * Cin, f"zgather tiled {name} {prec} "
                                                                  f"bias={bias is not None:d}")[1])
    print(f"TABLE zgather {ZT_KERNEL[prec]} {name} N={N} tiles={N * per}: worst {worst:.3f} of the bound")


# --------------------------------------------------------------------------- #
# RGB-input conv
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def rgb_packs(K):
    """case name -> {launch kind: its pack, b: the bias, gd: the GDN pack} (weights are seeded per case, not per N)"""
    cache = {}

    def get(name):
        if name not in cache:
            c = R.rgb_case(name, 1)
            w, b = c["w"].to(DEV), c["b"].to(DEV)
            conv6 = K.PackedConv(w, b, "conv", 2, K.PREC_X6)          # g_a.0 forward
            dec6 = K.PackedConv(w, None, "deconv", 2, K.PREC_X6)      # g_s.6: its input gradient is .bwd
            conv16 = K.PackedConv(w, b, "conv", 2, K.PREC_BF16)
            for p, prec in ((conv6.fwd, K.PREC_X6), (dec6.bwd, K.PREC_X6), (conv16.fwd, K.PREC_BF16)):
                assert p.order == K.ORDER_RGB5 and p.prec == prec, p
            gd = K.PackedGDN(c["beta"].to(DEV), c["gamma"].to(DEV)).x6()   # packed now: not a launch of the conv's
            cache[name] = dict(bias=conv6.fwd, gdn=conv6.fwd, igdn_bwd=dec6.bwd, bias_bf16=conv16.fwd, b=b, gd=gd)
        return cache[name]
    return get


def _rgb_launch(K, kind, packs, x4, saved, layout, threads):
    """-> (y, s or None), row-major on the device"""
    N, _, H, W, _ = x4.shape
    Ho, Wo = R.cdiv(H, 2), R.cdiv(W, 2)
    buf, out = _nan_out(N, R.C_RGB // 4, Ho, Wo, torch.bfloat16 if kind == "bias_bf16" else torch.float32)
    sbuf, sout = _nan_out(N, R.C_RGB // 4, Ho, Wo) if kind == "gdn" else (None, None)
    epi = {"bias": K.EPI_BIAS, "bias_bf16": K.EPI_BIAS, "gdn": K.EPI_GDN, "igdn_bwd": K.EPI_IGDN_BWD}[kind]
    K.last_launch()
    y = K.conv_ex(x4, 3, packs[kind], None if kind == "igdn_bwd" else packs["b"], R.C_RGB, 5, 2, 0, epi,
                  packs["gd"] if kind in ("gdn", "igdn_bwd") else None, save_s=sout, saved=saved, out=out,
                  layout=layout)
    name, thr = K.last_launch()
    assert y is out
    assert RGB_KERNEL[kind][0] in name and thr == threads, (name, thr, RGB_KERNEL[kind][0], threads)
    _guards(buf, name)
    if sbuf is not None:
        _guards(sbuf, name + " (saved s)")
    return out, sout


@pytest.mark.parametrize("name,kind", [(n, k) for n, c in R.RGB_CASES.items() for k in c[5]])
def test_rgb_input_conv(K, cus, rgb_packs, name, kind):
    H, W, n_fixed, per, split, _ = R.RGB_CASES[name]
    N = R.rgb_n(name, cus)
    total = N * per
    if n_fixed is None:
        assert total > 8 * cus   # more than one round of a forward block's 8 waves
    c = R.rgb_case(name, N)
    exp = R.rgb_expected(name, kind, N)
    packs = rgb_packs(name)
    kernel, tpb, waves = RGB_KERNEL[kind]
    layout = K.LAYOUT_OUT if split else 0
    lay_in = R.split4 if split else (lambda t: t)
    lay_out = R.merge4 if split else (lambda t: t)
    x4 = R.to_nc4(c["g"] if kind == "igdn_bwd" else c["x"]).to(DEV)
    saved = None
    if kind == "igdn_bwd":   # the saved pair (y, s = y / a) of the float64 IGDN, as fp32 tensors
        saved = tuple(lay_in(R.to_nc4(t.float())).to(DEV) for t in exp[1:3])

    def threads(n_img):
        return tpb * R.rgb_blocks(n_img * per, cus, waves)

    y4, s4 = _rgb_launch(K, kind, packs, x4, saved, layout, threads(N))
    tag = f"rgb5 {name} {kind} N={N} tiles={total}"
    got = R.from_nc4(lay_out(y4.float().cpu()), R.C_RGB)
    if kind in ("bias", "bias_bf16"):
        ok, ratio, worst = R.bias_rule(got, exp[0], exp[-1], 75, kind == "bias_bf16")
        print(f"TABLE {kernel} {tag}: max |d|/S {ratio:.2e} = {worst:.3f} of the bound")
        assert ok, (tag, ratio, worst)
    else:
        outs = [got] + ([R.from_nc4(lay_out(s4.cpu()), R.C_RGB)] if kind == "gdn" else [])
        res = []
        for o, g, e in zip(R.GDN_OUTPUTS[kind], outs, exp):
            tol = R.GDN_TOL[(name, kind, o)]
            ok, err = R.gdn_rule(g, e, tol)
            print(f"TABLE {kernel} {tag} {o}: rel_err {err:.2e} (tolerance {tol:.0e})")
            res.append((ok, o, err, tol))
        assert all(r[0] for r in res), (tag, res)
    if n_fixed is None:   # batch independence
        for i in (0, N // 2, N - 1):
            sv = None if saved is None else tuple(t[i:i + 1] for t in saved)
            ya, sa = _rgb_launch(K, kind, packs, x4[i:i + 1], sv, layout, threads(1))
            assert torch.equal(ya[0], y4[i]), (tag, i)
            assert sa is None or torch.equal(sa[0], s4[i]), (tag, i, "s")
