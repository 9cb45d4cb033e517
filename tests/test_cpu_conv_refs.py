"""The float64-capable references of tests/conv_refs.py and its two comparison rules, on the CPU.

* In fp32 each reference is the torch call the existing GPU tests compare with, bit for bit.
* The fp32 torch result passes the plain-bias rule (n + 8) 2^-24 S on every case: the bound holds for the reference.
* e_ref: the rel_err of the fp32 torch run of the GDN / IGDN_BWD compositions from the float64 one, on the GPU test's
  own seeded inputs; conv_refs.GDN_TOL is round_up_1digit(4 e_ref) of this table (`pytest -s` prints it):

      case          kind      out  e_ref     tolerance
      2x2           gdn       y    7.24e-08  3e-07
      2x2           gdn       s    7.10e-08  3e-07
      2x2           igdn_bwd  dx   6.30e-08  3e-07
      13x67         gdn       y    5.18e-07  3e-06
      13x67         gdn       s    5.72e-07  3e-06
      13x67         igdn_bwd  dx   3.69e-07  2e-06
      64x64         gdn       y    4.97e-07  2e-06
      64x64         gdn       s    6.29e-07  3e-06
      64x64         igdn_bwd  dx   5.59e-07  3e-06
      50x130_walk   gdn       y    4.61e-07  2e-06
      50x130_walk   gdn       s    6.90e-07  3e-06
      50x130_walk   igdn_bwd  dx   5.60e-07  3e-06
      48x68_split   gdn       y    4.70e-07  2e-06
      48x68_split   gdn       s    5.77e-07  3e-06
      48x68_split   igdn_bwd  dx   4.45e-07  2e-06

* Sensitivity: a float64 result with one small defect (one tap removed at one output pixel; one 16-channel chunk
  zeroed in one halo column at a tile seam; one output row taken from the neighbouring parity; one image's tile taken
  from the next image) fails its rule in every case family, so a kernel wrong in one tile class would fail
  tests/test_gpu_image_ends.py.

The walk cases (batch from the CU count) run here at the 256-CU batch for e_ref and at N = 2 for the bias rule, which
is per element and the same for every image.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import codec
from tests import conv_refs as R

F32, F64 = torch.float32, torch.float64


# --------------------------------------------------------------------------- #
# the case tables and the references themselves
# --------------------------------------------------------------------------- #
def test_tile_counts_follow_the_geometry():
    for name, (Cin, _, H, W, _, per, split) in R.ZP_CASES.items():
        assert per == R.cdiv(H, R.ZP_ROWS[Cin]) * R.cdiv(W, R.ZP_COLS), name
        assert not split or (H % 2 == 0 and W % 2 == 0)
    for name, (Cin, _, H, W, _, per) in R.ZT_CASES.items():
        assert per == R.cdiv(H, R.ZT_ROWS) * R.cdiv(W, R.ZT_COLS) and Cin % 16 == 0, name
    for name, (H, W, _, per, split, _) in R.RGB_CASES.items():
        Ho, Wo = R.cdiv(H, 2), R.cdiv(W, 2)
        assert per == R.cdiv(Wo, R.RGB_COLS) * Ho, name
        assert not split or (Ho % 2 == 0 and Wo % 2 == 0)
    # the walk batches at 256 CUs, and what they make the blocks do
    assert R.zp_n("c128_41x91_walk") == 26 and R.zp_n("c192_25x61_walk") == 35 and R.rgb_n("50x130_walk") == 28
    for name in ("c128_41x91_walk", "c192_25x61_walk"):
        tiles = R.zp_n(name) * R.ZP_CASES[name][5]
        assert 2 * 8 * 32 < tiles < 3 * 8 * 32 and R.zp_blocks(tiles, 256) == 256   # every block 2 tiles, some 3
    total = 28 * 75
    assert R.cdiv(total, R.rgb_blocks(total, 256, 8)) == 9 and R.cdiv(total, R.rgb_blocks(total, 256, 4)) == 9
    assert R.zp_blocks(27, 256) == 32 and R.zp_blocks(1, 256) == 8 and R.rgb_blocks(14, 256, 8) == 2


def test_layout_helpers():
    x = R.rnd((2, 3, 4, 6), 1)
    x4 = R.to_nc4(x)
    assert x4.shape == (2, 1, 4, 6, 4) and float(x4[..., 3].abs().max()) == 0.0
    assert torch.equal(R.from_nc4(x4, 3), x) and torch.equal(x4[1, 0, 2, 5, :3], x[1, :, 2, 5])
    s = R.split4(x4)
    assert torch.equal(R.merge4(s), x4)
    assert torch.equal(s.view(2, 1, 2, 2, 2, 3, 4)[:, :, 1, 0], x4[:, :, 1::2, 0::2])


def test_fp32_references_are_the_torch_calls():
    x, w, b, _ = R.zg_case("c128_11x31")
    assert torch.equal(R.up3_ref(x, w, b, F32), F.conv_transpose2d(x, w, b, stride=2, padding=2, output_padding=1))
    assert torch.equal(R.up3_ref(x, w, None, F32), codec.deconv(x, w, None))
    assert R.up3_ref(x, w, b).dtype == F64
    # the input-gradient view: autograd of the conv 3 -> Cin whose weight w is
    xi = torch.zeros((1, 3, 22, 62), dtype=F64, requires_grad=True)
    F.conv2d(xi, w.double(), None, stride=2, padding=2).backward(x.double())
    assert R.rel_err(xi.grad, R.up3_ref(x, w, None)) < 1e-13
    c = R.rgb_case("13x67")
    assert torch.equal(R.rgb_ref(c["x"], c["w"], c["b"], F32), F.conv2d(c["x"], c["w"], c["b"], stride=2, padding=2))
    pre = R.rgb_ref(c["x"], c["w"], c["b"], F32)
    y, s = R.rgb_compose(c, "gdn", F32)
    assert torch.equal(y, codec.gdn(pre, c["beta"], c["gamma"], False)) and y.dtype == F32
    assert R.rel_err(y / s, pre) < 1e-6
    # IGDN backward as tests/test_gpu_bf16.py::test_rgb_output_deconv_bf16 builds it
    ad = c["a"].clone().requires_grad_(True)
    yprev = codec.gdn(ad, c["beta"], c["gamma"], True)
    yprev.backward(F.conv2d(c["g"], c["w"], None, stride=2, padding=2))
    dx, ys, ss = R.rgb_compose(c, "igdn_bwd", F32)
    assert torch.equal(dx, ad.grad) and torch.equal(ys, yprev.detach()) and torch.equal(ss, (yprev / c["a"]).detach())
    assert R.rgb_compose(c, "igdn_bwd", F64)[0].dtype == F64
    # bf16 references: rounded operands, float64 arithmetic
    assert torch.equal(R.rgb_expected("13x67", "bias_bf16")[0], R.rgb_ref(R.bf(c["x"]), R.bf(c["w"]), c["b"]))
    assert torch.equal(R.zg_expected("c128_11x31", None, True)[0], R.up3_ref(R.bf(x), R.bf(w), None))


def test_abs_scale_bounds_every_term():
    x, w, b, _ = R.zg_case("c128_3x5")
    S = R.abs_scale(R.up3_ref, x, w, b)
    assert S.dtype == F64 and bool((S >= R.up3_ref(x, w, b).abs()).all())
    S0 = R.abs_scale(R.up3_ref, x, w, None)
    r, Sb = R.with_bias(R.up3_ref(x, w, None), S0, b)
    assert R.rel_err(Sb, S) < 1e-14 and R.rel_err(r, R.up3_ref(x, w, b)) < 1e-14
    assert float(b.abs().min()) >= 0.5   # a dropped bias is hundreds of bounds
    assert float((b.abs().min() / R.bias_bound(9 * 128, S).max())) > 100


# --------------------------------------------------------------------------- #
# the fp32 torch result passes the plain-bias rule
# --------------------------------------------------------------------------- #
def _cpu_n(table, name):
    return 2 if table[name][4 if table is not R.RGB_CASES else 2] is None else None


@pytest.mark.parametrize("name", list(R.ZP_CASES) + list(R.ZT_CASES))
def test_zgather_fp32_torch_passes_the_rule(name):
    table = R.ZP_CASES if name in R.ZP_CASES else R.ZT_CASES
    N = _cpu_n(table, name)
    x, w, b, Cin = R.zg_case(name, N)
    for prec in table[name][1]:
        rounded = prec == "bf16"
        xr, wr = (R.bf(x), R.bf(w)) if rounded else (x, w)
        ref0, S0 = R.zg_expected(name, N, rounded)
        for bias in (b, None):
            ref, S = R.with_bias(ref0, S0, bias)
            ok, ratio, worst = R.bias_rule(R.up3_ref(xr, wr, bias, F32), ref, S, 9 * Cin)
            print(f"fp32 torch {name:18s} {prec:4s} bias={bias is not None:d}  |d|/S {ratio:.2e}  of bound {worst:.3f}")
            assert ok and worst < 0.5   # a worst-case bound: round-to-nearest sums sit far below it


@pytest.mark.parametrize("name", list(R.RGB_CASES))
def test_rgb_fp32_torch_passes_the_rule(name):
    N = _cpu_n(R.RGB_CASES, name)
    c = R.rgb_case(name, N)
    for kind in ("bias", "bias_bf16"):
        x, w = (R.bf(c["x"]), R.bf(c["w"])) if kind == "bias_bf16" else (c["x"], c["w"])
        ref, S = R.rgb_expected(name, kind, N)
        got = R.rgb_ref(x, w, c["b"], F32)
        if kind == "bias_bf16":
            got = got.bfloat16()
        ok, ratio, worst = R.bias_rule(got, ref, S, 75, kind == "bias_bf16")
        print(f"fp32 torch rgb {name:12s} {kind:9s}  |d|/S {ratio:.2e}  of bound {worst:.3f}")
        assert ok


# --------------------------------------------------------------------------- #
# e_ref of the GDN launches
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", list(R.RGB_CASES))
def test_gdn_e_ref(name):
    c = R.rgb_case(name)
    for kind, outs in R.GDN_OUTPUTS.items():
        o32, o64 = R.rgb_compose(c, kind, F32), R.rgb_expected(name, kind)
        for i, out in enumerate(outs):
            assert o32[i].dtype == F32 and o64[i].dtype == F64
            e = R.rel_err(o32[i], o64[i])
            tol = R.round_up_1digit(4 * e)
            print(f"e_ref {name:12s} {kind:9s} {out:3s} {e:9.2e}   4x -> {tol:.0e}")
            assert e == e and 0 < e < 1e-5, (name, kind, out, e)   # finite, and a float32 distance
            # the stated tolerance is this rule's (e_ref moves a little with the CPU's summation order)
            have = R.GDN_TOL[(name, kind, out)]
            assert have / 2 <= tol <= have * 2, (name, kind, out, e, have)


# --------------------------------------------------------------------------- #
# sensitivity: one small defect fails the rule
# --------------------------------------------------------------------------- #
def _conv_defects(ref_fn, up, x, w, ref, tile_rows, tile_cols, px):
    """The four defects on the float64 conv result `ref` = ref_fn(x, w, None) (x of >= 2 images).  up: the
    transposed conv (output pixel = 2 x input pixel + parity) or the strided one.  tile_rows / tile_cols: the
    kernel's tile in OUTPUT pixels; px = (row, col) an output pixel off every seam."""
    x, w = x.double(), w.double()
    y0, x0 = px
    # 1. one tap (ky, kx) = (1, 3) removed at one output pixel of image 1
    ky, kx = 1, 3
    out = ref.clone()
    if up:
        assert (y0 + 2 - ky) % 2 == 0 and (x0 + 2 - kx) % 2 == 0
        out[1, :, y0, x0] -= w[:, :, ky, kx].T @ x[1, :, (y0 + 2 - ky) // 2, (x0 + 2 - kx) // 2]
    else:
        out[1, :, y0, x0] -= w[:, :, ky, kx] @ x[1, :, 2 * y0 + ky - 2, 2 * x0 + kx - 2]
    yield "tap", out
    # 2. one 16-channel chunk zeroed in the halo column at the first seam, for the tile that reads it as halo
    d = torch.zeros_like(x)
    out = ref.clone()
    if up:      # input column tile_cols / 2 is the right halo of column tile 0: input channels 0-15 dropped there
        col = tile_cols // 2
        d[0, :16, :, col] = x[0, :16, :, col]
        out[0, :, :, :tile_cols] -= ref_fn(d, w, None)[0, :, :, :tile_cols]
    else:       # input column 2 tile_cols - 1 is the left halo of column tile 1: dropped from output channels 16-31
        col = 2 * tile_cols - 1
        d[0, :, :, col] = x[0, :, :, col]
        out[0, 16:32, :, tile_cols] -= ref_fn(d, w, None)[0, 16:32, :, tile_cols]
    yield "halo chunk", out
    # 3. one output row taken from the neighbouring parity
    out = ref.clone()
    out[0, :, y0, :] = ref[0, :, y0 ^ 1, :]
    yield "row parity", out
    # 4. one image's tile taken from the next image
    out = ref.clone()
    r0 = (y0 // tile_rows) * tile_rows
    c0 = (x0 // tile_cols) * tile_cols
    out[0, :, r0:r0 + tile_rows, c0:c0 + tile_cols] = ref[1, :, r0:r0 + tile_rows, c0:c0 + tile_cols]
    yield "next image", out


ZG_FAMILIES = [("c128_21x61", False, 2 * 10, 2 * R.ZP_COLS, (23, 37)), ("c128_21x61", True, 2 * 10, 2 * R.ZP_COLS, (23, 37)),
               ("c192_13x61", False, 2 * 6, 2 * R.ZP_COLS, (15, 75)), ("c48_6x33", False, 2 * R.ZT_ROWS, 2 * R.ZT_COLS, (7, 37)),
               ("c16_6x33", False, 2 * R.ZT_ROWS, 2 * R.ZT_COLS, (9, 65))]


@pytest.mark.parametrize("name,rounded,rows,cols,px", ZG_FAMILIES)
def test_zgather_defects_fail_the_rule(name, rounded, rows, cols, px):
    x, w, b, Cin = R.zg_case(name)
    if rounded:
        x, w = R.bf(x), R.bf(w)
    ref0, S0 = R.zg_expected(name, None, rounded)
    assert R.bias_rule(ref0, ref0, S0, 9 * Cin)[0]
    seen = []
    for what, bad in _conv_defects(R.up3_ref, True, x, w, ref0, rows, cols, px):
        ok, ratio, worst = R.bias_rule(bad, ref0, S0, 9 * Cin)
        print(f"defect {name} bf16={rounded:d} {what:10s}: |d|/S {ratio:.2e} = {worst:.0f} bounds")
        assert not ok and worst > 20
        seen.append(what)
    assert len(seen) == 4
    # a dropped bias, and a NaN
    ref, S = R.with_bias(ref0, S0, b)
    assert not R.bias_rule(ref0, ref, S, 9 * Cin)[0]
    bad = ref.clone()
    bad[0, 0, 0, 0] = float("nan")
    assert not R.bias_rule(bad, ref, S, 9 * Cin)[0]


@pytest.mark.parametrize("kind", R.RGB_KINDS)
def test_rgb_defects_fail_the_rule(kind):
    name = "50x130_walk"   # Wout 65: column-tile seams at 32 and 64
    c = R.rgb_case(name, 2)
    x = c["g"] if kind == "igdn_bwd" else c["x"]
    b = None if kind == "igdn_bwd" else c["b"]
    w = c["w"]
    if kind == "bias_bf16":
        x, w = R.bf(x), R.bf(w)
    exp = R.rgb_expected(name, kind, 2)
    conv0 = R.rgb_ref(x, w, None)

    def add_b(t):
        return t if b is None else t + b.double().reshape(1, -1, 1, 1)

    pre0 = add_b(conv0)
    assert all(R.rel_err(a_, b_) < 1e-14 for a_, b_ in zip(R.rgb_compose(c, kind, F64, pre=pre0), exp))
    n = 0
    for what, bad in _conv_defects(R.rgb_ref, False, x, w, conv0, 1, R.RGB_COLS, (7, 40)):
        got = R.rgb_compose(c, kind, F64, pre=add_b(bad))
        if kind in ("bias", "bias_bf16"):
            ok, ratio, worst = R.bias_rule(got[0], exp[0], exp[-1], 75, kind == "bias_bf16")
            print(f"defect rgb {kind:9s} {what:10s}: |d|/S {ratio:.2e} = {worst:.0f} bounds")
            assert not ok and worst > 20
        else:
            for i, out in enumerate(R.GDN_OUTPUTS[kind]):
                tol = R.GDN_TOL[(name, kind, out)]
                ok, e = R.gdn_rule(got[i], exp[i], tol)
                print(f"defect rgb {kind:9s} {what:10s} {out}: rel_err {e:.2e} = {e / tol:.0f} tolerances")
                assert not ok and e > 20 * tol
        n += 1
    assert n == 4
