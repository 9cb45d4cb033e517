"""The balanced tiling of the latent-end x6 conv_down (128 -> 192 channels, level 3 -> level 4: g_a.6 forward and the
g_s.0 input gradient; launch_down_x6_cs2 in ica_conv_x6.hip): blocks of 4 x 48 output pixels over both 96-channel
blocks instead of 8 x 32 pixels over one.

A tiling moves outputs between lanes and blocks, not arithmetic: every output accumulates the same (chunk, tap) MFMA
sequence and runs the same epilogue, so the balanced tiling must be BIT-IDENTICAL to the 8 x 32 tiling it replaces
(both reached through hip_ops.x6_tiling, which also lets a few-pixel map run the large-grid kernels), and within the
x6 path's stated tolerance of the fp32-MFMA path (tests/test_gpu_x6.py: layer outputs rel <= 1e-4 of the tensor max).

Shapes: B = 3 at level-3 sides 20 x 36 -> level-4 10 x 18 (partial tiles in both directions: 3 row blocks of 4 with 2
rows used in the last, 18 of 48 columns, so the last column tile of every block is empty); B = 2 at 64 x 96 -> 32 x 48,
the workload's own whole-tile geometry; the level-3 input both parity-split and row-major.  The picker itself: a grid
that does not fill whole rounds of the 256 CUs keeps the previous kernel, the workload's B = 32 grid takes the new one.

The conv_up side of the latent end (192 -> 128) already runs whole rounds (768 blocks at PT = 1).  Its forward
(g_s.0: IGDN, saving s) moves from four waves to the 8-wave kernel at the same tiling and must keep its bits, on the
same two geometries (level-4 sides 10 x 18 and 32 x 48), with the level-3 output parity-split and row-major; its GDN
backward (the g_a.6 input gradient) keeps its kernel under every mode.  DESIGN §9 "Grid tails"."""
import pytest
import torch

from tests.conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CI, CO = 128, 192

NEW_KERNEL = "conv_down_x6_kernel<3, 0, 3, 2>"
PT2_KERNEL = "conv_down_x6_kernel<3, 0, 2, 1>"
PT1_KERNEL = "conv_down_x6_kernel<3, 0, 1, 1>"


def split4(x4):
    """row-major nChw4c -> parity-split: the four (y & 1, x & 1) sub-planes of (H/2) x (W/2) pixels in turn"""
    N, C4, H, W, _ = x4.shape
    return x4.view(N, C4, H // 2, 2, W // 2, 2, 4).permute(0, 1, 3, 5, 2, 4, 6).contiguous().view(N, C4, H, W, 4)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@pytest.fixture(scope="module")
def K():
    from imagecompression_adversarial_amd import hip_ops
    yield hip_ops
    hip_ops.x6_tiling(hip_ops.X6_TILING_AUTO)


@pytest.fixture(scope="module")
def layers(K):
    """kind -> (x6 pack, fp32 pack, bias): g_a.6 forward (a conv's forward, with bias) and the g_s.0 input gradient (a
    deconv's input gradient, no bias), the same weights in both precisions."""
    g = _gen(0)
    wc = (torch.rand(CO, CI, 5, 5, generator=g, device=DEV) - 0.5) * 0.04
    bc = (torch.rand(CO, generator=g, device=DEV) - 0.5) * 0.2
    wd = (torch.rand(CO, CI, 5, 5, generator=g, device=DEV) - 0.5) * 0.04   # ConvTranspose2d(192, 128) weight
    out = {}
    for prec in (K.PREC_X6, K.PREC_FP32):
        c = K.PackedConv(wc, bc, "conv", 2, prec)
        d = K.PackedConv(wd, None, "deconv", 2, prec)
        assert c.fwd_prec == prec and d.bwd_prec == prec
        out[prec] = {"fwd": (c.fwd, c.bias), "dgrad": (d.bwd, None)}
    return out


def _act(K, B, H, W, seed):
    return K.empty_nc4(B, CI, H, W, DEV).uniform_(-1.0, 1.0, generator=_gen(seed))


def _down(K, x4, pack, bias, mode, layout=0):
    """the launch under tiling `mode`; returns (y, kernel name, blocks)"""
    K.x6_tiling(mode)
    try:
        K.last_launch()
        y, _, _ = K.conv_down(x4, CI, pack, bias, CO, 5, 2, K.EPI_BIAS, layout=layout)
        name, threads = K.last_launch()
    finally:
        K.x6_tiling(K.X6_TILING_AUTO)
    return y, name, threads // 256


# (B, level-3 H, W): partial tiles with an empty last column tile; the workload's whole-tile geometry
SHAPES = [(3, 20, 36), (2, 64, 96)]


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
@pytest.mark.parametrize("split_in", [True, False])
def test_balanced_tiling_same_bits_as_8x32(K, layers, kind, B, H, W, split_in):
    pack, bias = layers[K.PREC_X6][kind]
    x = _act(K, B, H, W, 1)
    xin, lay = (split4(x), K.LAYOUT_IN) if split_in else (x, 0)
    y_new, k_new, b_new = _down(K, xin, pack, bias, K.X6_TILING_BALANCED, lay)
    y_old, k_old, b_old = _down(K, xin, pack, bias, K.X6_TILING_PREVIOUS, lay)
    assert NEW_KERNEL in k_new and PT2_KERNEL in k_old, (k_new, k_old)
    Ho, Wo = H // 2, W // 2
    assert b_new == B * ((Ho + 3) // 4) * ((Wo + 47) // 48)
    assert b_old == B * ((Ho + 7) // 8) * ((Wo + 31) // 32) * 2
    assert y_new.shape == y_old.shape == (B, CO // 4, Ho, Wo, 4)
    assert torch.equal(y_new, y_old), float((y_new - y_old).abs().max())
    # the fp32-MFMA path (row-major storage only) on the same weights
    p32, b32 = layers[K.PREC_FP32][kind]
    y32, _, _ = K.conv_down(x, CI, p32, b32, CO, 5, 2, K.EPI_BIAS)
    err = rel_err(y_new.cpu(), y32.cpu())
    print(f"{kind} B={B} {H}x{W} split={split_in}: rel err vs fp32 path {err:.3e}")
    assert err < 1e-4


@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_partial_rounds_keep_previous_kernel(K, layers, kind):
    """B = 2 at 32 x 48 latents: 16 balanced blocks are 6 % of one round of 256 CUs, so the picker stays with its
    earlier choice (PT = 1: fewer than 256 blocks at PT = 2), bit-identical to both other tilings."""
    pack, bias = layers[K.PREC_X6][kind]
    x = _act(K, 2, 64, 96, 2)
    y_auto, k_auto, b_auto = _down(K, x, pack, bias, K.X6_TILING_AUTO)
    assert PT1_KERNEL in k_auto and b_auto % 256 != 0, (k_auto, b_auto)
    y_new, k_new, _ = _down(K, x, pack, bias, K.X6_TILING_BALANCED)
    assert NEW_KERNEL in k_new
    assert torch.equal(y_auto, y_new)


def test_picker_takes_whole_rounds(K, layers):
    """The workload's own grid (B = 32, 32 x 48 latents): 256 balanced blocks, one per CU.  One fewer image leaves the
    last round 97 % full and still takes it; B = 24 (192 blocks, 75 %) does not."""
    pack, bias = layers[K.PREC_X6]["fwd"]
    x = _act(K, 32, 64, 96, 3)
    y, name, blocks = _down(K, x, pack, bias, K.X6_TILING_AUTO)
    assert NEW_KERNEL in name and blocks == 256, (name, blocks)
    y_old, k_old, b_old = _down(K, x, pack, bias, K.X6_TILING_PREVIOUS)
    assert PT2_KERNEL in k_old and b_old == 512
    assert torch.equal(y, y_old)
    _, name, blocks = _down(K, x[:31], pack, bias, K.X6_TILING_AUTO)
    assert NEW_KERNEL in name and blocks == 248
    _, name, blocks = _down(K, x[:24], pack, bias, K.X6_TILING_AUTO)
    assert PT2_KERNEL in name and blocks == 384


def merge4(xs):
    N, C4, H, W, _ = xs.shape
    return xs.view(N, C4, 2, 2, H // 2, W // 2, 4).permute(0, 1, 4, 2, 5, 3, 6).contiguous().view(N, C4, H, W, 4)


UP8_KERNEL = "conv_up_x6w_kernel<4, {epi}, 64, 1>"
UP4_KERNEL = "conv_up_x6_kernel<4, {epi}, 64, 1, 5, 0>"


@pytest.fixture(scope="module")
def up_layers(K):
    """g_s.0 forward (ConvTranspose2d(192, 128) + IGDN) in both precisions, and the GDN pack"""
    g = _gen(4)
    w = (torch.rand(CO, CI, 5, 5, generator=g, device=DEV) - 0.5) * 0.04
    b = (torch.rand(CI, generator=g, device=DEV) - 0.5) * 0.2
    gd = K.PackedGDN(torch.ones(CI, device=DEV) * 1.01, (0.1 * torch.eye(CI, device=DEV) + 0.001).sqrt())
    gd.x6()   # packed here, so that each conv launch below is the only launch since the previous last_launch()
    return {prec: K.PackedConv(w, b, "deconv", 2, prec) for prec in (K.PREC_X6, K.PREC_FP32)}, gd


def _up(K, x4, pc, gd, epi, mode, layout=0):
    K.x6_tiling(mode)
    try:
        K.last_launch()
        y, _, s = K.conv_up(x4, CO, pc.fwd, pc.bias, CI, epi, gd if epi == K.EPI_IGDN else None, epi == K.EPI_IGDN,
                            layout=layout)
        name, threads = K.last_launch()
    finally:
        K.x6_tiling(K.X6_TILING_AUTO)
    return y, s, name, threads


@pytest.mark.parametrize("B,H,W", [(3, 10, 18), (2, 32, 48)])   # level-4 sides: partial tiles; the workload's tiles
@pytest.mark.parametrize("epi", ["igdn", "bias"])
@pytest.mark.parametrize("split_out", [True, False])
def test_conv_up_forward_eight_waves_same_bits(K, up_layers, epi, B, H, W, split_out):
    """g_s.0 forward (192 -> 128, 64-channel groups) at PT = 1: the 8-wave kernel against the 4-wave one"""
    packs, gd = up_layers
    e = K.EPI_IGDN if epi == "igdn" else K.EPI_BIAS
    x = K.empty_nc4(B, CO, H, W, DEV).uniform_(-1.0, 1.0, generator=_gen(5))
    lay = K.LAYOUT_OUT if split_out else 0
    out = merge4 if split_out else (lambda t: t)
    y8, s8, k8, t8 = _up(K, x, packs[K.PREC_X6], gd, e, K.X6_TILING_BALANCED, lay)
    y4, s4, k4, t4 = _up(K, x, packs[K.PREC_X6], gd, e, K.X6_TILING_PREVIOUS, lay)
    assert UP8_KERNEL.format(epi=e) in k8 and UP4_KERNEL.format(epi=e) in k4, (k8, k4)
    blocks = B * ((H + 3) // 4) * ((W + 15) // 16)
    assert (t8, t4) == (512 * blocks, 256 * blocks)
    assert torch.equal(y8, y4), float((y8 - y4).abs().max())
    if e == K.EPI_IGDN:
        assert torch.equal(s8, s4), float((s8 - s4).abs().max())
    y32, s32, _, _ = _up(K, x, packs[K.PREC_FP32], gd, e, K.X6_TILING_AUTO)
    err = rel_err(out(y8).cpu(), y32.cpu())
    print(f"conv_up {epi} B={B} {H}x{W} split={split_out}: rel err vs fp32 path {err:.3e}")
    assert err < 1e-4
    if e == K.EPI_IGDN:
        assert rel_err(out(s8).cpu(), s32.cpu()) < 1e-4


def test_conv_up_picker(K, up_layers):
    """B = 32 at 32 x 48 latents: 768 blocks, three whole rounds, on eight waves"""
    packs, gd = up_layers
    x = K.empty_nc4(32, CO, 32, 48, DEV).uniform_(-1.0, 1.0, generator=_gen(6))
    y, s, name, threads = _up(K, x, packs[K.PREC_X6], gd, K.EPI_IGDN, K.X6_TILING_AUTO, K.LAYOUT_OUT)
    assert UP8_KERNEL.format(epi=K.EPI_IGDN) in name and threads == 768 * 512, (name, threads)
    y4, s4, k4, _ = _up(K, x, packs[K.PREC_X6], gd, K.EPI_IGDN, K.X6_TILING_PREVIOUS, K.LAYOUT_OUT)
    assert UP4_KERNEL.format(epi=K.EPI_IGDN) in k4
    assert torch.equal(y, y4) and torch.equal(s, s4)


@pytest.mark.parametrize("B,H,W", [(3, 10, 18), (2, 32, 48)])   # level-4 sides, as above
@pytest.mark.parametrize("split_out", [True, False])
def test_conv_up_gdn_backward_large_grid(K, up_layers, B, H, W, split_out):
    """The g_a.6 input gradient (conv_up 192 -> 128 with the GDN backward epilogue) has one large-grid kernel, the
    8-wave slab kernel at PT = 1; the override modes send these few-pixel maps to it instead of the small-grid
    kernel.  Its reference is the fp32-MFMA path on the same weights and saved (y, s)."""
    _, gd = up_layers
    g = _gen(7)
    w = (torch.rand(CO, CI, 5, 5, generator=g, device=DEV) - 0.5) * 0.04   # Conv2d(128, 192) weight
    p6, p32 = (K.PackedConv(w, None, "conv", 2, prec) for prec in (K.PREC_X6, K.PREC_FP32))
    assert p6.bwd_prec == K.PREC_X6 and p32.bwd_prec == K.PREC_FP32
    gy = K.empty_nc4(B, CO, H, W, DEV).uniform_(-1.0, 1.0, generator=g)
    sy = K.empty_nc4(B, CI, 2 * H, 2 * W, DEV).uniform_(0.0, 1.0, generator=g)
    ss = K.empty_nc4(B, CI, 2 * H, 2 * W, DEV).uniform_(0.5, 1.0, generator=g)
    gd.x6()
    saved = (split4(sy), split4(ss)) if split_out else (sy, ss)
    K.x6_tiling(K.X6_TILING_BALANCED)
    try:
        K.last_launch()
        y6 = K.conv_up(gy, CO, p6.bwd, None, CI, K.EPI_GDN_BWD, gd, saved=saved,
                       layout=K.LAYOUT_OUT if split_out else 0)[0]
        name, threads = K.last_launch()
    finally:
        K.x6_tiling(K.X6_TILING_AUTO)
    assert "conv_up_x6w_kernel<4, 4, 64, 1>" in name, name
    assert threads == 512 * B * ((H + 3) // 4) * ((W + 15) // 16)
    y32 = K.conv_up(gy, CO, p32.bwd, None, CI, K.EPI_GDN_BWD, gd, saved=(sy, ss))[0]
    err = rel_err((merge4(y6) if split_out else y6).cpu(), y32.cpu())
    print(f"conv_up gdn_bwd B={B} {H}x{W} split={split_out}: rel err vs fp32 path {err:.3e}")
    assert err < 1e-4


def test_tiling_mode_is_checked(K):
    with pytest.raises(RuntimeError, match="status -2"):
        K.x6_tiling(3)
