"""A packed weight describes itself (hip_ops.Pack) and no launch reads it as anything else: the Python wrappers
raise before launching, and ica_conv_ex returns -4 for an order its route does not read.  Shapes: the RGB ends
(3 <-> 128 channels) and a 128 -> 128 layer at N = 1, 32 x 32 pixels.  Nothing is compared numerically here (the
parity tests do that); every refused launch must leave ica_last_launch empty, i.e. no kernel ran."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    from imagecompression_adversarial_amd import hip_ops
    return hip_ops


def _rnd(shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) - 0.5).to(DEV)


@pytest.fixture(scope="module")
def S(K):
    """Packs of every layout, and inputs for them."""
    class S:
        pass
    w3, w128, wk3, b = _rnd((128, 3, 5, 5), 1), _rnd((128, 128, 5, 5), 2), _rnd((128, 128, 3, 3), 3), _rnd((128,), 4)
    S.b = b
    S.fp = K.PackedConv(w3, b, "conv", 2)
    S.bf = K.PackedConv(w3, b, "conv", 2, K.PREC_BF16)
    S.bf6 = K.PackedConv(w3, b, "conv", 2, K.PREC_BF16, it_fwd=6)
    S.x6 = K.PackedConv(w3, b, "conv", 2, K.PREC_X6)
    S.fp128 = K.PackedConv(w128, b, "conv", 2)
    S.x128 = K.PackedConv(w128, b, "conv", 2, K.PREC_X6)
    S.b1 = K.pack_conv_x6(wk3, 128, 128, 3, 128 * 9, 9, K.ORDER_DOWN, 4, K.PREC_B1)
    S.up_o3 = K.pack_conv(_rnd((128, 3, 5, 5), 5), 3, 128, 5, 25, 75, K.ORDER_UP, 16)   # conv_up order, 3 outputs
    S.img = K.to_nc4(_rnd((1, 3, 32, 32), 6))
    S.act = K.to_nc4(_rnd((1, 128, 16, 16), 7))
    torch.cuda.synchronize()
    return S


def test_pack_describes_itself(K, S):
    f = S.bf.fwd
    assert (f.O, f.C, f.KS, f.kind, f.order, f.prec, f.it, f.flip) == (128, 3, 5, 0, K.ORDER_RGB5, K.PREC_BF16, 4, False)
    assert f.data.dtype == torch.bfloat16
    assert S.bf6.fwd.order == K.ORDER_TG and S.bf6.fwd.it == 6 and S.bf6.it_fwd == 6
    assert (S.x6.fwd.order, S.x6.fwd.prec, S.x6.fwd.it) == (K.ORDER_RGB5, K.PREC_X6, 4)
    assert (S.fp.fwd.order, S.fp.fwd.prec, S.fp.fwd.data.dtype) == (K.ORDER_DOWN, K.PREC_FP32, torch.float32)
    for p, prec in ((S.fp, K.PREC_FP32), (S.bf, K.PREC_BF16), (S.x6, K.PREC_X6)):   # the Z-gather pack
        assert (p.bwd.order, p.bwd.kind, p.bwd.O, p.bwd.C, p.bwd.prec) == (K.ORDER_UP3, 1, 3, 128, prec)
        assert (p.fwd_prec, p.bwd_prec, p.it_fwd, p.it_bwd) == (p.fwd.prec, prec, p.fwd.it, p.bwd.it)
    assert (S.fp128.bwd.order, S.fp128.bwd.kind) == (K.ORDER_UP, 1)
    assert (S.x128.fwd.prec, S.x128.bwd.prec, S.x128.bwd.order) == (K.PREC_X6, K.PREC_X6, K.ORDER_UP)
    assert (S.b1.prec, S.b1.order, S.b1.KS) == (K.PREC_B1, K.ORDER_DOWN, 3)
    orders = (K.ORDER_DOWN, K.ORDER_UP, K.ORDER_RGB5, K.ORDER_TG, K.ORDER_UP3)
    assert len(set(orders)) == 5
    with pytest.raises(AttributeError):   # the PackedConv fields are views of the packs
        S.fp.fwd_prec = K.PREC_X6
    assert not isinstance(f, torch.Tensor) and not hasattr(f, "__dict__")


def _refused(K, exc, fn, match=None):
    K.last_launch()   # consume the record of whatever ran before
    with pytest.raises(exc, match=match):
        fn()
    assert K.last_launch() is None   # no kernel was launched


def test_wrappers_refuse_mismatched_pack(K, S):
    t = torch.empty_like(S.act)
    rgb = S.bf.fwd
    # the bf16 dense tap-row pack outside conv_rgb5_bf16's coverage (it used to be read as tap groups)
    _refused(K, ValueError, lambda: K.conv_down(S.img, 3, rgb, S.b, 128, 5, 2, K.EPI_RELU), "tap-row")
    _refused(K, ValueError, lambda: K.conv_down(S.img, 3, rgb, S.b, 128, 5, 2, K.EPI_BIAS, save_t=t), "tap-row")
    _refused(K, ValueError, lambda: K.conv_ex(S.img, 3, S.x6.fwd, S.b, 128, 5, 2, 0, K.EPI_LRELU), "tap-row")
    # conv_up order through conv_down and the reverse
    _refused(K, ValueError, lambda: K.conv_down(S.act, 128, S.fp128.bwd, None, 128, 5, 2), "kind=0.*kind=1")
    _refused(K, ValueError, lambda: K.conv_up(S.act, 128, S.fp128.fwd, None, 128), "kind=1.*kind=0")
    _refused(K, ValueError, lambda: K.conv_up(S.act, 128, S.x128.fwd, None, 128))
    # an x6 / one-plane pack under a description that says fp32
    for p in (S.b1, S.x128.fwd):
        forged = K.Pack(p.data, p.O, p.C, p.KS, p.order, K.PREC_FP32, p.it)
        _refused(K, ValueError, lambda: K.conv_down(S.act, 128, forged, None, 128, p.KS, 1 if p.KS == 3 else 2),
                 "bfloat16")
    # a caller may still state prec / it; a statement the pack contradicts is refused
    _refused(K, ValueError, lambda: K.conv_down(S.act, 128, S.x128.fwd, None, 128, 5, 2, prec=K.PREC_FP32), "stated")
    _refused(K, ValueError, lambda: K.conv_up(S.act, 128, S.fp128.bwd, None, 128, it=6), "stated")
    _refused(K, ValueError, lambda: K.conv_up(S.act, 128, S.x6.bwd, None, 3, prec=K.PREC_BF16), "stated")
    # wrong channel counts / kernel size
    _refused(K, ValueError, lambda: K.conv_down(S.img, 3, S.fp.fwd, None, 192, 5, 2), "O=192.*O=128")
    _refused(K, ValueError, lambda: K.conv_down(S.act, 128, S.fp.fwd, None, 128, 5, 2), "C=128.*C=3")
    _refused(K, ValueError, lambda: K.conv_down(S.act, 128, S.b1, None, 128, 5, 2), "KS=5.*KS=3")
    # the 3-channel conv_up reads the Z-gather pack only, and nothing else reads it
    _refused(K, ValueError, lambda: K.conv_up(S.act, 128, S.up_o3, None, 3), "UP3")
    _refused(K, ValueError, lambda: K.conv_ex(S.act, 128, S.fp.bwd, None, 3, 5, 2, 1), "3 channels")
    # a bare tensor
    _refused(K, TypeError, lambda: K.conv_down(S.img, 3, S.fp.fwd.data, None, 128, 5, 2))
    _refused(K, TypeError, lambda: K.conv_up(S.act, 128, S.fp.bwd.data, None, 3))
    _refused(K, TypeError, lambda: K.conv_ex(S.act, 128, S.b1.data, None, 128, 3, 1))


def _conv_ex_raw(K, x4, wp, Cin, Cout, KS, S, kind, epi, order, bias=None):
    """ica_conv_ex on a hand-filled argument block (pack precision and row tiles, the given order)."""
    from imagecompression_adversarial_amd._lib import ConvArgs, call, ptr, stream
    N, _, H, W, _ = x4.shape
    Ho, Wo = (2 * H, 2 * W) if kind else ((H + S - 1) // S, (W + S - 1) // S)
    y = K.empty_nc4(N, Cout, Ho, Wo, x4.device)
    a = ConvArgs(ptr(x4), ptr(y), ptr(wp.data), ptr(bias), None, None, None, None, None, None, None, None, None,
                 N, Cin, H, W, Cout, Ho, Wo, kind, KS, S, epi, wp.it, 0, 0, wp.prec, 0, order)
    call("ica_conv_ex", ctypes.c_void_p(ctypes.addressof(a)), stream())


def test_library_refuses_wrong_order(K, S):
    cases = [
        (S.img, S.fp.fwd, 3, 128, 5, 2, 0, K.EPI_BIAS, K.ORDER_UP),        # fp32 conv_down, conv_up order
        (S.img, S.fp.fwd, 3, 128, 5, 2, 0, K.EPI_BIAS, K.ORDER_TG),
        (S.act, S.fp128.bwd, 128, 128, 5, 2, 1, K.EPI_BIAS, K.ORDER_DOWN),  # fp32 conv_up, conv_down order
        (S.img, S.bf.fwd, 3, 128, 5, 2, 0, K.EPI_RELU, K.ORDER_RGB5),      # bf16 tap rows, epilogue not covered
        (S.img, S.bf.fwd, 3, 128, 5, 2, 0, K.EPI_BIAS, K.ORDER_DOWN),      # bf16 RGB input: tap groups or tap rows
        (S.img, S.x6.fwd, 3, 128, 5, 2, 0, K.EPI_BIAS, K.ORDER_DOWN),      # x6 RGB input: tap rows only
        (S.act, S.x128.fwd, 128, 128, 5, 2, 0, K.EPI_BIAS, K.ORDER_RGB5),
        (S.act, S.x128.bwd, 128, 128, 5, 2, 1, K.EPI_BIAS, K.ORDER_DOWN),
        (S.act, S.b1, 128, 128, 3, 1, 0, K.EPI_BIAS, K.ORDER_UP),          # one-plane k3 conv_down
        (S.act, S.fp128.fwd, 128, 128, 5, 2, 0, K.EPI_BIAS, K.ORDER_UP3),  # the Z-gather order is never read here
    ]
    for x4, wp, Cin, Cout, KS, St, kind, epi, order in cases:
        _refused(K, RuntimeError, lambda: _conv_ex_raw(K, x4, wp, Cin, Cout, KS, St, kind, epi, order, S.b),
                 "status -4")
    # the same blocks with the pack's own order run
    for x4, wp, Cin, Cout, KS, St, kind in ((S.img, S.fp.fwd, 3, 128, 5, 2, 0), (S.act, S.fp128.bwd, 128, 128, 5, 2, 1),
                                            (S.img, S.x6.fwd, 3, 128, 5, 2, 0), (S.act, S.b1, 128, 128, 3, 1, 0)):
        K.last_launch()
        _conv_ex_raw(K, x4, wp, Cin, Cout, KS, St, kind, K.EPI_BIAS, wp.order, S.b)
        assert K.last_launch() is not None
    torch.cuda.synchronize()
