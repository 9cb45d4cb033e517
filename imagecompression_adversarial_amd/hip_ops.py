"""Typed host wrappers over the C ABI (torch tensors in, torch tensors out).

Internal activation layout is nChw4c, stored as a torch tensor of shape
[N, ceil(C/4), H, W, 4] (fp32, contiguous); the logical channel count travels
with it.  All launches go on torch's current HIP stream.
"""
from __future__ import annotations

import math

import torch

from ._lib import ConvArgs, LayerDesc, call, lib, ptr, stream

EPI_BIAS, EPI_RELU, EPI_GDN, EPI_IGDN, EPI_GDN_BWD, EPI_IGDN_BWD, EPI_LRELU, EPI_LRELU_BWD = range(8)
FILL_PLAIN, FILL_LRELU_MASK, FILL_UNSHUFFLE = range(3)
# fragment orders of a packed weight (include/ica_hip.h ICA_ORDER_*): every layout a kernel reads has its own
ORDER_DOWN, ORDER_UP = 0, 1
ORDER_RGB5 = 2   # dense tap-row pack of a k5 conv_down with <= 3 input channels (bf16 and x6)
ORDER_TG = 3     # bf16 4-tap groups of a conv_down with <= 4 input channels
ORDER_UP3 = 4    # Z-gather pack of the conv_up to 3 channels (ica_conv_up3*)
_ORDER_NAME = ("DOWN", "UP", "RGB5", "TG", "UP3")
# parity-split tensors of an x6 k5 s2 launch (ica_conv_args.layout): the input x, the output-layout tensors
LAYOUT_IN, LAYOUT_OUT = 1, 2
GDN_BETA_BOUND = float((1e-6 + 2.0 ** -36) ** 0.5)  # NonNegativeParametrizer bound (utils/ops.py:67)


# Optional per-launch timing hook used by bench.py: {tag: [(ev0, ev1), ...]}.
# When set, every tagged conv launch is bracketed by HIP events recorded on
# the current stream (the stream the kernel runs on); no synchronisation.
EVENT_HOOK = None


def _ev_begin(tag, n):
    if EVENT_HOOK is None or tag is None:
        return None
    if LAUNCH_HOOK is not None:
        last_launch()   # consume the launch record: _ev_end sees only this tag's launches
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return (tag, e0, n)


def _ev_end(h, flops=None):
    """EVENT_HOOK[tag] gets (start event, end event, images in the launch)."""
    if h is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        EVENT_HOOK.setdefault(h[0], []).append((h[1], e1, h[2]))
        if flops is not None:
            FLOPS_HOOK[h[0]] = flops / max(h[2], 1)
        if LAUNCH_HOOK is not None:
            LAUNCH_HOOK.setdefault(h[0], set()).add(last_launch())


# kernels behind each tagged launch (filled while EVENT_HOOK and LAUNCH_HOOK are set): {tag: {(kernel, threads)}}
LAUNCH_HOOK = None


def source_hash() -> str:
    """sha256 (first 16 hex digits) of the HIP sources the library is built from (csrc/*.hip, *.h, in name order):
    the revision stamp of a PMC traffic measurement."""
    import glob
    import hashlib
    import os
    h = hashlib.sha256()
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.h"))):
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def last_launch():
    """(demangled kernel name, grid size in threads) of this thread's only kernel launch since the previous call
    (ica_last_launch, which consumes the record): the names and Grid_Size that rocprofv3 reports for the same
    dispatch.  None when there was no launch, ("<N launches>", 0) when there were several (no stamp matches that)."""
    import ctypes as C
    buf = C.create_string_buffer(512)
    thr = C.c_ulonglong(0)
    n = lib().ica_last_launch(buf, 512, C.byref(thr))
    if n <= 0:
        return None
    if n > 1:
        return f"<{n} launches>", 0
    return buf.value.decode(errors="replace"), int(thr.value)


X6_TILING_AUTO, X6_TILING_PREVIOUS, X6_TILING_BALANCED = 0, 1, 2


def x6_tiling(mode: int = X6_TILING_AUTO) -> None:
    """Which tiling the x6 k5 s2 pickers take (ica_x6_tiling; process-wide, for tests and A/B runs): AUTO = their own
    choice from the grid; PREVIOUS = the large-grid kernel a layer ran before it had a second one (conv_down: 8 x 32
    blocks, conv_up: PT = 1 with forward layers on four waves); BALANCED = the newer one wherever a layer has it
    (conv_down 128 -> 192: 4 x 48 blocks over both channel blocks; conv_up forward from 192 channels: eight waves).
    Both also skip the small-grid kernels.  The large-grid kernels of a layer give the same bits as each other; the
    small-grid kernels sum in another order, so on maps of <= 32 x 32 pixels PREVIOUS / BALANCED match AUTO to fp32
    rounding, not bit for bit.  Nothing in the package sets it: leave it at AUTO outside tests."""
    call("ica_x6_tiling", int(mode))


# operand precision of each tagged conv launch (filled while EVENT_HOOK is set): what actually ran, small-grid
# fp32 fallbacks of x6 layers included
PREC_HOOK = {}


_PREC_SUFFIX = {0: "fp32", 1: "bf16", 2: "x6", 3: "b1"}   # PREC_FP32, PREC_BF16, PREC_X6, PREC_B1


def _prec_note(tag, prec):
    """Record the operands a tagged launch runs on; returns the tag to time it under: a tag first seen with other
    operands (e.g. the fine-tune's fp32 train step next to its x6 inner attack) is timed as 'tag[fp32]'."""
    if EVENT_HOOK is None or tag is None:
        return tag
    first = PREC_HOOK.setdefault(tag, prec)
    if first != prec:
        tag = f"{tag}[{_PREC_SUFFIX.get(prec, prec)}]"
        PREC_HOOK.setdefault(tag, prec)
    return tag


# algorithmic FLOPs PER IMAGE of each tagged ica_conv_ex launch (filled while EVENT_HOOK is set): 2*MAC of the
# conv (a transposed conv counts the MACs of the conv it differentiates) + the GDN channel GEMM if fused
FLOPS_HOOK = {}


def _dev_check(t: torch.Tensor, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a HIP device tensor (no CPU fallback on the hot path)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def check_image(x, name, dev=True):
    """(B, H, W) of a planar [B, 3, H, W] batch: ValueError for anything else, then _dev_check (dev=False leaves the
    tensor checks to a caller that orders them itself)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1:
        shape = tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"{name} {shape} is not a [B, 3, H, W] batch")
    if dev:
        _dev_check(x, name)
    return x.shape[0], x.shape[2], x.shape[3]


def check_nc4(x, name):
    """(B, H, W) of a 3-channel nChw4c batch [B, 1, H, W, 4], checked like check_image."""
    if x.dim() != 5 or x.shape[1] != 1 or x.shape[4] != 4 or x.shape[0] < 1:
        raise ValueError(f"{name} {tuple(x.shape)} is not a 3-channel nChw4c batch [B, 1, H, W, 4]")
    _dev_check(x, name)
    return x.shape[0], x.shape[2], x.shape[3]


def positive_int(name, v):
    if not isinstance(v, int) or isinstance(v, bool) or v < 1:
        raise ValueError(f"{name} must be a positive int, got {v!r}")


def c4(C: int) -> int:
    return (C + 3) // 4


def empty_nc4(N, C, H, W, device, dtype=torch.float32):
    return torch.empty((N, c4(C), H, W, 4), dtype=dtype, device=device)


def cast_nc4(x4: torch.Tensor, dtype) -> torch.Tensor:
    """fp32 <-> bf16 copy of an nChw4c tensor (the ends of the bf16 conv path) on the HIP cast kernels."""
    if x4.dtype == dtype:
        return x4
    if not x4.is_cuda or not x4.is_contiguous():
        raise RuntimeError("cast_nc4 needs a contiguous HIP tensor")
    y = torch.empty(x4.shape, dtype=dtype, device=x4.device)
    if dtype == torch.bfloat16 and x4.dtype == torch.float32:
        call("ica_cast_f32_bf16", ptr(x4), ptr(y), x4.numel(), stream())
    elif dtype == torch.float32 and x4.dtype == torch.bfloat16:
        call("ica_cast_bf16_f32", ptr(x4), ptr(y), x4.numel(), stream())
    else:
        raise RuntimeError(f"cast_nc4 {x4.dtype} -> {dtype}")
    return y


def to_nc4(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    _dev_check(x, "x")
    N, C, H, W = x.shape
    y = empty_nc4(N, C, H, W, x.device)
    call("ica_nchw_to_nc4", ptr(x), ptr(y), N, C, H, W, stream())
    return y


def from_nc4(x4: torch.Tensor, C: int) -> torch.Tensor:
    _dev_check(x4, "x4")
    N, _, H, W, _ = x4.shape
    y = torch.empty((N, C, H, W), dtype=torch.float32, device=x4.device)
    call("ica_nc4_to_nchw", ptr(x4), ptr(y), N, C, H, W, stream())
    return y


# --------------------------------------------------------------------------- #
# Weight packing
# --------------------------------------------------------------------------- #
PREC_FP32, PREC_BF16, PREC_X6 = 0, 1, 2
# bf16 operands over fp32 activations: the k3 conv_downs (cheng2020 --precision bf16) on the hi plane of the x6 pack
# (RNE bf16 of activations and weights, fp32 accumulate, fp32 tensors; GDN epilogue GEMMs on the x6 gamma' pack)
PREC_B1 = 3


def x6_it(O: int) -> int:
    """Row tiles per wave the library uses by default for O output channels (4 for 128 channels, 3 for 192)."""
    return int(lib().ica_conv_it(O))


class Pack:
    """Packed weight fragments and what they are: W[O][C][KS][KS] in fragment order `order` (ORDER_*), operands
    `prec` (PREC_*), `it` row tiles per wave (resolved, > 0), taps reversed if `flip`.  kind: the launch that reads
    it (0 conv_down, 1 conv_up; ORDER_UP3 is the conv_up to 3 channels).  The launch wrappers take prec and it from
    here and refuse a launch whose geometry or kind differs."""
    __slots__ = ("data", "O", "C", "KS", "kind", "order", "prec", "it", "flip")

    def __init__(self, data, O, C, KS, order, prec=PREC_FP32, it=0, flip=False):
        self.data, self.O, self.C, self.KS = data, int(O), int(C), int(KS)
        self.order, self.prec, self.flip = int(order), int(prec), bool(flip)
        self.kind = 1 if order in (ORDER_UP, ORDER_UP3) else 0
        self.it = int(it) if it > 0 else x6_it(O)

    def __repr__(self):
        return (f"Pack(O={self.O}, C={self.C}, KS={self.KS}, kind={self.kind}, order={_ORDER_NAME[self.order]}, "
                f"prec={_PREC_SUFFIX[self.prec]}, it={self.it}, flip={self.flip})")


def _weight(w):
    w = w.detach().contiguous()
    _dev_check(w, "weight")
    return w


def pack_conv(w: torch.Tensor, O: int, Cc: int, KS: int, so: int, sc: int, order: int, CC: int,
              flip: bool = False, it: int = 0) -> Pack:
    """Pack a conv weight viewed as W[o][c][ky][kx] (strides so, sc; k contiguous); flip reverses the taps;
    it = 32-channel row tiles per wave (0: the library default for O)."""
    w = _weight(w)
    n = int(lib().ica_pack_conv_weight_size(O, Cc, KS, CC, it))
    dst = torch.empty(n, dtype=torch.float32, device=w.device)
    call("ica_pack_conv_weight", ptr(w), ptr(dst), O, Cc, KS, so, sc, CC, order, int(flip), it, stream())
    return Pack(dst, O, Cc, KS, order, PREC_FP32, it, flip)


def pack_conv_bf16(w: torch.Tensor, O: int, Cc: int, KS: int, so: int, sc: int, order: int, flip: bool = False,
                   it: int = 0) -> Pack:
    """bf16 fragments (PREC_BF16 launches): the CC=16 fp32 fragment order, each element rounded to bf16.  Cc <= 4
    with ORDER_DOWN writes the 4-tap groups of an RGB conv input: that pack is ORDER_TG."""
    w = _weight(w)
    n = int(lib().ica_pack_conv_weight_bf16_size(O, Cc, KS, it))
    dst = torch.empty(n, dtype=torch.bfloat16, device=w.device)
    call("ica_pack_conv_weight_bf16", ptr(w), ptr(dst), O, Cc, KS, so, sc, order, int(flip), it, stream())
    return Pack(dst, O, Cc, KS, ORDER_TG if (Cc <= 4 and order == ORDER_DOWN) else order, PREC_BF16, it, flip)


def pack_conv_x6(w: torch.Tensor, O: int, Cc: int, KS: int, so: int, sc: int, order: int, it: int,
                 prec: int = PREC_X6, flip: bool = False) -> Pack:
    """fp32-accurate bf16x6 fragments (PREC_X6 launches, ica_conv_x6.hip): three bf16 planes (hi, mid, lo: an exact
    split of each weight) of the CC=16 fragment order.  prec=PREC_B1: the same bytes, launched on the hi plane
    only.  flip packs the weight with its taps reversed."""
    w = _weight(w.flip(-1, -2) if flip else w)
    n = int(lib().ica_pack_conv_weight_x6_size(O, Cc, KS, it))
    dst = torch.empty(n, dtype=torch.bfloat16, device=w.device)
    call("ica_pack_conv_weight_x6", ptr(w), ptr(dst), O, Cc, KS, so, sc, order, it, stream())
    return Pack(dst, O, Cc, KS, order, prec, it, flip)


def x6_ok(O: int, C: int, it: int, kind: int) -> bool:
    """Whether PackedConv packs a k5 s2 launch with O output / C input channels for ica_conv_x6_dispatch
    (ica_conv_x6.hip): kind 0 (conv_down): C >= 16, a multiple of 16; O = 128-multiples (IT 4: bias, GDN, IGDN_BWD)
    or 96-multiples (IT 3: bias only -- the only IT 3 conv_downs, g_a.6 forward and the g_s.0 input gradient, have
    no epilogue); kind 1 (conv_up): IT 4 only (O a 128-multiple) with C = 64, 128 or a 64-multiple.  No explicit-IT
    (C = 192 GDN) launch.  Anything else keeps the fp32 pack.  This only chooses the pack: the launch carries the
    pack's order and precision, and the library rejects (-4) a pack its route does not read."""
    if it != 0 or C < 16 or C % 16:
        return False
    if kind == 0:
        return O % 128 == 0 or O % 96 == 0
    return O % 128 == 0 and (C in (64, 128) or C % 64 == 0)


def conv_cc(Cin: int) -> int:
    return 4 if Cin <= 4 else 16


def pack_up3(w_view: torch.Tensor, prec: int = 0) -> Pack:
    """Fragments for conv_up3 from a [Cin][3][5][5] transposed-conv weight view (prec 1: bf16, 2: x6)."""
    w = _weight(w_view)
    Cin = w.shape[0]
    n = int(lib().ica_pack_up3_size(Cin))
    if prec == PREC_FP32:
        dst = torch.empty(n, device=w.device)
    else:
        dst = torch.empty(3 * n if prec == PREC_X6 else n, dtype=torch.bfloat16, device=w.device)
    call("ica_pack_up3", ptr(w), ptr(dst), Cin, int(prec), stream())
    return Pack(dst, 3, Cin, 5, ORDER_UP3, prec)


def _pack_down(w, O, C, KS, S, so, sc, it, prec) -> Pack:
    """The pack of a conv_down launch (a conv's forward, a deconv's input gradient).  k5 s2 under PREC_BF16: bf16
    fragments (16-channel chunks, 4-tap groups for <= 4 input channels); under PREC_X6: x6 fragments where x6_ok.
    An RGB-sized input into 128 channels gets the dense tap-row pack (conv_rgb5_bf16 / conv_rgb5_x6: the 75 (tap,
    channel) pairs in 5 K steps).  Everything else, explicit 6-tile x6 layers included, is fp32."""
    if KS == 5 and S == 2:
        rgb5 = C <= 3 and O == 128
        if prec == PREC_BF16 and (C >= 16 or C <= 4):
            return pack_conv_bf16(w, O, C, 5, so, sc, ORDER_RGB5 if rgb5 and it in (0, 4) else ORDER_DOWN, it=it)
        if prec == PREC_X6 and rgb5 and it == 0:
            return pack_conv_x6(w, O, C, 5, so, sc, ORDER_RGB5, 4)
        if prec == PREC_X6 and x6_ok(O, C, it, 0):
            return pack_conv_x6(w, O, C, 5, so, sc, ORDER_DOWN, x6_it(O))
    return pack_conv(w, O, C, KS, so, sc, ORDER_DOWN, conv_cc(C), it=it)


def _pack_up(w, O, C, KS, S, so, sc, it, prec) -> Pack:
    """The pack of a conv_up launch (a deconv's forward, a k5 s2 conv's input gradient; w viewed [C][O][k][k]):
    the Z-gather pack for 3 output channels, else as _pack_down."""
    if O == 3 and KS == 5:
        return pack_up3(w, prec)
    if KS == 5 and prec == PREC_BF16:
        return pack_conv_bf16(w, O, C, 5, so, sc, ORDER_UP, it=it)
    if KS == 5 and S == 2 and prec == PREC_X6 and x6_ok(O, C, it, 1):
        return pack_conv_x6(w, O, C, 5, so, sc, ORDER_UP, x6_it(O))
    return pack_conv(w, O, C, KS, so, sc, ORDER_UP, 16, it=it)


class PackedConv:
    """Packed fragments for one conv layer, for both its forward and its dgrad.

    kind 'conv'   : nn.Conv2d weight [Cout][Cin][k][k]   fwd = conv_down, dgrad = conv_up
    kind 'deconv' : nn.ConvTranspose2d weight [Cin][Cout][k][k]  fwd = conv_up, dgrad = conv_down
    """

    def __init__(self, weight: torch.Tensor, bias, kind: str, stride: int, prec: int = PREC_FP32,
                 it_fwd: int = 0, it_bwd: int = 0):
        """prec=PREC_BF16 / PREC_X6 packs the k5 s2 layers as bf16 / x6 fragments where a kernel reads them
        (_pack_down / _pack_up); fwd_prec / bwd_prec are what each pack is.
        it_fwd / it_bwd: 32-channel row tiles per wave of the forward / input-gradient launches (0 = the library
        default; 6 for the C = 192 GDN layers of bmshj2018 q6-8, whose epilogue needs all channels in one wave; the
        bf16 path has IT = 6 kernels for those GDN / IGDN layers and their input gradients too)."""
        self.kind, self.stride = kind, stride
        self.KS = KS = weight.shape[-1]
        KK = KS * KS
        if kind == "conv":
            self.Cout, self.Cin = Co, Ci = weight.shape[0], weight.shape[1]
            self.fwd = _pack_down(weight, Co, Ci, KS, stride, Ci * KK, KK, it_fwd, prec)   # o = co, c = ci
            # dgrad: k5 s2 -> conv_up (o = ci, c = co); k3 s1 -> conv_down with the taps reversed
            self.bwd = None
            if KS == 3 and stride == 1 and Co % 16 == 0:
                self.bwd = pack_conv(weight, Ci, Co, 3, KK, Ci * KK, ORDER_DOWN, conv_cc(Co), flip=True)
            elif KS == 5 and stride == 2 and Co % 16 == 0:
                self.bwd = _pack_up(weight, Ci, Co, 5, 2, KK, Ci * KK, it_bwd, prec)
        elif kind == "deconv":
            self.Cin, self.Cout = Ci, Co = weight.shape[0], weight.shape[1]
            self.fwd = _pack_up(weight, Co, Ci, KS, stride, KK, Co * KK, it_fwd, prec)     # o = co, c = ci
            self.bwd = _pack_down(weight, Ci, Co, KS, stride, Co * KK, KK, it_bwd, prec)   # o = ci, c = co
        else:
            raise ValueError(kind)
        self.bias = None if bias is None else bias.detach().contiguous()

    fwd_prec = property(lambda self: self.fwd.prec)
    bwd_prec = property(lambda self: PREC_FP32 if self.bwd is None else self.bwd.prec)
    it_fwd = property(lambda self: self.fwd.it)
    it_bwd = property(lambda self: 0 if self.bwd is None else self.bwd.it)


class PackedGDN:
    def __init__(self, beta: torch.Tensor, gamma: torch.Tensor):
        C = beta.shape[0]
        self.C = C
        T = C // 32
        dev = beta.device
        beta = beta.detach().contiguous()
        gamma = gamma.detach().reshape(C, C).contiguous()
        self.gp = torch.empty(T * T * 64 * 16, device=dev)
        self.gpT = torch.empty(T * T * 64 * 16, device=dev)
        self.beta = torch.empty(C, device=dev)
        call("ica_pack_gdn", ptr(gamma), ptr(beta), ptr(self.gp), ptr(self.beta), C, 0, GDN_BETA_BOUND, stream())
        call("ica_pack_gdn", ptr(gamma), ptr(beta), ptr(self.gpT), ptr(self.beta), C, 1, GDN_BETA_BOUND, stream())
        self._src = (gamma, beta)
        self.gpb = self.gpbT = None
        self.gpx = self.gpxT = None

    def x6(self):
        """Three-plane bf16 splits of gamma' / gamma'^T for prec=2 epilogues (built once, on first use)."""
        if self.gpx is None:
            n = int(lib().ica_pack_gdn_x6_size(self.C))
            self.gpx = torch.empty(n // 2, dtype=torch.bfloat16, device=self.gp.device)
            self.gpxT = torch.empty_like(self.gpx)
            call("ica_pack_gdn_x6", ptr(self.gp), ptr(self.gpx), self.C, stream())
            call("ica_pack_gdn_x6", ptr(self.gpT), ptr(self.gpxT), self.C, stream())
        return self

    def bf16(self):
        """bf16x3 hi/lo fragments of gamma' / gamma'^T for prec=1 epilogues (built once, on first use)."""
        if self.gpb is None:
            gamma, beta = self._src
            T = self.C // 32
            self.gpb = torch.empty(T * T * 2048, dtype=torch.bfloat16, device=gamma.device)
            self.gpbT = torch.empty_like(self.gpb)
            call("ica_pack_gdn_bf16", ptr(gamma), ptr(beta), ptr(self.gpb), ptr(self.beta), self.C, 0,
                 GDN_BETA_BOUND, stream())
            call("ica_pack_gdn_bf16", ptr(gamma), ptr(beta), ptr(self.gpbT), ptr(self.beta), self.C, 1,
                 GDN_BETA_BOUND, stream())
        return self


# --------------------------------------------------------------------------- #
# Convolutions
# --------------------------------------------------------------------------- #
def _out_hw(H, W, KS, S, kind):
    if kind == 0:
        return (H + 2 * (KS // 2) - KS) // S + 1, (W + 2 * (KS // 2) - KS) // S + 1
    return 2 * H, 2 * W


def _check_pack(wp, Cin, Cout, KS, kind, prec=None, it=0):
    """A launch runs only on a pack that says it is that launch's weight.  prec / it: what a caller still states
    about the pack (nothing has to); a statement the pack contradicts is refused like any other mismatch."""
    if not isinstance(wp, Pack):
        raise TypeError(f"conv launch: wp must be a hip_ops.Pack (from a packer or a PackedConv), not "
                        f"{type(wp).__name__}")
    if (wp.O, wp.C, wp.KS, wp.kind) != (Cout, Cin, KS, kind):
        raise ValueError(f"conv launch (O={Cout}, C={Cin}, KS={KS}, kind={kind}) on {wp!r}")
    if (wp.data.dtype == torch.float32) != (wp.prec == PREC_FP32):
        raise ValueError(f"{wp!r} holds {wp.data.dtype} fragments")
    if (prec is not None and prec != wp.prec) or (it and it != wp.it):
        raise ValueError(f"conv launch stated prec={prec}, it={it} for {wp!r}")


def _conv3(x4, Cin, wp, bias, Cout, KS, S, kind, epi, gdn, save, saved, out, tag, save_t, layout, prec, it):
    """conv_down / conv_up through conv_ex: allocates save_s, returns (y4, save_x, save_s)."""
    _check_pack(wp, Cin, Cout, KS, kind, prec, it)
    ss = None
    if save and epi in (EPI_GDN, EPI_IGDN):
        # backward needs (y, s): y = x*s is this layer's output (kept alive anyway as the next
        # layer's input), so only s is written; the bwd epilogue recovers x = y / s.
        N, _, H, W, _ = x4.shape
        ss = empty_nc4(N, Cout, *_out_hw(H, W, KS, S, kind), x4.device,
                       torch.bfloat16 if wp.prec == PREC_BF16 else torch.float32)
    y = conv_ex(x4, Cin, wp, bias, Cout, KS, S, kind, epi, gdn, save_s=ss, saved=saved, save_t=save_t, out=out,
                tag=tag, layout=layout, _flops=False)
    return y, (y if ss is not None else None), ss


def conv_down(x4, Cin, wp: Pack, bias, Cout, KS, S, epi=EPI_BIAS, gdn: PackedGDN | None = None, save=False,
              saved=None, out=None, tag=None, save_t=None, layout=0, prec=None, it=0):
    """y = conv2d(x, W, stride S, pad KS//2) (+epilogue).  Returns (y4, save_x, save_s).  Operand precision and
    row tiles are the pack's (prec / it, if a caller states them, are only checked against it).
    save_t: optional nChw4c output of t = dL/dn for the GDN-bwd epilogues (GDN parameter gradients).
    layout: parity-split tensors (LAYOUT_IN: x, LAYOUT_OUT: y and the saved / output-layout tensors; x6 only)."""
    return _conv3(x4, Cin, wp, bias, Cout, KS, S, 0, epi, gdn, save, saved, out, tag, save_t, layout, prec, it)


def conv_up(x4, Cin, wp: Pack, bias, Cout, epi=EPI_BIAS, gdn: PackedGDN | None = None, save=False, saved=None,
            out=None, tag=None, save_t=None, layout=0, prec=None, it=0):
    """y = conv_transpose2d(x, W, stride 2, pad 2, output_padding 1) (+epilogue).  layout: as conv_down (the
    3-channel output of conv_up3 is always row-major)."""
    if Cout != 3:
        return _conv3(x4, Cin, wp, bias, Cout, 5, 2, 1, epi, gdn, save, saved, out, tag, save_t, layout, prec, it)
    _check_pack(wp, Cin, 3, 5, 1, prec, it)
    if wp.order != ORDER_UP3:
        raise ValueError(f"conv_up to 3 channels reads the Z-gather pack (ORDER_UP3), not {wp!r}")
    if epi != EPI_BIAS:
        raise RuntimeError("conv_up to 3 channels supports the bias epilogue only")
    N, _, H, W, _ = x4.shape
    y = out if out is not None else empty_nc4(N, 3, 2 * H, 2 * W, x4.device)
    ev = _ev_begin(_prec_note(tag, wp.prec), N)
    call("ica_conv_up3", ptr(x4), ptr(y), ptr(wp.data), ptr(bias), N, Cin, H, W, int(layout), int(wp.prec), stream())
    _ev_end(ev)
    return y, None, None


def conv_ex(x4, Cin, wp: Pack, bias, Cout, KS, S, kind=0, epi=EPI_BIAS, gdn: PackedGDN | None = None, res=None,
            save_x=None, save_s=None, saved=None, save_t=None, mask=None, fill_mode=FILL_PLAIN, ps=False,
            out=None, tag=None, alg_rows=None, layout=0, prec=None, it=0, _flops=True):
    """The conv launch (ica_conv_ex).  kind 0: conv2d(x, W, stride S, pad KS//2); kind 1: the stride-2
    transposed conv (dgrad of a stride-2 conv).  Operand precision, row tiles and fragment order are the pack's;
    a pack of another geometry or kind is refused (ValueError) before anything is launched.  fill_mode 2 views x
    ([N, Cin/16, 2H, 2W, 4]) as the PixelUnshuffle(2) tensor [N, Cin/4, H, W, 4] in rho order; ps stores
    PixelShuffle(2) of the rho-ordered Cout rows (y: [N, Cout/16, 2Ho, 2Wo, 4]).  save_x / save_s / save_t:
    caller-allocated outputs."""
    _check_pack(wp, Cin, Cout, KS, kind, prec, it)
    if wp.order == ORDER_UP3:
        raise ValueError(f"{wp!r} is launched by conv_up to 3 channels only")
    if wp.order == ORDER_RGB5 and (epi not in (EPI_BIAS, EPI_GDN, EPI_IGDN_BWD) or fill_mode != FILL_PLAIN or ps
                                   or any(t is not None for t in (res, save_x, save_t, mask))):
        raise ValueError(f"{wp!r}: the dense tap-row pack is read by conv_rgb5 only (bias / GDN / IGDN_BWD epilogue, "
                         f"plain fill, no extra tensors)")
    prec = wp.prec
    N, C4x, H, W, _ = x4.shape
    if fill_mode == FILL_UNSHUFFLE:
        if Cin != 16 * C4x:
            raise RuntimeError("unshuffled conv input: Cin must be 16 * input channel groups")
        H, W = H // 2, W // 2
    Ho, Wo = _out_hw(H, W, KS, S, kind)
    dt = torch.bfloat16 if prec == PREC_BF16 else torch.float32   # bf16 path: bf16 activations
    if out is not None:
        y = out
    elif ps:
        y = torch.empty((N, Cout // 16, 2 * Ho, 2 * Wo, 4), dtype=dt, device=x4.device)
    else:
        y = empty_nc4(N, Cout, Ho, Wo, x4.device, dt)
    in_x = in_s = None
    if saved is not None:
        in_x, in_s = saved
    gp = None
    if gdn is not None:
        if prec == PREC_BF16:
            gdn.bf16()
            gp = gdn.gpbT if epi in (EPI_GDN_BWD, EPI_IGDN_BWD) else gdn.gpb
        elif prec in (PREC_X6, PREC_B1):   # x6 epilogue GEMMs (k5 s2 and, since round 4, the k3 s1 conv_downs)
            gdn.x6()
            gp = gdn.gpxT if epi in (EPI_GDN_BWD, EPI_IGDN_BWD) else gdn.gpx
        else:   # fp32 epilogues (fp32 operands)
            gp = gdn.gpT if epi in (EPI_GDN_BWD, EPI_IGDN_BWD) else gdn.gp
    a = ConvArgs(ptr(x4), ptr(y), ptr(wp.data), ptr(bias), ptr(gp), ptr(None if gdn is None else gdn.beta),
                 ptr(save_x), ptr(save_s), ptr(in_x), ptr(in_s), ptr(save_t), ptr(res), ptr(mask), N, Cin, H, W, Cout,
                 Ho, Wo, kind, KS, S, epi, wp.it, fill_mode, int(bool(ps)), prec, int(layout), wp.order)
    import ctypes
    tag = _prec_note(tag, prec)
    ev = _ev_begin(tag, N)
    call("ica_conv_ex", ctypes.c_void_p(ctypes.addressof(a)), stream())
    if ev is not None:
        fl = None
        if _flops:   # direct conv_ex calls only (bench.py takes the bmshj2018 layers' FLOPs from its own table)
            px = N * (H * W if kind == 1 else Ho * Wo)
            # alg_rows: real (non-padding) rows of a rho-ordered subpel weight (4 * C)
            cin_alg = alg_rows if (fill_mode == FILL_UNSHUFFLE and alg_rows) else Cin
            cout_alg = alg_rows if (ps and alg_rows) else Cout
            fl = 2.0 * cin_alg * cout_alg * KS * KS * px
            if epi in (EPI_GDN, EPI_IGDN, EPI_GDN_BWD, EPI_IGDN_BWD):
                fl += 2.0 * Cout * Cout * N * Ho * Wo
        _ev_end(ev, fl)
    return y


def pack_up3k3_x6(w1: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """Fragments of conv_up3k3_x6 (three bf16 planes) from the conv1 [Cg][3][3][3] and skip [Cg][3][1][1] weights of
    cheng2020's g_a.0 (ResidualBlockWithStride(3, N))."""
    w1, ws = w1.detach().contiguous(), ws.detach().contiguous()
    _dev_check(w1, "weight")
    _dev_check(ws, "weight")
    Cg = w1.shape[0]
    if tuple(w1.shape) != (Cg, 3, 3, 3) or tuple(ws.shape) != (Cg, 3, 1, 1):
        raise RuntimeError("pack_up3k3_x6: conv1 [Cg][3][3][3] and skip [Cg][3][1][1] weights")
    dst = torch.empty(int(lib().ica_pack_up3k3_x6_size(Cg)) // 2, dtype=torch.bfloat16, device=w1.device)
    call("ica_pack_up3k3_x6", ptr(w1), ptr(ws), ptr(dst), Cg, stream())
    return dst


def conv_up3k3_x6(g1: torch.Tensor, gs: torch.Tensor, wp: torch.Tensor, Hout: int, Wout: int, tag=None):
    """dx = conv3x3_s2^T(g1) + conv1x1_s2^T(gs) for a 3-channel input (x6 operands, one pass; ica_conv_up3k3_x6).
    g1, gs: nChw4c [N][Cg/4][H][W][4] row-major; returns dx [N][1][Hout][Wout][4]."""
    for t, nm in ((g1, "g1"), (gs, "gs")):
        _dev_check(t, nm)
        if not t.is_contiguous() or t.dtype != torch.float32:
            raise RuntimeError(f"conv_up3k3_x6: {nm} must be contiguous fp32 nChw4c")
    if g1.shape != gs.shape:
        raise RuntimeError("conv_up3k3_x6: g1 and gs shapes differ")
    N, C4, H, W, _ = g1.shape
    dx = empty_nc4(N, 3, Hout, Wout, g1.device)
    ev = _ev_begin(tag, N)
    call("ica_conv_up3k3_x6", ptr(g1), ptr(gs), ptr(wp), ptr(dx), N, 4 * C4, H, W, Hout, Wout, stream())
    _ev_end(ev, 2.0 * 4 * C4 * 3 * (9 + 1) * N * H * W)
    return dx


# --------------------------------------------------------------------------- #
# Reductions / elementwise
# --------------------------------------------------------------------------- #
def blocks_per_image() -> int:
    return int(lib().ica_elem_blocks_per_image())


def reduce_rows(part: torch.Tensor, B: int, scale: float = 1.0, out=None):
    nblk = part.numel() // B
    o = out if out is not None else torch.empty(B, device=part.device)
    call("ica_reduce_rows", ptr(part), ptr(o), B, nblk, float(scale), stream())
    return o


def abs_(x: torch.Tensor) -> torch.Tensor:
    y = torch.empty_like(x)
    call("ica_abs", ptr(x), ptr(y), x.numel(), stream())
    return y


def round_(x: torch.Tensor) -> torch.Tensor:
    y = torch.empty_like(x)
    call("ica_round", ptr(x), ptr(y), x.numel(), stream())
    return y


def clamp01(x: torch.Tensor) -> torch.Tensor:
    y = torch.empty_like(x)
    call("ica_clamp01", ptr(x), ptr(y), x.numel(), stream())
    return y


def sqdiff_mean(a: torch.Tensor, b: torch.Tensor, clamp_a=False) -> torch.Tensor:
    """Per-image mean((clamp?(a) - b)^2) over the trailing dims (deterministic)."""
    B = a.shape[0]
    length = a[0].numel()
    part = torch.empty(B * blocks_per_image(), device=a.device)
    call("ica_sqdiff_partial", ptr(a.contiguous()), ptr(b.contiguous()), ptr(part), B, length, int(clamp_a), stream())
    return reduce_rows(part, B, 1.0 / length)


class PackedEB:
    NAMES = ([f"_matrix{i}" for i in range(5)] + [f"_bias{i}" for i in range(5)]
             + [f"_factor{i}" for i in range(4)] + ["quantiles"])

    def __init__(self, tensors: dict):
        import ctypes as C
        ts = [tensors[n].detach().contiguous() for n in self.NAMES]
        for t in ts:
            _dev_check(t, "entropy_bottleneck param")
        self.C = ts[-1].shape[0]
        dev = ts[0].device
        self.prm = torch.empty(self.C * 58, device=dev)
        self.med = torch.empty(self.C, device=dev)
        arr = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        self._keep = ts
        # the host array of device pointers is consumed synchronously by the launcher
        call("ica_pack_eb", C.cast(arr, C.c_void_p), ptr(self.prm), ptr(self.med), self.C, stream())


def eb_likelihood(z4: torch.Tensor, C: int, eb: PackedEB, training=False, qnoise4=None):
    """EntropyBottleneck forward on nc4 z: returns (z_hat4, lik4, per-image sum log lik)."""
    N, _, H, W, _ = z4.shape
    zh = torch.empty_like(z4)
    lik = torch.empty_like(z4)
    part = torch.empty(N * blocks_per_image(), device=z4.device)
    call("ica_eb_likelihood", ptr(z4), ptr(eb.prm), ptr(eb.med), ptr(qnoise4), ptr(zh), ptr(lik), ptr(part), N, C, H,
         W, int(training), stream())
    return zh, lik, reduce_rows(part, N)


def gc_likelihood(y4: torch.Tensor, C: int, scales4: torch.Tensor, means4=None, training=False, qnoise4=None):
    N, _, H, W, _ = y4.shape
    yh = torch.empty_like(y4)
    lik = torch.empty_like(y4)
    part = torch.empty(N * blocks_per_image(), device=y4.device)
    call("ica_gc_likelihood", ptr(y4), ptr(scales4), ptr(means4), ptr(qnoise4), ptr(yh), ptr(lik), ptr(part), N, C,
         H, W, int(training), stream())
    return yh, lik, reduce_rows(part, N)


def bits_to_bpp(sumlog: torch.Tensor, num_pixels: int) -> torch.Tensor:
    return sumlog / (-math.log(2) * num_pixels)


# --------------------------------------------------------------------------- #
# Bitrate attack: value gradients of the entropy models (ica_rate.hip)
# --------------------------------------------------------------------------- #
def _check_latent(x4, C, name):
    _dev_check(x4, name)
    if x4.dim() != 5 or x4.shape[4] != 4 or x4.shape[1] != c4(C):
        raise ValueError(f"{name} {tuple(x4.shape)} is not an nChw4c tensor of {C} channels")
    return x4.shape[0], x4.shape[2], x4.shape[3]


def rate_gc(y4: torch.Tensor, C: int, sigma4: torch.Tensor, scale: float):
    """L = scale * sum ln lik of the zero-noise train-mode GaussianConditional on the unrounded y (scale > 0):
    (dL/dy, dL/dsigma with h_s's final ReLU backward folded in, per-image sum ln lik [B])."""
    N, H, W = _check_latent(y4, C, "y4")
    if _check_latent(sigma4, C, "sigma4") != (N, H, W):
        raise ValueError("rate_gc: y4 and sigma4 shapes differ")
    gy, gs = torch.empty_like(y4), torch.empty_like(y4)
    part = torch.empty(N * int(lib().ica_rate_gc_blocks()), device=y4.device)
    call("ica_rate_gc", ptr(y4), ptr(sigma4), ptr(gy), ptr(gs), ptr(part), N, C, H, W, float(scale), stream())
    return gy, gs, reduce_rows(part, N)


def rate_eb(v4: torch.Tensor, C: int, eb: PackedEB, scale: float):
    """L = scale * sum ln lik of the zero-noise train-mode EntropyBottleneck on the unrounded v (scale > 0):
    (dL/dv, per-image sum ln lik [B]).  No parameter gradient."""
    N, H, W = _check_latent(v4, C, "v4")
    if eb.C != C:
        raise ValueError(f"rate_eb: the bottleneck has {eb.C} channels, the tensor {C}")
    gv = torch.empty_like(v4)
    part = torch.empty(N * int(lib().ica_rate_eb_blocks(C, H, W)), device=v4.device)
    call("ica_rate_eb", ptr(v4), ptr(eb.prm), ptr(gv), ptr(part), N, C, H, W, float(scale), stream())
    return gv, reduce_rows(part, N)


# --------------------------------------------------------------------------- #
# RD evaluation: the loss side of batch_test (ica_rdeval.hip)
# --------------------------------------------------------------------------- #
def _rd_check(fn, x_hat4, target, lik_y4, Cy, lik_z4, Cz):
    """The tensor checks rd_metrics and val_metrics share: (B, H, W, y shape, z shape), or a ValueError."""
    for t, nm in ((x_hat4, "x_hat4"), (target, "target"), (lik_y4, "lik_y4"), (lik_z4, "lik_z4")):
        if t is None and nm != "lik_z4":
            raise ValueError(f"{fn}: {nm} is missing")
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32
                              or not t.is_contiguous()):
            raise ValueError(f"{fn}: {nm} must be a contiguous float32 HIP tensor")
    B, H, W = check_image(target, "target")
    if x_hat4.dim() != 5 or tuple(x_hat4.shape) != (B, 1, H, W, 4):
        raise ValueError(f"{fn}: x_hat4 {tuple(x_hat4.shape)} is not the nChw4c reconstruction of target "
                         f"{tuple(target.shape)}")
    shapes = []
    for t, C, nm in ((lik_y4, Cy, "lik_y4"), (lik_z4, Cz, "lik_z4")):
        if t is None:
            if C:
                raise ValueError(f"{fn}: {C} z channels without a z plane")
            shapes.append((0, 0, 0))
            continue
        if not isinstance(C, int) or C < 1 or t.dim() != 5 or t.shape[4] != 4 or t.shape[1] != c4(C):
            raise ValueError(f"{fn}: {nm} {tuple(t.shape)} is not an nChw4c tensor of {C} channels")
        if t.shape[0] != B:
            raise ValueError(f"{fn}: {nm} holds {t.shape[0]} images, target {B}")
        shapes.append((C, t.shape[2], t.shape[3]))
    return B, H, W, shapes[0], shapes[1]


def _rd_status(fn, rc):
    if rc in (-5, -7):
        raise ValueError(f"{fn} refused its arguments (status {rc})")
    if rc != 0:
        raise RuntimeError(f"{fn} failed with status {rc}")


def rd_metrics(x_hat4: torch.Tensor, target: torch.Tensor, lik_y4: torch.Tensor, Cy: int, lik_z4=None, Cz: int = 0):
    """RateDistortionLoss(training=False)'s sums per image, in one launch on the eval forward's tensors:
    (sse [B] = sum (clamp(x_hat, 0, 1) - target)^2, lny [B] = sum ln max(lik_y, 2^-16), lnz [B] (0 without lik_z4),
    nclamp [B] int32 = likelihood elements below 2^-16, clamp(x_hat, 0, 1) as NCHW [B, 3, H, W]).
    x_hat4: fp32 nChw4c [B, 1, H, W, 4]; target: NCHW; lik_y4 / lik_z4: nChw4c of Cy / Cz channels.  Anything else
    is a ValueError and launches nothing."""
    B, H, W, ys, zs = _rd_check("rd_metrics", x_hat4, target, lik_y4, Cy, lik_z4, Cz)
    nblk = int(lib().ica_rd_metrics_blocks())
    dev = target.device
    out = torch.empty_like(target)
    part = torch.empty(B * 3 * nblk, device=dev)
    nclamp = torch.empty(B, dtype=torch.int32, device=dev)
    rc = lib().ica_rd_metrics(ptr(x_hat4), ptr(target), ptr(lik_y4), ptr(lik_z4), ptr(out), ptr(part), ptr(nclamp),
                              B, H, W, *ys, *zs, stream())
    _rd_status("ica_rd_metrics", rc)
    sums = reduce_rows(part, 3 * B).view(B, 3)
    return sums[:, 0], sums[:, 1], sums[:, 2], nclamp, out


def val_metrics(x_hat4: torch.Tensor, target: torch.Tensor, lik_y4: torch.Tensor, Cy: int, lik_z4=None, Cz: int = 0,
                want_x_hat: bool = False):
    """RateDistortionLoss(training=True)'s sums per image on an EVAL forward's tensors (the trainer's validation), in
    one launch: (sse [B] = sum (x_hat - target)^2 of the unclamped reconstruction, lny [B] = sum ln max(lik_y, 2^-16),
    lnz [B] (0 without lik_z4), the unclamped x_hat as NCHW [B, 3, H, W] when want_x_hat, else None).  Arguments and
    errors as rd_metrics."""
    B, H, W, ys, zs = _rd_check("val_metrics", x_hat4, target, lik_y4, Cy, lik_z4, Cz)
    nblk = int(lib().ica_rd_metrics_blocks())
    out = torch.empty_like(target) if want_x_hat else None
    part = torch.empty(B * 3 * nblk, device=target.device)
    rc = lib().ica_val_metrics(ptr(x_hat4), ptr(target), ptr(lik_y4), ptr(lik_z4), ptr(out), ptr(part),
                               B, H, W, *ys, *zs, stream())
    _rd_status("ica_val_metrics", rc)
    sums = reduce_rows(part, 3 * B).view(B, 3)
    return sums[:, 0], sums[:, 1], sums[:, 2], out


# --------------------------------------------------------------------------- #
# Layer-wise error propagation: the sums of every layer of a side in one launch (ica_layers.hip)
# --------------------------------------------------------------------------- #
LAYER_PAIR, LAYER_QUANT, LAYER_TRIPLE = 0, 1, 2
LAYERS_MAX = 16


def layer_sums(layers, B: int) -> torch.Tensor:
    """sums [n, B, 2] of n <= LAYERS_MAX layers in one launch (ica_layer_sums + ica_reduce_rows).  A layer is
    (mode, C, a, b[, c]): fp32 nChw4c tensors [B, ceil(C/4), H, W, 4] of one shape, each a contiguous run of B
    images (a slice of a larger batch along dim 0 is one), all in one storage layout.
      LAYER_PAIR    sum (a - b)^2, 0
      LAYER_QUANT   sum (a - round(b))^2, sum (round(a) - round(b))^2
      LAYER_TRIPLE  sum (a - c)^2, sum (b - c)^2
    Anything else is a ValueError and launches nothing."""
    positive_int("B", B)
    if not 1 <= len(layers) <= LAYERS_MAX:
        raise ValueError(f"layer_sums takes 1 .. {LAYERS_MAX} layers, not {len(layers)}")
    arr = (LayerDesc * len(layers))()
    dev = None
    for i, (mode, C, a, b, *rest) in enumerate(layers):
        if mode not in (LAYER_PAIR, LAYER_QUANT, LAYER_TRIPLE):
            raise ValueError(f"layer {i}: unknown mode {mode!r}")
        c = rest[0] if rest else None
        if (c is None) == (mode == LAYER_TRIPLE):
            raise ValueError(f"layer {i}: the triple mode, and only it, reads a third tensor")
        positive_int(f"layer {i}: C", C)
        for t in (a, b, c):
            if t is None:
                continue
            if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous()
                    or t.dim() != 5 or t.shape[0] != B or t.shape[1] != c4(C) or t.shape[4] != 4
                    or t.shape != a.shape or t.device != a.device):
                what = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"layer {i}: {what} is not a contiguous float32 HIP nChw4c tensor of {B} images and "
                                 f"{C} channels, shaped like the layer's first")
        dev = a.device if dev is None else dev
        if a.device != dev:
            raise ValueError(f"layer {i} is on {a.device}, layer 0 on {dev}")
        arr[i] = LayerDesc(a.data_ptr(), b.data_ptr(), None if c is None else c.data_ptr(), C, a.shape[2],
                           a.shape[3], mode)
    n = len(layers)
    ws = int(lib().ica_layer_sums_ws_size(n, B))
    if ws == 0:
        raise ValueError(f"ica_layer_sums does not take n, B = {(n, B)}")
    work = torch.empty(ws, dtype=torch.float32, device=dev)
    sums = torch.empty((n, B, 2), dtype=torch.float32, device=dev)
    import ctypes
    rc = lib().ica_layer_sums(ctypes.cast(arr, ctypes.c_void_p), n, B, ptr(sums), ptr(work), stream())
    _rd_status("ica_layer_sums", rc)
    return sums


# --------------------------------------------------------------------------- #
# Training-side wrappers (ica_train.hip)
# --------------------------------------------------------------------------- #
def wgrad(Sm4, A, Lg4, Bc, KS, S, out, accumulate=False, tag=None):
    """out[a][b][ky][kx] (+)= sum Sm[n][a][p] Lg[n][b][S p + k - KS//2]  (see include/ica_hip.h).
    tag: optional EVENT_HOOK tag (algorithmic FLOPs 2 * A * B * KS^2 * small-grid pixels)."""
    N, _, Hs, Ws, _ = Sm4.shape
    _, _, Hb, Wb, _ = Lg4.shape
    if out.numel() != A * Bc * KS * KS or not out.is_contiguous():
        raise RuntimeError("wgrad: output must be a contiguous [A][B][KS][KS] tensor")
    nsplit = int(lib().ica_wgrad_nsplit(A, Bc, N * Hs * ((Ws + 31) // 32)))
    ws = torch.empty(int(lib().ica_wgrad_ws_size(A, Bc, KS, nsplit)), device=Sm4.device)
    ev = _ev_begin(tag, N)
    call("ica_wgrad", ptr(Sm4), ptr(Lg4), ptr(ws), ptr(out), N, A, Bc, Hs, Ws, Hb, Wb, KS, S, KS // 2, nsplit,
         int(accumulate), stream())
    _ev_end(ev, 2.0 * A * Bc * KS * KS * N * Hs * Ws)
    return out


def channel_sum(x4, C, out, accumulate=False):
    N, _, H, W, _ = x4.shape
    call("ica_channel_sum", ptr(x4), ptr(out), N, C, H, W, int(accumulate), stream())
    return out


def relu_bwd_(g4, y4):
    call("ica_relu_bwd", ptr(g4), ptr(y4), g4.numel(), stream())
    return g4


def abs_bwd_(g4, x4):
    call("ica_abs_bwd", ptr(g4), ptr(x4), g4.numel(), stream())
    return g4


def lrelu_bwd(g4, a4):
    """g * lrelu'(a) into a new tensor (a: the saved leaky-ReLU output)."""
    out = torch.empty_like(g4)
    call("ica_lrelu_bwd", ptr(g4), ptr(a4), ptr(out), g4.numel(), stream())
    return out


def gdn_t(g4, y4, s4, inverse):
    """t = dL/dn of a GDN / IGDN layer from g = dL/dy and its saved (y, s) (ica_gdn_t)."""
    out = torch.empty_like(g4)
    call("ica_gdn_t", ptr(g4), ptr(y4), ptr(s4), ptr(out), g4.numel(), int(bool(inverse)), stream())
    return out


def gdn_xsq(y4, s4):
    out = torch.empty_like(y4)
    call("ica_gdn_xsq", ptr(y4), ptr(s4), ptr(out), y4.numel(), stream())
    return out


def reparam_bwd(p, gprime, gout, bound, accumulate=True):
    call("ica_reparam_bwd", ptr(p.detach().contiguous()), ptr(gprime.contiguous()), ptr(gout), p.numel(),
         float(bound), int(accumulate), stream())


def bpp_grad(lik4, scale):
    g = torch.empty_like(lik4)
    call("ica_bpp_grad", ptr(lik4), ptr(g), lik4.numel(), float(scale), stream())
    return g


def gc_bwd(yt4, sigma4, gl4, C):
    N, _, H, W, _ = yt4.shape
    gy, gs = torch.empty_like(yt4), torch.empty_like(yt4)
    call("ica_gc_bwd", ptr(yt4), ptr(sigma4), ptr(gl4), ptr(gy), ptr(gs), N, C, H, W, stream())
    return gy, gs


def eb_bwd(v4, gl4, eb: PackedEB, C):
    N, _, H, W, _ = v4.shape
    gv = torch.zeros_like(v4)
    gprm = torch.empty(C * 58, device=v4.device)
    call("ica_eb_bwd", ptr(v4), ptr(gl4), ptr(eb.prm), ptr(gv), ptr(gprm), N, C, H, W, stream())
    return gv, gprm


def eb_param_scatter(gprm, raw: list, graw: list, C):
    """Accumulate the 58-per-channel effective-parameter grads into the 14 raw EB parameter grads."""
    import ctypes as Cc
    for t in list(raw) + list(graw):
        if not t.is_contiguous():
            raise RuntimeError("entropy_bottleneck params/grads must be contiguous")
    ra = (Cc.c_void_p * 14)(*[t.data_ptr() for t in raw])
    ga = (Cc.c_void_p * 14)(*[t.data_ptr() for t in graw])
    call("ica_eb_param_scatter", ptr(gprm), Cc.cast(ra, Cc.c_void_p), Cc.cast(ga, Cc.c_void_p), C, stream())


def mse_grad_(xh4, x, g4, scale):
    B, _, H, W = x.shape
    call("ica_mse_grad", ptr(xh4), ptr(x.contiguous()), ptr(g4), B, H, W, float(scale), stream())
    return g4
