"""ctypes binding of libica_hip.so — the C-ABI boundary (include/ica_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950) and
travels with the repo.  There is NO fallback: if the library is missing or a
call returns non-zero, this raises.  torch must be imported first so that the
HIP runtime torch bundles (soname libamdhip64.so.7) is the one the library
binds to (single runtime, shared streams).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL load: shared HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ICA_HIP_LIB", os.path.join(_HERE, "libica_hip.so"))

_p = C.c_void_p
_i = C.c_int
_l = C.c_long
_f = C.c_float
_sz = C.c_size_t

# name -> argtypes (restype int unless listed in _RESTYPES)
_SIGS = {
    "ica_conv_it": [_i],
    "ica_pack_conv_weight_size": [_i, _i, _i, _i, _i],
    "ica_pack_conv_weight": [_p, _p, _i, _i, _i, _l, _l, _i, _i, _i, _i, _p],
    "ica_pack_conv_weight_bf16": [_p, _p, _i, _i, _i, _l, _l, _i, _i, _i, _p],
    "ica_pack_conv_weight_bf16_size": [_i, _i, _i, _i],
    "ica_pack_conv_weight_x6": [_p, _p, _i, _i, _i, _l, _l, _i, _i, _p],
    "ica_pack_conv_weight_x6_size": [_i, _i, _i, _i],
    "ica_pack_gdn_x6": [_p, _p, _i, _p],
    "ica_pack_gdn_x6_size": [_i],
    "ica_pack_up3k3_x6_size": [_i],
    "ica_pack_up3k3_x6": [_p, _p, _p, _i, _p],
    "ica_conv_up3k3_x6": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p],
    "ica_conv_ex": [_p, _p],
    "ica_last_launch": [_p, _i, _p],
    "ica_x6_tiling": [_i],
    "ica_pack_gdn": [_p, _p, _p, _p, _i, _i, _f, _p],
    "ica_pack_gdn_bf16": [_p, _p, _p, _p, _i, _i, _f, _p],
    "ica_pack_up3_size": [_i],
    "ica_pack_up3": [_p, _p, _i, _i, _p],
    "ica_conv_up3": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p],
    "ica_elem_blocks_per_image": [],
    "ica_nchw_to_nc4": [_p, _p, _i, _i, _i, _i, _p],
    "ica_nc4_to_nchw": [_p, _p, _i, _i, _i, _i, _p],
    "ica_reduce_rows": [_p, _p, _i, _i, _f, _p],
    "ica_attack_prologue": [_p, _p, _p, _p, _i, _i, _i, _f, _p],
    "ica_attack_prologue_ex": [_p, _p, _p, _p, _i, _i, _i, _f, _i, _p],
    "ica_attack_loss": [_p, _p, _p, _p, _i, _i, _i, _f, _i, _i, _p],
    "ica_attack_adam": [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _f, _f, _f, _p, _p, _p, _p],
    "ica_attack_adam_ex": [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _f, _f, _f, _p, _p, _p, _i, _p],
    # universal perturbation: one noise for the batch (ica_universal.hip)
    "ica_universal_prologue": [_p, _p, _p, _p, _i, _i, _i, _f, _p],
    "ica_universal_adam": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _f, _f, _f, _p, _p, _p],
    "ica_branch_select": [_p, _f, _i, _p, _p, _p],
    "ica_gather_images": [_p, _p, _p, _i, _l, _p],
    "ica_roi_prologue": [_p, _p, _p, _p, _i, _i, _i, _f, _i, _i, _i, _i, _f, _f, _p],
    "ica_roi_loss": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _f, _i, _p],
    "ica_roi_adam": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _f, _f, _p, _i, _i, _i, _i, _f, _f, _p, _p, _p],
    "ica_ifgsm_step": [_p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _i, _p],
    "ica_l1_partial": [_p, _p, _i, _i, _i, _p],
    # C&W-style binary-search attack (ica_cw.hip)
    "ica_cw_gate": [_p, _i, _f, _p, _p, _p, _p, _i, _p],
    "ica_cw_adam": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _p, _i, _p, _i, _p],
    "ica_cw_round": [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p],
    "ica_cw_reset": [_p, _p, _p, _p, _i, _l, _p],
    "ica_gc_likelihood": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p],
    "ica_eb_likelihood": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p],
    "ica_pack_eb": [_p, _p, _p, _i, _p],
    "ica_abs": [_p, _p, _l, _p],
    "ica_cast_f32_bf16": [_p, _p, _l, _p],
    "ica_cast_bf16_f32": [_p, _p, _l, _p],
    # eval-time defences (ica_defend.hip)
    "ica_flip_rot": [_p, _p, _l, _i, _i, _i, _p],
    "ica_bitdepth": [_p, _p, _l, _f, _p],
    "ica_resample_axis": [_p, _p, _l, _i, _i, _i, _i, _p, _p, _p, _i, _p],
    "ica_bitdepth_noise": [_p, _p, _p, _l, _f, _p],
    "ica_bitdepth_noise_bwd": [_p, _p, _l, _f, _p],
    "ica_add": [_p, _p, _p, _l, _p],
    "ica_ensemble_grad": [_p, _p, _p, _l, _f, _p],
    # latent range profile, clamp defence and detector (ica_latent.hip)
    "ica_latent_range": [_p, _i, _i, _i, _i, _p, _p, _p, _p],
    "ica_latent_clamp": [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p],
    "ica_latent_clamp_bwd": [_p, _p, _p, _p, _i, _i, _i, _i, _p],
    "ica_latent_detect": [_p, _p, _p, _p, _p, _i, _i, _p],
    # latent distribution: per-channel histogram, predicted distribution, bits (ica_distrib.hip)
    "ica_latent_distrib_ws_size": [_i, _i, _i, _i, _i],
    "ica_latent_distrib": [_p, _p, _p, _p, _i, _i, _i, _i, _f, _i, _f, _f, _p, _p, _p, _p, _p],
    # layer-wise error propagation: the sums of every layer of a side in one launch (ica_layers.hip)
    "ica_layer_sums_blocks": [_i, _i, _i],
    "ica_layer_sums_ws_size": [_i, _i],
    "ica_layer_sums": [_p, _i, _i, _p, _p, _p],
    # bitrate attack: entropy-model value gradients (ica_rate.hip)
    "ica_rate_gc_blocks": [],
    "ica_rate_eb_blocks": [_i, _i, _i],
    "ica_rate_gc": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _p],
    "ica_rate_eb": [_p, _p, _p, _p, _i, _i, _i, _i, _f, _p],
    # RD evaluation: the loss side of batch_test (ica_rdeval.hip)
    "ica_rd_metrics_blocks": [],
    "ica_rd_metrics": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "ica_val_metrics": [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    # patch-wise VI localisation (ica_patch.hip)
    "ica_patch_vi_ws_size": [_i, _i, _i, _i, _i],
    "ica_patch_vi": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p],
    "ica_patch_gather": [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p],
    # image-space degradations: Gaussian blur, the sigma sweep, additive noise (ica_degrade.hip)
    "ica_blur_sweep_chunk": [],
    "ica_gauss_blur_ws_size": [_i, _i, _i],
    "ica_gauss_blur": [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p],
    "ica_blur_sweep_ws_size": [_i, _i, _i],
    "ica_blur_sweep": [_p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _i, _p, _l, _p, _p, _p, _p, _p],
    "ica_noise_apply_ws_size": [_i, _i, _i],
    "ica_noise_apply": [_p, _p, _p, _i, _i, _i, _p, _p, _p, _p],
    # the JPEG round trip and its quality sweep (ica_jpeg.hip)
    "ica_jpeg_sweep_chunk": [],
    "ica_jpeg_roundtrip_ws_size": [_i, _i, _i, _i],
    "ica_jpeg_roundtrip": [_p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p],
    "ica_jpeg_roundtrip_bwd_ws_size": [_i, _i, _i, _i],
    "ica_jpeg_roundtrip_bwd": [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p],
    "ica_jpeg_sweep_ws_size": [_i, _i, _i, _i],
    "ica_jpeg_sweep":[_p, _p, _i, _i, _i, _i, _i, _f, _i, _p, _l, _p, _p, _p, _p, _p],
    # perturbation transfer: N noises x M targets (ica_transfer.hip)
    "ica_transfer_apply_ws_size": [_i, _i, _i, _i],
    "ica_transfer_apply": [_p, _p, _p, _i, _i, _i, _i, _p, _p, _p],
    "ica_transfer_score_ws_size": [_i, _i, _i, _i],
    "ica_transfer_score": [_p, _p, _i, _i, _i, _i, _i, _p, _p, _p],
    # frequency bands of a perturbation: study and band-limited attack step (ica_band.hip)
    "ica_band_split_chunk": [],
    "ica_band_max_variants": [],
    "ica_band_split_ws_size": [_i, _i, _i, _i],
    "ica_band_split": [_p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p],
    "ica_band_project": [_p, _i, _i, _i, _i, _p, _p],
    "ica_band_prologue_ws_size": [_i, _i, _i],
    "ica_band_prologue": [_p, _p, _p, _p, _i, _i, _i, _f, _i, _p, _p],
    "ica_band_adam": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _f, _f, _f, _p, _p, _p, _i, _p],
    # iterated re-compression: the step between two generations (ica_recompress.hip)
    "ica_requant8_ws_size": [_i, _i, _i],
    "ica_requant8": [_p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "ica_quant8_pack": [_p, _i, _i, _i, _p, _p, _p],
    "ica_floor_bits_ws_size": [_i, _i, _i, _i],
    "ica_floor_bits": [_p, _i, _i, _i, _i, _f, _p, _p, _p],
    "ica_gc_symbols": [_p, _p, _p, _p, _i, _f, _p, _p, _i, _i, _i, _i, _p],
    "ica_eb_symbols": [_p, _p, _p, _p, _i, _i, _i, _i, _p],
    "ica_dequantize": [_p, _p, _p, _p, _i, _i, _i, _i, _p],
    "ica_pmf_to_quantized_cdf": [_p, _i, _i, _p],
    "ica_rans_encode": [_p, _p, _l, _p, _i, _p, _p, _i, _p, _l, _p],
    "ica_rans_decode": [_p, _l, _p, _l, _p, _i, _p, _p, _i, _p],
    "ica_rans_dec_open": [_p, _l, _p],
    "ica_rans_dec_step": [_p, _i, _p, _l, _p, _i, _p, _p, _i, _p, _p],
    "ica_rans_dec_close": [_p],
    # autoregressive coding of the context models (ica_ar.hip)
    "ica_ar_lds_bytes": [_i, _i, _i],
    "ica_ar_step": [_p, _i, _i, _i, _p],
    "ica_round": [_p, _p, _l, _p],
    "ica_clamp01": [_p, _p, _l, _p],
    "ica_sqdiff_partial": [_p, _p, _p, _i, _l, _i, _p],
    "ica_nc4_bound_to_nchw": [_p, _p, _i, _i, _i, _i, _p],
    "ica_bound_bwd_nc4": [_p, _p, _p, _i, _i, _i, _i, _p],
    "ica_msssim_blocks": [_i, _i, _i, _i],
    "ica_msssim_level": [_p, _p, _i, _i, _i, _p, _i, _i, _f, _f, _p, _p, _p, _p, _p],
    "ica_msssim_level_bwd": [_p, _p, _p, _i, _i, _i, _p, _i, _i, _p, _p, _p],
    "ica_msssim_combine": [_p, _i, _i, _i, _p, _p, _p, _p, _p],
    "ica_avgpool2": [_p, _p, _i, _i, _i, _i, _i, _p],
    "ica_avgpool2_bwd": [_p, _p, _i, _i, _i, _i, _i, _p],
    "ica_scale": [_p, _l, _f, _p],
    # training side (ica_train.hip)
    "ica_wgrad_ws_size": [_i, _i, _i, _i],
    "ica_wgrad_nsplit": [_i, _i, _l],
    "ica_wgrad": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "ica_channel_sum": [_p, _p, _i, _i, _i, _i, _i, _p],
    "ica_relu_bwd": [_p, _p, _l, _p],
    "ica_abs_bwd": [_p, _p, _l, _p],
    "ica_gdn_xsq": [_p, _p, _p, _l, _p],
    "ica_lrelu_bwd": [_p, _p, _p, _l, _p],
    "ica_gdn_t": [_p, _p, _p, _p, _l, _i, _p],
    "ica_reparam_bwd": [_p, _p, _p, _l, _f, _i, _p],
    "ica_bpp_grad": [_p, _p, _l, _f, _p],
    "ica_gc_bwd": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p],
    "ica_eb_bwd": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p],
    "ica_eb_param_scatter": [_p, _p, _p, _i, _p],
    "ica_mse_grad": [_p, _p, _p, _i, _i, _i, _f, _p],
}
_RESTYPES = {"ica_pack_conv_weight_size": _sz, "ica_pack_conv_weight_bf16_size": _sz,
             "ica_pack_conv_weight_x6_size": _sz, "ica_pack_gdn_x6_size": _sz, "ica_pack_up3k3_x6_size": _sz, "ica_pack_up3_size": _sz, "ica_wgrad_ws_size": _sz,
             "ica_rans_encode": _l, "ica_ar_lds_bytes": _sz, "ica_patch_vi_ws_size": _sz,
             "ica_gauss_blur_ws_size": _sz, "ica_blur_sweep_ws_size": _sz, "ica_noise_apply_ws_size": _sz,
             "ica_transfer_apply_ws_size": _sz, "ica_transfer_score_ws_size": _sz,
             "ica_requant8_ws_size": _sz, "ica_floor_bits_ws_size": _sz, "ica_latent_distrib_ws_size": _sz,
             "ica_layer_sums_ws_size": _sz, "ica_jpeg_roundtrip_ws_size": _sz, "ica_jpeg_sweep_ws_size": _sz,
             "ica_jpeg_roundtrip_bwd_ws_size": _sz, "ica_band_split_ws_size": _sz,
             "ica_band_prologue_ws_size": _sz}



class ConvArgs(C.Structure):
    """include/ica_hip.h ica_conv_args."""
    _fields_ = ([(n, C.c_void_p) for n in ("x", "y", "wp", "bias", "gp", "beta", "save_x", "save_s", "in_x", "in_s",
                                            "save_t", "res", "mask")]
                + [(n, C.c_int) for n in ("N", "Cin", "Hin", "Win", "Cout", "Hout", "Wout", "kind", "KS", "S", "epi",
                                           "it", "fill_mode", "ps", "prec", "layout", "order")])


class ArArgs(C.Structure):
    """include/ica_hip.h ica_ar_args."""
    _fields_ = ([(n, C.c_void_p) for n in ("y", "params", "yhat", "sym", "idx", "sym_in", "means", "wc", "bc", "w1",
                                            "b1", "w2", "b2", "w3", "b3", "table")]
                + [("T", C.c_int), ("bound", C.c_float)]
                + [(n, C.c_int) for n in ("B", "M", "H", "W", "E1", "E2")])


class LayerDesc(C.Structure):
    """include/ica_hip.h ica_layer_desc."""
    _fields_ = [(n, C.c_void_p) for n in ("a", "b", "c")] + [(n, C.c_int) for n in ("C", "H", "W", "mode")]


_lib = None


def lib():
    """Load (once) and return the ctypes library; raises if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libica_hip.so not found at {LIB_PATH}: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                "There is no CPU/PyTorch fallback for the hot path.")
        L = C.CDLL(LIB_PATH)
        for name, args in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = _RESTYPES.get(name, _i)
        _lib = L
    return _lib


def exported_symbols():
    return list(_SIGS)


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed with status {rc}")
    return rc


def ptr(t):
    """Device pointer of a tensor (or None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
