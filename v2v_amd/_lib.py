"""ctypes binding of libv2v_hip.so (C ABI in the public headers under include/) and the one calling convention every module of the package
goes through.  Fails loudly when the library is missing.

    HEADERS / SIGNATURES / EXPORTS the one binding table: per header, its flat union, the names
    HEADERS_MORE / SIGNATURES_MORE the second table: headers added after ABI 6 was pinned (additive, same version)
    lib()                          the loaded library, every entry point of both tables bound
    ptr(t, offset_elems=0)         the address of a tensor as a C pointer argument, None -> NULL
    launch(name, device, *args)    the `_hip` entry point `name` on `device` and torch's current stream there, the stream last, status checked
    need(name, t, dtype, ...)      ValueError unless t is a contiguous CUDA tensor of that dtype and shape
    DTYPE_CODES                    torch dtype -> the dtype code of include/v2v_hip.h
    check(rc) / require_gpu()      status -> exception; the RuntimeError every compute call raises first without a GPU

Size queries (`*_bytes`, `*_elems`) take no stream and stay direct calls on lib().
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  -- imported FIRST so the process uses one HIP runtime (torch's libamdhip64.so.7)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("V2V_HIP_LIB") or os.path.join(_HERE, "libv2v_hip.so")   # override: kernel sweeps only

# enums of include/v2v_hip.h
U8, F32, F64, BF16 = 0, 1, 2, 3
DTYPE_CODES = {torch.uint8: U8, torch.float32: F32, torch.float64: F64, torch.bfloat16: BF16}   # a call site rejects what it does not take
RNG_NONE, RNG_PHILOX, RNG_REPLAY, RNG_PHILOX_FAST = 0, 1, 2, 3
BIN_SUM, BIN_BILINEAR = 0, 1
FLAG_NOISE_EXTERNAL = 0x1
FLAG_NO_NOISE = 0x2
FLAG_SYMMETRIC = 0x4
FLAG_MAP_4PX, FLAG_MAP_1PX, FLAG_MAP_2PX = 0x8, 0x10, 0x20
OK, ERR_NULL, ERR_SHAPE, ERR_BINS, ERR_DTYPE, ERR_MODE, ERR_ALIGN, ERR_HIP, ERR_PARAM = 0, -1, -2, -3, -4, -5, -6, -7, -8
ABI_VERSION = 6

EV_MAKE_VOXEL_DISCRETE, EV_MAKE_VOXEL_INTERP, EV_BILINEAR = 0, 1, 2
NORM_NONE, NORM_RADIX, NORM_COUNT = 0, 1, 2
VOXEL_STATS_WORDS = 516


class EsimReplay(C.Structure):
    _fields_ = [("u_init", C.c_void_p), ("u_hot", C.c_void_p), ("g_hot", C.c_void_p), ("g_base", C.c_void_p)]


class EsimExtras(C.Structure):
    _fields_ = [("stats", C.c_void_p), ("frame_index", C.c_void_p), ("clip_offsets", C.c_void_p), ("stored_frames", C.c_void_p), ("frames_elems", C.c_int64)]


class V2EParams(C.Structure):
    _fields_ = [("fps", C.c_double), ("threshold_model", C.c_int), ("thres_mean_mean", C.c_double),
                ("thres_mean_std", C.c_double), ("thres_diff_mean", C.c_double), ("thres_diff_std", C.c_double),
                ("cutoff_hz", C.c_double), ("leak_rate_hz", C.c_double), ("refractory_period_s", C.c_double),
                ("shot_noise_rate_hz", C.c_double), ("leak_jitter_fraction", C.c_double),
                ("noise_rate_cov_decades", C.c_double), ("uint8_wrap", C.c_int)]


class V2EReplay(C.Structure):
    _fields_ = [("pos_thres", C.c_void_p), ("neg_thres", C.c_void_p), ("thres_frame_stride", C.c_int64),
                ("noise_rate", C.c_void_p), ("leak_randn", C.c_void_p), ("shot_pos", C.c_void_p), ("shot_neg", C.c_void_p)]


V2E_MODELS = {"pn_related": 0, "spatial_independent": 1, "spatial_temporal_independent": 2}


class V2VError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libv2v_hip error {code}: {msg}")
        self.code = code


P, I, I64, U32, U64, F = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_float
_ESIM = [P, I] + [I64] * 6 + [P, I64, U32, I, U64, U64]                                  # frames..clip_id0
_ESIM_PADDED = _ESIM + [P, C.POINTER(EsimReplay), I, I, I, P, I, I64, I64, P]              # clip_keys..out_counts (the stream follows)

# The one binding table: public header under include/ -> {entry point: (restype, argtypes)}, each header's entries in the header's own order
# (tests/test_capi_contract.py holds every row to its prototype).  This table is ABI 6 as that test pins it -- five headers, 124 rows -- and
# stays as it is: a family added after it puts its header and its rows into HEADERS_MORE below, which lib() binds the same way and the
# same kind of contract test (tests/test_nam_capi_contract.py) holds to its header.  Additive, so v2v_version() stays 6.
HEADERS = {"v2v_hip.h": {
    # library info / errors
    "v2v_version": (I, []),
    "v2v_last_error": (C.c_char_p, []),
    "v2v_device_count": (I, []),
    # log-intensity tables
    "v2v_lut_get": (I, [I, P]),
    "v2v_lut_set": (I, [I, P]),
    # fused ESIM simulator + voxel binning
    "v2v_esim_voxel_hip": (I, _ESIM + [C.POINTER(EsimReplay), I, I, I, P, I, P, P]),
    "v2v_esim_voxel_keyed_hip": (I, _ESIM + [P, C.POINTER(EsimReplay), I, I, I, P, I, P, P]),
    "v2v_esim_voxel_padded_hip": (I, _ESIM_PADDED + [P]),
    "v2v_esim_voxel_bytes": (I64, [I] + [I64] * 4 + [I] * 4),
    # synthetic clips
    "v2v_synth_clips_hip": (I, [P, I] + [I64] * 4 + [U64, U64, P]),
    "v2v_events_to_voxel_segmented_hip": (I, [P, P, P, P, I64, P, I64, I, I, I64, I64, P, P, P]),
    # v2e-derived DVS model fused with voxel binning
    "v2v_v2e_workspace_bytes": (I64, [I64, I64]),
    "v2v_v2e_voxel_hip": (I, [P, I] + [I64] * 6 + [C.POINTER(V2EParams), I, U64, U64, C.POINTER(V2EReplay), I, I, I, P, I, P, P, P]),
    # event list -> voxel grid
    "v2v_events_to_voxel_hip": (I, [P, P, P, P, I64, I, I, I64, I64, P, P, P]),
    # decode-side front end
    "v2v_frontend_hip": (I, [P] + [I64] * 10 + [I, I, P, I64, P, P, P, P, P]),
    "v2v_frontend_batch_hip": (I, [P] + [I64] * 5 + [P, I64, I64, I, P, I64, P, P, P]),
    # voxel post-ops of the consumer
    "v2v_postops_workspace_bytes": (I64, [I64]),
    "v2v_normalize_pad_hip": (I, [P] + [I64] * 4 + [I, I, P, P, P]),
    "v2v_normalize_pad_ex_hip": (I, [P] + [I64] * 6 + [I, I, P, P, P]),
    "v2v_events_to_voxel_f32_hip": (I, [P, P, P, P, I64, I, I, I64, I64, P, P, P]),
    "v2v_events_to_voxel_f32_segmented_hip": (I, [P, P, P, P, I64, P, I64, I, I, I, I64, I64, P, P, P]),
    # the ConvLSTM step
    "v2v_convlstm_packed_bytes": (I, [I64, C.POINTER(U64)]),
    "v2v_convlstm_pack_weights_hip": (I, [P, I64, P, P]),
    "v2v_convlstm_step_hip": (I, [P] * 5 + [I64] * 4 + [P, P, P, I, I, P]),
    # the ConvGRU step (two launches behind one call)
    "v2v_convgru_packed_bytes": (I, [I64, C.POINTER(U64), C.POINTER(U64)]),
    "v2v_convgru_pack_weights_hip": (I, [P, P, P, I64, P, P, P]),
    "v2v_convgru_step_hip": (I, [P] * 7 + [I64] * 4 + [P] * 5 + [I] * 3 + [P]),
    # the 16-channel layer family (FireNet): one launch per layer
    "v2v_convgru16_packed_elems": (I64, []),
    "v2v_convgru16_pack_weights_hip": (I, [P] * 5),
    "v2v_convgru16_step_hip": (I, [P] * 6 + [I64] * 3 + [P] * 3 + [I, P]),
    "v2v_resblock16_packed_elems": (I64, []),
    "v2v_resblock16_pack_weights_hip": (I, [P] * 4),
    "v2v_resblock16_nhwc_hip": (I, [P] * 4 + [I64] * 3 + [P, P]),
    "v2v_conv_head16_packed_elems": (I64, []),
    "v2v_conv_head16_pack_weights_hip": (I, [P, I64, P, P]),
    "v2v_conv_head16_nhwc_hip": (I, [P] * 3 + [I] + [I64] * 3 + [P, P]),
    # convolution, head, 1x1, upsampling, layouts
    "v2v_conv3x3_pack_weights_hip": (I, [P, I64, I64, P, P]),
    "v2v_conv3x3_nhwc_hip": (I, [P, P, P, P, I] + [I64] * 5 + [P, I, P]),
    "v2v_conv_packed_elems": (I64, [I64, I64, I]),
    "v2v_conv_pack_weights_hip": (I, [P, I64, I64, I, P, P]),
    "v2v_conv_nhwc_hip": (I, [P, P, P, P, I] + [I64] * 5 + [I, I, P, I, P]),
    "v2v_upsample2x_nhwc_hip": (I, [P, P] + [I64] * 4 + [P, P]),
    "v2v_conv_head_packed_elems": (I64, [I]),
    "v2v_conv_head_pack_weights_hip": (I, [P, I64, I, P, P]),
    "v2v_to_nhwc8_bf16_hip": (I, [P] + [I64] * 8 + [P, P]),
    "v2v_to_nhwc8_bf16_scaled_hip": (I, [P] + [I64] * 8 + [P, P, P]),
    "v2v_conv_head_nhwc_hip": (I, [P, P, P, I, I64, I64, I64, I, P, P]),
    "v2v_conv1x1_nhwc_hip": (I, [P, P, P, P, I64, I64, I64, P, I, P]),
    "v2v_nchw_to_nhwc_bf16_hip": (I, [P, I] + [I64] * 4 + [I, P, P]),
    # backward passes (v2v_amd/train.py)
    "v2v_convlstm_step_bwd_hip": (I, [P] * 7 + [I64] * 4 + [P, P, P]),
    "v2v_relu_bwd_nhwc_hip": (I, [P, P, I64, I64, P, P]),
    "v2v_conv_dgrad_packed_elems": (I64, [I64, I64, I]),
    "v2v_conv_dgrad_pack_weights_hip": (I, [P, I64, I64, I, P, P, P]),
    "v2v_conv_dgrad_workspace_bytes": (I64, [I64] * 5 + [I]),
    "v2v_conv_dgrad_nhwc_hip": (I, [P, P, P] + [I64] * 5 + [I, I, P, P, P]),
    "v2v_conv_wgrad_workspace_bytes": (I64, [I64] * 5 + [I]),
    "v2v_conv_wgrad_nhwc_hip": (I, [P, P, I64, P, I64, I64, I64, I64, I64, I64, I, I, P, P, P, P]),
    "v2v_upsample2x_bwd_nhwc_hip": (I, [P] + [I64] * 4 + [P, P]),
    "v2v_conv1x1_bwd_workspace_bytes": (I64, [I64, I64]),
    "v2v_conv1x1_bwd_nhwc_hip": (I, [P, P, P, P, I64, I64, P, P, P, P, P]),
    # ESIM extras, voxel statistics and scales, clip frames
    "v2v_esim_voxel_ex_hip": (I, _ESIM_PADDED + [C.POINTER(EsimExtras), P]),
    "v2v_esim_voxel_stats_hip": (I, _ESIM_PADDED + [P, P]),
    "v2v_voxel_scales_hip": (I, [P, I64, I64, P, P]),
    "v2v_voxel_apply_scales_hip": (I, [P] + [I64] * 6 + [I, P, P, P]),
    "v2v_voxel_scales_select_hip": (I, [P] + [I64] * 6 + [I, P, P, P]),
    "v2v_clip_frames_f32_hip": (I, [P, I64, I64, P] + [I64] * 5 + [P, P]),
    "v2v_clip_frames_f32_ex_hip": (I, [P, I64, P, I64, P] + [I64] * 6 + [P, P]),
    "v2v_clip_frames_f32_bounded_hip": (I, [P, I64, P, I64, P, I64, P, I64] + [I64] * 5 + [P, P]),
    # the plain UNet (EVFlowNet): stem, concat-skip upsampling + adjoint, prediction backward for 1..3 outputs
    "v2v_conv_stem_packed_elems": (I64, []),
    "v2v_conv_stem_pack_weights_hip": (I, [P, I64, P, P]),
    "v2v_conv_stem_nhwc_hip": (I, [P, P, P, I, I64, I64, I64, P, P]),
    "v2v_upsample2x_cat_nhwc_hip": (I, [P, I64, P, I64, I64, I64, I64, P, P]),
    "v2v_upsample2x_cat_bwd_nhwc_hip": (I, [P] + [I64] * 6 + [P, P]),
    "v2v_conv1x1_bwd_cout_workspace_bytes": (I64, [I64, I64, I64]),
    "v2v_conv1x1_bwd_cout_nhwc_hip": (I, [P, P, P, P, I64, I64, I64, P, P, P, P, P]),
    "v2v_conv_nhwc_like_hip": (I, [P, P, P, P, I] + [I64] * 5 + [I, I, P, I64, P]),
    # HyperE2VID's dynamic decoder (v2v_amd/hyper.py): context staging, tanh, atoms, the dynamic convolution
    "v2v_hyper_context_hip": (I, [P] + [I64] * 4 + [P] + [I64] * 4 + [P, P]),
    "v2v_hyper_context_conv_hip": (I, [P, P, P] + [I64] * 4 + [P, P]),
    "v2v_tanh_bf16_hip": (I, [P, I64, P, P]),
    "v2v_hyper_atoms_hip": (I, [P, P, I64, P, P]),
    "v2v_hyper_dynconv_packed_elems": (I64, [I64, I64, I, I]),
    "v2v_hyper_dynconv_pack_weights_hip": (I, [P, I64, I64, I, P, P]),
    "v2v_hyper_dynconv_nhwc_hip": (I, [P, P, P, P, I] + [I64] * 5 + [I, I, P, P]),
    # the dynamic decoder's backward and BatchNorm on batch statistics (v2v_amd/train.py DynamicUpsampleFn)
    "v2v_hyper_train_last_error": (C.c_char_p, []),                 # deprecated alias of v2v_last_error
    "v2v_hyper_dynconv_pack_t_hip": (I, [P, P, P]),
    "v2v_hyper_dynconv_df_hip": (I, [P, P, I64, P, P]),
    "v2v_hyper_dynconv_datoms_hip": (I, [P, P, I64, I64, I64, P, P]),
    "v2v_hyper_dynconv_dx_hip": (I, [P, P, I64, I64, I64, P, P]),
    "v2v_hyper_dynconv_wgrad_workspace_bytes": (I64, [I64, I64, I64]),
    "v2v_hyper_dynconv_wgrad_hip": (I, [P, P, P, I64, I64, I64, P, P, P, P]),
    "v2v_hyper_bn_stats_hip": (I, [P, I64, I64, F, P, P, P, P]),
    "v2v_hyper_bn_apply_hip": (I, [P] * 5 + [I64] * 3 + [I, P, P]),
    "v2v_hyper_bn_bwd_hip": (I, [P, I] + [P] * 5 + [I64] * 3 + [I, P, P, P]),
    "v2v_hyper_atoms_bwd_hip": (I, [P, P, P, I64, P, P]),
    # the image losses of training (v2v_amd/loss_ops.py)
    "v2v_tc_loss_workspace_bytes": (I64, [I64] * 4 + [I]),
    "v2v_tc_loss_fwd_hip": (I, [P] * 5 + [I64] * 10 + [F] * 5 + [P] * 7),
    "v2v_tc_loss_bwd_hip": (I, [P] * 5 + [I64] * 10 + [F] * 5 + [P, I] + [P] * 4),
    "v2v_warp_bilinear_hip": (I, [P, P] + [I64] * 4 + [P, P]),
    "v2v_warp_bilinear_adjoint_hip": (I, [P, P] + [I64] * 4 + [P, P, P]),
    # the LPIPS-VGG perceptual loss (v2v_amd/lpips.py): stem, max-pool, compare, each forward and backward
    "v2v_lpips_stem_hip": (I, [P, I] + [I64] * 4 + [P] * 4 + [I, P, P]),
    "v2v_lpips_stem_bwd_hip": (I, [P] + [I64] * 4 + [P, P, I, P, P]),
    "v2v_lpips_pool_hip": (I, [P] + [I64] * 4 + [P, P]),
    "v2v_lpips_pool_bwd_hip": (I, [P, P, P, I] + [I64] * 4 + [P, P]),
    "v2v_lpips_compare_workspace_bytes": (I64, [I64, I64]),
    "v2v_lpips_compare_fwd_hip": (I, [P, P, P] + [I64] * 3 + [P, P, P]),
    "v2v_lpips_compare_bwd_hip": (I, [P, P, P, P] + [I64] * 3 + [P, P]),
}, "v2v_nernet.h": {                                            # NER-Net's learned voxelisation (v2v_amd/nernet.py)
    "v2v_learned_voxel_packed_elems": (I64, [P, I]),
    "v2v_learned_voxel_workspace_bytes": (I64, [I64, I64]),
    "v2v_learned_voxel_stats_hip": (I, [P, I, I64, P, I64, I64, P, P]),
    "v2v_learned_voxel_hip": (I, [P, I, I64, P, I64, I64, I, I64, I64, P, P, I, F, I, I, P, P, P, P]),
}, "v2v_metrics.h": {                                           # the evaluation metrics (v2v_amd/metrics.py)
    "v2v_image_metrics_workspace_bytes": (I64, [I64, I64, I64]),
    "v2v_image_metrics_hip": (I, [P, I64, P, I64, I64, I64, I64, F, C.c_double, P, P, P, P]),
    "v2v_flow_metrics_workspace_bytes": (I64, [I64, I64, I64]),
    "v2v_flow_metrics_hip": (I, [P, I64, P, I64, P, I64, I64, I64, I64, I64, P, P, P, P]),
}, "v2v_lpips_alex.h": {                                        # the LPIPS-AlexNet test metric (v2v_amd/lpips_alex.py)
    "v2v_lpips_alex_stem_hip": (I, [P, I64, I64, I64, I64, I64, F, I, P, P, P, P, P, P]),
    "v2v_lpips_alex_conv_hip": (I, [P, P, P, I64, I64, I64, I64, I64, I, I, P, P]),
    "v2v_lpips_alex_pool_hip": (I, [P, I64, I64, I64, I64, P, P]),
    "v2v_lpips_alex_compare_workspace_bytes": (I64, [I64, I64]),
    "v2v_lpips_alex_compare_hip": (I, [P, P, P, I64, I64, I64, I, P, P, P]),
    "v2v_lpips_alex_sum_hip": (I, [P, I64, P, P]),
}, "v2v_alex_train.h": {                                        # LPIPS-AlexNet's backward to the prediction (v2v_amd/lpips_alex.py)
    "v2v_alex_train_compare_bwd_hip": (I, [P, P, P, P, I64, I64, I64, I, P, P]),
    "v2v_alex_train_conv_dgrad_hip": (I, [P, P, P, P, I64, I64, I64, I64, I64, I, P, P]),
    "v2v_alex_train_pool_bwd_hip": (I, [P, P, P, I64, I64, I64, I64, I, P, P]),
    "v2v_alex_train_stem_bwd_hip": (I, [P, P, P, I64, I64, I64, I64, F, I, P, P]),
}}
SIGNATURES = {name: sig for table in HEADERS.values() for name, sig in table.items()}      # the flat union, in that order
EXPORTS = tuple(SIGNATURES)

# The second table, same shape: the headers added after ABI 6 was pinned.  Not part of HEADERS / SIGNATURES / EXPORTS; no name in both.
HEADERS_MORE = {"v2v_nam.h": {                                  # NER-Net's recurrent network: NAM cell, context block, 16-channel head, valid extent (v2v_amd/nhwc_ops.py)
    "v2v_nam_packed_elems": (I64, [I64]),
    "v2v_nam_pack_weights_hip": (I, [P] * 6 + [I64, P, P]),
    "v2v_nam_step_hip": (I, [P] * 5 + [I64] * 4 + [P] * 9 + [I, I, I64, I64, P]),
    "v2v_gcb_workspace_bytes": (I64, [I64] * 4),
    "v2v_gcb_nhwc_hip": (I, [P] * 12 + [F] + [I64] * 6 + [P, I64, P, P, P]),
    "v2v_conv_head16in_packed_elems": (I64, []),
    "v2v_conv_head16in_pack_weights_hip": (I, [P, I64, P, P]),
    "v2v_to_nhwc16_bf16_hip": (I, [P] + [I64] * 8 + [P, P]),
    "v2v_conv_head16in_nhwc_hip": (I, [P] * 3 + [I] + [I64] * 3 + [P, P]),
    "v2v_valid_extent_nhwc_hip": (I, [P, I] + [I64] * 6 + [I, P]),
}}
SIGNATURES_MORE = {name: sig for table in HEADERS_MORE.values() for name, sig in table.items()}

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C v2v_amd/csrc`).  v2v_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in (*SIGNATURES.items(), *SIGNATURES_MORE.items()):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    if L.v2v_version() != ABI_VERSION:
        raise ImportError(f"libv2v_hip.so ABI {L.v2v_version()} != binding ABI {ABI_VERSION}: rebuild")
    _lib = L
    return L


def check(rc: int):
    """Map a v2v_status to the exception the reference would raise at the same spot."""
    if rc == OK:
        return
    msg = lib().v2v_last_error().decode()
    if rc == ERR_BINS:
        raise AssertionError(msg)            # reference: `assert (N-1) % (num_bins*frames_per_bin) == 0`
    if rc in (ERR_SHAPE, ERR_DTYPE, ERR_MODE, ERR_PARAM, ERR_NULL, ERR_ALIGN):
        raise ValueError(msg)
    raise V2VError(rc, msg)


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("v2v_amd needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, offset_elems=0):
    """The address of tensor t (`offset_elems` elements in) as a pointer argument; None gives NULL.  CUDA and page-locked host tensors alike;
    the address is taken as it is (whether an empty tensor stands for NULL is the call site's to say)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr() + offset_elems * t.element_size()) if offset_elems else C.c_void_p(t.data_ptr())


def launch(name: str, device, *args) -> None:
    """The C entry point `name` on `device` and torch's current stream there: lib().<name>(*args, stream), status checked."""
    with torch.cuda.device(device):
        check(getattr(lib(), name)(*args, stream_ptr()))


def need(name: str, t, dtype=torch.bfloat16, dims: str = "[B,H,W,C]", shape=None, last=None, device=None, owner: str = "x"):
    """ValueError unless t is a contiguous CUDA tensor of `dtype`: 4-D, or of exactly `shape` when given; with `last` channels and on
    `device` (the device of the operand called `owner`) when given.  -> t"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() \
            or (t.dim() != 4 if shape is None else tuple(t.shape) != tuple(shape)) \
            or (last is not None and t.shape[3] != last) or (device is not None and t.device != device):
        where = f" on {owner}'s device" if device is not None else ""
        raise ValueError(f"{name} must be a contiguous {str(dtype)[6:]} CUDA tensor {list(shape) if shape is not None else dims}{where}")
    return t
