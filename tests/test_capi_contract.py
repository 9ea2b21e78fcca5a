"""CPU-side checks of the C ABI's contract, for every public header under include/: what every entry point answers to a call it must
refuse, through the library's ONE thread-local error slot, and the ctypes binding (the one table v2v_amd/_lib.py:HEADERS) against the
headers' prototypes.  No GPU: every call here fails argument validation before any HIP call.

The expected statuses and messages were recorded from the build of the commit before the entry points moved next to their launchers
(the dynamic decoder's training entry points then kept their text behind v2v_hyper_train_last_error(); read through v2v_last_error(),
those nine `_hip` calls returned the stale text of the failing call before them); those of the four newer headers from the build of the
commit before this module covered them."""
import ctypes as C
import os
import re
import threading

import pytest

from capi_calls import _D, _d, _zero

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from v2v_amd import _lib
    return _lib


# every export whose name ends in _hip, called with every pointer NULL and every number 0: (status, message).  v2v_hip.h's 80 answer
# V2V_ERR_NULL; an entry point of the newer headers that checks its shape first answers V2V_ERR_SHAPE
NULL_CALLS = {name: (-1, message) for name, message in {
    "v2v_esim_voxel_hip": "v2v_esim_voxel_hip: frames/params/out_voxel is NULL",
    "v2v_esim_voxel_keyed_hip": "v2v_esim_voxel_hip: frames/params/out_voxel is NULL",
    "v2v_esim_voxel_padded_hip": "v2v_esim_voxel_hip: frames/params/out_voxel is NULL",
    "v2v_synth_clips_hip": "v2v_synth_clips_hip: frames is NULL",
    "v2v_events_to_voxel_segmented_hip": "v2v_events_to_voxel: out_voxel/dropped is NULL",
    "v2v_v2e_voxel_hip": "v2v_v2e_voxel_hip: frames/params/out_voxel is NULL",
    "v2v_events_to_voxel_hip": "v2v_events_to_voxel: out_voxel/dropped is NULL",
    "v2v_frontend_hip": "v2v_frontend_hip: src/frame_idx/out_gray is NULL",
    "v2v_frontend_batch_hip": "v2v_frontend_batch_hip: src/clip_table/frame_idx/out_gray is NULL",
    "v2v_normalize_pad_hip": "v2v_normalize_pad_hip: voxel/out is NULL",
    "v2v_normalize_pad_ex_hip": "v2v_normalize_pad_hip: voxel/out is NULL",
    "v2v_events_to_voxel_f32_hip": "v2v_events_to_voxel_f32_hip: out_voxel/dropped is NULL",
    "v2v_events_to_voxel_f32_segmented_hip": "v2v_events_to_voxel_f32_segmented_hip: seg_offsets is NULL",
    "v2v_convlstm_pack_weights_hip": "v2v_convlstm_pack_weights_hip: gates_weight/packed is NULL",
    "v2v_convlstm_step_hip": "v2v_convlstm_step_hip: x/packed/gates_bias/h_state/c_state is NULL",
    "v2v_convgru_pack_weights_hip": "v2v_convgru_pack_weights_hip: a weight or packed pointer is NULL",
    "v2v_convgru_step_hip": "v2v_convgru_step_hip: x/packed_gates/packed_cand/gates_bias/out_bias/u_ws/hr_ws/h_state/h_state_f32 is NULL",
    "v2v_convgru16_pack_weights_hip": "v2v_convgru16_pack_weights_hip: a weight or packed pointer is NULL",
    "v2v_convgru16_step_hip": "v2v_convgru16_step_hip: x/packed/gates_bias/out_bias/h_state/h_state_f32 is NULL",
    "v2v_resblock16_pack_weights_hip": "v2v_resblock16_pack_weights_hip: w1/w2/packed is NULL",
    "v2v_resblock16_nhwc_hip": "v2v_resblock16_nhwc_hip: x/packed/b1/b2/out is NULL",
    "v2v_conv_head16_pack_weights_hip": "v2v_conv_head16_pack_weights_hip: weight/packed is NULL",
    "v2v_conv_head16_nhwc_hip": "v2v_conv_head16_nhwc_hip: x8/packed/bias/out is NULL",
    "v2v_conv3x3_pack_weights_hip": "v2v_conv_pack_weights_hip: weight/packed is NULL",
    "v2v_conv3x3_nhwc_hip": "v2v_conv_nhwc_hip: x/packed/bias/out is NULL",
    "v2v_conv_pack_weights_hip": "v2v_conv_pack_weights_hip: weight/packed is NULL",
    "v2v_conv_nhwc_hip": "v2v_conv_nhwc_hip: x/packed/bias/out is NULL",
    "v2v_upsample2x_nhwc_hip": "v2v_upsample2x_nhwc_hip: x/out is NULL",
    "v2v_conv_head_pack_weights_hip": "v2v_conv_head_pack_weights_hip: weight/packed is NULL",
    "v2v_to_nhwc8_bf16_hip": "v2v_to_nhwc8_bf16_hip: src/dst is NULL",
    "v2v_to_nhwc8_bf16_scaled_hip": "v2v_to_nhwc8_bf16_hip: src/dst is NULL",
    "v2v_conv_head_nhwc_hip": "v2v_conv_head_nhwc_hip: x8/packed/bias/out is NULL",
    "v2v_conv1x1_nhwc_hip": "v2v_conv1x1_nhwc_hip: x/weight/bias/out is NULL",
    "v2v_nchw_to_nhwc_bf16_hip": "v2v_nchw_to_nhwc_bf16_hip: src/dst is NULL",
    "v2v_convlstm_step_bwd_hip": "v2v_convlstm_step_bwd_hip: x/packed/bias/dh/dgates/dc_prev is NULL",
    "v2v_relu_bwd_nhwc_hip": "v2v_relu_bwd_nhwc_hip: dy/out is NULL",
    "v2v_conv_dgrad_pack_weights_hip": "v2v_conv_dgrad_pack_weights_hip: weight/scratch/packed is NULL",
    "v2v_conv_dgrad_nhwc_hip": "v2v_conv_dgrad_nhwc_hip: dy/packed/workspace/dx is NULL",
    "v2v_conv_wgrad_nhwc_hip": "v2v_conv_wgrad_nhwc_hip: dy/x1/workspace/dw is NULL",
    "v2v_upsample2x_bwd_nhwc_hip": "v2v_upsample2x_bwd_nhwc_hip: dout/dx is NULL",
    "v2v_conv1x1_bwd_nhwc_hip": "v2v_conv1x1_bwd_nhwc_hip: a required pointer is NULL",
    "v2v_esim_voxel_ex_hip": "v2v_esim_voxel_hip: frames/params/out_voxel is NULL",
    "v2v_esim_voxel_stats_hip": "v2v_esim_voxel_stats_hip: stats is NULL",
    "v2v_voxel_scales_hip": "v2v_voxel_scales_hip: stats/scales is NULL",
    "v2v_voxel_apply_scales_hip": "v2v_voxel_apply_scales_hip: voxel/out is NULL",
    "v2v_voxel_scales_select_hip": "v2v_voxel_scales_select_hip: voxel/scales/workspace is NULL",
    "v2v_clip_frames_f32_hip": "v2v_clip_frames_f32_hip: src/out is NULL",
    "v2v_clip_frames_f32_ex_hip": "v2v_clip_frames_f32_hip: src/out is NULL",
    "v2v_clip_frames_f32_bounded_hip": "v2v_clip_frames_f32_hip: src/out is NULL",
    "v2v_conv_stem_pack_weights_hip": "v2v_conv_stem_pack_weights_hip: weight/packed is NULL",
    "v2v_conv_stem_nhwc_hip": "v2v_conv_stem_nhwc_hip: x8/packed/bias/out is NULL",
    "v2v_upsample2x_cat_nhwc_hip": "v2v_upsample2x_cat_nhwc_hip: x/out (or skip with C2 > 0) is NULL",
    "v2v_upsample2x_cat_bwd_nhwc_hip": "v2v_upsample2x_cat_bwd_nhwc_hip: dout/dx is NULL",
    "v2v_conv1x1_bwd_cout_nhwc_hip": "v2v_conv1x1_bwd_cout_nhwc_hip: a required pointer is NULL",
    "v2v_conv_nhwc_like_hip": "v2v_conv_nhwc_like_hip: x/packed/bias/out is NULL",
    "v2v_hyper_context_hip": "v2v_hyper_context_hip: events/prev/dst is NULL",
    "v2v_hyper_context_conv_hip": "v2v_hyper_context_conv_hip: x8/weight/bias/out is NULL",
    "v2v_tanh_bf16_hip": "v2v_tanh_bf16_hip: x/out is NULL",
    "v2v_hyper_atoms_hip": "v2v_hyper_atoms_hip: coeff/bases/atoms is NULL",
    "v2v_hyper_dynconv_pack_weights_hip": "v2v_hyper_dynconv_pack_weights_hip: weight/packed is NULL",
    "v2v_hyper_dynconv_nhwc_hip": "v2v_hyper_dynconv_nhwc_hip: x/atoms/packed/bias/out is NULL",
    # the nine below: recorded from v2v_hyper_train_last_error() (see the module docstring)
    "v2v_hyper_dynconv_pack_t_hip": "v2v_hyper_dynconv_pack_t_hip: weight/packed_t is NULL",
    "v2v_hyper_dynconv_df_hip": "v2v_hyper_dynconv_df_hip: dz/packed_t/dF is NULL",
    "v2v_hyper_dynconv_datoms_hip": "v2v_hyper_dynconv_datoms_hip: x/dF/datoms is NULL",
    "v2v_hyper_dynconv_dx_hip": "v2v_hyper_dynconv_dx_hip: atoms/dF/dx is NULL",
    "v2v_hyper_dynconv_wgrad_hip": "v2v_hyper_dynconv_wgrad_hip: dz/x/atoms/workspace/dw/db is NULL",
    "v2v_hyper_bn_stats_hip": "v2v_hyper_bn_stats_hip: z/mean/var/rstd is NULL",
    "v2v_hyper_bn_apply_hip": "v2v_hyper_bn_apply_hip: a pointer is NULL",
    "v2v_hyper_bn_bwd_hip": "v2v_hyper_bn_bwd_hip: a pointer is NULL",
    "v2v_hyper_atoms_bwd_hip": "v2v_hyper_atoms_bwd_hip: datoms/pre/bases/dpre is NULL",
    "v2v_tc_loss_fwd_hip": "v2v_tc_loss_fwd_hip: image1/processed1 is NULL",
    "v2v_tc_loss_bwd_hip": "v2v_tc_loss_bwd_hip: image1/processed1 is NULL",
    "v2v_warp_bilinear_hip": "v2v_warp_bilinear_hip: img/flow/out is NULL",
    "v2v_warp_bilinear_adjoint_hip": "v2v_warp_bilinear_adjoint_hip: dout/flow/din/workspace is NULL",
    "v2v_lpips_stem_hip": "v2v_lpips_stem_hip: x/weight/bias/shift/scale/out is NULL",
    "v2v_lpips_stem_bwd_hip": "v2v_lpips_stem_bwd_hip: dz/weight/scale/dpred is NULL",
    "v2v_lpips_pool_hip": "v2v_lpips_pool_hip: x/out is NULL",
    "v2v_lpips_pool_bwd_hip": "v2v_lpips_pool_bwd_hip: dy/x/dx is NULL",
    "v2v_lpips_compare_fwd_hip": "v2v_lpips_compare_fwd_hip: f0/f1/w/dist/workspace is NULL",
    "v2v_lpips_compare_bwd_hip": "v2v_lpips_compare_bwd_hip: f0/f1/w/ddist/df0 is NULL",
}.items()}
NULL_CALLS.update({
    "v2v_learned_voxel_stats_hip": (-1, "v2v_learned_voxel_stats_hip: events/workspace is NULL"),
    "v2v_learned_voxel_hip": (-1, "v2v_learned_voxel_hip: events/workspace is NULL"),
    "v2v_image_metrics_hip": (-2, "v2v_image_metrics_hip: the 7x7 window needs H >= 7 and W >= 7 (got 0 x 0)"),
    "v2v_flow_metrics_hip": (-2, "v2v_flow_metrics_hip: need H, W >= 1 and H * W < 2^24, the reference's float32 counts (got 0 x 0)"),
    "v2v_lpips_alex_stem_hip": (-2, "v2v_lpips_alex_stem_hip: a frame has 1 or 3 channels (got 0)"),
    "v2v_lpips_alex_conv_hip": (-2, "v2v_lpips_alex_conv_hip: ks must be 3 or 5 (got 0)"),
    "v2v_lpips_alex_pool_hip": (-2, "v2v_lpips_alex_pool_hip: C must be a multiple of 4 (got 0)"),
    "v2v_lpips_alex_compare_hip": (-2, "v2v_lpips_alex_compare_hip: need HW >= 1 and [n,HW,384] below 2^31 elements (got n 0, HW 0)"),
    "v2v_lpips_alex_sum_hip": (0, None),           # a count of 0 is V2V_OK without a launch, and n is all this entry point has
    "v2v_alex_train_compare_bwd_hip": (-2, "v2v_alex_train_compare_bwd_hip: need HW >= 1 and [n,HW,384] below 2^31 elements (got n 0, HW 0)"),
    "v2v_alex_train_conv_dgrad_hip": (-2, "v2v_alex_train_conv_dgrad_hip: ks must be 3 or 5 (got 0)"),
    "v2v_alex_train_pool_bwd_hip": (-2, "v2v_alex_train_pool_bwd_hip: C must be a multiple of 4 (got 0)"),
    "v2v_alex_train_stem_bwd_hip": (-2, "v2v_alex_train_stem_bwd_hip: a frame has 1 or 3 channels (got 0)"),
})


def _null_call(L, name):
    return getattr(L.lib(), name)(*_zero(L.SIGNATURES[name][1]))


def test_null_table_covers_every_hip_export(L):
    assert sorted(NULL_CALLS) == sorted(n for n in L.SIGNATURES if n.endswith("_hip")) and len(NULL_CALLS) == 93
    assert (L.ERR_NULL, L.ERR_SHAPE, L.OK) == (-1, -2, 0) and all(NULL_CALLS[n][0] == L.ERR_NULL for n in L.HEADERS["v2v_hip.h"] if n in NULL_CALLS)


@pytest.mark.parametrize("name", sorted(NULL_CALLS))
def test_null_call_status_and_message(L, name):
    lib = L.lib()
    status, message = NULL_CALLS[name]
    assert _null_call(L, name) == status
    if status != L.OK:
        assert lib.v2v_last_error().decode() == message
        assert lib.v2v_hyper_train_last_error() == lib.v2v_last_error()        # the deprecated alias reads the same slot


def test_error_slot_is_per_thread(L):
    lib = L.lib()
    assert _null_call(L, "v2v_conv_nhwc_hip") == L.ERR_NULL
    mine = lib.v2v_last_error()
    seen = {}

    def other():
        seen["before"] = lib.v2v_last_error()
        seen["rc"] = _null_call(L, "v2v_hyper_dynconv_df_hip")
        seen["after"] = lib.v2v_last_error()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["rc"] == L.ERR_NULL and seen["before"] == b"" and seen["after"] == NULL_CALLS["v2v_hyper_dynconv_df_hip"][1].encode()
    assert lib.v2v_last_error() == mine == NULL_CALLS["v2v_conv_nhwc_hip"][1].encode()


# per family whose entry points moved next to their launchers (and the dynamic decoder's training family, whose error slot moved): one
# shape and one alignment failure.  Dummy non-null pointers, never dereferenced: every case fails validation before any HIP call.
_ODD = C.c_void_p(_D + 8)                        # 8-byte aligned only

VALIDATION_CASES = {
    "convlstm shape": ("v2v_conv_nhwc_hip", lambda: [_d(), _d(1), _d(2), None, 0, 1, 4, 4, 48, 64, 3, 1, _d(3), 0, None], -2,
                       "need B,H,W >= 1, Cin % 64 == 0 (or Cin 32 with Cout 64 / 128), Cout in {32, 64, 128} or a multiple of 256"),
    "convlstm align": ("v2v_conv_nhwc_hip", lambda: [_ODD, _d(1), _d(2), None, 0, 1, 4, 4, 64, 64, 3, 1, _d(3), 0, None], -6,
                       "x/packed need 16-byte alignment"),
    "convlstm step shape": ("v2v_convlstm_step_hip", lambda: [_d(), _d(1), _d(2), _d(3), _d(4), 1, 4, 4, 48, _d(5), _d(6), None, 0, 0, None], -2,
                            "need B,H,W >= 1 and C % 64 == 0, C <= 4096"),
    "convlstm step align": ("v2v_convlstm_step_hip", lambda: [_ODD, _d(1), _d(2), _d(3), _d(4), 1, 4, 4, 64, _d(5), _d(6), None, 0, 0, None], -6,
                            "x/h_prev/packed/h_nchw need 16-byte alignment"),
    "dgrad shape": ("v2v_conv_dgrad_nhwc_hip", lambda: [_d(), _d(1), None, 1, 4, 4, 64, 12, 3, 1, _d(2), _d(3), None], -2,
                    "need the transposed convolution Cout -> Cin to be a shape the convolution kernel takes, Hin, Win multiples of the stride, "
                    "(Hin*Win) % 4 == 0, tensors below 2^31 elements"),
    "dgrad align": ("v2v_conv_dgrad_nhwc_hip", lambda: [_d(), _d(1), None, 1, 4, 4, 64, 64, 3, 1, C.c_void_p(_D * 3 + 16), _d(3), None], -6,
                    "dy/packed need 16-byte, workspace 256-byte alignment"),
    "convgru shape": ("v2v_convgru_step_hip", lambda: [_d(), _d(1), _d(2), _d(3), _d(4), _d(5), _d(6), 1, 4, 4, 48, _d(7), _d(8), _d(9), _d(10), None, 0, 0, 0, None],
                      -2, "need B,H,W >= 1 and C % 64 == 0, C <= 4096"),
    "convgru align": ("v2v_convgru_step_hip", lambda: [_ODD, _d(1), _d(2), _d(3), _d(4), _d(5), _d(6), 1, 4, 4, 64, _d(7), _d(8), _d(9), _d(10), None, 0, 0, 0, None],
                      -6, "x/h_prev/hr_ws/packed_gates/packed_cand/h_nchw need 16-byte alignment"),
    "narrow shape": ("v2v_resblock16_nhwc_hip", lambda: [_d(), _d(1), _d(2), _d(3), 0, 4, 4, _d(4), None], -2,
                     "v2v_resblock16_nhwc_hip: need B,H,W >= 1 and B*H*W*16 < 2^31 (got 0x4x4)"),
    "narrow align": ("v2v_resblock16_nhwc_hip", lambda: [_ODD, _d(1), _d(2), _d(3), 1, 4, 4, _d(4), None], -6, "x/packed/out need 16-byte alignment"),
    "train shape": ("v2v_relu_bwd_nhwc_hip", lambda: [_d(), _d(1), 16, 4, _d(2), None], -2, "need M >= 1, C % 8 == 0, M*C below 2^31"),
    "train align": ("v2v_relu_bwd_nhwc_hip", lambda: [_ODD, _d(1), 16, 8, _d(2), None], -6, "dy/y/out need 16-byte alignment"),
    "wgrad shape": ("v2v_conv_wgrad_nhwc_hip", lambda: [_d(), _d(1), 64, None, 0, 64, 1, 4, 4, 48, 3, 1, _d(2), _d(3), None, None], -2,
                    "need B,H,W >= 1, C1 >= 1, 1 <= Cin_out <= C1 + C2, Cout a multiple of 32, tensors below 2^31 elements"),
    "wgrad align": ("v2v_conv_wgrad_nhwc_hip", lambda: [C.c_void_p(_D + 1), _d(1), 64, None, 0, 64, 1, 4, 4, 64, 3, 1, _d(2), _d(3), None, None], -6,
                    "buffers misaligned"),
    "hyper shape": ("v2v_hyper_dynconv_nhwc_hip", lambda: [_d(), _d(1), _d(2), _d(3), 1, 1, 8, 16, 128, 128, 6, 5, _d(4), None], -2,
                    "the dynamic convolution takes Cin 256, Cout 128, 6 atoms, a 5 x 5 window (got 128 -> 128, 6 atoms, ks 5)"),
    "hyper align": ("v2v_hyper_dynconv_nhwc_hip", lambda: [_ODD, _d(1), _d(2), _d(3), 1, 1, 8, 16, 256, 128, 6, 5, _d(4), None], -6,
                    "x/packed need 16-byte, atoms 8-byte alignment"),
    "hyper train shape": ("v2v_hyper_dynconv_df_hip", lambda: [_d(), _d(1), 0, _d(2), None], -2, "need 1 <= M and M * 1536 below 2^33"),
    "hyper train align": ("v2v_hyper_dynconv_df_hip", lambda: [_ODD, _d(1), 32, _d(2), None], -6, "dz/packed_t/dF need 16-byte alignment"),
    "loss shape": ("v2v_warp_bilinear_hip", lambda: [_d(), _d(1), 1, 1, 1, 8, _d(2), None], -2,
                   "v2v_warp_bilinear_hip: h and w must be at least 2, the sampling grid divides by h - 1 and w - 1 (got 1 x 8)"),
    "loss align": ("v2v_warp_bilinear_hip", lambda: [C.c_void_p(_D + 2), _d(1), 1, 1, 8, 8, _d(2), None], -6,
                   "v2v_warp_bilinear_hip: float32 pointers need 4-byte alignment"),
    "tc loss shape": ("v2v_tc_loss_fwd_hip", lambda: [_d(), _d(1), _d(2), _d(3), _d(4), 1, 1, 64, 64, 128, 128, 0, 1, 8, 1 << 20, 50.0, 1.0, 1.0, 0.0, 0.0, _d(5),
                                                      None, None, None, None, _d(6), None], -2,
                      "v2v_tc_loss_fwd_hip: h*w = 8388608 is above 2^22, the bound of the adjoint's fixed-point accumulator"),
    "tc loss align": ("v2v_tc_loss_fwd_hip", lambda: [_d(), _d(1), _d(2), _d(3), _d(4), 1, 1, 64, 64, 128, 128, 0, 1, 8, 8, 50.0, 1.0, 1.0, 0.0, 0.0, _d(5),
                                                      None, None, None, None, _ODD, None], -6,
                      "v2v_tc_loss_fwd_hip: losses needs 4-byte, workspace 16-byte alignment"),
    "lpips shape": ("v2v_lpips_pool_hip", lambda: [_d(), 1, 3, 4, 64, _d(1), None], -2,
                    "v2v_lpips_pool_hip: need B >= 1, H and W even, C a multiple of 8, the tensor below 2^31 elements (got 1 x 3 x 4 x 64)"),
    "lpips align": ("v2v_lpips_pool_hip", lambda: [_ODD, 1, 4, 4, 64, _d(1), None], -6, "v2v_lpips_pool_hip: x/out need 16-byte alignment"),
}


@pytest.mark.parametrize("case", sorted(VALIDATION_CASES))
def test_validation_status_and_message(L, case):
    name, args, status, message = VALIDATION_CASES[case]
    lib = L.lib()
    rc = getattr(lib, name)(*args())
    assert rc not in (L.OK, L.ERR_HIP), "the case must fail validation before any HIP call"
    assert rc == status == (L.ERR_SHAPE if case.endswith("shape") else L.ERR_ALIGN)
    assert lib.v2v_last_error().decode() == message
    assert lib.v2v_hyper_train_last_error() == lib.v2v_last_error()


# ---- the binding against the header ---------------------------------------------------------------------------------------------------
def _c_class(decl):
    decl = " ".join(decl.split())
    if "*" in decl:
        return "pointer"
    words = decl.split()
    for t, cls in (("int64_t", "i64"), ("uint64_t", "i64"), ("int32_t", "i32"), ("uint32_t", "i32"), ("int", "i32"), ("float", "float"), ("double", "double")):
        if t in words:
            return cls
    raise AssertionError(f"unknown C type in {decl!r}")


def _ctypes_class(t):
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    return {C.c_int64: "i64", C.c_uint64: "i64", C.c_int: "i32", C.c_uint32: "i32", C.c_int32: "i32", C.c_float: "float", C.c_double: "double"}[t]


def _header_prototypes(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(v2v_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        params = [p for p in (q.strip() for q in params.split(",")) if p and p != "void"]
        protos[name] = (_c_class(ret), [_c_class(p) for p in params])
    return protos


# entry points per header, and the names the newer headers were introduced with (v2v_nernet.h: its two launching ones)
HEADER_ENTRIES = {"v2v_hip.h": 106, "v2v_nernet.h": 4, "v2v_metrics.h": 4, "v2v_lpips_alex.h": 6, "v2v_alex_train.h": 4}
PINNED_NAMES = {
    "v2v_nernet.h": ["v2v_learned_voxel_stats_hip", "v2v_learned_voxel_hip"],
    "v2v_metrics.h": ["v2v_image_metrics_workspace_bytes", "v2v_image_metrics_hip", "v2v_flow_metrics_workspace_bytes", "v2v_flow_metrics_hip"],
    "v2v_lpips_alex.h": ["v2v_lpips_alex_stem_hip", "v2v_lpips_alex_conv_hip", "v2v_lpips_alex_pool_hip", "v2v_lpips_alex_compare_workspace_bytes",
                         "v2v_lpips_alex_compare_hip", "v2v_lpips_alex_sum_hip"],
    "v2v_alex_train.h": ["v2v_alex_train_compare_bwd_hip", "v2v_alex_train_conv_dgrad_hip", "v2v_alex_train_pool_bwd_hip", "v2v_alex_train_stem_bwd_hip"],
}


@pytest.mark.parametrize("header", HEADER_ENTRIES)
def test_binding_matches_header_prototypes(L, header):
    protos, table = _header_prototypes(header), L.HEADERS[header]
    assert list(protos) == list(table), "the header's table lists the header's entry points, in the header's order"
    for name, (res, args) in table.items():
        want_res, want_args = protos[name]
        assert _ctypes_class(res) == want_res, name
        assert len(args) == len(want_args), (name, len(args), len(want_args))
        got = [_ctypes_class(t) for t in args]
        assert got == want_args, (name, [i for i, (g, w) in enumerate(zip(got, want_args)) if g != w])
    if header != "v2v_hip.h":
        assert '#include "v2v_hip.h"' in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_one_table_over_the_headers(L):
    assert list(L.HEADERS) == list(HEADER_ENTRIES) and {h: len(t) for h, t in L.HEADERS.items()} == HEADER_ENTRIES
    assert sum(len(t) for t in L.HEADERS.values()) == len(L.SIGNATURES) == 124, "no name in two headers"
    assert L.EXPORTS == tuple(L.SIGNATURES) == tuple(n for t in L.HEADERS.values() for n in t)
    assert sum(n.endswith("_hip") for n in L.SIGNATURES) == 93
    for header, names in PINNED_NAMES.items():
        assert [n for n in L.HEADERS[header] if header != "v2v_nernet.h" or n.endswith("_hip")] == names
    assert not any(n.startswith("v2v_lpips_alex_") for n in L.HEADERS["v2v_alex_train.h"])
    lib = L.lib()
    for name in L.SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.v2v_version() == L.ABI_VERSION == 6


def test_library_holds_no_other_name_of_the_alex_families(L):
    """the names in the library's bytes (its dynamic symbol table, the entry points' own names in their messages) are the declared ones --
    but for one translation unit's own name, which the Makefile hands to the compiler as the compilation-unit id"""
    blob = open(L.LIB_PATH, "rb").read()
    assert set(n.decode() for n in re.findall(rb"v2v_lpips_alex_[a-z0-9_]+", blob)) == set(L.HEADERS["v2v_lpips_alex.h"])
    assert set(n.decode() for n in re.findall(rb"v2v_alex_train_[a-z0-9_]+", blob)) - {"v2v_alex_train_tu"} == set(L.HEADERS["v2v_alex_train.h"])
