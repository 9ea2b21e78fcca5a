/*
 * v2v_nam.h -- C ABI of the operators of NER-Net's recurrent network (UNetNIAM_STcell_GCB of the reference) in libv2v_hip.so (gfx950).
 * An extension of v2v_hip.h under the same rules: device pointers, sizes and a stream; a v2v_status comes back and its text is behind
 * v2v_last_error(); no entry point allocates or synchronises; arguments are validated before any HIP call.  Additive: v2v_version()
 * stays 6, and the binding keeps these rows in a table of their own (v2v_amd/_lib.py: HEADERS_MORE).
 *
 * The NAM cell (NAM_withoutGCB.forward, model/nernet/submodules.py:585-642 of the reference; formulas and the packed layout in
 * v2v_amd/csrc/v2v_nam.hpp), one call = three launches on the matrix cores, bf16 operands, fp32 accumulation and gate arithmetic:
 *
 *   v2v_nam_pack_weights_hip   conv_x [7C,C,3,3], conv_h [4C,C,3,3], conv_m [3C,C,3,3], conv_o [C,2C,3,3], conv_last [C,2C], LAG_conv [C,C]
 *                              (float32, the module's tensors) -> packed bf16 [v2v_nam_packed_elems(C)], the three launches' streams
 *   v2v_nam_step_hip           x, m_t [B,H,W,C] bf16 NHWC; h_prev bf16 and c_prev float32, both NULL = the zero state; C in {64, 128, 256},
 *                              (H*W) % 4 == 0.  Written: m_state bf16 (+ m_state_f32 when not NULL), c_state float32 (may be c_prev) and
 *                              c_state_bf16 = its RNE copy, h_state bf16 = the RNE copy of h_state_f32, optionally h as [B,C,H,W] in
 *                              h_nchw_dtype; alpha_ws = exp(sigmoid(LAG_conv(x))) and o_pre_ws = o_x + o_h, float32 [B,H,W,C] each, are
 *                              the workspaces between the launches.  tile: 0 by shape, 1 = 64-pixel, 2 = 128-pixel workgroup tiles.
 *                              Hv, Wv: the valid extent of the canvas (1 <= Hv <= H, 1 <= Wv <= W).  Smaller than the canvas, the bf16
 *                              outputs m_state, c_state_bf16 (in front of the last launch, whose 3x3 window reads them) and h_state are
 *                              cleared outside it; the operands must be zero there already.  The float32 outputs are not touched.
 *
 * The global context block with the 1x1 convolution in front of it and the residual behind it (RecurrentConvLayer_NAM_GCB.forward,
 * model/nernet/submodules.py:747-778 and ContextBlock2d, :365-442 of the reference), per image and in float32 arithmetic:
 *
 *     g = conv_1x1(x);  w = softmax over the valid pixels of conv_mask(g);  ctx[c] = sum_p g[c, p] w[p]
 *     add = wb . PReLU(LayerNorm(wa . ctx + ba)) + bb;  out = bf16(x + g + add)
 *
 * x, out    [B,H,W,C] bfloat16 (the canvas), C in {32, 64, 128}, 16-byte aligned, not the same buffer.
 * Hv, Wv    the valid extent, 1 <= Hv <= H, 1 <= Wv <= W: only pixels with row < Hv and column < Wv are pooled; x is read as zero and out
 *           is written as zero outside it (what the stride-2 convolution behind the block has to find there).
 * w1t       float32 [C][C]: w1t[ci][co] = conv_1x1.weight[co, ci], the TRANSPOSE of the module's tensor;  b1 float32 [C]
 * wmask     float32 [C] = GCB.conv_mask.weight;  bmask float32 [1] its bias (device memory)
 * wa, ba    float32 [C/4][C], [C/4] = GCB.channel_add_conv.0;  ln_w, ln_b float32 [C/4] = .1 (LayerNorm, eps as given);  prelu float32 [1] = .2
 * wb, bb    float32 [C][C/4], [C] = GCB.channel_add_conv.3
 * workspace v2v_gcb_workspace_bytes(B, H, W, C) bytes, 4-byte aligned: the per-tile softmax partials, written and read by the call
 * ctx_add   float32 [B][2][C], written: the pooled context and the channel-add term of every image
 *
 * The result is bitwise the same from run to run: the pooling is a two-level reduction in an order the shape alone fixes, no atomics.
 *
 * The head for 9 to 16 input channels (ConvLayer(2 * num_bins = 10, 32, 5, padding=2) + ReLU; v2v_conv_head_nhwc_hip of v2v_hip.h takes 8 at
 * most): v2v_to_nhwc16_bf16_hip turns float32 [B,C,H,W] of any non-negative element strides into bf16 [B,H,W,16] with the channels
 * zero-padded; v2v_conv_head16in_pack_weights_hip turns the weight float32 [32,Cin,5,5] into packed bf16
 * [v2v_conv_head16in_packed_elems()]; v2v_conv_head16in_nhwc_hip computes out = [relu](conv5x5(x16, pad 2) + bias), bf16 [B,H,W,32],
 * for any H and W: one v_mfma_f32_32x32x16_bf16 per tap, fp32 accumulation, one rounding.
 *
 * v2v_valid_extent_nhwc_hip: in place on an NHWC canvas [B,H,W,C] of float32 or bfloat16 (C a whole number of 16-byte pieces): pixels
 * outside the valid extent are cleared; with replicate != 0 the first row and the first column outside (row Hv, column Wv) take the
 * nearest valid pixel instead, which makes the x2 upsampling's read past the last valid row / column the reference's clamped read.
 * Hv == H and Wv == W is V2V_OK without a launch.
 */
#ifndef V2V_NAM_H
#define V2V_NAM_H

#include "v2v_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t v2v_nam_packed_elems(int64_t C);
int v2v_nam_pack_weights_hip(const float *conv_x, const float *conv_h, const float *conv_m, const float *conv_o, const float *conv_last, const float *lag_conv,
                             int64_t C, void *packed, void *stream);
int v2v_nam_step_hip(const void *x, const void *m_t, const void *h_prev, const float *c_prev, const void *packed, int64_t B, int64_t H, int64_t W, int64_t C,
                     float *alpha_ws, float *o_pre_ws, void *m_state, float *m_state_f32, float *c_state, void *c_state_bf16, void *h_state,
                     float *h_state_f32, void *h_nchw, int h_nchw_dtype, int tile, int64_t Hv, int64_t Wv, void *stream);
int64_t v2v_gcb_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t C);
int v2v_gcb_nhwc_hip(const void *x, const float *w1t, const float *b1, const float *wmask, const float *bmask, const float *wa, const float *ba,
                     const float *ln_w, const float *ln_b, const float *prelu, const float *wb, const float *bb, float eps, int64_t B, int64_t H,
                     int64_t W, int64_t C, int64_t Hv, int64_t Wv, void *workspace, int64_t workspace_bytes, float *ctx_add, void *out, void *stream);
int64_t v2v_conv_head16in_packed_elems(void);
int v2v_conv_head16in_pack_weights_hip(const float *weight, int64_t Cin, void *packed, void *stream);
int v2v_to_nhwc16_bf16_hip(const float *src, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, int64_t B, int64_t C, int64_t H, int64_t W,
                           void *dst, void *stream);
int v2v_conv_head16in_nhwc_hip(const void *x16, const void *packed, const float *bias, int relu, int64_t B, int64_t H, int64_t W, void *out, void *stream);
int v2v_valid_extent_nhwc_hip(void *x, int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int64_t Hv, int64_t Wv, int replicate, void *stream);

#ifdef __cplusplus
}
#endif
#endif
