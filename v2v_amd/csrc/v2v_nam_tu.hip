// v2v_nam_tu.hip -- translation unit of NER-Net's recurrent network (include/v2v_nam.h): the NAM cell -- the EPI = 5 / 6 / 7 instances of
// convlstm_step_kernel (main loop in v2v_convlstm.hpp, epilogues / packing / layouts in v2v_nam.hpp) -- the global context block and the
// valid-extent helper (v2v_gcb.hpp) and the head for 9 to 16 input channels (v2v_nam_head.hpp), with their launchers and C entry points.
#include "../../include/v2v_nam.h"
#include "v2v_nam.hpp"
#include "v2v_gcb.hpp"
#include "v2v_nam_head.hpp"
#include "v2v_status.hpp"

using v2v::aligned;
using v2v::fail;
using v2v::hip_fail;
using v2v::launched;

namespace {

constexpr int64_t kMaxElems = 0x7FFFFFFFLL;

// Instance codes of the cell (v2v_nam_step_hip's tile; 0 = by shape), pixels x columns per workgroup:
//   1: M and C 64 x 256, H 64 x 128 (two stages)        2: M and C 128 x 256, H 128 x 128 (three stages)
// the tiles launch_convlstm_step and launch_convgru_gates ship under the same numbers.  By shape: the 128-pixel tiles once they give every
// CU a workgroup, the rule of launch_convlstm_step; nothing NAM-specific has been measured yet.
template <int EPI>
hipError_t launch_nam_4c(const v2v::ConvLstmArgs &a0, int tile, hipStream_t s)
{
    v2v::ConvLstmArgs a = a0;
    a.pack_cols = 256;
    return tile == 2 ? v2v::launch_step_t<1, 4, 3, EPI, 2, 4>(a, s) : v2v::launch_step_t<1, 2, 2, EPI, 2, 4>(a, s);
}

hipError_t launch_nam_h(const v2v::ConvLstmArgs &a0, int tile, hipStream_t s)
{
    v2v::ConvLstmArgs a = a0;
    a.pack_cols = v2v::nam_h_pack_cols(a.C);
    return tile == 2 ? v2v::launch_step_t<1, 4, 3, 7, 2, 2>(a, s) : v2v::launch_step_t<1, 2, 2, 7, 2, 2>(a, s);
}

int nam_channels_check(const char *who, int64_t C)
{
    if (C != 64 && C != 128 && C != 256) return fail(V2V_ERR_SHAPE, "%s: C must be 64, 128 or 256 (got %lld)", who, (long long)C);
    return V2V_OK;
}

// B, H, W, C and the valid extent of a canvas, shared by the entry points
int canvas_check(const char *who, int64_t B, int64_t H, int64_t W, int64_t Hv, int64_t Wv)
{
    if (B < 1 || H < 1 || W < 1 || B > 65535 || H > kMaxElems || W > kMaxElems)
        return fail(V2V_ERR_SHAPE, "%s: need 1 <= B <= 65535 and H, W >= 1 (got %lld x %lld x %lld)", who, (long long)B, (long long)H, (long long)W);
    if (Hv < 1 || Wv < 1 || Hv > H || Wv > W)
        return fail(V2V_ERR_SHAPE, "%s: the valid extent %lld x %lld must lie inside the canvas %lld x %lld and hold a pixel", who, (long long)Hv, (long long)Wv,
                    (long long)H, (long long)W);
    return V2V_OK;
}

int gcb_channels_check(const char *who, int64_t C)
{
    if (C != 32 && C != 64 && C != 128) return fail(V2V_ERR_SHAPE, "%s: C must be 32, 64 or 128 (got %lld)", who, (long long)C);
    return V2V_OK;
}

int64_t gcb_tiles(int64_t H, int64_t W) { return (H * W + v2v::kGcbPix - 1) / v2v::kGcbPix; }

template <int C>
int launch_gcb(const v2v::GcbArgs &a, hipStream_t s)
{
    const dim3 grid((unsigned)a.tiles, (unsigned)a.B), block(v2v::kGcbThreads);
    hipLaunchKernelGGL((v2v::gcb_tile_kernel<C, false>), grid, block, 0, s, a);
    if (const int rc = launched("gcb_tile_kernel (pooling) launch")) return rc;
    hipLaunchKernelGGL((v2v::gcb_combine_kernel<C>), dim3((unsigned)a.B), block, 0, s, a);
    if (const int rc = launched("gcb_combine_kernel launch")) return rc;
    hipLaunchKernelGGL((v2v::gcb_tile_kernel<C, true>), grid, block, 0, s, a);
    return launched("gcb_tile_kernel (apply) launch");
}

}  // namespace

extern "C" {

int64_t v2v_nam_packed_elems(int64_t C)
{
    if (const int rc = nam_channels_check("v2v_nam_packed_elems", C)) return rc;
    return 2 * v2v::nam_mc_elems((int)C) + v2v::nam_h_elems((int)C);
}

int v2v_nam_pack_weights_hip(const float *conv_x, const float *conv_h, const float *conv_m, const float *conv_o, const float *conv_last, const float *lag_conv,
                             int64_t C, void *packed, void *stream)
{
    if (!conv_x || !conv_h || !conv_m || !conv_o || !conv_last || !lag_conv || !packed)
        return fail(V2V_ERR_NULL, "v2v_nam_pack_weights_hip: a weight or the packed pointer is NULL");
    if (const int rc = nam_channels_check("v2v_nam_pack_weights_hip", C)) return rc;
    if (!aligned(conv_x, 4) || !aligned(conv_h, 4) || !aligned(conv_m, 4) || !aligned(conv_o, 4) || !aligned(conv_last, 4) || !aligned(lag_conv, 4) || !aligned(packed, 16))
        return fail(V2V_ERR_ALIGN, "v2v_nam_pack_weights_hip: weights need 4-byte, the packed stream 16-byte alignment");
    const int64_t n = 2 * v2v::nam_mc_elems((int)C) + v2v::nam_h_elems((int)C);
    hipLaunchKernelGGL(v2v::nam_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), conv_x, conv_h, conv_m, conv_o,
                       conv_last, lag_conv, static_cast<uint16_t *>(packed), (int)C);
    return launched("nam_pack_kernel launch");
}

int v2v_nam_step_hip(const void *x, const void *m_t, const void *h_prev, const float *c_prev, const void *packed, int64_t B, int64_t H, int64_t W, int64_t C,
                     float *alpha_ws, float *o_pre_ws, void *m_state, float *m_state_f32, float *c_state, void *c_state_bf16, void *h_state,
                     float *h_state_f32, void *h_nchw, int h_nchw_dtype, int tile, int64_t Hv, int64_t Wv, void *stream)
{
    if (!x || !m_t || !packed) return fail(V2V_ERR_NULL, "v2v_nam_step_hip: x/m_t/packed is NULL");
    if (!alpha_ws || !o_pre_ws) return fail(V2V_ERR_NULL, "v2v_nam_step_hip: a workspace (alpha_ws/o_pre_ws) is NULL");
    if (!m_state || !c_state || !c_state_bf16 || !h_state || !h_state_f32)
        return fail(V2V_ERR_NULL, "v2v_nam_step_hip: m_state/c_state/c_state_bf16/h_state/h_state_f32 is NULL");
    if ((h_prev == nullptr) != (c_prev == nullptr)) return fail(V2V_ERR_NULL, "v2v_nam_step_hip: h_prev and c_prev come together (both NULL: the zero state)");
    if (h_nchw && h_nchw_dtype != V2V_F32 && h_nchw_dtype != V2V_BF16) return fail(V2V_ERR_DTYPE, "v2v_nam_step_hip: h_nchw_dtype must be V2V_F32 or V2V_BF16");
    if (const int rc = nam_channels_check("v2v_nam_step_hip", C)) return rc;
    if (B < 1 || H < 1 || W < 1 || (H * W) % 4 != 0 || H * W > kMaxElems / (B * C))
        return fail(V2V_ERR_SHAPE, "v2v_nam_step_hip: need B,H,W >= 1, (H*W) %% 4 == 0 and B*H*W*C < 2^31 (got %lldx%lldx%lldx%lld)", (long long)B, (long long)H,
                    (long long)W, (long long)C);
    if (const int rc = canvas_check("v2v_nam_step_hip", B, H, W, Hv, Wv)) return rc;
    if (tile < 0 || tile > 2) return fail(V2V_ERR_PARAM, "v2v_nam_step_hip: tile must be 0 (by shape), 1 or 2 (got %d)", tile);
    if (m_state == m_t || m_state == x || c_state_bf16 == x || c_state_bf16 == h_prev || c_state_bf16 == m_t || c_state_bf16 == m_state || h_state == c_state_bf16 ||
        h_state == m_state || h_state == x || h_state == m_t || alpha_ws == o_pre_ws || alpha_ws == c_state || alpha_ws == c_prev || o_pre_ws == c_state ||
        o_pre_ws == c_prev || h_state_f32 == o_pre_ws || h_state_f32 == c_state || h_state_f32 == alpha_ws ||
        (m_state_f32 && (m_state_f32 == alpha_ws || m_state_f32 == o_pre_ws || m_state_f32 == c_state || m_state_f32 == c_prev || m_state_f32 == h_state_f32)))
        return fail(V2V_ERR_PARAM, "v2v_nam_step_hip: m_state / c_state_bf16 / h_state must not alias an operand a later launch or a neighbouring tile reads, "
                                   "the workspaces not each other or a state");
    if (!aligned(x, 16) || !aligned(m_t, 16) || !aligned(h_prev, 16) || !aligned(packed, 16) || !aligned(m_state, 16) || !aligned(c_state_bf16, 16) ||
        !aligned(h_state, 16) || !aligned(h_nchw, 16) || !aligned(c_prev, 4) || !aligned(c_state, 4) || !aligned(alpha_ws, 4) || !aligned(o_pre_ws, 4) ||
        !aligned(m_state_f32, 4) || !aligned(h_state_f32, 4))
        return fail(V2V_ERR_ALIGN, "v2v_nam_step_hip: x/m_t/h_prev/packed/m_state/c_state_bf16/h_state/h_nchw need 16-byte, the float32 buffers 4-byte alignment");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (tile == 0) tile = (B * H * W / 128) * (C / 64) >= v2v::device_cus() ? 2 : 1;
    const uint16_t *wp = static_cast<const uint16_t *>(packed);
    const int64_t n_mc = v2v::nam_mc_elems((int)C);
    v2v::ConvLstmArgs m{};
    m.x = static_cast<const uint16_t *>(x); m.h_prev = static_cast<const uint16_t *>(m_t); m.wp = wp;
    m.h_state = static_cast<uint16_t *>(m_state); m.c_state = alpha_ws; m.dc_prev = m_state_f32;
    m.B = (int)B; m.H = (int)H; m.W = (int)W; m.C = (int)C;
    hipError_t e = launch_nam_4c<5>(m, tile, s);
    if (e != hipSuccess) return hip_fail(e, "NAM launch M");
    v2v::ConvLstmArgs c{};
    c.x = m.x; c.h_prev = static_cast<const uint16_t *>(h_prev); c.c_prev = c_prev; c.dh = alpha_ws; c.wp = wp + n_mc;
    c.h_state = static_cast<uint16_t *>(c_state_bf16); c.c_state = c_state; c.dc_prev = o_pre_ws;
    c.B = m.B; c.H = m.H; c.W = m.W; c.C = m.C;
    e = launch_nam_4c<6>(c, tile, s);
    if (e != hipSuccess) return hip_fail(e, "NAM launch C");
    // a canvas larger than its valid extent: launch H reads c' and m' through a 3x3 window and must find the reference's zero padding there
    const bool canvas = Hv < H || Wv < W;
    auto clear = [&](void *t) {
        hipLaunchKernelGGL(v2v::valid_extent_kernel, dim3((unsigned)((B * H * W * (C / 8) + 255) / 256)), dim3(256), 0, s, static_cast<uint4 *>(t), (int)B, (int)H,
                           (int)W, (int)(C / 8), (int)Hv, (int)Wv, 0);
        return launched("valid_extent_kernel launch");
    };
    if (canvas) {
        if (const int rc = clear(m_state)) return rc;
        if (const int rc = clear(c_state_bf16)) return rc;
    }
    v2v::ConvLstmArgs h{};
    h.x = static_cast<const uint16_t *>(c_state_bf16); h.h_prev = static_cast<const uint16_t *>(m_state); h.dh = o_pre_ws; h.wp = wp + 2 * n_mc;
    h.h_state = static_cast<uint16_t *>(h_state); h.c_state = h_state_f32; h.h_nchw = h_nchw; h.h_nchw_bf16 = h_nchw_dtype == V2V_BF16;
    h.B = m.B; h.H = m.H; h.W = m.W; h.C = m.C;
    e = launch_nam_h(h, tile, s);
    if (e != hipSuccess) return hip_fail(e, "NAM launch H");
    return canvas ? clear(h_state) : V2V_OK;
}

int64_t v2v_gcb_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t C)
{
    if (const int rc = gcb_channels_check("v2v_gcb_workspace_bytes", C)) return rc;
    if (const int rc = canvas_check("v2v_gcb_workspace_bytes", B, H, W, 1, 1)) return rc;
    if (H * W > kMaxElems / (B * C)) return fail(V2V_ERR_SHAPE, "v2v_gcb_workspace_bytes: the tensor must stay below 2^31 elements");
    return B * gcb_tiles(H, W) * (C + 2) * 4;
}

int v2v_gcb_nhwc_hip(const void *x, const float *w1t, const float *b1, const float *wmask, const float *bmask, const float *wa, const float *ba,
                     const float *ln_w, const float *ln_b, const float *prelu, const float *wb, const float *bb, float eps, int64_t B, int64_t H,
                     int64_t W, int64_t C, int64_t Hv, int64_t Wv, void *workspace, int64_t workspace_bytes, float *ctx_add, void *out, void *stream)
{
    if (!x || !out || !ctx_add) return fail(V2V_ERR_NULL, "v2v_gcb_nhwc_hip: x/out/ctx_add is NULL");
    if (!w1t || !b1 || !wmask || !bmask || !wa || !ba || !ln_w || !ln_b || !prelu || !wb || !bb) return fail(V2V_ERR_NULL, "v2v_gcb_nhwc_hip: a weight pointer is NULL");
    if (!workspace) return fail(V2V_ERR_NULL, "v2v_gcb_nhwc_hip: workspace is NULL (v2v_gcb_workspace_bytes gives its size)");
    if (const int rc = gcb_channels_check("v2v_gcb_nhwc_hip", C)) return rc;
    if (const int rc = canvas_check("v2v_gcb_nhwc_hip", B, H, W, Hv, Wv)) return rc;
    if (H * W > kMaxElems / (B * C)) return fail(V2V_ERR_SHAPE, "v2v_gcb_nhwc_hip: the tensor must stay below 2^31 elements");
    const int64_t need = B * gcb_tiles(H, W) * (C + 2) * 4;
    if (workspace_bytes < need)
        return fail(V2V_ERR_SHAPE, "v2v_gcb_nhwc_hip: the workspace holds %lld bytes, the call needs %lld", (long long)workspace_bytes, (long long)need);
    if (!(eps > 0.0f)) return fail(V2V_ERR_PARAM, "v2v_gcb_nhwc_hip: LayerNorm's eps must be positive");
    if (!aligned(x, 16) || !aligned(out, 16) || !aligned(workspace, 4) || !aligned(ctx_add, 4) || !aligned(w1t, 4) || !aligned(wa, 4) || !aligned(wb, 4))
        return fail(V2V_ERR_ALIGN, "v2v_gcb_nhwc_hip: x/out need 16-byte, the float32 buffers 4-byte alignment");
    if (out == x) return fail(V2V_ERR_PARAM, "v2v_gcb_nhwc_hip: out must not alias x (x is read again after the pooling)");
    v2v::GcbArgs a{};
    a.x = static_cast<const uint16_t *>(x);
    a.w1t = w1t; a.b1 = b1; a.wmask = wmask; a.bmask = bmask;
    a.wa = wa; a.ba = ba; a.ln_w = ln_w; a.ln_b = ln_b; a.prelu = prelu; a.wb = wb; a.bb = bb;
    a.ws = static_cast<float *>(workspace);
    a.ctx_add = ctx_add;
    a.out = static_cast<uint16_t *>(out);
    a.B = (int)B; a.H = (int)H; a.W = (int)W; a.Hv = (int)Hv; a.Wv = (int)Wv;
    a.tiles = (int)gcb_tiles(H, W);
    a.eps = eps;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return C == 32 ? launch_gcb<32>(a, s) : C == 64 ? launch_gcb<64>(a, s) : launch_gcb<128>(a, s);
}

int64_t v2v_conv_head16in_packed_elems(void) { return v2v::kHead16Packed; }

int v2v_conv_head16in_pack_weights_hip(const float *weight, int64_t Cin, void *packed, void *stream)
{
    if (!weight || !packed) return fail(V2V_ERR_NULL, "v2v_conv_head16in_pack_weights_hip: weight/packed is NULL");
    if (Cin < 9 || Cin > 16)
        return fail(V2V_ERR_SHAPE, "v2v_conv_head16in_pack_weights_hip: this head takes 9 to 16 input channels, v2v_conv_head_nhwc_hip takes up to 8 (got %lld)", (long long)Cin);
    if (!aligned(weight, 4) || !aligned(packed, 16)) return fail(V2V_ERR_ALIGN, "v2v_conv_head16in_pack_weights_hip: weight needs 4-byte, packed 16-byte alignment");
    hipLaunchKernelGGL(v2v::conv_head16in_pack_kernel, dim3((v2v::kHead16Packed + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), weight, (int)Cin,
                       static_cast<uint16_t *>(packed));
    return launched("conv_head16in_pack_kernel launch");
}

int v2v_to_nhwc16_bf16_hip(const float *src, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, int64_t B, int64_t C, int64_t H, int64_t W,
                           void *dst, void *stream)
{
    if (!src || !dst) return fail(V2V_ERR_NULL, "v2v_to_nhwc16_bf16_hip: src/dst is NULL");
    if (C < 9 || C > 16) return fail(V2V_ERR_SHAPE, "v2v_to_nhwc16_bf16_hip: this layout takes 9 to 16 channels, v2v_to_nhwc8_bf16_hip takes up to 8 (got %lld)", (long long)C);
    if (B < 1 || H < 1 || W < 1 || H > kMaxElems || W > kMaxElems || H * W > kMaxElems / (B * 32) || stride_b < 0 || stride_c < 0 || stride_h < 0 || stride_w < 0)
        return fail(V2V_ERR_SHAPE, "v2v_to_nhwc16_bf16_hip: need B,H,W >= 1, strides >= 0 and B*H*W*32 < 2^31 (got %lld x %lld x %lld)", (long long)B, (long long)H,
                    (long long)W);
    if (!aligned(src, 4) || !aligned(dst, 16)) return fail(V2V_ERR_ALIGN, "v2v_to_nhwc16_bf16_hip: src needs 4-byte, dst 16-byte alignment");
    const int64_t n = B * H * W;
    hipLaunchKernelGGL(v2v::to_nhwc16_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), src, stride_b, stride_c, stride_h,
                       stride_w, (int)B, (int)C, (int)H, (int)W, static_cast<uint16_t *>(dst));
    return launched("to_nhwc16_bf16_kernel launch");
}

int v2v_conv_head16in_nhwc_hip(const void *x16, const void *packed, const float *bias, int relu, int64_t B, int64_t H, int64_t W, void *out, void *stream)
{
    if (!x16 || !packed || !bias || !out) return fail(V2V_ERR_NULL, "v2v_conv_head16in_nhwc_hip: x16/packed/bias/out is NULL");
    if (B < 1 || H < 1 || W < 1 || H > kMaxElems || W > kMaxElems || H * W > kMaxElems / (B * 32))
        return fail(V2V_ERR_SHAPE, "v2v_conv_head16in_nhwc_hip: need B,H,W >= 1 and B*H*W*32 < 2^31 (got %lld x %lld x %lld)", (long long)B, (long long)H, (long long)W);
    if (!aligned(x16, 16) || !aligned(packed, 16) || !aligned(bias, 4) || !aligned(out, 2))
        return fail(V2V_ERR_ALIGN, "v2v_conv_head16in_nhwc_hip: x16/packed need 16-byte alignment");
    if (out == x16) return fail(V2V_ERR_PARAM, "v2v_conv_head16in_nhwc_hip: out must not alias x16");
    const int64_t n = B * H * W;
    hipLaunchKernelGGL(v2v::conv_head16in_kernel, dim3((unsigned)((n + 127) / 128)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint16_t *>(x16),
                       static_cast<const uint16_t *>(packed), bias, static_cast<uint16_t *>(out), (int)B, (int)H, (int)W, relu ? 1 : 0);
    return launched("conv_head16in_kernel launch");
}

int v2v_valid_extent_nhwc_hip(void *x, int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int64_t Hv, int64_t Wv, int replicate, void *stream)
{
    if (!x) return fail(V2V_ERR_NULL, "v2v_valid_extent_nhwc_hip: x is NULL");
    if (dtype != V2V_F32 && dtype != V2V_BF16) return fail(V2V_ERR_DTYPE, "v2v_valid_extent_nhwc_hip: dtype must be V2V_F32 or V2V_BF16");
    if (const int rc = canvas_check("v2v_valid_extent_nhwc_hip", B, H, W, Hv, Wv)) return rc;
    const int64_t per16 = dtype == V2V_F32 ? 4 : 8;
    if (C < per16 || C % per16 != 0 || H * W > kMaxElems / (B * C))
        return fail(V2V_ERR_SHAPE, "v2v_valid_extent_nhwc_hip: a pixel must be whole 16-byte pieces (C %% %lld == 0) and the tensor below 2^31 elements (got C %lld)",
                    (long long)per16, (long long)C);
    if (!aligned(x, 16)) return fail(V2V_ERR_ALIGN, "v2v_valid_extent_nhwc_hip: x needs 16-byte alignment");
    if (Hv == H && Wv == W) return V2V_OK;           // nothing lies outside
    const int64_t n = B * H * W * (C / per16);
    hipLaunchKernelGGL(v2v::valid_extent_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<uint4 *>(x), (int)B,
                       (int)H, (int)W, (int)(C / per16), (int)Hv, (int)Wv, replicate ? 1 : 0);
    return launched("valid_extent_kernel launch");
}

}  // extern "C"
