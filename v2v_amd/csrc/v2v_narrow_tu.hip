// v2v_narrow_tu.hip -- translation unit of the 16-channel layer family (FireNet): the fused ConvGRU step, the fused residual block, the
// 16-output head and their weight packing, with their C entry points (include/v2v_hip.h).  Kernels and layouts in v2v_narrow.hpp.
#define V2V_NARROW_KERNELS
#include "../../include/v2v_hip.h"
#include "v2v_narrow.hpp"
#include "v2v_status.hpp"

using v2v::aligned;
using v2v::fail;
using v2v::launched;

namespace {

unsigned narrow_grid(const v2v::NarrowArgs &a) { return (unsigned)((int64_t)a.B * a.tiles_x * a.tiles_y); }

int narrow_shape(const char *who, int64_t B, int64_t H, int64_t W, v2v::NarrowArgs &a)
{
    if (B < 1 || H < 1 || W < 1 || B * H * W * 16 > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "%s: need B,H,W >= 1 and B*H*W*16 < 2^31 (got %lldx%lldx%lld)", who, (long long)B, (long long)H, (long long)W);
    a.B = (int)B; a.H = (int)H; a.W = (int)W; a.tiles_x = (int)((W + 15) / 16); a.tiles_y = (int)((H + 15) / 16);
    if (B * a.tiles_x * a.tiles_y > 0x7FFFFFFFLL) return fail(V2V_ERR_SHAPE, "%s: too many tiles", who);
    return V2V_OK;
}

}  // namespace

extern "C" {

int64_t v2v_convgru16_packed_elems(void) { return (int64_t)v2v::kGru16Frags * v2v::kNarrowFragElems; }
int64_t v2v_resblock16_packed_elems(void) { return (int64_t)v2v::kRes16Frags * v2v::kNarrowFragElems; }
int64_t v2v_conv_head16_packed_elems(void) { return (int64_t)v2v::kHead16Frags * v2v::kNarrowFragElems; }

int v2v_convgru16_pack_weights_hip(const float *update_weight, const float *reset_weight, const float *out_weight, void *packed, void *stream)
{
    if (!update_weight || !reset_weight || !out_weight || !packed) return fail(V2V_ERR_NULL, "v2v_convgru16_pack_weights_hip: a weight or packed pointer is NULL");
    if (!aligned(update_weight, 4) || !aligned(reset_weight, 4) || !aligned(out_weight, 4) || !aligned(packed, 16))
        return fail(V2V_ERR_ALIGN, "weights need 4-byte, packed 16-byte alignment");
    hipLaunchKernelGGL(v2v::narrow_pack_kernel, dim3(v2v::kGru16Frags * v2v::kNarrowFragElems / 256), dim3(256), 0, static_cast<hipStream_t>(stream), 0,
                       update_weight, reset_weight, out_weight, 0, static_cast<uint16_t *>(packed));
    return launched("narrow_pack_kernel launch");
}

int v2v_convgru16_step_hip(const void *x, const void *h_prev, const float *h_prev_f32, const void *packed, const float *gates_bias,
                           const float *out_bias, int64_t B, int64_t H, int64_t W, void *h_state, float *h_state_f32, void *h_nchw,
                           int h_nchw_dtype, void *stream)
{
    if (h_nchw && h_nchw_dtype != V2V_F32 && h_nchw_dtype != V2V_BF16) return fail(V2V_ERR_DTYPE, "h_nchw_dtype must be V2V_F32 or V2V_BF16");
    if (!x || !packed || !gates_bias || !out_bias || !h_state || !h_state_f32)
        return fail(V2V_ERR_NULL, "v2v_convgru16_step_hip: x/packed/gates_bias/out_bias/h_state/h_state_f32 is NULL");
    if ((h_prev == nullptr) != (h_prev_f32 == nullptr)) return fail(V2V_ERR_NULL, "h_prev and h_prev_f32 come together (both NULL: the zero state)");
    v2v::NarrowArgs a{};
    if (const int rc = narrow_shape("v2v_convgru16_step_hip", B, H, W, a)) return rc;
    if (h_state == h_prev || h_state == x || (h_prev_f32 && h_state_f32 == h_prev_f32) ||
        (h_nchw && (h_nchw == x || h_nchw == h_prev || h_nchw == h_prev_f32)))
        return fail(V2V_ERR_PARAM, "h_state must not alias h_prev or x, h_state_f32 not h_prev_f32 (neighbouring tiles read them)");
    if (!aligned(x, 16) || !aligned(h_prev, 16) || !aligned(packed, 16) || !aligned(h_state, 16) || !aligned(h_prev_f32, 4) || !aligned(h_state_f32, 4) ||
        !aligned(gates_bias, 4) || !aligned(out_bias, 4) || !aligned(h_nchw, 4))
        return fail(V2V_ERR_ALIGN, "x/h_prev/packed/h_state need 16-byte alignment");
    a.x = static_cast<const uint16_t *>(x); a.h_prev = static_cast<const uint16_t *>(h_prev); a.h_prev_f32 = h_prev_f32;
    a.wp = static_cast<const uint16_t *>(packed); a.bias1 = gates_bias; a.bias2 = out_bias;
    a.out = static_cast<uint16_t *>(h_state); a.out_f32 = h_state_f32; a.h_nchw = h_nchw; a.h_nchw_bf16 = h_nchw_dtype == V2V_BF16;
    hipLaunchKernelGGL(v2v::narrow_two_conv_kernel<0>, dim3(narrow_grid(a)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return launched("narrow_two_conv_kernel<0> (ConvGRU) launch");
}

int v2v_resblock16_pack_weights_hip(const float *w1, const float *w2, void *packed, void *stream)
{
    if (!w1 || !w2 || !packed) return fail(V2V_ERR_NULL, "v2v_resblock16_pack_weights_hip: w1/w2/packed is NULL");
    if (!aligned(w1, 4) || !aligned(w2, 4) || !aligned(packed, 16)) return fail(V2V_ERR_ALIGN, "weights need 4-byte, packed 16-byte alignment");
    hipLaunchKernelGGL(v2v::narrow_pack_kernel, dim3(v2v::kRes16Frags * v2v::kNarrowFragElems / 256), dim3(256), 0, static_cast<hipStream_t>(stream), 1, w1, w2,
                       static_cast<const float *>(nullptr), 0, static_cast<uint16_t *>(packed));
    return launched("narrow_pack_kernel launch");
}

int v2v_resblock16_nhwc_hip(const void *x, const void *packed, const float *b1, const float *b2, int64_t B, int64_t H, int64_t W, void *out, void *stream)
{
    if (!x || !packed || !b1 || !b2 || !out) return fail(V2V_ERR_NULL, "v2v_resblock16_nhwc_hip: x/packed/b1/b2/out is NULL");
    v2v::NarrowArgs a{};
    if (const int rc = narrow_shape("v2v_resblock16_nhwc_hip", B, H, W, a)) return rc;
    if (out == x) return fail(V2V_ERR_PARAM, "out must not alias x (neighbouring tiles read it)");
    if (!aligned(x, 16) || !aligned(packed, 16) || !aligned(out, 16) || !aligned(b1, 4) || !aligned(b2, 4)) return fail(V2V_ERR_ALIGN, "x/packed/out need 16-byte alignment");
    a.x = static_cast<const uint16_t *>(x); a.wp = static_cast<const uint16_t *>(packed); a.bias1 = b1; a.bias2 = b2; a.out = static_cast<uint16_t *>(out);
    hipLaunchKernelGGL(v2v::narrow_two_conv_kernel<1>, dim3(narrow_grid(a)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return launched("narrow_two_conv_kernel<1> (residual block) launch");
}

int v2v_conv_head16_pack_weights_hip(const float *weight, int64_t Cin, void *packed, void *stream)
{
    if (!weight || !packed) return fail(V2V_ERR_NULL, "v2v_conv_head16_pack_weights_hip: weight/packed is NULL");
    if (Cin < 1 || Cin > 8) return fail(V2V_ERR_SHAPE, "need 1 <= Cin <= 8 (16 output channels, 3x3)");
    if (!aligned(weight, 4) || !aligned(packed, 16)) return fail(V2V_ERR_ALIGN, "weight needs 4-byte, packed 16-byte alignment");
    hipLaunchKernelGGL(v2v::narrow_pack_kernel, dim3(v2v::kHead16Frags * v2v::kNarrowFragElems / 256), dim3(256), 0, static_cast<hipStream_t>(stream), 2, weight,
                       static_cast<const float *>(nullptr), static_cast<const float *>(nullptr), (int)Cin, static_cast<uint16_t *>(packed));
    return launched("narrow_pack_kernel launch");
}

int v2v_conv_head16_nhwc_hip(const void *x8, const void *packed, const float *bias, int relu, int64_t B, int64_t H, int64_t W, void *out, void *stream)
{
    if (!x8 || !packed || !bias || !out) return fail(V2V_ERR_NULL, "v2v_conv_head16_nhwc_hip: x8/packed/bias/out is NULL");
    v2v::NarrowArgs a{};
    if (const int rc = narrow_shape("v2v_conv_head16_nhwc_hip", B, H, W, a)) return rc;
    if (out == x8) return fail(V2V_ERR_PARAM, "out must not alias x8");
    if (!aligned(x8, 16) || !aligned(packed, 16) || !aligned(out, 16) || !aligned(bias, 4)) return fail(V2V_ERR_ALIGN, "x8/packed/out need 16-byte alignment");
    a.x = static_cast<const uint16_t *>(x8); a.wp = static_cast<const uint16_t *>(packed); a.bias1 = bias; a.relu = relu ? 1 : 0; a.out = static_cast<uint16_t *>(out);
    hipLaunchKernelGGL(v2v::narrow_head_kernel, dim3(narrow_grid(a)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return launched("narrow_head_kernel launch");
}

}  // extern "C"
