// v2v_loss_tu.hip -- translation unit of the training losses (v2v_loss.hpp): their kernels and their C entry points (include/v2v_hip.h).
#define V2V_LOSS_KERNELS
#include "../../include/v2v_hip.h"
#include "v2v_loss.hpp"
#include "v2v_status.hpp"

using v2v::aligned;
using v2v::fail;
using v2v::hip_fail;
using v2v::kLossTile;
using v2v::launched;

namespace {

dim3 loss_grid(const v2v::LossArgs &a) { return dim3((unsigned)(a.n_img * a.tiles)); }

// n contiguous [c,h,w] images with a [n,2,h,w] flow, every one of them warped
v2v::LossArgs plain_args(const float *flow, int64_t n, int c, int h, int w)
{
    v2v::LossArgs a{};
    a.flow = flow;
    a.inner = 1;
    a.so = (int64_t)c * h * w;
    a.fso = (int64_t)2 * h * w;
    a.n_img = n;
    a.c = c;
    a.h = h;
    a.w = w;
    a.tiles = (h * w + kLossTile - 1) / kLossTile;
    a.flow_sign = 1.0f;
    a.w_tc = 1.0f;
    return a;
}

constexpr int64_t kLossMaxPixels = (int64_t)1 << 22;       // the fixed-point accumulator of the warp adjoint holds h*w contributions of < 2^38

int loss_shape_check(const char *who, int64_t n_img, int64_t c, int64_t h, int64_t w)
{
    if (n_img < 0 || c < 1) return fail(V2V_ERR_SHAPE, "%s: need a non-negative image count and c >= 1 (got %lld, %lld)", who, (long long)n_img, (long long)c);
    if (h < 2 || w < 2) return fail(V2V_ERR_SHAPE, "%s: h and w must be at least 2, the sampling grid divides by h - 1 and w - 1 (got %lld x %lld)", who, (long long)h, (long long)w);
    if (h * w > kLossMaxPixels) return fail(V2V_ERR_SHAPE, "%s: h*w = %lld is above 2^22, the bound of the adjoint's fixed-point accumulator", who, (long long)(h * w));
    const int64_t tiles = (h * w + v2v::kLossTile - 1) / v2v::kLossTile;
    if (c > 65536 || n_img * tiles > 0x7FFFFFFFLL || n_img * c > ((int64_t)1 << 40) / (h * w))
        return fail(V2V_ERR_SHAPE, "%s: %lld images of %lld x %lld x %lld are more than one launch takes", who, (long long)n_img, (long long)c, (long long)h, (long long)w);
    return V2V_OK;
}

int64_t loss_round16(int64_t b) { return (b + 15) / 16 * 16; }

// backward workspace: acc int64 [E] | maxbits u32 [n_img] (these two are zeroed by every call) | dwarp f32 [E] | dp1 f32 [E]
struct LossWorkspace {
    unsigned long long *acc;
    unsigned *maxbits;
    float *dwarp, *dp1;
    int64_t zero_bytes, bytes;
};

LossWorkspace loss_workspace(void *base, int64_t n_img, int64_t c, int64_t h, int64_t w)
{
    const int64_t e = n_img * c * h * w;
    char *p = static_cast<char *>(base);
    LossWorkspace ws;
    ws.acc = reinterpret_cast<unsigned long long *>(p);
    ws.maxbits = reinterpret_cast<unsigned *>(p + loss_round16(8 * e));
    ws.zero_bytes = loss_round16(8 * e) + loss_round16(4 * n_img);
    ws.dwarp = reinterpret_cast<float *>(p + ws.zero_bytes);
    ws.dp1 = reinterpret_cast<float *>(p + ws.zero_bytes + loss_round16(4 * e));
    ws.bytes = ws.zero_bytes + 2 * loss_round16(4 * e);
    return ws;
}

int loss_args(const char *who, v2v::LossArgs &a, const float *image0, const float *image1, const float *processed0, const float *processed1, const float *flow,
              int64_t outer, int64_t inner, int64_t so, int64_t si, int64_t fso, int64_t fsi, int64_t tc_first, int64_t c, int64_t h, int64_t w, float alpha,
              float flow_sign, float w_tc, float w_l1, float w_l2)
{
    if (!image1 || !processed1) return fail(V2V_ERR_NULL, "%s: image1/processed1 is NULL", who);
    if (outer < 0 || inner < 0) return fail(V2V_ERR_SHAPE, "%s: outer and inner must not be negative", who);
    if (const int rc = loss_shape_check(who, outer * inner, c, h, w)) return rc;
    if (tc_first < 0) return fail(V2V_ERR_PARAM, "%s: tc_first must not be negative", who);
    if (w_tc != 0.0f && tc_first < inner && (!image0 || !processed0 || !flow)) return fail(V2V_ERR_NULL, "%s: image0/processed0/flow is NULL with a temporal term", who);
    if (!aligned(image1, 4) || !aligned(processed1, 4) || !aligned(image0, 4) || !aligned(processed0, 4) || !aligned(flow, 4))
        return fail(V2V_ERR_ALIGN, "%s: float32 pointers need 4-byte alignment", who);
    a = v2v::LossArgs{image0, image1, processed0, processed1, flow, inner, so, si, fso, fsi, tc_first, outer * inner,
                      (int)c, (int)h, (int)w, (int)((h * w + v2v::kLossTile - 1) / v2v::kLossTile), alpha, flow_sign, w_tc, w_l1, w_l2};
    return V2V_OK;
}

}  // namespace

extern "C" {

int64_t v2v_tc_loss_workspace_bytes(int64_t n_img, int64_t c, int64_t h, int64_t w, int backward)
{
    if (const int rc = loss_shape_check("v2v_tc_loss_workspace_bytes", n_img, c, h, w)) return rc;
    if (backward) return loss_workspace(nullptr, n_img, c, h, w).bytes;
    return loss_round16(n_img * ((h * w + v2v::kLossTile - 1) / v2v::kLossTile) * 3 * 4);
}

int v2v_tc_loss_fwd_hip(const float *image0, const float *image1, const float *processed0, const float *processed1, const float *flow, int64_t outer,
                        int64_t inner, int64_t img_stride_outer, int64_t img_stride_inner, int64_t flow_stride_outer, int64_t flow_stride_inner,
                        int64_t tc_first, int64_t c, int64_t h, int64_t w, float alpha, float flow_sign, float w_tc, float w_l1, float w_l2, float *losses,
                        float *image0_warped, float *processed0_warped, float *visibility_mask, float *error_map, void *workspace, void *stream)
{
    v2v::LossArgs a;
    if (const int rc = loss_args("v2v_tc_loss_fwd_hip", a, image0, image1, processed0, processed1, flow, outer, inner, img_stride_outer, img_stride_inner,
                                 flow_stride_outer, flow_stride_inner, tc_first, c, h, w, alpha, flow_sign, w_tc, w_l1, w_l2))
        return rc;
    if (!losses || !workspace) return fail(V2V_ERR_NULL, "v2v_tc_loss_fwd_hip: losses/workspace is NULL");
    if (!aligned(losses, 4) || !aligned(workspace, 16)) return fail(V2V_ERR_ALIGN, "v2v_tc_loss_fwd_hip: losses needs 4-byte, workspace 16-byte alignment");
    if (a.n_img == 0) return V2V_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *partials = static_cast<float *>(workspace);
    hipLaunchKernelGGL(v2v::tc_loss_fwd_kernel, loss_grid(a), dim3(kLossTile), 0, s, a, partials, image0_warped, processed0_warped, visibility_mask, error_map);
    hipLaunchKernelGGL(v2v::loss_reduce_kernel, dim3((unsigned)a.n_img), dim3(64), 0, s, partials, losses, a.n_img, a.tiles, (float)((int64_t)a.c * a.h * a.w), a.w_tc,
                       a.w_l1, a.w_l2);
    return launched("tc_loss_fwd_kernel launch");
}

// chain != 0: processed0 of image (a, b) IS processed1 of image (a, b - 1); dprocessed1 then also receives what the next step scatters
// (dprocessed0 unused)
int v2v_tc_loss_bwd_hip(const float *image0, const float *image1, const float *processed0, const float *processed1, const float *flow, int64_t outer,
                        int64_t inner, int64_t img_stride_outer, int64_t img_stride_inner, int64_t flow_stride_outer, int64_t flow_stride_inner,
                        int64_t tc_first, int64_t c, int64_t h, int64_t w, float alpha, float flow_sign, float w_tc, float w_l1, float w_l2, const float *gout,
                        int chain, float *dprocessed1, float *dprocessed0, void *workspace, void *stream)
{
    v2v::LossArgs a;
    if (const int rc = loss_args("v2v_tc_loss_bwd_hip", a, image0, image1, processed0, processed1, flow, outer, inner, img_stride_outer, img_stride_inner,
                                 flow_stride_outer, flow_stride_inner, tc_first, c, h, w, alpha, flow_sign, w_tc, w_l1, w_l2))
        return rc;
    const bool tc = w_tc != 0.0f && tc_first < inner;
    if (!gout || !dprocessed1 || !workspace || (tc && !chain && !dprocessed0)) return fail(V2V_ERR_NULL, "v2v_tc_loss_bwd_hip: gout/dprocessed1/dprocessed0/workspace is NULL");
    if (chain && tc && (tc_first < 1 || processed0 != processed1 + (tc_first - 1) * img_stride_inner))
        return fail(V2V_ERR_PARAM, "v2v_tc_loss_bwd_hip: chain needs tc_first >= 1 and processed0 = processed1 + (tc_first - 1) * img_stride_inner");
    if (!aligned(gout, 4) || !aligned(dprocessed1, 4) || !aligned(dprocessed0, 4) || !aligned(workspace, 16))
        return fail(V2V_ERR_ALIGN, "v2v_tc_loss_bwd_hip: float32 pointers need 4-byte, workspace 16-byte alignment");
    if (a.n_img == 0) return V2V_OK;
    const LossWorkspace ws = loss_workspace(workspace, a.n_img, c, h, w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (tc) {
        const hipError_t e = hipMemsetAsync(workspace, 0, (size_t)ws.zero_bytes, s);
        if (e != hipSuccess) return hip_fail(e, "v2v_tc_loss_bwd_hip: clearing the accumulator");
        hipLaunchKernelGGL(v2v::tc_loss_bwd_kernel, loss_grid(a), dim3(kLossTile), 0, s, a, gout, ws.dp1, ws.dwarp, ws.maxbits);
        hipLaunchKernelGGL(v2v::warp_adjoint_kernel, loss_grid(a), dim3(kLossTile), 0, s, a, ws.dwarp, ws.maxbits, ws.acc);
    }
    hipLaunchKernelGGL(v2v::warp_adjoint_finish_kernel, loss_grid(a), dim3(kLossTile), 0, s, a, gout, chain ? 1 : 0, ws.acc, ws.dp1, ws.maxbits, dprocessed1, dprocessed0);
    return launched("tc_loss_bwd_kernel launch");
}

int v2v_warp_bilinear_hip(const float *img, const float *flow, int64_t n, int64_t c, int64_t h, int64_t w, float *out, void *stream)
{
    if (!img || !flow || !out) return fail(V2V_ERR_NULL, "v2v_warp_bilinear_hip: img/flow/out is NULL");
    if (const int rc = loss_shape_check("v2v_warp_bilinear_hip", n, c, h, w)) return rc;
    if (!aligned(img, 4) || !aligned(flow, 4) || !aligned(out, 4)) return fail(V2V_ERR_ALIGN, "v2v_warp_bilinear_hip: float32 pointers need 4-byte alignment");
    if (out == img) return fail(V2V_ERR_PARAM, "v2v_warp_bilinear_hip: out must not alias img");
    if (n == 0) return V2V_OK;
    const v2v::LossArgs a = plain_args(flow, n, (int)c, (int)h, (int)w);
    hipLaunchKernelGGL(v2v::warp_bilinear_kernel, loss_grid(a), dim3(kLossTile), 0, static_cast<hipStream_t>(stream), a, img, out);
    return launched("warp_bilinear_kernel launch");
}

int v2v_warp_bilinear_adjoint_hip(const float *dout, const float *flow, int64_t n, int64_t c, int64_t h, int64_t w, float *din, void *workspace, void *stream)
{
    if (!dout || !flow || !din || !workspace) return fail(V2V_ERR_NULL, "v2v_warp_bilinear_adjoint_hip: dout/flow/din/workspace is NULL");
    if (const int rc = loss_shape_check("v2v_warp_bilinear_adjoint_hip", n, c, h, w)) return rc;
    if (!aligned(dout, 4) || !aligned(flow, 4) || !aligned(din, 4) || !aligned(workspace, 16))
        return fail(V2V_ERR_ALIGN, "v2v_warp_bilinear_adjoint_hip: float32 pointers need 4-byte, workspace 16-byte alignment");
    if (n == 0) return V2V_OK;
    const LossWorkspace ws = loss_workspace(workspace, n, c, h, w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)ws.zero_bytes, s);
    if (e != hipSuccess) return hip_fail(e, "v2v_warp_bilinear_adjoint_hip: clearing the accumulator");
    const v2v::LossArgs a = plain_args(flow, n, (int)c, (int)h, (int)w);
    const int64_t per_img = a.so, total = n * per_img;
    const unsigned bx = (unsigned)((per_img + kLossTile - 1) / kLossTile < 64 ? (per_img + kLossTile - 1) / kLossTile : 64);
    hipLaunchKernelGGL(v2v::warp_absmax_kernel, dim3(bx, (unsigned)n), dim3(kLossTile), 0, s, dout, per_img, ws.maxbits);
    hipLaunchKernelGGL(v2v::warp_adjoint_kernel, loss_grid(a), dim3(kLossTile), 0, s, a, dout, ws.maxbits, ws.acc);
    hipLaunchKernelGGL(v2v::warp_adjoint_plain_finish_kernel, dim3((unsigned)((total + kLossTile - 1) / kLossTile)), dim3(kLossTile), 0, s, ws.acc, ws.maxbits, per_img, total, din);
    return launched("warp_adjoint_kernel launch");
}

}  // extern "C"
