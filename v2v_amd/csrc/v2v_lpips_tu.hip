// v2v_lpips_tu.hip -- translation unit of the LPIPS-VGG loss (v2v_lpips.hpp): its kernels and their C entry points (include/v2v_hip.h).
#define V2V_LPIPS_KERNELS
#include "../../include/v2v_hip.h"
#include "v2v_lpips.hpp"
#include "v2v_status.hpp"

using v2v::aligned;
using v2v::fail;
using v2v::launched;

namespace {

unsigned blocks256(int64_t threads) { return (unsigned)((threads + 255) / 256); }

int lpips_image_check(const char *who, int64_t B, int64_t Cin, int64_t H, int64_t W)
{
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 32768 || W > 32768) return fail(V2V_ERR_SHAPE, "%s: need 1 <= B <= 65535 and 1 <= H, W <= 32768 (got %lld, %lld x %lld)", who, (long long)B, (long long)H, (long long)W);
    if (Cin != 1 && Cin != 3) return fail(V2V_ERR_SHAPE, "%s: the image has 1 or 3 channels (got %lld)", who, (long long)Cin);
    if (B * H * W * 64 > 0x7FFFFFFFLL) return fail(V2V_ERR_SHAPE, "%s: [B,H,W,64] must stay below 2^31 elements", who);
    return V2V_OK;
}

int lpips_pool_check(const char *who, int64_t B, int64_t H, int64_t W, int64_t C)
{
    if (B < 1 || H < 2 || W < 2 || H % 2 != 0 || W % 2 != 0 || C < 8 || C % 8 != 0 || H > 32768 || W > 32768 || C > 4096 || B * H * W * C > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "%s: need B >= 1, H and W even, C a multiple of 8, the tensor below 2^31 elements (got %lld x %lld x %lld x %lld)", who,
                    (long long)B, (long long)H, (long long)W, (long long)C);
    return V2V_OK;
}

int lpips_compare_check(const char *who, int64_t n_img, int64_t HW, int64_t Cc)
{
    if (Cc != 64 && Cc != 128 && Cc != 256 && Cc != 512) return fail(V2V_ERR_SHAPE, "%s: Cc must be 64, 128, 256 or 512 (got %lld)", who, (long long)Cc);
    if (n_img < 1 || n_img > 65535 || HW < 1 || HW > 0x7FFFFFFFLL / 512 || n_img * HW * Cc > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "%s: need 1 <= n_img <= 65535, HW >= 1 and [n_img,HW,Cc] below 2^31 elements (got %lld, %lld)", who, (long long)n_img, (long long)HW);
    return V2V_OK;
}

}  // namespace

extern "C" {

int v2v_lpips_stem_hip(const void *x, int x_dtype, int64_t B, int64_t Cin, int64_t H, int64_t W, const float *weight, const float *bias, const float *shift,
                       const float *scale, int normalize, void *out, void *stream)
{
    if (!x || !weight || !bias || !shift || !scale || !out) return fail(V2V_ERR_NULL, "v2v_lpips_stem_hip: x/weight/bias/shift/scale/out is NULL");
    if (x_dtype != V2V_F32 && x_dtype != V2V_BF16) return fail(V2V_ERR_DTYPE, "v2v_lpips_stem_hip: x_dtype must be V2V_F32 or V2V_BF16");
    if (const int rc = lpips_image_check("v2v_lpips_stem_hip", B, Cin, H, W)) return rc;
    if (!aligned(x, x_dtype == V2V_F32 ? 4 : 2) || !aligned(weight, 4) || !aligned(bias, 4) || !aligned(shift, 4) || !aligned(scale, 4) || !aligned(out, 16))
        return fail(V2V_ERR_ALIGN, "v2v_lpips_stem_hip: out needs 16-byte alignment, float32 pointers 4-byte");
    const unsigned tiles = (unsigned)(((H + v2v::kLpStemTile - 1) / v2v::kLpStemTile) * ((W + v2v::kLpStemTile - 1) / v2v::kLpStemTile));
    hipLaunchKernelGGL(v2v::lpips_stem_kernel, dim3(tiles, (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), x, (int)(x_dtype == V2V_BF16), (int)Cin,
                       (int)H, (int)W, weight, bias, shift, scale, normalize ? 1 : 0, static_cast<uint16_t *>(out));
    return launched("lpips_stem_kernel launch");
}

int v2v_lpips_stem_bwd_hip(const void *dz, int64_t B, int64_t Cin, int64_t H, int64_t W, const float *weight, const float *scale, int normalize,
                           float *dpred, void *stream)
{
    if (!dz || !weight || !scale || !dpred) return fail(V2V_ERR_NULL, "v2v_lpips_stem_bwd_hip: dz/weight/scale/dpred is NULL");
    if (const int rc = lpips_image_check("v2v_lpips_stem_bwd_hip", B, Cin, H, W)) return rc;
    if (!aligned(dz, 16) || !aligned(weight, 4) || !aligned(scale, 4) || !aligned(dpred, 4))
        return fail(V2V_ERR_ALIGN, "v2v_lpips_stem_bwd_hip: dz needs 16-byte alignment, float32 pointers 4-byte");
    hipLaunchKernelGGL(v2v::lpips_stem_bwd_kernel, dim3(blocks256(H * W), (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(dz), (int)Cin, (int)H, (int)W, weight, scale, normalize ? 1 : 0, dpred);
    return launched("lpips_stem_bwd_kernel launch");
}

int v2v_lpips_pool_hip(const void *x, int64_t B, int64_t H, int64_t W, int64_t C, void *out, void *stream)
{
    if (!x || !out) return fail(V2V_ERR_NULL, "v2v_lpips_pool_hip: x/out is NULL");
    if (const int rc = lpips_pool_check("v2v_lpips_pool_hip", B, H, W, C)) return rc;
    if (!aligned(x, 16) || !aligned(out, 16)) return fail(V2V_ERR_ALIGN, "v2v_lpips_pool_hip: x/out need 16-byte alignment");
    const int64_t total = B * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(v2v::lpips_pool_kernel, dim3(blocks256(total)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint16_t *>(x), (int)H,
                       (int)W, (int)C, total, static_cast<uint16_t *>(out));
    return launched("lpips_pool_kernel launch");
}

int v2v_lpips_pool_bwd_hip(const void *dy, const void *x, const void *dtap, int relu_mask, int64_t B, int64_t H, int64_t W, int64_t C, void *dx, void *stream)
{
    if (!dy || !x || !dx) return fail(V2V_ERR_NULL, "v2v_lpips_pool_bwd_hip: dy/x/dx is NULL");
    if (const int rc = lpips_pool_check("v2v_lpips_pool_bwd_hip", B, H, W, C)) return rc;
    if (!aligned(dy, 16) || !aligned(x, 16) || !aligned(dtap, 16) || !aligned(dx, 16)) return fail(V2V_ERR_ALIGN, "v2v_lpips_pool_bwd_hip: dy/x/dtap/dx need 16-byte alignment");
    if (dx == dy) return fail(V2V_ERR_PARAM, "v2v_lpips_pool_bwd_hip: dx must not alias dy");
    const int64_t total = B * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(v2v::lpips_pool_bwd_kernel, dim3(blocks256(total)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint16_t *>(dy),
                       static_cast<const uint16_t *>(x), static_cast<const uint16_t *>(dtap), relu_mask ? 1 : 0, (int)H, (int)W, (int)C, total,
                       static_cast<uint16_t *>(dx));
    return launched("lpips_pool_bwd_kernel launch");
}

int64_t v2v_lpips_compare_workspace_bytes(int64_t n_img, int64_t HW)
{
    if (n_img < 1 || HW < 1) return V2V_ERR_SHAPE;
    return (n_img * ((HW + v2v::kLpCmpTile - 1) / v2v::kLpCmpTile) * 4 + 15) / 16 * 16;
}

int v2v_lpips_compare_fwd_hip(const void *f0, const void *f1, const float *w, int64_t n_img, int64_t HW, int64_t Cc, float *dist, void *workspace, void *stream)
{
    if (!f0 || !f1 || !w || !dist || !workspace) return fail(V2V_ERR_NULL, "v2v_lpips_compare_fwd_hip: f0/f1/w/dist/workspace is NULL");
    if (const int rc = lpips_compare_check("v2v_lpips_compare_fwd_hip", n_img, HW, Cc)) return rc;
    if (!aligned(f0, 16) || !aligned(f1, 16) || !aligned(w, 4) || !aligned(dist, 4) || !aligned(workspace, 16))
        return fail(V2V_ERR_ALIGN, "v2v_lpips_compare_fwd_hip: f0/f1/workspace need 16-byte alignment, w/dist 4-byte");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *partials = static_cast<float *>(workspace);
    const int tiles = ((int)HW + v2v::kLpCmpTile - 1) / v2v::kLpCmpTile;
    hipLaunchKernelGGL(v2v::lpips_compare_fwd_kernel, dim3((unsigned)tiles, (unsigned)n_img), dim3(256), 0, s, static_cast<const uint16_t *>(f0),
                       static_cast<const uint16_t *>(f1), w, (int)HW, (int)Cc, tiles, partials);
    hipLaunchKernelGGL(v2v::lpips_compare_reduce_kernel, dim3((unsigned)n_img), dim3(64), 0, s, partials, tiles, (int)HW, dist);
    return launched("lpips_compare_fwd_kernel launch");
}

int v2v_lpips_compare_bwd_hip(const void *f0, const void *f1, const float *w, const float *ddist, int64_t n_img, int64_t HW, int64_t Cc, void *df0, void *stream)
{
    if (!f0 || !f1 || !w || !ddist || !df0) return fail(V2V_ERR_NULL, "v2v_lpips_compare_bwd_hip: f0/f1/w/ddist/df0 is NULL");
    if (const int rc = lpips_compare_check("v2v_lpips_compare_bwd_hip", n_img, HW, Cc)) return rc;
    if (!aligned(f0, 16) || !aligned(f1, 16) || !aligned(w, 4) || !aligned(ddist, 4) || !aligned(df0, 16))
        return fail(V2V_ERR_ALIGN, "v2v_lpips_compare_bwd_hip: f0/f1/df0 need 16-byte alignment, w/ddist 4-byte");
    const int tiles = ((int)HW + v2v::kLpCmpTile - 1) / v2v::kLpCmpTile;
    hipLaunchKernelGGL(v2v::lpips_compare_bwd_kernel, dim3((unsigned)tiles, (unsigned)n_img), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(f0), static_cast<const uint16_t *>(f1), w, ddist, (int)HW, (int)Cc, static_cast<uint16_t *>(df0));
    return launched("lpips_compare_bwd_kernel launch");
}

}  // extern "C"
