// v2v_lpips_tu.hip -- translation unit of the LPIPS-VGG loss kernels (v2v_lpips.hpp): launchers.
#define V2V_LPIPS_KERNELS
#include "v2v_lpips.hpp"

namespace v2v {

namespace {

unsigned blocks256(int64_t threads) { return (unsigned)((threads + 255) / 256); }

}  // namespace

hipError_t launch_lpips_stem(const void *x, int x_bf16, int B, int Cin, int H, int W, const float *weight, const float *bias, const float *shift,
                             const float *scale, int normalize, uint16_t *out, hipStream_t s)
{
    const unsigned tiles = (unsigned)(((H + kLpStemTile - 1) / kLpStemTile) * ((W + kLpStemTile - 1) / kLpStemTile));
    hipLaunchKernelGGL(lpips_stem_kernel, dim3(tiles, (unsigned)B), dim3(256), 0, s, x, x_bf16, Cin, H, W, weight, bias, shift, scale, normalize, out);
    return hipGetLastError();
}

hipError_t launch_lpips_stem_bwd(const uint16_t *dz, int B, int Cin, int H, int W, const float *weight, const float *scale, int normalize, float *dpred,
                                 hipStream_t s)
{
    hipLaunchKernelGGL(lpips_stem_bwd_kernel, dim3(blocks256((int64_t)H * W), (unsigned)B), dim3(256), 0, s, dz, Cin, H, W, weight, scale, normalize, dpred);
    return hipGetLastError();
}

hipError_t launch_lpips_pool(const uint16_t *x, int B, int H, int W, int C, uint16_t *out, hipStream_t s)
{
    const int64_t total = (int64_t)B * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(lpips_pool_kernel, dim3(blocks256(total)), dim3(256), 0, s, x, H, W, C, total, out);
    return hipGetLastError();
}

hipError_t launch_lpips_pool_bwd(const uint16_t *dy, const uint16_t *x, const uint16_t *dtap, int relu_mask, int B, int H, int W, int C, uint16_t *dx,
                                 hipStream_t s)
{
    const int64_t total = (int64_t)B * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(lpips_pool_bwd_kernel, dim3(blocks256(total)), dim3(256), 0, s, dy, x, dtap, relu_mask, H, W, C, total, dx);
    return hipGetLastError();
}

hipError_t launch_lpips_compare_fwd(const uint16_t *f0, const uint16_t *f1, const float *w, int n_img, int HW, int Cc, float *partials, float *dist,
                                    hipStream_t s)
{
    const int tiles = (HW + kLpCmpTile - 1) / kLpCmpTile;
    hipLaunchKernelGGL(lpips_compare_fwd_kernel, dim3((unsigned)tiles, (unsigned)n_img), dim3(256), 0, s, f0, f1, w, HW, Cc, tiles, partials);
    hipLaunchKernelGGL(lpips_compare_reduce_kernel, dim3((unsigned)n_img), dim3(64), 0, s, partials, tiles, HW, dist);
    return hipGetLastError();
}

hipError_t launch_lpips_compare_bwd(const uint16_t *f0, const uint16_t *f1, const float *w, const float *ddist, int n_img, int HW, int Cc, uint16_t *df0,
                                    hipStream_t s)
{
    const int tiles = (HW + kLpCmpTile - 1) / kLpCmpTile;
    hipLaunchKernelGGL(lpips_compare_bwd_kernel, dim3((unsigned)tiles, (unsigned)n_img), dim3(256), 0, s, f0, f1, w, ddist, HW, Cc, df0);
    return hipGetLastError();
}

}  // namespace v2v
