// v2v_loss_tu.hip -- translation unit of the training losses (v2v_loss.hpp): launchers.
#define V2V_LOSS_KERNELS
#include "v2v_loss.hpp"

namespace v2v {

namespace {

dim3 loss_grid(const LossArgs &a) { return dim3((unsigned)(a.n_img * a.tiles)); }

// n contiguous [c,h,w] images with a [n,2,h,w] flow, every one of them warped
LossArgs plain_args(const float *flow, int64_t n, int c, int h, int w)
{
    LossArgs a{};
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

}  // namespace

hipError_t launch_tc_loss_fwd(const LossArgs &a, float *partials, float *losses, float *image0_warped, float *processed0_warped, float *visibility,
                              float *error_map, hipStream_t s)
{
    hipLaunchKernelGGL(tc_loss_fwd_kernel, loss_grid(a), dim3(kLossTile), 0, s, a, partials, image0_warped, processed0_warped, visibility, error_map);
    hipLaunchKernelGGL(loss_reduce_kernel, dim3((unsigned)a.n_img), dim3(64), 0, s, partials, losses, a.n_img, a.tiles, (float)((int64_t)a.c * a.h * a.w), a.w_tc,
                       a.w_l1, a.w_l2);
    return hipGetLastError();
}

hipError_t launch_tc_loss_bwd(const LossArgs &a, const float *gout, int chain, float *dprocessed1, float *dprocessed0, unsigned long long *acc, float *dwarp,
                              float *dp1, unsigned *maxbits, hipStream_t s)
{
    if (a.w_tc != 0.0f && a.tc_first < a.inner) {
        hipLaunchKernelGGL(tc_loss_bwd_kernel, loss_grid(a), dim3(kLossTile), 0, s, a, gout, dp1, dwarp, maxbits);
        hipLaunchKernelGGL(warp_adjoint_kernel, loss_grid(a), dim3(kLossTile), 0, s, a, dwarp, maxbits, acc);
    }
    hipLaunchKernelGGL(warp_adjoint_finish_kernel, loss_grid(a), dim3(kLossTile), 0, s, a, gout, chain, acc, dp1, maxbits, dprocessed1, dprocessed0);
    return hipGetLastError();
}

hipError_t launch_warp_bilinear(const float *img, const float *flow, int64_t n, int c, int h, int w, float *out, hipStream_t s)
{
    const LossArgs a = plain_args(flow, n, c, h, w);
    hipLaunchKernelGGL(warp_bilinear_kernel, loss_grid(a), dim3(kLossTile), 0, s, a, img, out);
    return hipGetLastError();
}

hipError_t launch_warp_bilinear_adjoint(const float *dout, const float *flow, int64_t n, int c, int h, int w, float *din, unsigned long long *acc, unsigned *maxbits,
                                        hipStream_t s)
{
    const LossArgs a = plain_args(flow, n, c, h, w);
    const int64_t per_img = a.so, total = n * per_img;
    const unsigned bx = (unsigned)((per_img + kLossTile - 1) / kLossTile < 64 ? (per_img + kLossTile - 1) / kLossTile : 64);
    hipLaunchKernelGGL(warp_absmax_kernel, dim3(bx, (unsigned)n), dim3(kLossTile), 0, s, dout, per_img, maxbits);
    hipLaunchKernelGGL(warp_adjoint_kernel, loss_grid(a), dim3(kLossTile), 0, s, a, dout, maxbits, acc);
    hipLaunchKernelGGL(warp_adjoint_plain_finish_kernel, dim3((unsigned)((total + kLossTile - 1) / kLossTile)), dim3(kLossTile), 0, s, acc, maxbits, per_img, total, din);
    return hipGetLastError();
}

}  // namespace v2v
