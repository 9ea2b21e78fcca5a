// v2v_alex_train_tu.hip -- translation unit of LPIPS-AlexNet's backward to the prediction (v2v_alex_train.hpp): its kernels and their C
// entry points (include/v2v_alex_train.h).
#include "../../include/v2v_alex_train.h"
#include "v2v_alex_train.hpp"
#include "v2v_status.hpp"

#include <cmath>

using v2v::aligned;
using v2v::fail;
using v2v::launched;

namespace {

constexpr int64_t kMaxElems = 0x7FFFFFFFLL;
constexpr int64_t kMaxSide = 1 << 20;

// n >= 0 and [n][H][W][C] below 2^31 elements, H and W in lo..2^20
int nhwc_check(const char *who, int64_t n, int64_t H, int64_t W, int64_t C, int64_t lo)
{
    if (n < 0) return fail(V2V_ERR_SHAPE, "%s: n must be >= 0 (got %lld)", who, (long long)n);
    if (H < lo || W < lo || H > kMaxSide || W > kMaxSide) return fail(V2V_ERR_SHAPE, "%s: need H and W >= %lld (got %lld x %lld)", who, (long long)lo, (long long)H, (long long)W);
    if (C < 1 || C > 65536 || H * W > kMaxElems / C || (n > 0 && H * W * C > kMaxElems / n))
        return fail(V2V_ERR_SHAPE, "%s: [n,H,W,C] must stay below 2^31 elements (got %lld x %lld x %lld x %lld)", who, (long long)n, (long long)H, (long long)W, (long long)C);
    return V2V_OK;
}

}  // namespace

extern "C" {

int v2v_alex_train_compare_bwd_hip(const float *f0, const float *f1, const float *w, const float *ddist, int64_t n, int64_t HW, int64_t C, int relu_mask,
                                   float *dz, void *stream)
{
    const char *who = "v2v_alex_train_compare_bwd_hip";
    if (n != 0 && (!f0 || !f1 || !w || !ddist || !dz)) return fail(V2V_ERR_NULL, "%s: f0/f1/w/ddist/dz is NULL", who);
    if (n < 0 || n > 65535) return fail(V2V_ERR_SHAPE, "%s: need 0 <= n <= 65535 (got %lld)", who, (long long)n);
    if (HW < 1 || HW > kMaxElems / 384 || (n > 0 && HW * 384 > kMaxElems / n))
        return fail(V2V_ERR_SHAPE, "%s: need HW >= 1 and [n,HW,384] below 2^31 elements (got n %lld, HW %lld)", who, (long long)n, (long long)HW);
    if (C != 64 && C != 192 && C != 256 && C != 384) return fail(V2V_ERR_SHAPE, "%s: C must be 64, 192, 256 or 384 (got %lld)", who, (long long)C);
    if (n == 0) return V2V_OK;
    if (!aligned(f0, 4) || !aligned(f1, 4) || !aligned(w, 4) || !aligned(ddist, 4) || !aligned(dz, 4)) return fail(V2V_ERR_ALIGN, "%s: f0/f1/w/ddist/dz need 4-byte alignment", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rm = relu_mask ? 1 : 0;
    const dim3 grid((unsigned)((HW + v2v::kAlexCmpPix - 1) / v2v::kAlexCmpPix), (unsigned)n), block(v2v::kAlexThreads);
    switch (C) {
    case 64: hipLaunchKernelGGL(v2v::alex_compare_bwd_kernel<1>, grid, block, 0, s, f0, f1, w, ddist, (int)HW, rm, dz); break;
    case 192: hipLaunchKernelGGL(v2v::alex_compare_bwd_kernel<3>, grid, block, 0, s, f0, f1, w, ddist, (int)HW, rm, dz); break;
    case 256: hipLaunchKernelGGL(v2v::alex_compare_bwd_kernel<4>, grid, block, 0, s, f0, f1, w, ddist, (int)HW, rm, dz); break;
    default: hipLaunchKernelGGL(v2v::alex_compare_bwd_kernel<6>, grid, block, 0, s, f0, f1, w, ddist, (int)HW, rm, dz); break;
    }
    return launched("alex_compare_bwd_kernel launch");
}

int v2v_alex_train_conv_dgrad_hip(const float *dy, const float *weight, const float *dtap, const float *mask, int64_t n, int64_t H, int64_t W, int64_t Cin,
                                  int64_t Cout, int ks, float *dx, void *stream)
{
    const char *who = "v2v_alex_train_conv_dgrad_hip";
    if (n != 0 && (!dy || !weight || !dx)) return fail(V2V_ERR_NULL, "%s: dy/weight/dx is NULL", who);
    if (ks != 3 && ks != 5) return fail(V2V_ERR_SHAPE, "%s: ks must be 3 or 5 (got %d)", who, ks);
    if (Cout < 32 || Cout > 4096 || Cout % 32 != 0 || Cin < 64 || Cin > 4096 || Cin % 64 != 0)
        return fail(V2V_ERR_SHAPE, "%s: Cout must be a multiple of 32 and Cin a multiple of 64, both <= 4096 (got %lld -> %lld)", who, (long long)Cin, (long long)Cout);
    if (const int rc = nhwc_check(who, n, H, W, Cin > Cout ? Cin : Cout, 1)) return rc;
    if (n == 0) return V2V_OK;
    if (!aligned(dy, 16) || !aligned(weight, 16) || !aligned(dx, 16) || !aligned(dtap, 16) || !aligned(mask, 16))
        return fail(V2V_ERR_ALIGN, "%s: dy/weight/dtap/mask/dx need 16-byte alignment", who);
    // the forward's main loop reads a.x [M][a.Cin] against a.w [ks * ks * a.Cin][a.Cout]: here a.Cin is the forward's Cout and vice versa
    v2v::AlexConvArgs a{};
    a.x = dy;
    a.w = weight;
    a.bias = nullptr;
    a.y = dx;
    a.M = (int)(n * H * W);
    a.H = (int)H;
    a.W = (int)W;
    a.Cin = (int)Cout;
    a.Cout = (int)Cin;
    a.relu = 0;
    const dim3 grid((unsigned)((a.M + v2v::kAlexBM - 1) / v2v::kAlexBM), (unsigned)(Cin / v2v::kAlexBN));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ks == 5)
        hipLaunchKernelGGL(v2v::alex_dgrad_kernel<5>, grid, dim3(v2v::kAlexThreads), 0, s, a, dtap, mask);
    else
        hipLaunchKernelGGL(v2v::alex_dgrad_kernel<3>, grid, dim3(v2v::kAlexThreads), 0, s, a, dtap, mask);
    return launched("alex_dgrad_kernel launch");
}

int v2v_alex_train_pool_bwd_hip(const float *x, const float *dy, const float *dtap, int64_t n, int64_t H, int64_t W, int64_t C, int relu_mask, float *dx,
                                void *stream)
{
    const char *who = "v2v_alex_train_pool_bwd_hip";
    if (n != 0 && (!x || !dy || !dx)) return fail(V2V_ERR_NULL, "%s: x/dy/dx is NULL", who);
    if (C < 4 || C % 4 != 0) return fail(V2V_ERR_SHAPE, "%s: C must be a multiple of 4 (got %lld)", who, (long long)C);
    if (const int rc = nhwc_check(who, n, H, W, C, 3)) return rc;
    if (n == 0) return V2V_OK;
    if (!aligned(x, 16) || !aligned(dy, 16) || !aligned(dx, 16) || !aligned(dtap, 16)) return fail(V2V_ERR_ALIGN, "%s: x/dy/dtap/dx need 16-byte alignment", who);
    const int OH = (int)((H - 3) / 2 + 1), OW = (int)((W - 3) / 2 + 1);
    const int64_t total = n * H * W * (C / 4);
    hipLaunchKernelGGL(v2v::alex_pool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(v2v::kAlexThreads), 0, static_cast<hipStream_t>(stream), x, dy, dtap, (int)H,
                       (int)W, OH, OW, (int)C, relu_mask ? 1 : 0, total, dx);
    return launched("alex_pool_bwd_kernel launch");
}

int v2v_alex_train_stem_bwd_hip(const float *dz, const float *weight, const float *scale, int64_t n, int64_t cin, int64_t H, int64_t W, float divisor,
                                int normalize, float *dpred, void *stream)
{
    const char *who = "v2v_alex_train_stem_bwd_hip";
    if (n != 0 && (!dz || !weight || !scale || !dpred)) return fail(V2V_ERR_NULL, "%s: dz/weight/scale/dpred is NULL", who);
    if (cin != 1 && cin != 3) return fail(V2V_ERR_SHAPE, "%s: a frame has 1 or 3 channels (got %lld)", who, (long long)cin);
    if (const int rc = nhwc_check(who, n, H, W, 64, 31)) return rc;
    if (n > 65535) return fail(V2V_ERR_SHAPE, "%s: need n <= 65535 (got %lld)", who, (long long)n);
    if (!(std::isfinite(divisor) && divisor != 0.0f)) return fail(V2V_ERR_PARAM, "%s: divisor must be finite and non-zero (got %g)", who, (double)divisor);
    if (n == 0) return V2V_OK;
    if (!aligned(dz, 16) || !aligned(weight, 16) || !aligned(scale, 4) || !aligned(dpred, 4))
        return fail(V2V_ERR_ALIGN, "%s: dz/weight need 16-byte alignment, scale/dpred 4-byte", who);
    const int OH = (int)((H - 7) / 4 + 1), OW = (int)((W - 7) / 4 + 1);
    const int tx = (int)((W + v2v::kAlexSbTile - 1) / v2v::kAlexSbTile), ty = (int)((H + v2v::kAlexSbTile - 1) / v2v::kAlexSbTile);
    hipLaunchKernelGGL(v2v::alex_stem_bwd_kernel, dim3((unsigned)(tx * ty), (unsigned)n), dim3(v2v::kAlexThreads), 0, static_cast<hipStream_t>(stream), dz, weight, scale,
                       (int)cin, (int)H, (int)W, OH, OW, tx, divisor, normalize ? 1 : 0, dpred);
    return launched("alex_stem_bwd_kernel launch");
}

}  // extern "C"
