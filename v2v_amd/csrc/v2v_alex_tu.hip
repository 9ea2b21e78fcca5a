// v2v_alex_tu.hip -- translation unit of the LPIPS-AlexNet test metric (v2v_alex.hpp): its kernels and their C entry points
// (include/v2v_lpips_alex.h).
#include "../../include/v2v_lpips_alex.h"
#include "v2v_alex.hpp"
#include "v2v_status.hpp"

#include <cmath>

using v2v::aligned;
using v2v::fail;
using v2v::launched;

namespace {

constexpr int64_t kMaxElems = 0x7FFFFFFFLL;
constexpr int64_t kMaxSide = 1 << 20;

unsigned blocks256(int64_t threads) { return (unsigned)((threads + 255) / 256); }

// n >= 0 and [n][H][W][C] below 2^31 elements, H and W in lo..2^20
int nhwc_check(const char *who, int64_t n, int64_t H, int64_t W, int64_t C, int64_t lo)
{
    if (n < 0) return fail(V2V_ERR_SHAPE, "%s: n must be >= 0 (got %lld)", who, (long long)n);
    if (H < lo || W < lo || H > kMaxSide || W > kMaxSide) return fail(V2V_ERR_SHAPE, "%s: need H and W >= %lld (got %lld x %lld)", who, (long long)lo, (long long)H, (long long)W);
    if (C < 1 || C > 65536 || H * W > kMaxElems / C || (n > 0 && H * W * C > kMaxElems / n))
        return fail(V2V_ERR_SHAPE, "%s: [n,H,W,C] must stay below 2^31 elements (got %lld x %lld x %lld x %lld)", who, (long long)n, (long long)H, (long long)W, (long long)C);
    return V2V_OK;
}

int64_t compare_tiles(const char *who, int64_t n, int64_t HW)
{
    if (n < 0 || n > 65535) return fail(V2V_ERR_SHAPE, "%s: need 0 <= n <= 65535 (got %lld)", who, (long long)n);
    if (HW < 1 || HW > kMaxElems / 384 || (n > 0 && HW * 384 > kMaxElems / n))
        return fail(V2V_ERR_SHAPE, "%s: need HW >= 1 and [n,HW,384] below 2^31 elements (got n %lld, HW %lld)", who, (long long)n, (long long)HW);
    return (HW + v2v::kAlexCmpPix - 1) / v2v::kAlexCmpPix;
}

}  // namespace

extern "C" {

int v2v_lpips_alex_stem_hip(const float *frames, int64_t frame_stride, int64_t n, int64_t cin, int64_t H, int64_t W, float divisor, int normalize,
                            const float *shift, const float *scale, const float *weight, const float *bias, float *out, void *stream)
{
    const char *who = "v2v_lpips_alex_stem_hip";
    if (n != 0 && (!frames || !shift || !scale || !weight || !bias || !out)) return fail(V2V_ERR_NULL, "%s: frames/shift/scale/weight/bias/out is NULL", who);
    if (cin != 1 && cin != 3) return fail(V2V_ERR_SHAPE, "%s: a frame has 1 or 3 channels (got %lld)", who, (long long)cin);
    if (const int rc = nhwc_check(who, n, H, W, 64, 31)) return rc;
    if (n > 65535) return fail(V2V_ERR_SHAPE, "%s: need n <= 65535 (got %lld)", who, (long long)n);
    if (frame_stride < 0) return fail(V2V_ERR_SHAPE, "%s: the frame stride must be >= 0", who);
    if (!(std::isfinite(divisor) && divisor != 0.0f)) return fail(V2V_ERR_PARAM, "%s: divisor must be finite and non-zero (got %g)", who, (double)divisor);
    if (n == 0) return V2V_OK;
    if (!aligned(frames, 4) || !aligned(shift, 4) || !aligned(scale, 4) || !aligned(bias, 4) || !aligned(weight, 16) || !aligned(out, 16))
        return fail(V2V_ERR_ALIGN, "%s: weight/out need 16-byte alignment, frames/shift/scale/bias 4-byte", who);
    const int OH = (int)((H - 7) / 4 + 1), OW = (int)((W - 7) / 4 + 1);
    const int tx = (OW + v2v::kAlexStemTX - 1) / v2v::kAlexStemTX, ty = (OH + v2v::kAlexStemTY - 1) / v2v::kAlexStemTY;
    hipLaunchKernelGGL(v2v::alex_stem_kernel, dim3((unsigned)(tx * ty), (unsigned)n), dim3(v2v::kAlexThreads), 0, static_cast<hipStream_t>(stream), frames, frame_stride,
                       (int)cin, (int)H, (int)W, OH, OW, tx, divisor, normalize ? 1 : 0, shift, scale, weight, bias, out);
    return launched("alex_stem_kernel launch");
}

int v2v_lpips_alex_conv_hip(const float *x, const float *weight, const float *bias, int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ks,
                            int relu, float *y, void *stream)
{
    const char *who = "v2v_lpips_alex_conv_hip";
    if (n != 0 && (!x || !weight || !bias || !y)) return fail(V2V_ERR_NULL, "%s: x/weight/bias/y is NULL", who);
    if (ks != 3 && ks != 5) return fail(V2V_ERR_SHAPE, "%s: ks must be 3 or 5 (got %d)", who, ks);
    if (Cin < 32 || Cin > 4096 || Cin % 32 != 0 || Cout < 64 || Cout > 4096 || Cout % 64 != 0)
        return fail(V2V_ERR_SHAPE, "%s: Cin must be a multiple of 32 and Cout a multiple of 64, both <= 4096 (got %lld -> %lld)", who, (long long)Cin, (long long)Cout);
    if (const int rc = nhwc_check(who, n, H, W, Cin > Cout ? Cin : Cout, 1)) return rc;
    if (n == 0) return V2V_OK;
    if (!aligned(x, 16) || !aligned(weight, 16) || !aligned(y, 16) || !aligned(bias, 4)) return fail(V2V_ERR_ALIGN, "%s: x/weight/y need 16-byte alignment, bias 4-byte", who);
    v2v::AlexConvArgs a{};
    a.x = x;
    a.w = weight;
    a.bias = bias;
    a.y = y;
    a.M = (int)(n * H * W);
    a.H = (int)H;
    a.W = (int)W;
    a.Cin = (int)Cin;
    a.Cout = (int)Cout;
    a.relu = relu ? 1 : 0;
    const dim3 grid((unsigned)((a.M + v2v::kAlexBM - 1) / v2v::kAlexBM), (unsigned)(Cout / v2v::kAlexBN));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ks == 5)
        hipLaunchKernelGGL(v2v::alex_conv_kernel<5>, grid, dim3(v2v::kAlexThreads), 0, s, a);
    else
        hipLaunchKernelGGL(v2v::alex_conv_kernel<3>, grid, dim3(v2v::kAlexThreads), 0, s, a);
    return launched("alex_conv_kernel launch");
}

int v2v_lpips_alex_pool_hip(const float *x, int64_t n, int64_t H, int64_t W, int64_t C, float *y, void *stream)
{
    const char *who = "v2v_lpips_alex_pool_hip";
    if (n != 0 && (!x || !y)) return fail(V2V_ERR_NULL, "%s: x/y is NULL", who);
    if (C < 4 || C % 4 != 0) return fail(V2V_ERR_SHAPE, "%s: C must be a multiple of 4 (got %lld)", who, (long long)C);
    if (const int rc = nhwc_check(who, n, H, W, C, 3)) return rc;
    if (n == 0) return V2V_OK;
    if (!aligned(x, 16) || !aligned(y, 16)) return fail(V2V_ERR_ALIGN, "%s: x/y need 16-byte alignment", who);
    const int OH = (int)((H - 3) / 2 + 1), OW = (int)((W - 3) / 2 + 1);
    const int64_t total = n * OH * OW * (C / 4);
    hipLaunchKernelGGL(v2v::alex_pool_kernel, dim3(blocks256(total)), dim3(v2v::kAlexThreads), 0, static_cast<hipStream_t>(stream), x, (int)H, (int)W, OH, OW, (int)C,
                       total, y);
    return launched("alex_pool_kernel launch");
}

int64_t v2v_lpips_alex_compare_workspace_bytes(int64_t n, int64_t HW)
{
    const int64_t tiles = compare_tiles("v2v_lpips_alex_compare_workspace_bytes", n, HW);
    return tiles < 0 ? tiles : n * tiles * 8;
}

int v2v_lpips_alex_compare_hip(const float *f0, const float *f1, const float *w, int64_t n, int64_t HW, int64_t C, int tap, void *workspace, double *taps,
                               void *stream)
{
    const char *who = "v2v_lpips_alex_compare_hip";
    if (n != 0 && (!f0 || !f1 || !w || !workspace || !taps)) return fail(V2V_ERR_NULL, "%s: f0/f1/w/workspace/taps is NULL", who);
    const int64_t tiles = compare_tiles(who, n, HW);
    if (tiles < 0) return (int)tiles;
    if (C != 64 && C != 192 && C != 256 && C != 384) return fail(V2V_ERR_SHAPE, "%s: C must be 64, 192, 256 or 384 (got %lld)", who, (long long)C);
    if (tap < 0 || tap > 4) return fail(V2V_ERR_SHAPE, "%s: tap must be 0..4 (got %d)", who, tap);
    if (n == 0) return V2V_OK;
    if (!aligned(f0, 4) || !aligned(f1, 4) || !aligned(w, 4) || !aligned(workspace, 8) || !aligned(taps, 8))
        return fail(V2V_ERR_ALIGN, "%s: f0/f1/w need 4-byte, workspace/taps 8-byte alignment", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *slots = static_cast<double *>(workspace);
    const dim3 grid((unsigned)tiles, (unsigned)n), block(v2v::kAlexThreads);
    switch (C) {
    case 64: hipLaunchKernelGGL(v2v::alex_compare_kernel<1>, grid, block, 0, s, f0, f1, w, (int)HW, (int)tiles, slots); break;
    case 192: hipLaunchKernelGGL(v2v::alex_compare_kernel<3>, grid, block, 0, s, f0, f1, w, (int)HW, (int)tiles, slots); break;
    case 256: hipLaunchKernelGGL(v2v::alex_compare_kernel<4>, grid, block, 0, s, f0, f1, w, (int)HW, (int)tiles, slots); break;
    default: hipLaunchKernelGGL(v2v::alex_compare_kernel<6>, grid, block, 0, s, f0, f1, w, (int)HW, (int)tiles, slots); break;
    }
    if (const int rc = launched("alex_compare_kernel launch")) return rc;
    hipLaunchKernelGGL(v2v::alex_reduce_kernel, dim3(blocks256(n)), block, 0, s, slots, (int)n, (int)tiles, (double)HW, tap, taps);
    return launched("alex_reduce_kernel launch");
}

int v2v_lpips_alex_sum_hip(const double *taps, int64_t n, float *dist, void *stream)
{
    const char *who = "v2v_lpips_alex_sum_hip";
    if (n != 0 && (!taps || !dist)) return fail(V2V_ERR_NULL, "%s: taps/dist is NULL", who);
    if (n < 0 || n > kMaxElems / 5) return fail(V2V_ERR_SHAPE, "%s: need 0 <= n < 2^31 / 5 (got %lld)", who, (long long)n);
    if (n == 0) return V2V_OK;
    if (!aligned(taps, 8) || !aligned(dist, 4)) return fail(V2V_ERR_ALIGN, "%s: taps needs 8-byte, dist 4-byte alignment", who);
    hipLaunchKernelGGL(v2v::alex_sum_kernel, dim3(blocks256(n)), dim3(v2v::kAlexThreads), 0, static_cast<hipStream_t>(stream), taps, (int)n, dist);
    return launched("alex_sum_kernel launch");
}

}  // extern "C"
