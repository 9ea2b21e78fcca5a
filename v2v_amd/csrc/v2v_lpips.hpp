// v2v_lpips.hpp -- the pieces of the LPIPS-VGG perceptual loss (PerceptualSimilarity/models/networks_basic.py:PNetLin, model/loss.py:95-119)
// that are not a 64..512-channel 3x3 convolution; those twelve convolutions and their data gradients run on the convolution kernel of
// v2v_convlstm.hpp (conv_nhwc / the dgrad-packed stream), this file adds what sits around them.
//
// Kernels in this file (launched by the C entry points in v2v_lpips_tu.hip):
//   lpips_stem_kernel            [B,1|3,H,W] float32 / bf16 -> optional 2x - 1, (x - shift) / scale, 3x3 conv 3 -> 64, bias, ReLU -> bf16 NHWC.
//                                K = 27 on the vector ALU: a 16 x 16 pixel tile with its halo, scaled, in LDS (zero padding is zero AFTER the
//                                scaling layer), the 27 x 64 weights in LDS (wave-uniform broadcast reads), one pixel per thread
//   lpips_stem_bwd_kernel        dz bf16 NHWC (ReLU-masked) -> dpred float32 NCHW: the transposed conv 64 -> 3 in float32, times
//                                (2 if normalize else 1) / scale_c, the three channels summed for a one-channel pred
//   lpips_pool_kernel            2x2 max-pool on NHWC bf16
//   lpips_pool_bwd_kernel        its backward: the gradient goes to the FIRST maximum of the window in row-major order (autograd's rule);
//                                optionally + a second gradient of the pooled tensor (the compare kernel's), added in float32 and rounded to
//                                bf16 once, optionally through the ReLU mask x > 0: tap gradient + pool gradient + mask in one launch
//   lpips_compare_fwd_kernel     per pixel n = f / (sqrt(sum f^2) + 1e-10) for both halves of a tap, sum_c w_c (n0_c - n1_c)^2; one partial
//   lpips_compare_reduce_kernel  per 64-pixel tile into a fixed slot, then per sample the tiles in a fixed order: dist[b] += sum / HW
//   lpips_compare_bwd_kernel     df0 (bf16) from ddist[b]: g_c = 2 w_c (n0_c - n1_c) ddist / HW, df0_c = g_c / (r + eps) - f0_c (sum_k g_k f0_k) /
//                                (r (r + eps)^2) with r = |f0|; at r == 0 the second term is DEFINED as 0 (autograd gives NaN: sqrt' at 0)
//
// A pixel's C channels are spread over C / 8 lanes (16 bytes per lane per load), so 8 / 4 / 2 / 1 pixels per wave at 64 / 128 / 256 / 512
// channels; sums over the channels are xor butterflies inside that lane group (every lane ends with the same bits).  No float atomics:
// every reduction has one fixed order, and a sample's result does not depend on what else is in the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v2v {

constexpr int kLpStemTile = 16;                 // the stem's tile: 16 x 16 pixels = 256 threads
constexpr int kLpCmpTile = 64;                  // pixels per workgroup of the compare kernels
constexpr float kLpEps = 1e-10f;                // normalize_tensor's eps (PerceptualSimilarity/models/__init__.py:48-50)

#ifdef V2V_LPIPS_KERNELS

typedef __bf16 lp_hwbf16x2 __attribute__((ext_vector_type(2)));
typedef float lp_f32x2 __attribute__((ext_vector_type(2)));

// float -> bf16 round to nearest even (v_cvt_pk_bf16_f32), NaN stays NaN
__device__ __forceinline__ uint32_t lp_pack_bf16(float lo, float hi)
{
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(lp_f32x2{lo, hi}, lp_hwbf16x2));
}
__device__ __forceinline__ float lp_f32(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// the 8 bf16 of a 16-byte vector as floats, and back
__device__ __forceinline__ void lp_unpack8(const uint4 &v, float (&f)[8])
{
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xFFFF0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xFFFF0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xFFFF0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xFFFF0000u);
}
__device__ __forceinline__ uint4 lp_pack8(const float (&f)[8])
{
    return make_uint4(lp_pack_bf16(f[0], f[1]), lp_pack_bf16(f[2], f[3]), lp_pack_bf16(f[4], f[5]), lp_pack_bf16(f[6], f[7]));
}

// sum over the `g` lanes (8, 16, 32 or 64, aligned) that share a pixel; every lane of the group ends with the same bits
__device__ __forceinline__ float lp_group_sum(float v, int g)
{
    for (int o = g >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- stem ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lpips_stem_kernel(const void *x, int x_bf16, int Cin, int H, int W, const float *weight, const float *bias,
                                                         const float *shift, const float *scale, int normalize, uint16_t *out)
{
    constexpr int T = kLpStemTile, P = T + 2;
    __shared__ float s_in[3][P][P];                                  // the scaled tile with its halo; outside the image: 0
    __shared__ __attribute__((aligned(16))) float s_w[27][64];       // [ci * 9 + ky * 3 + kx][co]
    __shared__ float s_b[64];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int tiles_x = (W + T - 1) / T;
    const int ty0 = ((int)blockIdx.x / tiles_x) * T, tx0 = ((int)blockIdx.x % tiles_x) * T;
    for (int i = tid; i < 27 * 64; i += 256) {
        const int co = i / 27, k = i - co * 27;                      // weight [64][3][3][3]
        s_w[k][co] = weight[i];
    }
    if (tid < 64) s_b[tid] = bias[tid];
    for (int i = tid; i < 3 * P * P; i += 256) {
        const int c = i / (P * P), r = i - c * (P * P), py = r / P, px = r - py * P;
        const int y = ty0 + py - 1, xx = tx0 + px - 1;
        float v = 0.0f;
        if ((unsigned)y < (unsigned)H && (unsigned)xx < (unsigned)W) {
            const int64_t idx = (((int64_t)b * Cin + (Cin == 3 ? c : 0)) * H + y) * W + xx;      // one channel stands for three equal ones
            float raw = x_bf16 ? lp_f32(static_cast<const uint16_t *>(x)[idx]) : static_cast<const float *>(x)[idx];
            if (normalize) raw = 2.0f * raw - 1.0f;
            v = (raw - shift[c]) / scale[c];
        }
        s_in[c][py][px] = v;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15, y = ty0 + ty, xx = tx0 + tx;
    float in[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) in[c * 9 + ky * 3 + kx] = s_in[c][ty + ky][tx + kx];
    if (y >= H || xx >= W) return;                                   // (no barrier below)
    uint4 *o = reinterpret_cast<uint4 *>(out + (((int64_t)b * H + y) * W + xx) * 64);
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {                                    // 16 output channels at a time: 16 accumulators per thread
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const float4 *wr = reinterpret_cast<const float4 *>(&s_w[k][g * 16]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 w4 = wr[q];
                acc[4 * q + 0] = fmaf(in[k], w4.x, acc[4 * q + 0]);
                acc[4 * q + 1] = fmaf(in[k], w4.y, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(in[k], w4.z, acc[4 * q + 2]);
                acc[4 * q + 3] = fmaf(in[k], w4.w, acc[4 * q + 3]);
            }
        }
        float r0[8], r1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            r0[j] = fmaxf(acc[j] + s_b[g * 16 + j], 0.0f);
            r1[j] = fmaxf(acc[8 + j] + s_b[g * 16 + 8 + j], 0.0f);
        }
        o[2 * g] = lp_pack8(r0);
        o[2 * g + 1] = lp_pack8(r1);
    }
}

// dxs[ci][Y][X] = sum_{ky,kx,co} dz[Y - ky + 1][X - kx + 1][co] * w[co][ci][ky][kx]: with (oy, ox) = (1 - ky, 1 - kx) a 3x3 gather of dz
__global__ void __launch_bounds__(256) lpips_stem_bwd_kernel(const uint16_t *dz, int Cin, int H, int W, const float *weight, const float *scale,
                                                             int normalize, float *dpred)
{
    __shared__ __attribute__((aligned(16))) float s_w[9][64][4];     // [(oy + 1) * 3 + (ox + 1)][co][ci, one pad]
    const int tid = threadIdx.x, b = blockIdx.y;
    for (int i = tid; i < 9 * 64 * 4; i += 256) {
        const int t = i >> 8, co = (i >> 2) & 63, ci = i & 3;
        s_w[t][co][ci] = ci < 3 ? weight[((co * 3 + ci) * 3 + (2 - t / 3)) * 3 + (2 - t % 3)] : 0.0f;
    }
    __syncthreads();
    const int HW = H * W, pix = (int)blockIdx.x * 256 + tid;
    if (pix >= HW) return;                                           // (no barrier below)
    const int Y = pix / W, X = pix - Y * W;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
        const int yy = Y + t / 3 - 1, xx = X + t % 3 - 1;
        if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
        const uint4 *p = reinterpret_cast<const uint4 *>(dz + (((int64_t)b * H + yy) * W + xx) * 64);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            float d[8];
            lp_unpack8(p[g], d);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float4 w4 = *reinterpret_cast<const float4 *>(&s_w[t][g * 8 + j][0]);
                a0 = fmaf(d[j], w4.x, a0);
                a1 = fmaf(d[j], w4.y, a1);
                a2 = fmaf(d[j], w4.z, a2);
            }
        }
    }
    const float k = normalize ? 2.0f : 1.0f;
    const float g0 = a0 * (k / scale[0]), g1 = a1 * (k / scale[1]), g2 = a2 * (k / scale[2]);
    if (Cin == 3) {
        float *o = dpred + (int64_t)b * 3 * HW + pix;
        o[0] = g0;
        o[HW] = g1;
        o[2 * (int64_t)HW] = g2;
    } else {
        dpred[(int64_t)b * HW + pix] = (g0 + g1) + g2;
    }
}

// ---- 2x2 max-pool ---------------------------------------------------------------------------------------------------------------------------
// one thread per output pixel and 8 channels; total = B * (H/2) * (W/2) * (C/8) threads
struct LpWindow {
    int64_t i00, i01, i10, i11, o;                                   // element offsets of the four inputs and of the output
};

__device__ __forceinline__ bool lp_window(int64_t idx, int64_t total, int H, int W, int C, LpWindow &w)
{
    if (idx >= total) return false;
    const int cg = C >> 3, Ho = H >> 1, Wo = W >> 1;
    const int c8 = (int)(idx % cg);
    const int64_t op = idx / cg;
    const int ox = (int)(op % Wo);
    const int64_t r = op / Wo;
    const int oy = (int)(r % Ho);
    const int64_t b = r / Ho;
    w.i00 = (((b * H + 2 * oy) * W + 2 * ox) * (int64_t)C) + 8 * c8;
    w.i01 = w.i00 + C;
    w.i10 = w.i00 + (int64_t)W * C;
    w.i11 = w.i10 + C;
    w.o = op * C + 8 * c8;
    return true;
}

__global__ void __launch_bounds__(256) lpips_pool_kernel(const uint16_t *x, int H, int W, int C, int64_t total, uint16_t *out)
{
    LpWindow w;
    if (!lp_window((int64_t)blockIdx.x * 256 + threadIdx.x, total, H, W, C, w)) return;
    float a[8], b[8], c[8], d[8], m[8];
    lp_unpack8(*reinterpret_cast<const uint4 *>(x + w.i00), a);
    lp_unpack8(*reinterpret_cast<const uint4 *>(x + w.i01), b);
    lp_unpack8(*reinterpret_cast<const uint4 *>(x + w.i10), c);
    lp_unpack8(*reinterpret_cast<const uint4 *>(x + w.i11), d);
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = fmaxf(fmaxf(a[j], b[j]), fmaxf(c[j], d[j]));
    *reinterpret_cast<uint4 *>(out + w.o) = lp_pack8(m);            // bf16 values: the conversion is exact
}

__global__ void __launch_bounds__(256) lpips_pool_bwd_kernel(const uint16_t *dy, const uint16_t *x, const uint16_t *dtap, int relu_mask, int H, int W,
                                                             int C, int64_t total, uint16_t *dx)
{
    LpWindow w;
    if (!lp_window((int64_t)blockIdx.x * 256 + threadIdx.x, total, H, W, C, w)) return;
    const int64_t off[4] = {w.i00, w.i01, w.i10, w.i11};
    float v[4][8], g[8], r[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) lp_unpack8(*reinterpret_cast<const uint4 *>(x + off[q]), v[q]);
    lp_unpack8(*reinterpret_cast<const uint4 *>(dy + w.o), g);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (dtap) {
            lp_unpack8(*reinterpret_cast<const uint4 *>(dtap + off[q]), r[q]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[q][j] = 0.0f;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int first = 0;                                               // the first maximum in row-major order: a later one must be strictly larger
        float best = v[0][j];
        if (v[1][j] > best) { best = v[1][j]; first = 1; }
        if (v[2][j] > best) { best = v[2][j]; first = 2; }
        if (v[3][j] > best) { best = v[3][j]; first = 3; }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float sum = r[q][j] + (first == q ? g[j] : 0.0f);  // float32; rounded to bf16 once, below
            r[q][j] = (relu_mask && !(v[q][j] > 0.0f)) ? 0.0f : sum;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<uint4 *>(dx + off[q]) = lp_pack8(r[q]);
}

// ---- compare --------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lpips_compare_fwd_kernel(const uint16_t *f0, const uint16_t *f1, const float *w, int HW, int Cc, int tiles,
                                                                float *partials)
{
    __shared__ float s_acc[32];
    const int G = Cc >> 3, ngroups = 256 / G;
    const int grp = (int)threadIdx.x / G, gl = (int)threadIdx.x % G;
    const int b = blockIdx.y, tile = blockIdx.x;
    float wv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wv[j] = w[gl * 8 + j];
    float acc = 0.0f;
    for (int p = grp; p < kLpCmpTile; p += ngroups) {
        const int pix = tile * kLpCmpTile + p;
        const bool live = pix < HW;                                  // uniform in the lane group; a dead pixel reads zeros and adds 0
        const int64_t off = ((int64_t)b * HW + (live ? pix : 0)) * Cc + gl * 8;
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        float x0[8], x1[8];
        lp_unpack8(live ? *reinterpret_cast<const uint4 *>(f0 + off) : z, x0);
        lp_unpack8(live ? *reinterpret_cast<const uint4 *>(f1 + off) : z, x1);
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s0 += x0[j] * x0[j];
            s1 += x1[j] * x1[j];
        }
        const float den0 = sqrtf(lp_group_sum(s0, G)) + kLpEps, den1 = sqrtf(lp_group_sum(s1, G)) + kLpEps;
        float d = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float e = x0[j] / den0 - x1[j] / den1;
            d += wv[j] * (e * e);
        }
        acc += lp_group_sum(d, G);
    }
    if (gl == 0) s_acc[grp] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int g = 0; g < ngroups; ++g) t += s_acc[g];
        partials[(int64_t)b * tiles + tile] = t;
    }
}

// one wave per sample: lane l adds tiles l, l + 64, ... in order, then the wave tree; dist[b] += sum / HW
__global__ void __launch_bounds__(64) lpips_compare_reduce_kernel(const float *partials, int tiles, int HW, float *dist)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    float t = 0.0f;
    for (int i = lane; i < tiles; i += 64) t += partials[(int64_t)b * tiles + i];
    t = lp_group_sum(t, 64);
    if (lane == 0) dist[b] = dist[b] + t / (float)HW;
}

__global__ void __launch_bounds__(256) lpips_compare_bwd_kernel(const uint16_t *f0, const uint16_t *f1, const float *w, const float *ddist, int HW, int Cc,
                                                                uint16_t *df0)
{
    const int G = Cc >> 3, ngroups = 256 / G;
    const int grp = (int)threadIdx.x / G, gl = (int)threadIdx.x % G;
    const int b = blockIdx.y, tile = blockIdx.x;
    const float k = ddist[b] / (float)HW;
    float wv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wv[j] = w[gl * 8 + j];
    for (int p = grp; p < kLpCmpTile; p += ngroups) {
        const int pix = tile * kLpCmpTile + p;
        const bool live = pix < HW;
        const int64_t off = ((int64_t)b * HW + (live ? pix : 0)) * Cc + gl * 8;
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        float x0[8], x1[8], g[8];
        lp_unpack8(live ? *reinterpret_cast<const uint4 *>(f0 + off) : z, x0);
        lp_unpack8(live ? *reinterpret_cast<const uint4 *>(f1 + off) : z, x1);
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s0 += x0[j] * x0[j];
            s1 += x1[j] * x1[j];
        }
        const float r0 = sqrtf(lp_group_sum(s0, G));
        const float den0 = r0 + kLpEps, den1 = sqrtf(lp_group_sum(s1, G)) + kLpEps;
        float dot = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            g[j] = 2.0f * wv[j] * (x0[j] / den0 - x1[j] / den1) * k;
            dot += g[j] * x0[j];
        }
        dot = lp_group_sum(dot, G);
        const float back = r0 > 0.0f ? dot / (r0 * (den0 * den0)) : 0.0f;     // r == 0: the second term is defined as 0
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = g[j] / den0 - x0[j] * back;
        if (live) *reinterpret_cast<uint4 *>(df0 + off) = lp_pack8(g);
    }
}

#endif  // V2V_LPIPS_KERNELS

}  // namespace v2v
