// v2v_alex.hpp -- the LPIPS-AlexNet test metric as device kernels, float32 throughout: float32 NHWC activations, float32
// weights, float32 accumulation on the float32-input matrix-core instruction v_mfma_f32_32x32x2_f32 (bit for bit a k-ordered fmaf chain).
//
//   alex_stem_kernel      frames -> /divisor, 2x - 1, scaling layer, 11x11 / stride 4 / pad 2 convolution to 64 channels, bias, ReLU
//   alex_conv_kernel      KS x KS (5 or 3) / stride 1 / pad KS/2 convolution as an implicit GEMM over the n*H*W flattened pixels, bias, ReLU
//   alex_pool_kernel      3x3 / stride 2 max-pool, floor mode
//   alex_compare_kernel   two taps -> per 64-pixel tile  sum_pixels sum_c w_c (n0_c - n1_c)^2  in float64, into a fixed slot
//   alex_reduce_kernel    adds the slots of an image in slot order, writes the tap's mean
//   alex_sum_kernel       dist = the five tap means, each rounded to float32, added in tap order
//
// No split-K and no choice that depends on the number of images: the summation order of an output element is one fixed order of k, so
// a frame's bits do not depend on what shares its launch.  No float atomics.  Built with -ffp-contract=off like the whole library.
// The tile constants and the convolution's main loop (alex_conv_tile) live in v2v_alex_tile.hpp, shared with the backward's kernels.
#pragma once
#include "v2v_alex_tile.hpp"

namespace v2v {

// grid (tiles_x * tiles_y, n), 256 threads.  w [3][122][64]: row k = ky * 11 + kx of input channel c, row 121 zero.  For every input
// channel in turn the workgroup writes the scaled 23 x 135 patch of that channel (zero outside the image: the padding is zero AFTER the
// scaling layer) and the channel's weights into LDS, then every wave runs 61 k-steps.  Lane l of wave w holds output pixel (row w,
// column l & 31) and k = 2s + (l >> 5) of step s; k = 121 reads a slot that holds 0.
__global__ __launch_bounds__(kAlexThreads) void alex_stem_kernel(const float *__restrict__ frames, int64_t frame_stride, int cin, int H, int W, int OH, int OW,
                                                                 int tiles_x, float divisor, int normalize, const float *__restrict__ shift,
                                                                 const float *__restrict__ scale, const float *__restrict__ w, const float *__restrict__ bias,
                                                                 float *__restrict__ out)
{
    constexpr int kPatch = kAlexStemPH * kAlexStemPW;
    __shared__ float patch[kPatch + 1];
    __shared__ __attribute__((aligned(16))) float Bs[kAlexStemKP][kAlexBPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
    const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x, img = blockIdx.y;
    const int ox0 = bx * kAlexStemTX, oy0 = by * kAlexStemTY;
    const int ix0 = ox0 * kAlexStemStride - kAlexStemPad, iy0 = oy0 * kAlexStemStride - kAlexStemPad;
    const float *src = frames + (int64_t)img * frame_stride;
    const bool scaled = divisor != 1.0f;

    alex_f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
    const int base = wave * kAlexStemStride * kAlexStemPW + col * kAlexStemStride;

    for (int c = 0; c < 3; ++c) {
        __syncthreads();
        const float sh = shift[c], sc = scale[c];
        const float *plane = src + (cin == 3 ? (int64_t)c * H * W : 0);
        for (int i = tid; i < kPatch; i += kAlexThreads) {
            const int r = i / kAlexStemPW, q = i - r * kAlexStemPW, iy = iy0 + r, ix = ix0 + q;
            float v = 0.0f;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
                v = plane[(int64_t)iy * W + ix];
                if (scaled) v = v / divisor;
                if (normalize) v = 2.0f * v - 1.0f;
                v = (v - sh) / sc;
            }
            patch[i] = v;
        }
        if (tid == 0) patch[kPatch] = 0.0f;
        const float4 *wc = reinterpret_cast<const float4 *>(w + (int64_t)c * kAlexStemKP * kAlexBN);
        for (int i = tid; i < kAlexStemKP * (kAlexBN / 4); i += kAlexThreads) {
            const int k = i / (kAlexBN / 4), q = i - k * (kAlexBN / 4);
            *reinterpret_cast<float4 *>(&Bs[k][q * 4]) = wc[i];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kAlexStemKP / 2; ++s) {
            const int k0 = 2 * s, k1 = 2 * s + 1;
            const int off0 = base + (k0 / kAlexStemKS) * kAlexStemPW + (k0 % kAlexStemKS);
            const int off1 = k1 == kAlexStemK ? kPatch : base + (k1 / kAlexStemKS) * kAlexStemPW + (k1 % kAlexStemKS);
            const float a = patch[half ? off1 : off0];
            const float b0 = Bs[2 * s + half][col], b1 = Bs[2 * s + half][32 + col];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
        }
    }
    // C/D map: channel = lane & 31 (+ 32 for the second accumulator), pixel of the wave's row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const int oy = oy0 + wave;
    if (oy >= OH) return;
    const float bia0 = bias[col], bia1 = bias[32 + col];
    float *orow = out + (((int64_t)img * OH + oy) * OW) * kAlexBN;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ox = ox0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (ox < OW) {
            const float v0 = acc0[r] + bia0, v1 = acc1[r] + bia1;
            orow[(int64_t)ox * kAlexBN + col] = v0 > 0.0f ? v0 : 0.0f;
            orow[(int64_t)ox * kAlexBN + 32 + col] = v1 > 0.0f ? v1 : 0.0f;
        }
    }
}

// + bias, ReLU when a.relu
struct AlexBiasRelu {
    float bia0, bia1;
    __device__ __forceinline__ void operator()(const AlexConvArgs &a, int m, int ch, float s0, float s1) const
    {
        float v0 = s0 + bia0, v1 = s1 + bia1;
        if (a.relu) {
            v0 = v0 > 0.0f ? v0 : 0.0f;
            v1 = v1 > 0.0f ? v1 : 0.0f;
        }
        float *o = a.y + (int64_t)m * a.Cout + ch;
        o[0] = v0;
        o[32] = v1;
    }
};

template <int KS>
__global__ __launch_bounds__(kAlexThreads) void alex_conv_kernel(const AlexConvArgs a)
{
    const int ch = blockIdx.y * kAlexBN + (threadIdx.x & 31);
    alex_conv_tile<KS>(a, AlexBiasRelu{a.bias[ch], a.bias[ch + 32]});
}

// one thread per four channels of an output pixel; total = n * OH * OW * C / 4
__global__ __launch_bounds__(kAlexThreads) void alex_pool_kernel(const float *__restrict__ x, int H, int W, int OH, int OW, int C, int64_t total,
                                                                 float *__restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * kAlexThreads + threadIdx.x;
    if (i >= total) return;
    const int c4 = C / 4;
    const int q = (int)(i % c4);
    int64_t p = i / c4;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const int64_t img = p / OH;
    const float *src = x + ((img * H + 2 * oy) * W + 2 * ox) * C + q * 4;
    float4 m = *reinterpret_cast<const float4 *>(src);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float4 v = *reinterpret_cast<const float4 *>(src + ((int64_t)dy * W + dx) * C);
            m.x = v.x > m.x ? v.x : m.x;
            m.y = v.y > m.y ? v.y : m.y;
            m.z = v.z > m.z ? v.z : m.z;
            m.w = v.w > m.w ? v.w : m.w;
        }
    *reinterpret_cast<float4 *>(y + i * 4) = m;
}

// grid (tiles, n), 256 threads; a workgroup takes 64 pixels of one image, wave w pixels 16 w .. 16 w + 15 one after another, a lane the
// channels lane, lane + 64, ...  (NC = C / 64).  Per pixel, in float64: s = sum_c f_c^2 (lanes in a fixed tree), nrm = sqrt(s) + 1e-10,
// d_c = f0_c / nrm0 - f1_c / nrm1, sum_c w_c d_c^2.  A pixel whose features are all zero gives 0 / 1e-10 = 0.
template <int NC>
__global__ __launch_bounds__(kAlexThreads) void alex_compare_kernel(const float *__restrict__ f0, const float *__restrict__ f1, const float *__restrict__ w, int HW,
                                                                    int tiles, double *__restrict__ slots)
{
    constexpr int C = NC * 64;
    __shared__ double part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tile = blockIdx.x, img = blockIdx.y;
    double wc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) wc[k] = (double)w[lane + 64 * k];
    double total = 0.0;
    for (int i = 0; i < kAlexCmpPix / 4; ++i) {
        const int p = tile * kAlexCmpPix + wave * (kAlexCmpPix / 4) + i;
        if (p >= HW) break;   // uniform over the wave
        const float *a = f0 + ((int64_t)img * HW + p) * C + lane, *b = f1 + ((int64_t)img * HW + p) * C + lane;
        double x0[NC], x1[NC], s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            x0[k] = (double)a[64 * k];
            x1[k] = (double)b[64 * k];
            s0 += x0[k] * x0[k];
            s1 += x1[k] * x1[k];
        }
        s0 = __shfl(alex_wave_sum(s0), 0);
        s1 = __shfl(alex_wave_sum(s1), 0);
        const double n0 = __builtin_sqrt(s0) + 1e-10, n1 = __builtin_sqrt(s1) + 1e-10;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const double d = x0[k] / n0 - x1[k] / n1;
            acc += wc[k] * (d * d);
        }
        total += alex_wave_sum(acc);
    }
    if (lane == 0) part[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) slots[(int64_t)img * tiles + tile] = ((part[0] + part[1]) + part[2]) + part[3];
}

// grid (ceil(n / 256)), 256 threads: thread = image; adds the image's slots in slot order, taps[img][tap] = sum / HW
__global__ __launch_bounds__(kAlexThreads) void alex_reduce_kernel(const double *__restrict__ slots, int n, int tiles, double den, int tap, double *__restrict__ taps)
{
    const int img = blockIdx.x * kAlexThreads + threadIdx.x;
    if (img >= n) return;
    double s = 0.0;
    for (int k = 0; k < tiles; ++k) s += slots[(int64_t)img * tiles + k];
    taps[(int64_t)img * 5 + tap] = s / den;
}

// thread = image: val = res[0]; val += res[l], every term a float32 as the reference's are
__global__ __launch_bounds__(kAlexThreads) void alex_sum_kernel(const double *__restrict__ taps, int n, float *__restrict__ dist)
{
    const int img = blockIdx.x * kAlexThreads + threadIdx.x;
    if (img >= n) return;
    float v = (float)taps[(int64_t)img * 5];
    for (int l = 1; l < 5; ++l) v += (float)taps[(int64_t)img * 5 + l];
    dist[img] = v;
}

}  // namespace v2v
