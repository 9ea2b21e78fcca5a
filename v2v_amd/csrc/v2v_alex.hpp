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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v2v {

using alex_f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kAlexThreads = 256;
// convolution: a workgroup computes 128 pixels x 64 channels, a wave 32 pixels x 64 channels (two 32x32 accumulators); K in chunks of 32
constexpr int kAlexBM = 128, kAlexBN = 64, kAlexBK = 32;
constexpr int kAlexAPitch = kAlexBK + 4;   // floats per pixel row of the A tile: 16-byte rows, b128 reads of 16 lanes on distinct banks
constexpr int kAlexBPitch = kAlexBN + 8;   // floats per k row of the B tile: the two lane halves read rows 4 apart, 32 banks apart
// stem: a workgroup computes 4 x 32 output pixels x 64 channels, a wave one row of 32; one input channel (121 k, padded to 122) at a time
constexpr int kAlexStemKS = 11, kAlexStemStride = 4, kAlexStemPad = 2;
constexpr int kAlexStemTY = 4, kAlexStemTX = 32;
constexpr int kAlexStemPH = (kAlexStemTY - 1) * kAlexStemStride + kAlexStemKS;   // 23 input rows
constexpr int kAlexStemPW = (kAlexStemTX - 1) * kAlexStemStride + kAlexStemKS;   // 135 input columns
constexpr int kAlexStemK = kAlexStemKS * kAlexStemKS;                            // 121
constexpr int kAlexStemKP = kAlexStemK + 1;                                      // 122: the k-step of the instruction is 2
constexpr int kAlexCmpPix = 64;                                                  // pixels per workgroup of the compare kernel

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

struct AlexConvArgs {
    const float *x;     // [M][Cin], M = n * H * W
    const float *w;     // [KS * KS * Cin][Cout], k = (ky * KS + kx) * Cin + ci
    const float *bias;  // [Cout]
    float *y;           // [M][Cout]
    int M, H, W, Cin, Cout, relu;
};

// the A and B values of one chunk (tap, channels c0 .. c0 + 31) that one thread stages: four float4 of pixel rows, two of weight rows
template <int KS>
__device__ __forceinline__ void alex_conv_fetch(const AlexConvArgs &a, int tap, int c0, const int (&py)[4], const int (&px)[4], const int64_t (&pbase)[4], int bcol,
                                                int brow, float4 (&ra)[4], float4 &rb0, float4 &rb1)
{
    constexpr int P = KS / 2;
    const int dy = tap / KS - P, dx = tap % KS - P;
    const int64_t shift = ((int64_t)dy * a.W + dx) * a.Cin + c0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int yy = py[i] + dy, xx = px[i] + dx;
        ra[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) ra[i] = *reinterpret_cast<const float4 *>(a.x + pbase[i] + shift);
    }
    const float *wk = a.w + ((int64_t)tap * a.Cin + c0) * a.Cout + bcol;
    rb0 = *reinterpret_cast<const float4 *>(wk + (int64_t)brow * a.Cout);
    rb1 = *reinterpret_cast<const float4 *>(wk + (int64_t)(brow + 16) * a.Cout);
}

// grid (ceil(M / 128), Cout / 64), 256 threads.  K runs over the taps (ky, kx) and, inside a tap, over Cin in chunks of 32 -- Cin is a
// multiple of 32, so a chunk lies in one tap and is one 128-byte run of every pixel.  A thread fetches four float4 of the A tile (pixel
// rows tid / 8 + 32 i, floats 4 (tid & 7) ..) and two of the B tile one chunk ahead, into registers.  In a chunk, lane l of wave w reads
// for j = 0..3 one float4 A[32 w + (l & 31)][8 j + 4 (l >> 5) ..]; element e of it is the operand of k-step 4 j + e, whose two k are
// 8 j + e (lanes 0-31) and 8 j + 4 + e (lanes 32-63): a fixed permutation of k inside the chunk, the same for every output element.
template <int KS>
__global__ __launch_bounds__(kAlexThreads) void alex_conv_kernel(const AlexConvArgs a)
{
    __shared__ __attribute__((aligned(16))) float As[kAlexBM][kAlexAPitch];
    __shared__ __attribute__((aligned(16))) float Bs[kAlexBK][kAlexBPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
    const int m0 = blockIdx.x * kAlexBM, n0 = blockIdx.y * kAlexBN;
    const int HW = a.H * a.W;

    // the four pixel rows this thread stages
    const int arow = tid >> 3, aseg = (tid & 7) * 4;
    int py[4], px[4];
    int64_t pbase[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + arow + 32 * i;
        if (m < a.M) {
            const int rem = m % HW;
            py[i] = rem / a.W;
            px[i] = rem - py[i] * a.W;
        } else {
            py[i] = -0x10000;   // every tap falls outside: zeros
            px[i] = 0;
        }
        pbase[i] = (int64_t)m * a.Cin + aseg;
    }
    const int brow = tid >> 4, bseg = (tid & 15) * 4;
    const int chunks = a.Cin / kAlexBK, nk = KS * KS * chunks;

    float4 ra[4], rb0, rb1;
    alex_f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;

    int tap = 0, c0 = 0;
    alex_conv_fetch<KS>(a, 0, 0, py, px, pbase, n0 + bseg, brow, ra, rb0, rb1);
    for (int kc = 0; kc < nk; ++kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4 *>(&As[arow + 32 * i][aseg]) = ra[i];
        *reinterpret_cast<float4 *>(&Bs[brow][bseg]) = rb0;
        *reinterpret_cast<float4 *>(&Bs[brow + 16][bseg]) = rb1;
        __syncthreads();
        c0 += kAlexBK;
        if (c0 == a.Cin) {
            c0 = 0;
            ++tap;
        }
        alex_conv_fetch<KS>(a, tap < KS * KS ? tap : 0, c0, py, px, pbase, n0 + bseg, brow, ra, rb0, rb1);   // after the last chunk: chunk 0 again, unused
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 a4 = *reinterpret_cast<const float4 *>(&As[wave * 32 + col][8 * j + 4 * half]);
            const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float b0 = Bs[8 * j + 4 * half + e][col], b1 = Bs[8 * j + 4 * half + e][32 + col];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], b1, acc1, 0, 0, 0);
            }
        }
        __syncthreads();
    }

    const float bia0 = a.bias[n0 + col], bia1 = a.bias[n0 + 32 + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < a.M) {
            float v0 = acc0[r] + bia0, v1 = acc1[r] + bia1;
            if (a.relu) {
                v0 = v0 > 0.0f ? v0 : 0.0f;
                v1 = v1 > 0.0f ? v1 : 0.0f;
            }
            float *o = a.y + (int64_t)m * a.Cout + n0 + col;
            o[0] = v0;
            o[32] = v1;
        }
    }
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

// sum over the 64 lanes in a fixed tree; the total is valid in lane 0
__device__ __forceinline__ double alex_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
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
