// v2v_alex_tile.hpp -- what the forward (v2v_alex.hpp) and the backward (v2v_alex_train.hpp) of LPIPS-AlexNet share: the tile constants,
// the implicit-GEMM main loop of the stride-1 convolutions with its epilogue left open, and the wave sum.  No kernel is defined here, so
// both translation units include it.
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
// The epilogue decides what becomes of an accumulator: epi(a, m, n0 + col, acc of channel n0 + col, acc of channel n0 + 32 + col) per
// pixel row m < M.  alex_conv_kernel adds the bias and applies the ReLU; the input-gradient kernel of v2v_alex_train.hpp is this loop
// over the flipped, transposed weights with an epilogue of its own.
template <int KS, class Epilogue>
__device__ __forceinline__ void alex_conv_tile(const AlexConvArgs &a, const Epilogue &epi)
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

#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < a.M) epi(a, m, n0 + col, acc0[r], acc1[r]);
    }
}

// sum over the 64 lanes in a fixed tree; the total is valid in lane 0
__device__ __forceinline__ double alex_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

}  // namespace v2v
