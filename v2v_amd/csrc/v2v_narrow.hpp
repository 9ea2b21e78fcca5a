// v2v_narrow.hpp -- the 16-channel layer family (FireNet, model/model.py:264-311): activations NHWC bf16 [B,H,W,16] = 32 bytes per pixel,
// bf16 operands, fp32 accumulation on the matrix cores (v_mfma_f32_16x16x32_bf16: 16 pixels x 16 output channels x K = 32 per instruction).
// Kernels are compiled by v2v_narrow_tu.hip only (V2V_NARROW_KERNELS), which also holds the family's C entry points and their launches.
//
// One skeleton, "two dependent 3x3 convolutions through LDS" (narrow_two_conv_kernel): a workgroup of 4 waves owns a 16 x 16 pixel tile.
//   stage 0   the tile + a 2-pixel halo (20 x 20) of the inputs -> LDS, zero outside the image
//   stage 1   first convolution on the tile + a 1-pixel ring (18 x 18 = 324 pixels = 21 blocks of 16 rows), epilogue -> bf16 into LDS;
//             ring positions OUTSIDE THE IMAGE are written as zero: they are the zero padding of the second convolution
//   stage 2   second convolution on the tile out of LDS (16 blocks = the tile's rows), epilogue, store
// The intermediate never reaches HBM.  Any B, H, W >= 1: partial tiles are guarded on both axes.  Two instances:
//   MODE 0  ConvGRU step (model/submodules.py:260-278), one launch.  Staged pixel = x | h_prev (64 B), so one tap of cat(x, h) is one
//           K = 32 step.  Stage 1: 9 taps x (update, reset) columns; u = sigmoid(.) kept in fp32 in LDS for the tile pixels,
//           hr = rne_bf16(h_f32 * r) on tile + ring.  Stage 2: K over x | hr, h' = h_f32 (1 - u) + tanh(acc + b) u in fp32, stored as fp32 and
//           as its bf16 RNE copy (+ optional NCHW copy): the precision contract of the 64+-channel step (v2v_convgru.hpp).  Zero state
//           (h_prev == null): the h half of K is staged as zeros.
//   MODE 1  residual block (model/submodules.py:143-177, norm=None).  Staged pixel = x (32 B); K = 32 holds two taps, 9 taps padded to 10
//           with a zero block.  Stage 1: mid = relu(conv1(x) + b1).  Stage 2: out = relu(conv2(mid) + b2 + x), one rounding to bf16.
// and a single-stage head (narrow_head_kernel): x8 [B,H,W,8] (v2v_to_nhwc8_bf16) -> [relu](conv3x3 + bias) [B,H,W,16]; K = 32 holds four taps.
//
// Fragment maps of v_mfma_f32_16x16x32_bf16, lane l, fr = l & 15, fg = l >> 4: A[row fr][k = 8 fg + j], B[k = 8 fg + j][col fr], j = 0..7
// (one 16-byte read each); C/D[row 4 fg + e][col fr], e = 0..3.  Rows are pixels, columns output channels.
// Packed weights: fragment f, lane l, element j at wp[(f * 64 + l) * 8 + j] -- every lane's B fragment is one 16-byte load, held in registers:
//   GRU   f = 2 tap + gate (0 update, 1 reset) for f < 18, f = 18 + tap the candidate; k <-> channel 8 fg + j of cat(x, h)          27 fragments
//   res   f = 5 conv + t; k-group fg <-> tap 2 t + (fg >> 1), channel 8 (fg & 1) + j (tap 9: zeros)                                  10 fragments
//   head  f = m; k-group fg <-> tap 4 m + fg, channel j (< Cin, else zero; taps 9..11: zeros)                                          3 fragments
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v2v {

struct NarrowArgs {
    const uint16_t *x;                     // bf16 [B,H,W,16] (head: [B,H,W,8])
    const uint16_t *h_prev;                // GRU: bf16 [B,H,W,16] or null (zero state)
    const float *h_prev_f32;               // GRU: its fp32 master or null
    const uint16_t *wp;                    // packed weights (layout above)
    const float *bias1, *bias2;            // GRU: [32] update | reset, [16] out_gate; residual block: conv1's, conv2's; head: bias1
    uint16_t *out;                         // bf16 [B,H,W,16] (GRU: the new state)
    float *out_f32;                        // GRU: the new state's fp32 master
    void *h_nchw;                          // GRU: optional [B,16,H,W] copy of the new state
    int32_t h_nchw_bf16;                   // its dtype: 0 fp32, 1 bf16
    int32_t relu;                          // head
    int32_t B, H, W, tiles_x, tiles_y;
};

constexpr int kGru16Frags = 27, kRes16Frags = 10, kHead16Frags = 3, kNarrowFragElems = 512;

}  // namespace v2v

#ifdef V2V_NARROW_KERNELS
#define V2V_CL_STEP_ONLY
#include "v2v_convlstm.hpp"                // cl_bf16x8, cl_pack_bf16 / f32_to_bf16_rne, cl_sigmoid / cl_tanh: the step kernels' own

namespace v2v {

typedef float nr_f32x4 __attribute__((ext_vector_type(4)));
constexpr int kNrIn = 20, kNrRing = 18, kNrRingPix = kNrRing * kNrRing, kNrRingBlocks = (kNrRingPix + 15) / 16;

__device__ __forceinline__ cl_bf16x8 nr_ld16(const unsigned char *p) { return *reinterpret_cast<const cl_bf16x8 *>(p); }
__device__ __forceinline__ cl_bf16x8 nr_zero8() { return __builtin_bit_cast(cl_bf16x8, make_uint4(0u, 0u, 0u, 0u)); }
__device__ __forceinline__ float nr_bf16_f32(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ float nr_relu(float v) { return v > 0.0f ? v : (v != v ? v : 0.0f); }     // NaN stays NaN, as torch.relu

template <int MODE>
__global__ void __launch_bounds__(256) narrow_two_conv_kernel(const NarrowArgs a)
{
    constexpr int PB = MODE == 0 ? 64 : 32;                            // bytes per staged input pixel
    constexpr int CPP = PB / 16;                                       // 16-byte chunks per staged pixel
    constexpr int kInBytes = kNrIn * kNrIn * PB, kMidBytes = kNrRingPix * 32, kUBytes = MODE == 0 ? 256 * 16 * 4 : 0;
    __shared__ __attribute__((aligned(16))) unsigned char lds[kInBytes + kMidBytes + kUBytes];
    unsigned char *const in_l = lds, *const mid_l = lds + kInBytes;
    float *const u_l = reinterpret_cast<float *>(lds + kInBytes + kMidBytes);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int H = a.H, W = a.W;
    const int tx = blockIdx.x % a.tiles_x, ty = (blockIdx.x / a.tiles_x) % a.tiles_y, b = blockIdx.x / (a.tiles_x * a.tiles_y);
    const int y0 = ty * 16, x0 = tx * 16;

    // stage 0: tile + 2-pixel halo, zero outside the image (and for the h half of a zero state)
    for (int i = threadIdx.x; i < kNrIn * kNrIn * CPP; i += 256) {
        const int p = i / CPP, part = i - p * CPP;
        const int hy = p / kNrIn, hx = p - hy * kNrIn;
        const int iy = y0 + hy - 2, ix = x0 + hx - 2;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
            const int64_t e = ((((int64_t)b * H + iy) * W) + ix) * 16 + (part & 1) * 8;
            if (part < 2) v = *reinterpret_cast<const uint4 *>(a.x + e);
            else if (a.h_prev) v = *reinterpret_cast<const uint4 *>(a.h_prev + e);
        }
        *reinterpret_cast<uint4 *>(in_l + p * PB + part * 16) = v;
    }
    constexpr int NW1 = MODE == 0 ? 18 : 5, NW2 = MODE == 0 ? 9 : 5;
    const uint16_t *const wl = a.wp + lane * 8;
    {
        cl_bf16x8 w1[NW1];
#pragma unroll
        for (int f = 0; f < NW1; ++f) w1[f] = *reinterpret_cast<const cl_bf16x8 *>(wl + f * kNarrowFragElems);
        __syncthreads();

        // stage 1: first convolution on tile + ring; block = 16 consecutive pixels of the ring region in row-major order
        for (int blk = wave; blk < kNrRingBlocks; blk += 4) {
            const int q = min(blk * 16 + fr, kNrRingPix - 1);          // this lane's A row (rows past the region repeat the last pixel, not stored)
            const int ry = q / kNrRing, rx = q - ry * kNrRing;
            nr_f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (MODE == 0) {
                const unsigned char *const ap = in_l + (ry * kNrIn + rx) * 64 + fg * 16;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const cl_bf16x8 af = nr_ld16(ap + ((tap / 3) * kNrIn + tap % 3) * 64);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, w1[2 * tap], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, w1[2 * tap + 1], acc1, 0, 0, 0);
                }
            } else {
                const unsigned char *const ap = in_l + (ry * kNrIn + rx) * 32 + (fg & 1) * 16;
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    const int tap = 2 * t + (fg >> 1);
                    const bool live = tap < 9;
                    const int tp = live ? tap : 8;
                    cl_bf16x8 af = nr_ld16(ap + ((tp / 3) * kNrIn + tp % 3) * 32);
                    if (!live) af = nr_zero8();
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, w1[t], acc0, 0, 0, 0);
                }
            }
            // accumulator element e of this lane: pixel blk * 16 + 4 fg + e, channel fr
            const float b0 = a.bias1[fr], b1 = MODE == 0 ? a.bias1[16 + fr] : 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int qe = blk * 16 + fg * 4 + e;
                if (qe >= kNrRingPix) continue;
                const int ey = qe / kNrRing, ex = qe - ey * kNrRing;
                const int iy = y0 - 1 + ey, ix = x0 - 1 + ex;
                const bool inside = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                uint16_t m = 0;                                        // outside the image: the second convolution's zero padding
                if constexpr (MODE == 0) {
                    if (inside) {
                        const int64_t idx = ((((int64_t)b * H + iy) * W) + ix) * 16 + fr;
                        const float hp = a.h_prev_f32 ? a.h_prev_f32[idx] : 0.0f;
                        m = f32_to_bf16_rne(hp * cl_sigmoid(acc1[e] + b1));
                    }
                    if (ey >= 1 && ey <= 16 && ex >= 1 && ex <= 16) u_l[((ey - 1) * 16 + (ex - 1)) * 16 + fr] = cl_sigmoid(acc0[e] + b0);
                } else {
                    if (inside) m = f32_to_bf16_rne(nr_relu(acc0[e] + b0));
                }
                reinterpret_cast<uint16_t *>(mid_l)[qe * 16 + fr] = m;
            }
        }
    }
    cl_bf16x8 w2[NW2];
#pragma unroll
    for (int f = 0; f < NW2; ++f) w2[f] = *reinterpret_cast<const cl_bf16x8 *>(wl + (NW1 + f) * kNarrowFragElems);
    __syncthreads();

    // stage 2: second convolution on the tile; block = one tile row (16 pixels)
    const float bo = a.bias2[fr];
    for (int row = wave; row < 16; row += 4) {
        nr_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (MODE == 0) {
            // k-groups 0, 1: x at the tile pixel's place in the staged input; 2, 3: hr in the ring buffer
            const unsigned char *const ap = fg < 2 ? in_l + ((row + 1) * kNrIn + fr + 1) * 64 + fg * 16 : mid_l + (row * kNrRing + fr) * 32 + (fg & 1) * 16;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int off = fg < 2 ? ((tap / 3) * kNrIn + tap % 3) * 64 : ((tap / 3) * kNrRing + tap % 3) * 32;
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nr_ld16(ap + off), w2[tap], acc, 0, 0, 0);
            }
        } else {
            const unsigned char *const ap = mid_l + (row * kNrRing + fr) * 32 + (fg & 1) * 16;
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const int tap = 2 * t + (fg >> 1);
                const bool live = tap < 9;
                const int tp = live ? tap : 8;
                cl_bf16x8 af = nr_ld16(ap + ((tp / 3) * kNrRing + tp % 3) * 32);
                if (!live) af = nr_zero8();
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, w2[t], acc, 0, 0, 0);
            }
        }
        const int iy = y0 + row;
        if (iy >= H) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int px = fg * 4 + e, ix = x0 + px;
            if (ix >= W) continue;
            const int64_t idx = ((((int64_t)b * H + iy) * W) + ix) * 16 + fr;
            if constexpr (MODE == 0) {
                const float go = cl_tanh(acc[e] + bo), gu = u_l[(row * 16 + px) * 16 + fr];
                const float hp = a.h_prev_f32 ? a.h_prev_f32[idx] : 0.0f;
                const float hn = hp * (1.0f - gu) + go * gu;
                a.out_f32[idx] = hn;
                a.out[idx] = f32_to_bf16_rne(hn);
                if (a.h_nchw) {
                    const int64_t o = ((((int64_t)b * 16 + fr) * H) + iy) * W + ix;
                    if (a.h_nchw_bf16) static_cast<uint16_t *>(a.h_nchw)[o] = f32_to_bf16_rne(hn);
                    else static_cast<float *>(a.h_nchw)[o] = hn;
                }
            } else {
                const float xr = nr_bf16_f32(reinterpret_cast<const uint16_t *>(in_l)[((row + 2) * kNrIn + px + 2) * 16 + fr]);
                a.out[idx] = f32_to_bf16_rne(nr_relu(acc[e] + bo + xr));
            }
        }
    }
}

// head: x8 [B,H,W,8] -> [relu](conv3x3 + bias) [B,H,W,16]; tile + 1-pixel halo (18 x 18 x 16 B) staged once, K = 32 = four taps x 8 channels
__global__ void __launch_bounds__(256) narrow_head_kernel(const NarrowArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char patch[kNrRingPix * 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int H = a.H, W = a.W;
    const int tx = blockIdx.x % a.tiles_x, ty = (blockIdx.x / a.tiles_x) % a.tiles_y, b = blockIdx.x / (a.tiles_x * a.tiles_y);
    const int y0 = ty * 16, x0 = tx * 16;
    for (int p = threadIdx.x; p < kNrRingPix; p += 256) {
        const int hy = p / kNrRing, hx = p - hy * kNrRing;
        const int iy = y0 + hy - 1, ix = x0 + hx - 1;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v = *reinterpret_cast<const uint4 *>(a.x + ((((int64_t)b * H + iy) * W) + ix) * 8);
        *reinterpret_cast<uint4 *>(patch + p * 16) = v;
    }
    cl_bf16x8 w[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) w[f] = *reinterpret_cast<const cl_bf16x8 *>(a.wp + lane * 8 + f * kNarrowFragElems);
    __syncthreads();
    const float bv = a.bias1[fr];
    for (int row = wave; row < 16; row += 4) {
        nr_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        const unsigned char *const ap = patch + (row * kNrRing + fr) * 16;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const int tap = 4 * m + fg;
            const bool live = tap < 9;
            const int tp = live ? tap : 8;
            cl_bf16x8 af = nr_ld16(ap + ((tp / 3) * kNrRing + tp % 3) * 16);
            if (!live) af = nr_zero8();
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, w[m], acc, 0, 0, 0);
        }
        const int iy = y0 + row;
        if (iy >= H) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ix = x0 + fg * 4 + e;
            if (ix >= W) continue;
            float v = acc[e] + bv;
            if (a.relu) v = nr_relu(v);
            a.out[((((int64_t)b * H + iy) * W) + ix) * 16 + fr] = f32_to_bf16_rne(v);
        }
    }
}

// one thread per packed element (layouts at the top); weights fp32 in the modules' layouts: [16, 32, 3, 3] x 3, [16, 16, 3, 3] x 2, [16, Cin, 3, 3]
__global__ void __launch_bounds__(256) narrow_pack_kernel(int kind, const float *w0, const float *w1, const float *w2, int Cin, uint16_t *wp)
{
    const int n_frag = kind == 0 ? kGru16Frags : kind == 1 ? kRes16Frags : kHead16Frags;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_frag * kNarrowFragElems) return;
    const int f = i >> 9, l = (i >> 3) & 63, j = i & 7, n = l & 15, g = l >> 4;
    float v = 0.0f;
    if (kind == 0) {
        const int tap = f < 18 ? f >> 1 : f - 18;
        const float *w = f >= 18 ? w2 : (f & 1) ? w1 : w0;            // update, reset, out_gate
        v = w[(n * 32 + 8 * g + j) * 9 + tap];
    } else if (kind == 1) {
        const int tap = 2 * (f % 5) + (g >> 1);
        const float *w = f >= 5 ? w1 : w0;
        if (tap < 9) v = w[(n * 16 + 8 * (g & 1) + j) * 9 + tap];
    } else {
        const int tap = 4 * f + g;
        if (tap < 9 && j < Cin) v = w0[(n * Cin + j) * 9 + tap];
    }
    wp[i] = f32_to_bf16_rne(v);
}

}  // namespace v2v
#endif  // V2V_NARROW_KERNELS
