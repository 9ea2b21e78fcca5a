// v2v_nam_head.hpp -- the head of NER-Net's recurrent network: 9 to 16 input channels (2 * num_bins = 10 in the shipped configuration) ->
// 32 channels, 5x5, stride 1, pad 2, bias, ReLU, at full resolution (ConvLayer(10, 32, 5, padding=2) of UNetNIAM_STcell_GCB,
// model/nernet/unet.py of the reference).  The head of v2v_convlstm.hpp takes 8 channels at most and H, W multiples of 16; it stays as it is.
//
//   to_nhwc16_bf16_kernel     float32 [B,C,H,W] of any strides, C <= 16 -> bf16 [B,H,W,16], channels C.. zero: 32 bytes per pixel
//   conv_head16in_kernel      a wave owns 32 consecutive pixels (of the flattened B*H*W, any H and W) x the 32 output channels: ONE
//                             v_mfma_f32_32x32x16_bf16 per tap, K = the 16 channels.  Lane l (r = l & 31, h = l >> 5) loads its A fragment --
//                             channels 8h .. 8h+7 of pixel r at the tap's offset, 16 bytes, zero outside the image -- and its B fragment --
//                             channels 8h .. of output channel r -- straight from global memory: no reuse inside a wave to stage for, the 25.6 KB
//                             of weights stay in L1 / L2.  fp32 accumulation, + bias, ReLU, one rounding to bf16 -> [B,H,W,32].
// Packed weights: wp[tap = 5 ky + kx][output channel 0..31][input channel 0..15] bf16, zero for input channels past Cin.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v2v {

constexpr int kHead16Taps = 25, kHead16Packed = kHead16Taps * 32 * 16;

typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 h16_bf16x8;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float h16_f32x16;

__device__ __forceinline__ uint16_t h16_rne(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }

__global__ void __launch_bounds__(256) to_nhwc16_bf16_kernel(const float *src, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int B, int C, int H, int W, uint16_t *dst)
{
    const int64_t n = (int64_t)B * H * W, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const int64_t b = i / ((int64_t)H * W);
    const float *p = src + b * sb + y * sh + x * sw;
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t lo = 2 * k < C ? h16_rne(p[(2 * k) * sc]) : 0u, hi = 2 * k + 1 < C ? h16_rne(p[(2 * k + 1) * sc]) : 0u;
        w[k] = lo | (hi << 16);
    }
    uint4 *o = reinterpret_cast<uint4 *>(dst + i * 16);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// nn.Conv2d(Cin <= 16, 32, 5).weight fp32 [32, Cin, 5, 5] -> wp (layout above); one thread per packed element
__global__ void __launch_bounds__(256) conv_head16in_pack_kernel(const float *w, int Cin, uint16_t *wp)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kHead16Packed) return;
    const int ci = i & 15, co = (i >> 4) & 31, tap = i >> 9;
    wp[i] = ci < Cin ? h16_rne(w[(co * Cin + ci) * kHead16Taps + tap]) : (uint16_t)0;
}

__global__ void __launch_bounds__(256) conv_head16in_kernel(const uint16_t *x16, const uint16_t *wp, const float *bias, uint16_t *out, int B, int H, int W, int relu)
{
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t M = (int64_t)B * H * W, m0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;     // the wave's first pixel
    if (m0 >= M) return;                                                                                // wave-uniform
    const int64_t m = m0 + r;
    const bool live = m < M;
    const int x = (int)(m % W), y = (int)((m / W) % H);
    const uint16_t *centre = x16 + m * 16 + h * 8;
    h16_f32x16 acc;
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0f;
#pragma unroll 5
    for (int tap = 0; tap < kHead16Taps; ++tap) {
        const int dy = tap / 5 - 2, dx = tap % 5 - 2;
        const bool in = live && (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W;
        uint4 av = make_uint4(0, 0, 0, 0);
        if (in) av = *reinterpret_cast<const uint4 *>(centre + ((int64_t)dy * W + dx) * 16);
        const uint4 bv = *reinterpret_cast<const uint4 *>(wp + (tap * 32 + r) * 16 + h * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(h16_bf16x8, av), __builtin_bit_cast(h16_bf16x8, bv), acc, 0, 0, 0);
    }
    // accumulator element k of lane l: output channel l & 31, pixel (k & 3) + 8 (k >> 2) + 4 (l >> 5) of the wave's 32
    const float bs = bias[r];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int64_t pm = m0 + (k & 3) + 8 * (k >> 2) + 4 * h;
        if (pm >= M) continue;
        float v = acc[k] + bs;
        if (relu) v = v > 0.0f ? v : (v != v ? v : 0.0f);                                               // torch.relu keeps NaN
        out[pm * 32 + r] = h16_rne(v);
    }
}

}  // namespace v2v
