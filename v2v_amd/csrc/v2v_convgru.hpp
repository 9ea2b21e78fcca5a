// v2v_convgru.hpp -- the ConvGRU step on the matrix cores: the two epilogues (EPI = 3 / 4) of convlstm_step_kernel (v2v_convlstm.hpp) and
// the weight packing.  Included by v2v_convgru_tu.hip only, so the instances of every other translation unit are untouched.
//
// Replaces one ConvGRU.forward of the reference's recurrent encoders (model/submodules.py:260-278):
//     u = sigmoid(update_gate(cat(x, h)));  r = sigmoid(reset_gate(cat(x, h)))
//     o = tanh(out_gate(cat(x, h * r)));    h' = h * (1 - u) + o * u
// Unlike the LSTM step these are TWO dependent convolutions -- the candidate reads h * r through a 3x3 window, so a tile of it needs its
// neighbours' reset gates -- hence two launches on the same main loop (NHWC bf16 through LDS-DMA, v_mfma_f32_32x32x16_bf16, fp32 accumulation):
//   gates     (EPI = 3): K over x | h (bf16),  2C columns -> u fp32 [B,H,W,C],  hr = rne_bf16(h_f32 * r) bf16 [B,H,W,C]
//   candidate (EPI = 4): K over x | hr,         C columns -> h'_f32 = h_f32 (1 - u) + tanh(acc + b) u  (fp32) and its bf16 RNE copy
// Neither gate pre-activation nor the candidate reaches HBM.  The hidden state is carried in fp32 beside the bf16 copy the convolutions
// read (as the LSTM's cell state is): with a bf16-only state an update below half a bf16 ulp of h would be lost at every step.
// Zero state (h_prev == null): K runs over x only in both launches, hr = 0, h' = o * u.
//
// ConvLstmArgs as the two launches read it (no field of their own, so the struct -- and every shipped instance's kernarg layout -- stays):
//                 x        h_prev      c_prev          bias                  c_state      h_state     dh     h_nchw
//   gates         x        h bf16      h fp32 | null   [2C] update | reset   u (out)      hr (out)    -      -
//   candidate     x        hr | null   h fp32 | null   [C] out_gate          h' fp32      h' bf16     u      optional NCHW copy of h'
// pack_cols = columns per packed weight tile (below).
//
// Packed weights, both streams: wp[col tile t][chunk ck = tap * (2C/64) + cc][column n = 0..P-1][k = 0..63] bf16, k <-> input channel cc*64 + k
//   gates      P = 256 when C % 128 == 0, else 128:  n = q * 64 + gate * 32 + c32  <->  gate (0 update, 1 reset), hidden channel t * P/2 + q * 32 + c32
//   candidate  P = 256 / 128 / 64 (the largest that divides C):  n  <->  hidden channel t * P + n
// An instance whose tile is narrower than P takes the sub-tile `ct % (P / tile)` of a packed tile, as the EPI = 1 instances do.
#pragma once
#define V2V_CL_STEP_ONLY
#include "v2v_convlstm.hpp"

namespace v2v {

__host__ __device__ constexpr int gru_gate_pack_cols(int C) { return C % 128 == 0 ? 256 : 128; }
__host__ __device__ constexpr int gru_cand_pack_cols(int C) { return C % 256 == 0 ? 256 : C % 128 == 0 ? 128 : 64; }

// accumulator element r of lane l: column l & 31, row (pixel) (r & 3) + 8 (r >> 2) + 4 (l >> 5); fragments 2 s / 2 s + 1 of a wave are the
// update / reset pre-activations of hidden channels ch0 + 32 s ..
template <int MF, int NF>
__device__ __forceinline__ void gru_epilogue_gates(const ConvLstmArgs &a, cl_f32x16 (&acc)[MF][NF], int64_t mw0, int ch0, int fh, int64_t M)
{
    const int C = a.C;
#pragma unroll
    for (int s = 0; s < NF / 2; ++s) {
        const int ch = ch0 + 32 * s;
        const float b_u = a.bias[ch], b_r = a.bias[C + ch];
#pragma unroll
        for (int i = 0; i < MF; ++i) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t mq = mw0 + i * 32 + q * 8 + fh * 4;                    // first of 4 consecutive pixels
                if (mq >= M) continue;                                               // past the last pixel (partial last tile)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = q * 4 + e;
                    const int64_t idx = (mq + e) * C + ch;
                    const float gu = cl_sigmoid(acc[i][2 * s][r] + b_u), gr = cl_sigmoid(acc[i][2 * s + 1][r] + b_r);
                    const float hp = a.c_prev ? a.c_prev[idx] : 0.0f;
                    a.c_state[idx] = gu;
                    a.h_state[idx] = f32_to_bf16_rne(hp * gr);
                }
            }
        }
    }
}

template <int MF, int NF>
__device__ __forceinline__ void gru_epilogue_candidate(const ConvLstmArgs &a, cl_f32x16 (&acc)[MF][NF], int64_t mw0, int col0, int fh, int64_t M)
{
    const int C = a.C, HW = a.H * a.W;
#pragma unroll
    for (int g = 0; g < NF; ++g) {
        const int ch = col0 + 32 * g;
        const float b_o = a.bias[ch];
#pragma unroll
        for (int i = 0; i < MF; ++i) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float hv[4];
                const int64_t mq = mw0 + i * 32 + q * 8 + fh * 4;
                if (mq >= M) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = q * 4 + e;
                    const int64_t idx = (mq + e) * C + ch;
                    const float go = cl_tanh(acc[i][g][r] + b_o), gu = a.dh[idx];
                    const float hp = a.c_prev ? a.c_prev[idx] : 0.0f;
                    const float hn = hp * (1.0f - gu) + go * gu;
                    a.c_state[idx] = hn;
                    a.h_state[idx] = f32_to_bf16_rne(hn);
                    hv[e] = hn;
                }
                if (a.h_nchw) {
                    const int64_t b = mq / HW, p = mq - b * HW;                      // HW % 4 == 0: the 4 pixels share an image
                    const int64_t o = (b * C + ch) * HW + p;
                    if (a.h_nchw_bf16) {
                        const uint32_t lo = cl_pack_bf16(hv[0], hv[1]), hi = cl_pack_bf16(hv[2], hv[3]);
                        *reinterpret_cast<uint2 *>(static_cast<uint16_t *>(a.h_nchw) + o) = make_uint2(lo, hi);
                    } else {
                        *reinterpret_cast<float4 *>(static_cast<float *>(a.h_nchw) + o) = make_float4(hv[0], hv[1], hv[2], hv[3]);
                    }
                }
            }
        }
    }
}

// update_gate.weight, reset_gate.weight, out_gate.weight (fp32 [C, 2C, 3, 3] each) -> the two packed bf16 streams (layout above); one
// thread per element of the gates stream (2C * 2C * 9) and of the candidate stream (C * 2C * 9) behind it
__global__ void __launch_bounds__(256) convgru_pack_kernel(const float *w_u, const float *w_r, const float *w_o, uint16_t *wp_gates, uint16_t *wp_cand, int C)
{
    const int64_t n_g = (int64_t)2 * C * 2 * C * 9, n_c = (int64_t)C * 2 * C * 9;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_g + n_c) return;
    const bool gates = i < n_g;
    const int P = gates ? gru_gate_pack_cols(C) : gru_cand_pack_cols(C);
    const int cc_all = 2 * C / kClBK;
    int64_t r = gates ? i : i - n_g;
    const int k = (int)(r % kClBK); r /= kClBK;
    const int col = (int)(r % P); r /= P;
    const int ck = (int)(r % (9 * cc_all)); r /= 9 * cc_all;
    const int t = (int)r;
    const int tap = ck / cc_all, ic = (ck % cc_all) * kClBK + k;
    if (gates) {
        const int oc = t * (P / 2) + (col >> 6) * 32 + (col & 31);
        const float *w = ((col >> 5) & 1) ? w_r : w_u;
        wp_gates[i] = f32_to_bf16_rne(w[((int64_t)oc * 2 * C + ic) * 9 + tap]);
    } else {
        const int oc = t * P + col;
        wp_cand[i - n_g] = f32_to_bf16_rne(w_o[((int64_t)oc * 2 * C + ic) * 9 + tap]);
    }
}

}  // namespace v2v
