// v2v_nam.hpp -- NER-Net's NAM cell on the matrix cores: the three epilogues (EPI = 5 / 6 / 7) of convlstm_step_kernel (v2v_convlstm.hpp)
// and the weight packing.  Included by v2v_nam_tu.hip only, so the instances of every other translation unit are untouched.
//
// Replaces one NAM_withoutGCB.forward of the reference (model/nernet/submodules.py:585-642; no biases, x_t, h_t, m_t all C channels):
//     conv_x (C -> 7C) splits into i, f, g, i', f', g', o;   conv_h (C -> 4C) into i, f, g, o;   conv_m (C -> 3C) into i', f', g'
//     i_t = s(i_x + i_h);  alpha = exp(s(LAG_conv(x_t)));  f_t = s(s(f_x + f_h + 1) - alpha i_t);  c' = f_t c + i_t tanh(g_x + g_h)
//     m' = s(f'_x + f_m + 1) m_t + s(i'_x + i_m) tanh(g'_x + g_m)
//     h' = s(o_x + o_h + conv_o(cat(c', m'))) tanh(conv_last(cat(c', m')))                     s = sigmoid
// conv_o reads c' and m' through a 3x3 window, so the cell is dependent convolutions: three launches on the step's main loop (NHWC bf16
// through LDS-DMA, v_mfma_f32_32x32x16_bf16, fp32 accumulation), each on a tile geometry that already ships:
//   M (EPI = 5): K over x | m_t,   4C columns (i', f', g', lag)   -> m' bf16 (+ optional fp32), alpha fp32            the ConvLSTM step's geometry
//   C (EPI = 6): K over x | h,     4C columns (i, f, g, o)        -> c' fp32 + its bf16 RNE copy, o_pre = o_x + o_h fp32  the same
//   H (EPI = 7): K over c' | m',   2C columns (conv_o, conv_last) -> h' fp32 + its bf16 RNE copy, optional NCHW copy    the ConvGRU gates' geometry
// The two 1x1 convolutions (LAG_conv over x, conv_last over c' | m') ride along as 3x3 columns whose weights are zero off the centre tap:
// 8/9 of those columns' flops are wasted, two launches and two round trips through HBM are saved.  No gate pre-activation reaches HBM.
// The cell state is carried in fp32 (as the ConvLSTM's is); h' is written in fp32 beside the bf16 copy the next step's convolutions read.
// Zero state (h_prev == null, c_prev == null): launch C walks K over x only.
//
// ConvLstmArgs as the three launches read it (no field of their own, so the struct -- and every shipped instance's kernarg layout -- stays):
//         x         h_prev         c_prev          dh       h_state      c_state     dc_prev             h_nchw
//   M     x         m_t bf16       -               -        m' bf16      alpha       m' fp32 | null      -
//   C     x         h bf16 | null  c fp32 | null   alpha    c' bf16      c' fp32     o_pre               -
//   H     c' bf16   m' bf16        -               o_pre    h' bf16      h' fp32     -                   optional NCHW copy of h'
//
// Packed weights, three streams behind each other in ONE buffer: wp[col tile t][chunk ck = tap * (2C/64) + cc][column n = 0..P-1][k = 0..63]
// bf16, k <-> input channel cc * 64 + k of the launch's two K halves, tap = 3 dy + dx
//   M, C   P = 256, t over C/64:  n = wn * 128 + gate * 32 + c32  <->  gate, hidden channel t * 64 + wn * 32 + c32   (the ConvLSTM step's layout)
//          M gates 0..3 = i', f', g' (conv_x chunks 3, 4, 5 | conv_m chunks 0, 1, 2) and lag (LAG_conv at the centre tap | 0)
//          C gates 0..3 = i, f, g, o (conv_x chunks 0, 1, 2, 6 | conv_h chunks 0, 1, 2, 3)
//   H      P = 256 when C % 128 == 0, else 128:  n = q * 64 + gate * 32 + c32  <->  gate, hidden channel t * P/2 + q * 32 + c32  (the ConvGRU gates' layout)
//          gates 0, 1 = conv_o, conv_last (centre tap only); both over cat(c', m')
// Sizes: M and C 4C * 2C * 9 elements each, H 2C * 2C * 9.
#pragma once
#define V2V_CL_STEP_ONLY
#include "v2v_convlstm.hpp"

namespace v2v {

__host__ __device__ constexpr int nam_h_pack_cols(int C) { return C % 128 == 0 ? 256 : 128; }
__host__ __device__ constexpr int64_t nam_mc_elems(int C) { return (int64_t)4 * C * 2 * C * 9; }
__host__ __device__ constexpr int64_t nam_h_elems(int C) { return (int64_t)2 * C * 2 * C * 9; }

// accumulator element r of lane l: column l & 31, row (pixel) (r & 3) + 8 (r >> 2) + 4 (l >> 5); fragment g of a wave = gate g of hidden channel ch
template <int MF, int NF>
__device__ __forceinline__ void nam_epilogue_m(const ConvLstmArgs &a, cl_f32x16 (&acc)[MF][NF], int64_t mw0, int ch, int fh, int64_t M)
{
    static_assert(NF == 4, "four columns per hidden channel");
    const int C = a.C;
#pragma unroll
    for (int i = 0; i < MF; ++i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t mq = mw0 + i * 32 + q * 8 + fh * 4;                        // first of 4 consecutive pixels
            if (mq >= M) continue;                                                   // past the last pixel (partial last tile)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = q * 4 + e;
                const int64_t idx = (mq + e) * C + ch;
                const float mt = __uint_as_float((uint32_t)a.h_prev[idx] << 16);
                const float mn = cl_sigmoid(acc[i][1][r] + 1.0f) * mt + cl_sigmoid(acc[i][0][r]) * cl_tanh(acc[i][2][r]);
                a.h_state[idx] = f32_to_bf16_rne(mn);
                if (a.dc_prev) a.dc_prev[idx] = mn;
                a.c_state[idx] = __builtin_amdgcn_exp2f(cl_sigmoid(acc[i][3][r]) * 1.4426950408889634f);
            }
        }
    }
}

template <int MF, int NF>
__device__ __forceinline__ void nam_epilogue_c(const ConvLstmArgs &a, cl_f32x16 (&acc)[MF][NF], int64_t mw0, int ch, int fh, int64_t M)
{
    static_assert(NF == 4, "four columns per hidden channel");
    const int C = a.C;
#pragma unroll
    for (int i = 0; i < MF; ++i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t mq = mw0 + i * 32 + q * 8 + fh * 4;
            if (mq >= M) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = q * 4 + e;
                const int64_t idx = (mq + e) * C + ch;
                const float gi = cl_sigmoid(acc[i][0][r]);
                const float gf = cl_sigmoid(cl_sigmoid(acc[i][1][r] + 1.0f) - a.dh[idx] * gi);
                const float cp = a.c_prev ? a.c_prev[idx] : 0.0f;
                const float cn = gf * cp + gi * cl_tanh(acc[i][2][r]);
                a.c_state[idx] = cn;
                a.h_state[idx] = f32_to_bf16_rne(cn);
                a.dc_prev[idx] = acc[i][3][r];
            }
        }
    }
}

// fragments 2 s / 2 s + 1 of a wave are conv_o / conv_last of hidden channels ch0 + 32 s ..
template <int MF, int NF>
__device__ __forceinline__ void nam_epilogue_h(const ConvLstmArgs &a, cl_f32x16 (&acc)[MF][NF], int64_t mw0, int ch0, int fh, int64_t M)
{
    const int C = a.C, HW = a.H * a.W;
#pragma unroll
    for (int s = 0; s < NF / 2; ++s) {
        const int ch = ch0 + 32 * s;
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
                    const float hn = cl_sigmoid(a.dh[idx] + acc[i][2 * s][r]) * cl_tanh(acc[i][2 * s + 1][r]);
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

// the six reference tensors -> the three packed streams (layout above), one thread per packed element: conv_x fp32 [7C, C, 3, 3],
// conv_h [4C, C, 3, 3], conv_m [3C, C, 3, 3], conv_o [C, 2C, 3, 3], conv_last [C, 2C], LAG_conv [C, C]
__global__ void __launch_bounds__(256) nam_pack_kernel(const float *w_x, const float *w_h, const float *w_m, const float *w_o, const float *w_last,
                                                       const float *w_lag, uint16_t *wp, int C)
{
    const int64_t n_mc = nam_mc_elems(C), n_h = nam_h_elems(C);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * n_mc + n_h) return;
    const int launch = i < n_mc ? 0 : i < 2 * n_mc ? 1 : 2;                      // M, C, H
    const int P = launch == 2 ? nam_h_pack_cols(C) : 256;
    const int cc_all = 2 * C / kClBK;
    int64_t r = i - launch * n_mc;
    const int k = (int)(r % kClBK); r /= kClBK;
    const int col = (int)(r % P); r /= P;
    const int ck = (int)(r % (9 * cc_all)); r /= 9 * cc_all;
    const int t = (int)r;
    const int tap = ck / cc_all, ic = (ck % cc_all) * kClBK + k;
    const bool second = ic >= C;                                                 // the launch's second K half
    const int icc = second ? ic - C : ic;
    float v = 0.0f;
    if (launch < 2) {
        const int oc = t * 64 + (col >> 7) * 32 + (col & 31), gate = (col >> 5) & 3;
        if (launch == 0) {
            if (gate == 3) v = (!second && tap == 4) ? w_lag[(int64_t)oc * C + icc] : 0.0f;
            else v = second ? w_m[((int64_t)(gate * C + oc) * C + icc) * 9 + tap] : w_x[((int64_t)((3 + gate) * C + oc) * C + icc) * 9 + tap];
        } else {
            v = second ? w_h[((int64_t)(gate * C + oc) * C + icc) * 9 + tap] : w_x[((int64_t)((gate == 3 ? 6 : gate) * C + oc) * C + icc) * 9 + tap];
        }
    } else {
        const int oc = t * (P / 2) + (col >> 6) * 32 + (col & 31);
        if ((col >> 5) & 1) v = tap == 4 ? w_last[(int64_t)oc * 2 * C + ic] : 0.0f;
        else v = w_o[((int64_t)oc * 2 * C + ic) * 9 + tap];
    }
    wp[i] = f32_to_bf16_rne(v);
}

}  // namespace v2v
