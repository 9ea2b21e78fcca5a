// v2v_train_tu.hip -- backward passes of the recurrent UNet's layers (training with trainable=True, v2v_amd/train.py).
//
// Kernels in this file:  conv_wgrad_kernel + wgrad_reduce_kernel (weight / bias gradient of every convolution: K = the pixels, split
// into slabs, fixed-order sum) | relu_mask_stuff_kernel (ReLU backward from the saved post-ReLU output, optionally spread onto the
// stride-2 input grid) | dgrad_flip_kernel (weights flipped and transposed: the data gradient of a convolution is a convolution that
// runs on the forward kernels) | upsample2x_cat_bwd_kernel (adjoint of the x2 bilinear upsampling, whole tensor or one channel slice) |
// conv1x1_bwd_cout_kernel + conv1x1_bwd_cout_reduce_kernel (the prediction layer, 1..3 outputs).  The ConvLSTM step's backward is an epilogue of convlstm_step_kernel (EPI = 2,
// v2v_convlstm.hpp).  Numerics: bf16 MFMA operands, fp32 accumulation, fp32 parameter gradients; no float atomics anywhere, so every
// gradient is bitwise reproducible from run to run.
// The C entry points of the backward operators (include/v2v_hip.h) follow the kernels and their launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/v2v_hip.h"
#include "v2v_args.hpp"
#include "v2v_status.hpp"

namespace v2v {

namespace {
typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 tr_bf16x8;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float tr_f32x16;
typedef __bf16 tr_hwbf16x2 __attribute__((ext_vector_type(2)));
typedef float tr_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint16_t tr_bf16(float f)     // round to nearest even (v_cvt_pk_bf16_f32), NaN stays NaN
{
    return (uint16_t)__builtin_bit_cast(uint32_t, __builtin_convertvector(tr_f32x2{f, f}, tr_hwbf16x2));
}
__device__ __forceinline__ float tr_f32(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

constexpr int kWgTileN = 128;                            // weight-gradient columns per workgroup (4 waves x 32)
}  // namespace

// ---- weight gradient: dW[co][tap, ci] = sum_p dy[p][co] * x[p + tap][ci] -------------------------------------------------------
// One MFMA GEMM per convolution: M = Cout (32-row fragments), N = taps * Cin (n = tap * Cin + ci), K = the B*Ho*Wo output pixels.
// K is split into `S` slabs (grid z); slab s writes its partial sums ws[s][co][n] (fp32) and its bias partial wsb[s][co]; the reduce
// kernel adds the slabs in slab order.  The input is x1 (C1 channels) | x2 (C2 channels, may be null = zero): the ConvLSTM gates'
// cat(x, h_prev) without the copy.  A lane's 8 k values are 8 consecutive pixels: 2-byte gathers from the NHWC tensors (32 lanes of a
// fragment row read 64 consecutive bytes of one pixel).
__global__ void __launch_bounds__(256) conv_wgrad_kernel(const uint16_t *dy, const uint16_t *x1, int C1, const uint16_t *x2, int C2, float *ws,
                                                         float *wsb, int B, int Hin, int Win, int Ho, int Wo, int Cout, int ks, int stride,
                                                         int N, int Npad, int k_slab)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, fh = lane >> 5;
    const int Cin = C1 + C2, pad = ks >> 1;
    const int co = blockIdx.y * 32 + fr;
    const int n = blockIdx.x * kWgTileN + wave * 32 + fr;
    const int tap = n / Cin, ci = n - tap * Cin;
    const int ty = tap / ks - pad, tx = tap % ks - pad;
    const bool live = n < N;
    const uint16_t *src = ci < C1 ? x1 : x2;
    const int csrc = ci < C1 ? C1 : C2, coff = ci < C1 ? ci : ci - C1;
    const int M = B * Ho * Wo, HWo = Ho * Wo;
    const int k0 = blockIdx.z * k_slab, k1 = min(M, k0 + k_slab);
    const bool do_bias = blockIdx.x == 0 && wave == 0;
    tr_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    float bsum = 0.0f;
    for (int k = k0; k < k1; k += 16) {
        tr_bf16x8 af, bf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int p = k + 8 * fh + j;
            uint16_t av = 0, bv = 0;
            if (p < k1) {
                av = dy[(int64_t)p * Cout + co];
                const int b = p / HWo, q = p - b * HWo, oy = q / Wo, ox = q - oy * Wo;
                const int iy = oy * stride + ty, ix = ox * stride + tx;
                if (live && src && (unsigned)iy < (unsigned)Hin && (unsigned)ix < (unsigned)Win)
                    bv = src[(((int64_t)b * Hin + iy) * Win + ix) * csrc + coff];
            }
            if (do_bias) bsum += tr_f32(av);
            af[j] = __builtin_bit_cast(__bf16, av);
            bf[j] = __builtin_bit_cast(__bf16, bv);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
    }
    // accumulator element r: row (co) (r & 3) + 8 (r >> 2) + 4 fh, column (n) fr
    float *const wsl = ws + ((int64_t)blockIdx.z * Cout + blockIdx.y * 32) * Npad + n;
#pragma unroll
    for (int r = 0; r < 16; ++r) wsl[(int64_t)((r & 3) + 8 * (r >> 2) + 4 * fh) * Npad] = acc[r];
    if (do_bias) {
        const float other = __shfl_xor(bsum, 32);
        if (fh == 0) wsb[(int64_t)blockIdx.z * Cout + co] = bsum + other;
    }
}

// dW in nn.Conv2d's layout [Cout, Cin_out, ks, ks] (Cin_out <= C1 + C2: the head's padded channels dropped) and db [Cout]: one
// work-item per element, slabs added in slab order
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float *ws, const float *wsb, float *dw, float *db, int S, int Cout, int Cin,
                                                           int Cin_out, int taps, int Npad)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nw = (int64_t)Cout * Cin_out * taps;
    if (i < nw) {
        const int tap = (int)(i % taps), ci = (int)((i / taps) % Cin_out), co = (int)(i / ((int64_t)taps * Cin_out));
        const float *p = ws + (int64_t)co * Npad + tap * Cin + ci;
        float s = 0.0f;
        for (int k = 0; k < S; ++k) s += p[(int64_t)k * Cout * Npad];
        dw[i] = s;
    } else if (i < nw + Cout && db) {
        const int co = (int)(i - nw);
        float s = 0.0f;
        for (int k = 0; k < S; ++k) s += wsb[(int64_t)k * Cout + co];
        db[co] = s;
    }
}

// slabs of the weight gradient: about 2048 workgroups in all, at least 256 pixels per slab
int64_t wgrad_slabs(int64_t M, int Cout, int64_t N)
{
    const int64_t tiles = ((N + kWgTileN - 1) / kWgTileN) * (Cout / 32);
    int64_t s = (2048 + tiles - 1) / tiles;
    const int64_t smax = (M + 255) / 256;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    const int64_t k_slab = ((M + s - 1) / s + 15) / 16 * 16;
    return (M + k_slab - 1) / k_slab;
}

hipError_t launch_conv_wgrad(const uint16_t *dy, const uint16_t *x1, int C1, const uint16_t *x2, int C2, int Cin_out, float *dw, float *db, float *ws,
                             int B, int Hin, int Win, int Ho, int Wo, int Cout, int ks, int stride, hipStream_t s)
{
    const int64_t M = (int64_t)B * Ho * Wo;
    const int N = ks * ks * (C1 + C2), ntiles = (N + kWgTileN - 1) / kWgTileN, Npad = ntiles * kWgTileN;
    const int64_t S = wgrad_slabs(M, Cout, N);
    const int k_slab = (int)((M + S - 1) / S + 15) / 16 * 16;
    float *wsb = ws + S * Cout * Npad;
    hipLaunchKernelGGL(conv_wgrad_kernel, dim3((unsigned)ntiles, (unsigned)(Cout / 32), (unsigned)S), dim3(256), 0, s, dy, x1, C1, x2, C2, ws, wsb,
                       B, Hin, Win, Ho, Wo, Cout, ks, stride, N, Npad, k_slab);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t n = (int64_t)Cout * Cin_out * ks * ks + Cout;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws, wsb, dw, db, (int)S, Cout, C1 + C2, Cin_out,
                       ks * ks, Npad);
    return hipGetLastError();
}

// ---- ReLU backward (+ the stride-2 spread) ---------------------------------------------------------------------------------------
// out = dy where y > 0 else 0 (y = the saved post-ReLU output; null: no mask).  stride 2: out is [B, 2 Ho, 2 Wo, C] with the masked
// dy at the even positions and zeros between -- the data gradient of a stride-2 convolution is then the stride-1 convolution of
// this grid with the flipped weights.  One work-item per pixel and 8 channels.
__global__ void __launch_bounds__(256) relu_mask_stuff_kernel(const uint16_t *dy, const uint16_t *y, uint16_t *out, int B, int Ho, int Wo, int C, int stride)
{
    const int G = C / 8, Hs = Ho * stride, Ws = Wo * stride;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * Hs * Ws * G) return;
    const int g = (int)(i % G);
    const int64_t pix = i / G;
    const int sx = (int)(pix % Ws), sy = (int)((pix / Ws) % Hs), b = (int)(pix / ((int64_t)Ws * Hs));
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (sx % stride == 0 && sy % stride == 0) {
        const int64_t src = (((int64_t)b * Ho + sy / stride) * Wo + sx / stride) * C + g * 8;
        v = *reinterpret_cast<const uint4 *>(dy + src);
        if (y) {
            const uint4 m = *reinterpret_cast<const uint4 *>(y + src);
            uint32_t *vv = reinterpret_cast<uint32_t *>(&v);
            const uint32_t *mm = reinterpret_cast<const uint32_t *>(&m);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t lo = tr_f32((uint16_t)(mm[j] & 0xFFFFu)) > 0.0f ? 0x0000FFFFu : 0u;
                const uint32_t hi = tr_f32((uint16_t)(mm[j] >> 16)) > 0.0f ? 0xFFFF0000u : 0u;
                vv[j] &= lo | hi;
            }
        }
    }
    *reinterpret_cast<uint4 *>(out + i * 8) = v;
}

hipError_t launch_relu_mask_stuff(const uint16_t *dy, const uint16_t *y, uint16_t *out, int B, int Ho, int Wo, int C, int stride, hipStream_t s)
{
    const int64_t n = (int64_t)B * Ho * stride * Wo * stride * (C / 8);
    hipLaunchKernelGGL(relu_mask_stuff_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dy, y, out, B, Ho, Wo, C, stride);
    return hipGetLastError();
}

// ---- data gradient: the weights of the transposed convolution ------------------------------------------------------------------
// w [Cout, Cin, ks, ks] -> wt [Cin, Cout, ks, ks] with both taps reversed: dx = conv(dy, wt) (pad ks/2, stride 1), packed afterwards
// by the forward's own packing kernel for Cin' = Cout, Cout' = Cin
__global__ void __launch_bounds__(256) dgrad_flip_kernel(const float *w, float *wt, int Cout, int Cin, int ks)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int taps = ks * ks;
    if (i >= (int64_t)Cout * Cin * taps) return;
    const int tap = (int)(i % taps), co = (int)((i / taps) % Cout), ci = (int)(i / ((int64_t)taps * Cout));
    wt[i] = w[((int64_t)co * Cin + ci) * taps + (taps - 1 - tap)];
}

// ---- adjoint of the x2 bilinear upsampling (align_corners=False, clamped edges) -------------------------------------------------
// Forward (upsample2x_nhwc_bf16_kernel / upsample2x_cat_nhwc_bf16_kernel): output row 2m reads rows (max(m-1, 0), m) with weights
// (0.25, 0.75), row 2m+1 reads (m, min(m+1, H-1)) with (0.75, 0.25); columns alike.  Gather form: input row k receives from output
// rows 2k-1 .. 2k+2, each with the sum of the weights under which it read k.  One work-item per input pixel and 8 channels, fp32
// sums, one bf16 rounding.
__device__ __forceinline__ float up_w(int j, int k, int n)
{
    const int m = j >> 1;
    const int lo = (j & 1) ? m : (m > 0 ? m - 1 : 0), hi = (j & 1) ? (m + 1 < n ? m + 1 : n - 1) : m;
    const float wlo = (j & 1) ? 0.75f : 0.25f, whi = (j & 1) ? 0.25f : 0.75f;
    return (lo == k ? wlo : 0.0f) + (hi == k ? whi : 0.0f);
}

// One channel slice [c0, c0 + C) of dout [B,2H,2W,Ctot] -> dx [B,H,W,C], read at pixel pitch Ctot.  The sum-skip layers run it with
// c0 = 0, C = Ctot (the result is the gradient of x AND of the skip: their forward upsamples x + skip); the concat-skip layers once for
// the gradient of x (c0 = 0) and once for the skip's (c0 = C1).
__global__ void __launch_bounds__(256) upsample2x_cat_bwd_kernel(const uint16_t *dout, uint16_t *dx, int B, int H, int W, int Ctot, int c0, int C)
{
    const int G = C / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * H * W * G) return;
    const int g = (int)(i % G);
    const int64_t pix = i / G;
    const int kx = (int)(pix % W), ky = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
    const int H2 = 2 * H, W2 = 2 * W;
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int jy = 2 * ky - 1; jy <= 2 * ky + 2; ++jy) {
        if (jy < 0 || jy >= H2) continue;
        const float wy = up_w(jy, ky, H);
        float row[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int jx = 2 * kx - 1; jx <= 2 * kx + 2; ++jx) {
            if (jx < 0 || jx >= W2) continue;
            const float wx = up_w(jx, kx, W);
            const uint4 v = *reinterpret_cast<const uint4 *>(dout + (((int64_t)b * H2 + jy) * W2 + jx) * Ctot + c0 + g * 8);
            const uint32_t *vv = reinterpret_cast<const uint32_t *>(&v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                row[2 * j] += wx * tr_f32((uint16_t)(vv[j] & 0xFFFFu));
                row[2 * j + 1] += wx * tr_f32((uint16_t)(vv[j] >> 16));
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += wy * row[j];
    }
    uint4 o;
    uint32_t *oo = reinterpret_cast<uint32_t *>(&o);
#pragma unroll
    for (int j = 0; j < 4; ++j) oo[j] = (uint32_t)tr_bf16(acc[2 * j]) | ((uint32_t)tr_bf16(acc[2 * j + 1]) << 16);
    *reinterpret_cast<uint4 *>(dx + pix * C + g * 8) = o;
}

hipError_t launch_upsample2x_cat_bwd(const uint16_t *dout, uint16_t *dx, int B, int H, int W, int Ctot, int c0, int C, hipStream_t s)
{
    const int64_t n = (int64_t)B * H * W * (C / 8);
    hipLaunchKernelGGL(upsample2x_cat_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dout, dx, B, H, W, Ctot, c0, C);
    return hipGetLastError();
}

// ---- the prediction layer's backward (1x1, C -> COUT = 1..3, on bf16(x + skip); E2VID's image: 1, EVFlowNet's flow: 2) ------------
// dy fp32 [M][COUT] (the loss gradient of the prediction, unrounded); dx[m][c] = bf16(sum_o dy[m][o] * bf16(w[o][c])) (o ascending) --
// the gradient of x and of the skip; dW[o][c] = sum_m dy[m][o] * bf16(x + skip)[m][c], db[o] = sum_m dy[m][o].
// One workgroup per slab of kC1x1Slab pixels: C / 8 lanes per pixel (8 channels each), the workgroup's partial sums meet in LDS in
// a fixed order and go to ws[slab][o][C + 1]; the reduce kernel adds the slabs in slab order.  No float atomics.
constexpr int kC1x1Slab = 2048;
int64_t conv1x1_bwd_slabs(int64_t M) { return (M + kC1x1Slab - 1) / kC1x1Slab; }

template <int COUT>
__global__ void __launch_bounds__(256) conv1x1_bwd_cout_kernel(const float *dy, const uint16_t *x, const uint16_t *skip, const float *w, uint16_t *dx,
                                                               float *ws, int64_t M, int C)
{
    __shared__ float red[COUT][256 * 9];
    const int G = C / 8, rows = 256 / G;
    const int g = threadIdx.x % G, pr = threadIdx.x / G;
    float wb[COUT][8], acc[COUT][8], accb[COUT];
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
        accb[o] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { wb[o][j] = tr_f32(tr_bf16(w[o * C + g * 8 + j])); acc[o][j] = 0.0f; }
    }
    const int64_t p0 = (int64_t)blockIdx.x * kC1x1Slab, p1 = p0 + kC1x1Slab < M ? p0 + kC1x1Slab : M;
    for (int64_t p = p0 + pr; p < p1; p += rows) {
        float d[COUT];
#pragma unroll
        for (int o = 0; o < COUT; ++o) d[o] = dy[p * COUT + o];
        const uint4 xv = *reinterpret_cast<const uint4 *>(x + p * C + g * 8);
        uint4 sv = make_uint4(0u, 0u, 0u, 0u);
        if (skip) sv = *reinterpret_cast<const uint4 *>(skip + p * C + g * 8);
        const uint32_t *xx = reinterpret_cast<const uint32_t *>(&xv), *ss = reinterpret_cast<const uint32_t *>(&sv);
        uint4 ov;
        uint32_t *oo = reinterpret_cast<uint32_t *>(&ov);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float xs0 = tr_f32((uint16_t)(xx[j] & 0xFFFFu)), xs1 = tr_f32((uint16_t)(xx[j] >> 16));
            if (skip) {
                xs0 = tr_f32(tr_bf16(xs0 + tr_f32((uint16_t)(ss[j] & 0xFFFFu))));
                xs1 = tr_f32(tr_bf16(xs1 + tr_f32((uint16_t)(ss[j] >> 16))));
            }
            float g0 = d[0] * wb[0][2 * j], g1 = d[0] * wb[0][2 * j + 1];
            acc[0][2 * j] += d[0] * xs0;
            acc[0][2 * j + 1] += d[0] * xs1;
#pragma unroll
            for (int o = 1; o < COUT; ++o) {
                g0 += d[o] * wb[o][2 * j];
                g1 += d[o] * wb[o][2 * j + 1];
                acc[o][2 * j] += d[o] * xs0;
                acc[o][2 * j + 1] += d[o] * xs1;
            }
            oo[j] = (uint32_t)tr_bf16(g0) | ((uint32_t)tr_bf16(g1) << 16);
        }
        *reinterpret_cast<uint4 *>(dx + p * C + g * 8) = ov;
#pragma unroll
        for (int o = 0; o < COUT; ++o) accb[o] += d[o];
    }
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[o][threadIdx.x * 9 + j] = acc[o][j];
        red[o][threadIdx.x * 9 + 8] = accb[o];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < COUT * (C + 1); idx += 256) {   // (o, c < C): channel c of output o; (o, C): its bias (from the lanes of channel group 0)
        const int o = idx / (C + 1), c = idx - o * (C + 1), cg = c < C ? c / 8 : 0, slot = c < C ? c % 8 : 8;
        float s = 0.0f;
        for (int r = 0; r < rows; ++r) s += red[o][(r * G + cg) * 9 + slot];
        ws[((int64_t)blockIdx.x * COUT + o) * (C + 1) + c] = s;
    }
}

__global__ void __launch_bounds__(256) conv1x1_bwd_cout_reduce_kernel(const float *ws, float *dw, float *db, int S, int C, int Cout)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Cout * (C + 1)) return;
    const int o = idx / (C + 1), c = idx - o * (C + 1);
    float s = 0.0f;
    for (int k = 0; k < S; ++k) s += ws[((int64_t)k * Cout + o) * (C + 1) + c];
    if (c < C) dw[o * C + c] = s;
    else db[o] = s;
}

hipError_t launch_conv1x1_bwd_cout(const float *dy, const uint16_t *x, const uint16_t *skip, const float *w, uint16_t *dx, float *dw, float *db, float *ws,
                                   int64_t M, int C, int Cout, hipStream_t s)
{
    const int64_t S = conv1x1_bwd_slabs(M);
    const dim3 grid((unsigned)S), block(256);
    switch (Cout) {
    case 1: hipLaunchKernelGGL(conv1x1_bwd_cout_kernel<1>, grid, block, 0, s, dy, x, skip, w, dx, ws, M, C); break;
    case 2: hipLaunchKernelGGL(conv1x1_bwd_cout_kernel<2>, grid, block, 0, s, dy, x, skip, w, dx, ws, M, C); break;
    case 3: hipLaunchKernelGGL(conv1x1_bwd_cout_kernel<3>, grid, block, 0, s, dy, x, skip, w, dx, ws, M, C); break;
    default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(conv1x1_bwd_cout_reduce_kernel, dim3((unsigned)((Cout * (C + 1) + 255) / 256)), dim3(256), 0, s, ws, dw, db, (int)S, C, Cout);
    return hipGetLastError();
}

}  // namespace v2v

using v2v::aligned;
using v2v::fail;
using v2v::hip_fail;

extern "C" {

int v2v_convlstm_step_bwd_hip(const void *x, const void *h_prev, const float *c_prev, const void *packed, const float *bias, const float *dh,
                              const float *dc, int64_t B, int64_t H, int64_t W, int64_t C, void *dgates, float *dc_prev, void *stream)
{
    if (!x || !packed || !bias || !dh || !dgates || !dc_prev) return fail(V2V_ERR_NULL, "v2v_convlstm_step_bwd_hip: x/packed/bias/dh/dgates/dc_prev is NULL");
    if (B < 1 || H < 1 || W < 1 || C < 64 || C % 64 != 0 || C > 4096 || (H * W) % 4 != 0 || B * H * W * 4 * C > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need B,H,W >= 1, C %% 64 == 0, C <= 4096, (H*W) %% 4 == 0, tensors below 2^31 elements");
    if (dgates == x || dgates == h_prev) return fail(V2V_ERR_PARAM, "dgates must not alias x or h_prev (neighbouring tiles read them)");
    if (!aligned(x, 16) || !aligned(h_prev, 16) || !aligned(packed, 16) || !aligned(c_prev, 4) || !aligned(dh, 4) || !aligned(dc, 4)
        || !aligned(dgates, 2) || !aligned(dc_prev, 4) || !aligned(bias, 4))
        return fail(V2V_ERR_ALIGN, "x/h_prev/packed need 16-byte alignment, c_prev/dh/dc/dc_prev/bias 4-byte, dgates 2-byte");
    v2v::ConvLstmArgs a{};
    a.x = static_cast<const uint16_t *>(x); a.h_prev = static_cast<const uint16_t *>(h_prev); a.c_prev = c_prev;
    a.wp = static_cast<const uint16_t *>(packed); a.bias = bias;
    a.B = (int)B; a.H = (int)H; a.W = (int)W; a.C = (int)C;
    a.dh = dh; a.dc = dc; a.dgates = static_cast<uint16_t *>(dgates); a.dc_prev = dc_prev;
    const hipError_t e = v2v::launch_convlstm_step_bwd(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "convlstm_step_kernel (EPI = 2) launch");
}

int v2v_relu_bwd_nhwc_hip(const void *dy, const void *y, int64_t M, int64_t C, void *out, void *stream)
{
    if (!dy || !out) return fail(V2V_ERR_NULL, "v2v_relu_bwd_nhwc_hip: dy/out is NULL");
    if (M < 1 || C < 8 || C % 8 != 0 || M * C > 0x7FFFFFFFLL) return fail(V2V_ERR_SHAPE, "need M >= 1, C %% 8 == 0, M*C below 2^31");
    if (!aligned(dy, 16) || !aligned(y, 16) || !aligned(out, 16)) return fail(V2V_ERR_ALIGN, "dy/y/out need 16-byte alignment");
    const hipError_t e = v2v::launch_relu_mask_stuff(static_cast<const uint16_t *>(dy), static_cast<const uint16_t *>(y), static_cast<uint16_t *>(out),
                                                     1, 1, (int)M, (int)C, 1, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "relu_mask_stuff_kernel launch");
}

int64_t v2v_conv_dgrad_packed_elems(int64_t Cin, int64_t Cout, int ks) { return v2v_conv_packed_elems(Cout, Cin, ks); }

int v2v_conv_dgrad_pack_weights_hip(const float *weight, int64_t Cin, int64_t Cout, int ks, float *scratch, void *packed, void *stream)
{
    if (!weight || !scratch || !packed) return fail(V2V_ERR_NULL, "v2v_conv_dgrad_pack_weights_hip: weight/scratch/packed is NULL");
    if ((ks != 3 && ks != 5) || v2v_conv_dgrad_packed_elems(Cin, Cout, ks) < 0)
        return fail(V2V_ERR_SHAPE, "the transposed convolution (Cout -> Cin, ks 3 or 5) is not a shape the convolution kernel takes");
    if (!aligned(packed, 16) || !aligned(scratch, 4)) return fail(V2V_ERR_ALIGN, "packed needs 16-byte alignment");
    const int64_t n = Cout * Cin * ks * ks;
    hipLaunchKernelGGL(v2v::dgrad_flip_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), weight, scratch, (int)Cout,
                       (int)Cin, ks);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = v2v::launch_conv_pack(scratch, static_cast<uint16_t *>(packed), (int)Cout, (int)Cin, ks, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "dgrad weight packing launch");
}

// (v2v_conv_dgrad_nhwc_hip itself runs on the forward convolution's instances and lives with them, in v2v_convlstm_tu.hip)
int64_t v2v_conv_dgrad_workspace_bytes(int64_t B, int64_t Hin, int64_t Win, int64_t Cin, int64_t Cout, int stride)
{
    if (B < 1 || Hin < 1 || Win < 1 || Cin < 1 || Cout < 1 || (stride != 1 && stride != 2)) return -1;
    return (Cin * 4 + 255) / 256 * 256 + (stride == 2 ? B * Hin * Win * Cout * 2 : 0);
}

int64_t v2v_conv_wgrad_workspace_bytes(int64_t B, int64_t Ho, int64_t Wo, int64_t Cin, int64_t Cout, int ks)
{
    if (B < 1 || Ho < 1 || Wo < 1 || Cin < 1 || Cout < 32 || Cout % 32 != 0 || (ks != 1 && ks != 3 && ks != 5)) return -1;
    const int64_t N = (int64_t)ks * ks * Cin, Npad = (N + 127) / 128 * 128;
    const int64_t S = v2v::wgrad_slabs(B * Ho * Wo, (int)Cout, N);
    return S * Cout * (Npad + 1) * 4;
}

int v2v_conv_wgrad_nhwc_hip(const void *dy, const void *x1, int64_t C1, const void *x2, int64_t C2, int64_t Cin_out, int64_t B, int64_t Hin, int64_t Win,
                            int64_t Cout, int ks, int stride, void *workspace, float *dw, float *db, void *stream)
{
    if (!dy || !x1 || !workspace || !dw) return fail(V2V_ERR_NULL, "v2v_conv_wgrad_nhwc_hip: dy/x1/workspace/dw is NULL");
    if ((ks != 1 && ks != 3 && ks != 5) || (stride != 1 && stride != 2)) return fail(V2V_ERR_PARAM, "ks must be 1, 3 or 5, stride 1 or 2");
    const int64_t Ho = (Hin - 1) / stride + 1, Wo = (Win - 1) / stride + 1;
    if (B < 1 || Hin < 1 || Win < 1 || C1 < 1 || C2 < 0 || Cin_out < 1 || Cin_out > C1 + C2 || Cout < 32 || Cout % 32 != 0
        || B * Hin * Win * (C1 > C2 ? C1 : C2) > 0x7FFFFFFFLL || B * Ho * Wo * Cout > 0x7FFFFFFFLL || (int64_t)ks * ks * (C1 + C2) > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need B,H,W >= 1, C1 >= 1, 1 <= Cin_out <= C1 + C2, Cout a multiple of 32, tensors below 2^31 elements");
    if (!aligned(dy, 2) || !aligned(x1, 2) || !aligned(x2, 2) || !aligned(workspace, 4) || !aligned(dw, 4) || !aligned(db, 4))
        return fail(V2V_ERR_ALIGN, "buffers misaligned");
    const hipError_t e = v2v::launch_conv_wgrad(static_cast<const uint16_t *>(dy), static_cast<const uint16_t *>(x1), (int)C1,
                                                static_cast<const uint16_t *>(x2), (int)C2, (int)Cin_out, dw, db, static_cast<float *>(workspace),
                                                (int)B, (int)Hin, (int)Win, (int)Ho, (int)Wo, (int)Cout, ks, stride, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "conv_wgrad_kernel launch");
}

int v2v_upsample2x_bwd_nhwc_hip(const void *dout, int64_t B, int64_t H, int64_t W, int64_t C, void *dx, void *stream)
{
    if (!dout || !dx) return fail(V2V_ERR_NULL, "v2v_upsample2x_bwd_nhwc_hip: dout/dx is NULL");
    if (B < 1 || H < 1 || W < 1 || C < 8 || C % 8 != 0 || B * 4 * H * W * C > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need B,H,W >= 1, C %% 8 == 0, tensors below 2^31 elements");
    if (!aligned(dout, 16) || !aligned(dx, 16)) return fail(V2V_ERR_ALIGN, "dout/dx need 16-byte alignment");
    const hipError_t e = v2v::launch_upsample2x_cat_bwd(static_cast<const uint16_t *>(dout), static_cast<uint16_t *>(dx), (int)B, (int)H, (int)W, (int)C,
                                                        0, (int)C, static_cast<hipStream_t>(stream));    // the whole tensor as one slice
    return e == hipSuccess ? V2V_OK : hip_fail(e, "upsample2x_cat_bwd_kernel launch");
}

int64_t v2v_conv1x1_bwd_workspace_bytes(int64_t M, int64_t C)
{
    if (M < 1 || C < 8 || C > 128 || (C & (C - 1)) != 0) return -1;
    return v2v::conv1x1_bwd_slabs(M) * (C + 1) * 4;
}

int v2v_conv1x1_bwd_nhwc_hip(const float *dy, const void *x, const void *skip, const float *weight, int64_t M, int64_t C, void *dx, float *dw, float *db,
                             void *workspace, void *stream)
{
    if (!dy || !x || !weight || !dx || !dw || !db || !workspace) return fail(V2V_ERR_NULL, "v2v_conv1x1_bwd_nhwc_hip: a required pointer is NULL");
    if (M < 1 || C < 8 || C > 128 || (C & (C - 1)) != 0 || M * C > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need M >= 1 and C a power of two in 8..128 (one output channel)");
    if (!aligned(dy, 4) || !aligned(x, 16) || !aligned(skip, 16) || !aligned(dx, 16) || !aligned(weight, 4) || !aligned(workspace, 4))
        return fail(V2V_ERR_ALIGN, "x/skip/dx need 16-byte alignment, dy/weight/workspace 4-byte");
    const hipError_t e = v2v::launch_conv1x1_bwd_cout(dy, static_cast<const uint16_t *>(x), static_cast<const uint16_t *>(skip), weight,
                                                      static_cast<uint16_t *>(dx), dw, db, static_cast<float *>(workspace), M, (int)C, 1,
                                                      static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "conv1x1_bwd_cout_kernel launch");
}

// ---- the plain UNet (EVFlowNet): the concat-skip upsampling's adjoint, the prediction backward for 1..3 outputs ------------------------
int v2v_upsample2x_cat_bwd_nhwc_hip(const void *dout, int64_t B, int64_t H, int64_t W, int64_t Ctot, int64_t c0, int64_t C, void *dx, void *stream)
{
    if (!dout || !dx) return fail(V2V_ERR_NULL, "v2v_upsample2x_cat_bwd_nhwc_hip: dout/dx is NULL");
    if (B < 1 || H < 1 || W < 1 || C < 8 || C % 8 != 0 || Ctot % 8 != 0 || c0 < 0 || c0 % 8 != 0 || c0 + C > Ctot || B * 4 * H * W * Ctot > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need B,H,W >= 1, C, c0 and Ctot multiples of 8, c0 + C <= Ctot, tensors below 2^31 elements");
    if (!aligned(dout, 16) || !aligned(dx, 16)) return fail(V2V_ERR_ALIGN, "dout/dx need 16-byte alignment");
    if (dx == dout) return fail(V2V_ERR_PARAM, "dx must not alias dout");
    const hipError_t e = v2v::launch_upsample2x_cat_bwd(static_cast<const uint16_t *>(dout), static_cast<uint16_t *>(dx), (int)B, (int)H, (int)W, (int)Ctot,
                                                        (int)c0, (int)C, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "upsample2x_cat_bwd_kernel launch");
}

int64_t v2v_conv1x1_bwd_cout_workspace_bytes(int64_t M, int64_t C, int64_t Cout)
{
    if (M < 1 || C < 8 || C > 128 || (C & (C - 1)) != 0 || Cout < 1 || Cout > 3) return -1;
    return v2v::conv1x1_bwd_slabs(M) * Cout * (C + 1) * 4;
}

int v2v_conv1x1_bwd_cout_nhwc_hip(const float *dy, const void *x, const void *skip, const float *weight, int64_t M, int64_t C, int64_t Cout, void *dx,
                                  float *dw, float *db, void *workspace, void *stream)
{
    if (!dy || !x || !weight || !dx || !dw || !db || !workspace) return fail(V2V_ERR_NULL, "v2v_conv1x1_bwd_cout_nhwc_hip: a required pointer is NULL");
    if (M < 1 || C < 8 || C > 128 || (C & (C - 1)) != 0 || Cout < 1 || Cout > 3 || M * C > 0x7FFFFFFFLL)
        return fail(V2V_ERR_SHAPE, "need M >= 1, C a power of two in 8..128, Cout 1..3");
    if (!aligned(dy, 4) || !aligned(x, 16) || !aligned(skip, 16) || !aligned(dx, 16) || !aligned(weight, 4) || !aligned(workspace, 4) || !aligned(dw, 4)
        || !aligned(db, 4))
        return fail(V2V_ERR_ALIGN, "x/skip/dx need 16-byte alignment, dy/weight/dw/db/workspace 4-byte");
    const hipError_t e = v2v::launch_conv1x1_bwd_cout(dy, static_cast<const uint16_t *>(x), static_cast<const uint16_t *>(skip), weight,
                                                      static_cast<uint16_t *>(dx), dw, db, static_cast<float *>(workspace), M, (int)C, (int)Cout,
                                                      static_cast<hipStream_t>(stream));
    return e == hipSuccess ? V2V_OK : hip_fail(e, "conv1x1_bwd_cout_kernel launch");
}

}  // extern "C"
