// v2v_nernet.hpp -- NER-Net's learned event voxelisation (gfx950): a statistics pre-pass and one fused value-and-scatter kernel.
//
// Replaces, for inference, the front of NER-Net:
//   model/nernet/representation_modules.py:12-54    ValueLayer (the MLP  Linear(1,h1) - act - ... - Linear(h,1))
//   model/nernet/representation_modules.py:175-261  QuantizationLayer_trail            -> [B, 2C, H, W]
//   model/nernet/representation_modules.py:91-172   QuantizationLayer_trail_combined   -> [B, C, H, W]
// Every event row (x, y, t, p, b) adds  t_n * MLP(t_n - bin)  to each of the C bins of its pixel.  The stock layer runs C passes of the
// MLP over [1, N, width] activations in HBM and C put_(accumulate=True) calls behind a Python loop over the batch; here one work-item
// owns one event: 5 values in (40 B for the dataset's float64 rows), the hidden vector in registers, C float32 atomics out.
//
// Where things live.  The MLP's weights are wave-uniform: they are read from the packed parameter block (layout below) through a
// `const __restrict__` kernel argument with uniform indices, i.e. by scalar loads into SGPRs that feed v_fma_f32 directly -- they never sit
// in per-lane registers.  The layer's input vector h[KP] is a register array with compile-time indices (KP = padded width, a template
// parameter).  A layer's outputs are produced four rows at a time in a run-time loop -- a run-time index into a register array would turn
// it into scratch -- so each finished output goes to the lane's own LDS column hs[j*64 + lane] and is read back as the next layer's h[].
// One wave per workgroup, a lane only ever reads what it wrote itself: no barrier.  Activations never reach HBM.
//
// Packed parameter block (float32), KP = the largest hidden width rounded up to a multiple of 16, every gap zero:
//   w0[KP] b0[KP]                         Linear(1, h1).weight[:, 0], .bias
//   { W[KP][KP] b[KP] } per hidden Linear  row j = .weight[j, :]
//   wL[KP] bL[KP]                         Linear(h_last, 1).weight[0, :], .bias in bL[0]
// Zero rows give act(0) = 0 activations, zero columns ignore them: padding changes no sum.
//
// Semantics kept from the reference (file:line of representation_modules.py):
//   * per batch id, t_first / t_last are the t of the first / last ROW with that id, not min / max (:210); normalize=True divides by
//     max(t - t_first) (:204-207), which is fl(t_max - t_first) because rounding is monotone;
//   * dt == 0 leaves t raw (:211 `continue`); normalize with max == 0 leaves t - t_first, which the reference has already stored (:204);
//     rows whose batch id is not one of 0..B-1 keep raw t;
//   * the normalisation runs in the rows' own dtype (a true subtract, divide, multiply, in that order), then rounds once to float32 (:215);
//   * the flat index is formed in the rows' dtype, term by term as :219-223 and :243 write it, truncated toward zero, clamped at the top to
//     numel - 1 (:246); put_ wraps an index in [-numel, -1] once.  Below that put_ raises: such a term is DROPPED here (as is a NaN index);
//   * cat(vox[:, 1], vox[:, 0]) (:253) is folded into the address: the positive-polarity half is written first.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v2v {

constexpr int kNerLanes = 64;          // one wave per workgroup (the LDS column trick needs no barrier)
constexpr int kNerMaxWidth = 128;      // hidden widths 1..128
constexpr int kNerMaxLinear = 5;       // mlp_layers has 3..6 entries

struct LearnedVoxelArgs {
    const void *events;                // [n, 5] rows (x, y, t, p, b), float64 or float32
    const int64_t *seg;                // optional [n_seg + 1] ascending row offsets: rows [seg[f], seg[f+1]) form grid f (nullptr: one grid)
    int64_t n_seg, n;
    int32_t B, C, H, W;
    int32_t normalize, combined;
    int32_t n_linear;                  // Linear layers: 2..5
    int32_t width[kNerMaxLinear + 1];  // mlp_layers
    float slope;                       // LeakyReLU slope (0: ReLU)
    unsigned long long *stats;         // [n_seg * B][3]: ~first row, last row + 1, ordered key of max t; 0 = no row
    float *out;                        // [n_seg][B, 2C, H, W] (combined: [B, C, H, W]), cleared by the caller
    float *t_out;                      // optional [n]: the normalised t, float32
};

__device__ __forceinline__ bool ner_segment(const int64_t *seg, int64_t n_seg, int64_t n, int64_t i, int64_t &f)
{
    f = 0;
    if (!seg) return true;
    int64_t l = 0, r = n_seg;                                             // seg[l] <= i < seg[r]
    while (r - l > 1) { const int64_t m = (l + r) >> 1; if (seg[m] <= i) l = m; else r = m; }
    f = l;
    return i >= seg[l] && i < seg[l + 1] && seg[l + 1] <= n;
}

// the batch id of a row, or -1 when it is none of 0..B-1 (the reference's mask `events[:, -1] == bi` matches no such row)
template <typename T> __device__ __forceinline__ int ner_batch(T b, int B)
{
    if (!(b >= (T)0 && b < (T)B)) return -1;
    const int bi = (int)b;
    return (T)bi == b ? bi : -1;
}

// monotone map double -> uint64 (larger value, larger key; every key of a real number is > 0)
__device__ __forceinline__ unsigned long long ner_key(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ner_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

// Pre-pass: integer atomics on row indices (and on the ordered key of t), so the statistics do not depend on scheduling.  All three are
// maxima (the first row as ~index).  A wave first reduces the rows that share a (segment, batch id) by shuffles -- one pass per distinct
// pair among its 64 rows, usually one -- and its leader issues the atomics, and only those that can still raise the value: millions of
// atomics on the same three words would otherwise serialise in L2.
template <typename T>
__global__ void __launch_bounds__(256) learned_voxel_stats_kernel(const T *__restrict__ ev, const int64_t *__restrict__ seg, int64_t n_seg, int64_t n, int B,
                                                                  unsigned long long *stats)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int64_t f = 0;
    int bi = -1;
    if (i < n && ner_segment(seg, n_seg, n, i, f)) bi = ner_batch(ev[i * 5 + 4], B);
    const bool active = bi >= 0;
    const unsigned long long key = active ? (unsigned long long)(f * B + bi) : ~0ull;
    const unsigned long long v0 = active ? ~(unsigned long long)i : 0ull, v1 = active ? (unsigned long long)i + 1 : 0ull;
    const unsigned long long v2 = active ? ner_key((double)ev[i * 5 + 2]) : 0ull;
    unsigned long long todo = __ballot(active);
    while (todo) {                                                        // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned long long k = __shfl(key, leader);
        const bool mine = active && key == k;
        unsigned long long a0 = mine ? v0 : 0ull, a1 = mine ? v1 : 0ull, a2 = mine ? v2 : 0ull;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const unsigned long long o0 = __shfl_xor(a0, off), o1 = __shfl_xor(a1, off), o2 = __shfl_xor(a2, off);
            a0 = o0 > a0 ? o0 : a0;
            a1 = o1 > a1 ? o1 : a1;
            a2 = o2 > a2 ? o2 : a2;
        }
        if (lane == leader) {
            unsigned long long *s = stats + k * 3;
            if (a0 > __hip_atomic_load(s + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(s + 0, a0);
            if (a1 > __hip_atomic_load(s + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(s + 1, a1);
            if (a2 > __hip_atomic_load(s + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(s + 2, a2);
        }
        todo &= ~__ballot(mine);
    }
}

template <typename T, int KP>
__global__ void __launch_bounds__(kNerLanes) learned_voxel_kernel(const LearnedVoxelArgs a, const T *__restrict__ ev, const float *__restrict__ prm)
{
    __shared__ float hs[KP * kNerLanes];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kNerLanes + lane;
    if (i >= a.n) return;
    int64_t f;
    if (!ner_segment(a.seg, a.n_seg, a.n, i, f)) return;                  // a row outside every interval: not this call's business
    const T x = ev[i * 5 + 0], y = ev[i * 5 + 1], t = ev[i * 5 + 2], p = ev[i * 5 + 3], b = ev[i * 5 + 4];
    const int C = a.C;

    // ---- normalisation, in the rows' dtype (:201-213) ----
    T tn = t;
    const int bi = ner_batch(b, a.B);
    if (bi >= 0) {
        const unsigned long long *s = a.stats + (f * a.B + bi) * 3;
        const unsigned long long first = ~s[0], last = s[1] - 1;
        if (first < (unsigned long long)a.n && last < (unsigned long long)a.n) {    // always, after the pre-pass of the same rows
            const T t0 = ev[first * 5 + 2];
            if (a.normalize) {
                const T u = t - t0;
                const T m = (T)ner_unkey(s[2]) - t0;
                tn = (m == (T)0) ? u : u / m;
            } else {
                const T dt = ev[last * 5 + 2] - t0;
                if (!(dt == (T)0)) tn = (t - t0) / dt * (T)(C - 1);
            }
        }
    }
    const float tf = (float)tn;                                          // :215
    if (a.t_out) a.t_out[i] = tf;

    // ---- flat index before the bin term, in the rows' dtype (:219-223; combined :136-139) ----
    const int64_t WH = (int64_t)a.W * a.H, WHC = WH * C;
    T idx0 = x + (T)a.W * y;
    idx0 = idx0 + (T)0;
    int64_t numel;
    float fac;
    if (a.combined) {
        idx0 = idx0 + (T)WHC * b;
        numel = WHC * a.B;
        fac = (float)p * tf;                                             // :134 (float32 rows only)
    } else {
        const T p01 = (p + (T)1) / (T)2;                                 // :217
        idx0 = idx0 + (T)WHC * p01;
        idx0 = idx0 + (T)(WHC * 2) * b;
        numel = 2 * WHC * a.B;
        fac = tf;
    }
    float *grid = a.out + f * numel;

    const int nl = a.n_linear;
    const float slope = a.slope;
    const float *wlast = prm + 2 * KP + (nl - 2) * (KP * KP + KP);
    float h[KP];
    for (int ib = 0; ib < C; ++ib) {
        const float sb = a.normalize ? (float)((double)ib / (double)(C - 1)) : (float)ib;     // :236 / :239: a Python scalar, rounded to float32
        const float xin = fac - sb;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const float z = __builtin_fmaf(prm[k], xin, prm[KP + k]);
            h[k] = z > 0.0f ? z : z * slope;
        }
        for (int l = 1; l < nl - 1; ++l) {
            const float *wl = prm + 2 * KP + (l - 1) * (KP * KP + KP), *bl = wl + KP * KP;
            const int rows = (a.width[l + 1] + 3) & ~3;
            for (int j = 0; j < rows; j += 4) {
                // two partial sums per output (even / odd k), the bias last as a GEMM adds it: half the rounding steps per chain
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
                const float *w = wl + j * KP;
#pragma unroll
                for (int k = 0; k < KP; k += 2) {
                    a0 = __builtin_fmaf(w[k], h[k], a0);
                    a1 = __builtin_fmaf(w[KP + k], h[k], a1);
                    a2 = __builtin_fmaf(w[2 * KP + k], h[k], a2);
                    a3 = __builtin_fmaf(w[3 * KP + k], h[k], a3);
                    c0 = __builtin_fmaf(w[k + 1], h[k + 1], c0);
                    c1 = __builtin_fmaf(w[KP + k + 1], h[k + 1], c1);
                    c2 = __builtin_fmaf(w[2 * KP + k + 1], h[k + 1], c2);
                    c3 = __builtin_fmaf(w[3 * KP + k + 1], h[k + 1], c3);
                }
                a0 = (a0 + c0) + bl[j];
                a1 = (a1 + c1) + bl[j + 1];
                a2 = (a2 + c2) + bl[j + 2];
                a3 = (a3 + c3) + bl[j + 3];
                hs[(j + 0) * kNerLanes + lane] = a0 > 0.0f ? a0 : a0 * slope;
                hs[(j + 1) * kNerLanes + lane] = a1 > 0.0f ? a1 : a1 * slope;
                hs[(j + 2) * kNerLanes + lane] = a2 > 0.0f ? a2 : a2 * slope;
                hs[(j + 3) * kNerLanes + lane] = a3 > 0.0f ? a3 : a3 * slope;
            }
#pragma unroll
            for (int k = 0; k < KP; ++k) h[k] = k < rows ? hs[k * kNerLanes + lane] : 0.0f;
        }
        float y0 = 0.0f, y1 = 0.0f, y2 = 0.0f, y3 = 0.0f;
#pragma unroll
        for (int k = 0; k < KP; k += 4) {
            y0 = __builtin_fmaf(wlast[k], h[k], y0);
            y1 = __builtin_fmaf(wlast[k + 1], h[k + 1], y1);
            y2 = __builtin_fmaf(wlast[k + 2], h[k + 2], y2);
            y3 = __builtin_fmaf(wlast[k + 3], h[k + 3], y3);
        }
        const float yv = ((y0 + y1) + (y2 + y3)) + wlast[KP];
        const float v = fac * yv;                                        // :241

        const T idx = idx0 + (T)(WH * ib);                               // :243
        if (!(idx > (T)-9.0e18)) continue;                               // NaN or far below -numel, where put_ raises: dropped
        int64_t li = idx >= (T)9.0e18 ? numel - 1 : (int64_t)idx;        // .long(): toward zero
        if (li > numel - 1) li = numel - 1;                              // :246
        if (li < -numel) continue;                                       // put_ raises: dropped
        if (li < 0) li += numel;                                         // put_ wraps once
        if (!a.combined) {                                               // :251-253: [B, 2, C, H, W] -> cat(half 1, half 0)
            const int64_t bb = li / (2 * WHC), r = li - bb * 2 * WHC;
            li = r < WHC ? li + WHC : li - WHC;
        }
        atomicAdd(grid + li, v);
    }
}

}  // namespace v2v
