// v2v_metrics.hpp -- the evaluation metrics of the reference's test loop as device kernels:
//
//   image_metrics_kernel   MSE and skimage's structural_similarity (7x7 uniform window, sample covariance, K1 0.01, K2 0.03) of T frame
//                          pairs; one 32x8 tile of windows per workgroup, per-tile partial sums into fixed slots
//   flow_metrics_kernel    the masks, end-point error, counts and sums of FlowModelInterface.compute_metrics, 2048 pixels per workgroup
//   metrics_reduce_kernel  adds the slots of a frame in slot order (one workgroup per frame)
//
// No float atomics anywhere: a slot is written by exactly one workgroup and the slots are added in a fixed order, so two runs agree bit
// for bit.  All moment arithmetic is float64 (a product of two float32 values is exact there); the library is built with
// -ffp-contract=off, so the formula below is evaluated operation by operation as written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v2v {

constexpr int kMetThreads = 256;
constexpr int kSsimWin = 7;                      // skimage's default window
constexpr int kSsimTX = 32, kSsimTY = 8;         // windows per workgroup: one per thread
constexpr int kSsimHX = kSsimTX + kSsimWin - 1;  // halo tile: 38 x 14 pixels of each image
constexpr int kSsimHY = kSsimTY + kSsimWin - 1;
constexpr int kFlowPix = 8;                      // pixels per thread of the flow kernel
constexpr int kFlowTile = kMetThreads * kFlowPix;
constexpr int kImgSlots = 2;                     // (sum of squared differences, sum of S)
constexpr int kFlowSlots = 8;                    // (EE sum dense, sparse | n_dense, n_sparse, dense >1, dense >3, sparse >1, sparse >3)

struct ImageMetricsArgs {
    const float *pred, *image;
    int64_t pred_stride, image_stride;  // elements between frames
    int H, W, tiles_x, tiles_y;
    float divisor;
    double c1, c2;
    double *slots;  // [T][tiles_y * tiles_x][2]
    double *map;    // optional [T][H-6][W-6]
};

struct FlowMetricsArgs {
    const float *pred, *gt, *events;
    int64_t pred_stride, gt_stride, ev_stride;  // elements between frames
    int C, HW, tiles;
    unsigned long long *slots;  // [T][tiles][8], the first two words hold doubles
};

// Sum over the 256 threads in a fixed tree: lanes by shuffles, then the four waves in order.  `part` holds four values.
__device__ __forceinline__ double met_block_sum(double v, double *part)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

__device__ __forceinline__ unsigned long long met_block_sum(unsigned long long v, unsigned long long *part)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// grid (T * tiles_y * tiles_x), 256 threads.  The halo tile of both images goes through LDS once (divided by `divisor` on the way, a
// float32 true division as the reference's `/ 255`); the thread that stages a pixel also takes its squared difference, every pixel of the
// image being owned by exactly one tile (the last tile of a row / column owns the six trailing columns / rows).  Each thread then takes
// the five sums of its window directly, 49 taps row-major, in float64.
__global__ __launch_bounds__(kMetThreads) void image_metrics_kernel(const ImageMetricsArgs a)
{
    __shared__ float sx[kSsimHY][kSsimHX], sy[kSsimHY][kSsimHX];
    __shared__ double part[4];
    const int tid = threadIdx.x, bx = blockIdx.x % a.tiles_x, by = blockIdx.x / a.tiles_x % a.tiles_y, t = blockIdx.x / (a.tiles_x * a.tiles_y);
    const float *px = a.pred + (int64_t)t * a.pred_stride, *py = a.image + (int64_t)t * a.image_stride;
    const int x0 = bx * kSsimTX, y0 = by * kSsimTY;
    const bool last_x = bx == a.tiles_x - 1, last_y = by == a.tiles_y - 1, scale = a.divisor != 1.0f;

    double sq = 0.0;
    for (int i = tid; i < kSsimHX * kSsimHY; i += kMetThreads) {
        const int r = i / kSsimHX, c = i - r * kSsimHX, gy = y0 + r, gx = x0 + c;
        float x = 0.0f, y = 0.0f;
        if (gy < a.H && gx < a.W) {
            const int64_t o = (int64_t)gy * a.W + gx;
            x = px[o];
            y = py[o];
            if (scale) {
                x = x / a.divisor;
                y = y / a.divisor;
            }
            if ((r < kSsimTY || last_y) && (c < kSsimTX || last_x)) {
                const double d = (double)(x - y);  // the difference in float32, as the reference's operands are
                sq += d * d;
            }
        }
        sx[r][c] = x;
        sy[r][c] = y;
    }
    __syncthreads();

    const int tx = tid & (kSsimTX - 1), ty = tid / kSsimTX, ox = x0 + tx, oy = y0 + ty;
    double S = 0.0;
    if (oy < a.H - (kSsimWin - 1) && ox < a.W - (kSsimWin - 1)) {
        double s_x = 0.0, s_y = 0.0, s_xx = 0.0, s_yy = 0.0, s_xy = 0.0;
#pragma unroll
        for (int dy = 0; dy < kSsimWin; ++dy)
#pragma unroll
            for (int dx = 0; dx < kSsimWin; ++dx) {
                const double x = (double)sx[ty + dy][tx + dx], y = (double)sy[ty + dy][tx + dx];
                s_x += x;
                s_y += y;
                s_xx += x * x;
                s_yy += y * y;
                s_xy += x * y;
            }
        constexpr double NP = (double)(kSsimWin * kSsimWin);
        const double ux = s_x / NP, uy = s_y / NP, uxx = s_xx / NP, uyy = s_yy / NP, uxy = s_xy / NP;
        const double cov = NP / (NP - 1.0);
        const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
        const double A1 = 2.0 * ux * uy + a.c1, A2 = 2.0 * vxy + a.c2;
        const double B1 = ux * ux + uy * uy + a.c1, B2 = vx + vy + a.c2;
        S = (A1 * A2) / (B1 * B2);
        if (a.map) a.map[((int64_t)t * (a.H - (kSsimWin - 1)) + oy) * (a.W - (kSsimWin - 1)) + ox] = S;
    }
    const double sq_sum = met_block_sum(sq, part);
    const double s_sum = met_block_sum(S, part);
    if (tid == 0) {
        double *slot = a.slots + (((int64_t)t * a.tiles_y + by) * a.tiles_x + bx) * kImgSlots;
        slot[0] = sq_sum;
        slot[1] = s_sum;
    }
}

// grid (T * tiles), 256 threads, 8 pixels per thread (coalesced: pixel = tile * 2048 + k * 256 + thread).  Per pixel, as the reference
// writes it: valid = !(isnan(gt0) | isnan(gt1) | (gt0 == 0 & gt1 == 0)); ev = (sum_c |events_c|) > 0 in float32, channel order;
// EE = sqrtf(d0 * d0 + d1 * d1) in float32.  A NaN EE on a valid pixel makes the sum NaN and counts in neither threshold.
__global__ __launch_bounds__(kMetThreads) void flow_metrics_kernel(const FlowMetricsArgs a)
{
    __shared__ double partd[4];
    __shared__ unsigned long long partu[4];
    const int tid = threadIdx.x, tile = blockIdx.x % a.tiles, t = blockIdx.x / a.tiles;
    const float *p = a.pred + (int64_t)t * a.pred_stride, *g = a.gt + (int64_t)t * a.gt_stride, *e = a.events + (int64_t)t * a.ev_stride;
    double sum_d = 0.0, sum_s = 0.0;
    unsigned n_d = 0, n_s = 0, d1 = 0, d3 = 0, s1 = 0, s3 = 0;
#pragma unroll
    for (int k = 0; k < kFlowPix; ++k) {
        const int i = tile * kFlowTile + k * kMetThreads + tid;
        if (i < a.HW) {
            const float g0 = g[i], g1 = g[i + a.HW];
            const float e0 = p[i] - g0, e1 = p[i + a.HW] - g1;
            float ev = 0.0f;
            for (int c = 0; c < a.C; ++c) ev += fabsf(e[(int64_t)c * a.HW + i]);
            const bool valid = !((g0 != g0) | (g1 != g1) | ((g0 == 0.0f) & (g1 == 0.0f)));
            const bool sparse = valid & (ev > 0.0f);
            const float ee = __builtin_sqrtf(e0 * e0 + e1 * e1);  // correctly rounded (HIP default)
            const unsigned gt1 = ee > 1.0f, gt3 = ee > 3.0f;
            if (valid) {
                sum_d += (double)ee;
                n_d += 1;
                d1 += gt1;
                d3 += gt3;
            }
            if (sparse) {
                sum_s += (double)ee;
                n_s += 1;
                s1 += gt1;
                s3 += gt3;
            }
        }
    }
    const double sd = met_block_sum(sum_d, partd), ss = met_block_sum(sum_s, partd);
    const unsigned long long c0 = met_block_sum((unsigned long long)n_d, partu), c1 = met_block_sum((unsigned long long)n_s, partu);
    const unsigned long long c2 = met_block_sum((unsigned long long)d1, partu), c3 = met_block_sum((unsigned long long)d3, partu);
    const unsigned long long c4 = met_block_sum((unsigned long long)s1, partu), c5 = met_block_sum((unsigned long long)s3, partu);
    if (tid == 0) {
        unsigned long long *slot = a.slots + ((int64_t)t * a.tiles + tile) * kFlowSlots;
        slot[0] = (unsigned long long)__double_as_longlong(sd);
        slot[1] = (unsigned long long)__double_as_longlong(ss);
        slot[2] = c0;
        slot[3] = c1;
        slot[4] = c2;
        slot[5] = c3;
        slot[6] = c4;
        slot[7] = c5;
    }
}

// grid (T), 256 threads.  slots [T][n_slots][NQ] 8-byte words: the first NF of a slot are doubles, the others 64-bit counts.  A chunk of 256
// slots is staged in LDS by the whole workgroup, then thread q adds quantity q of the chunk in slot order.  out_f [T][NF] gets
// sum / den[q] (a division by 1 is exact), out_i [T][NQ - NF] the counts.
template <int NQ, int NF>
__global__ __launch_bounds__(kMetThreads) void metrics_reduce_kernel(const unsigned long long *slots, int64_t n_slots, double den0, double den1, double *out_f,
                                                                     long long *out_i)
{
    static_assert(NF == 2 && NQ >= NF, "two float64 sums lead every slot");
    __shared__ unsigned long long stage[kMetThreads][NQ];
    const int tid = threadIdx.x, t = blockIdx.x;
    const unsigned long long *src = slots + (int64_t)t * n_slots * NQ;
    double facc = 0.0;
    unsigned long long iacc = 0;
    for (int64_t base = 0; base < n_slots; base += kMetThreads) {
        const int n = (int)(n_slots - base < kMetThreads ? n_slots - base : kMetThreads);
        __syncthreads();
        if (tid < n)
#pragma unroll
            for (int q = 0; q < NQ; ++q) stage[tid][q] = src[(base + tid) * NQ + q];
        __syncthreads();
        if (tid < NF)
            for (int k = 0; k < n; ++k) facc += __longlong_as_double((long long)stage[k][tid]);
        else if (tid < NQ)
            for (int k = 0; k < n; ++k) iacc += stage[k][tid];
    }
    if (tid < NF) {
        const double den = tid == 0 ? den0 : den1;
        out_f[(int64_t)t * NF + tid] = facc / den;
    } else if (tid < NQ)
        out_i[(int64_t)t * (NQ - NF) + (tid - NF)] = (long long)iacc;
}

}  // namespace v2v
