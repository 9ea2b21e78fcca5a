// v2v_alex_train.hpp -- LPIPS-AlexNet as a training loss: the backward to the prediction, float32 NHWC like the forward
// of v2v_alex.hpp, whose activations it reads.
//
//   alex_compare_bwd_kernel   two taps, the lin weights and d dist -> the gradient at the pred tap, per pixel in float64, rounded once
//   alex_dgrad_kernel         input gradient of a stride-1 KS x KS convolution: alex_conv_kernel's main loop over the flipped, transposed
//                             weights, epilogue  dx = acc + dtap, 0 where the saved post-ReLU activation is not > 0
//   alex_pool_bwd_kernel      3x3 / stride 2 max-pool backward as a gather over the up to four windows of an input pixel
//   alex_stem_bwd_kernel      11x11 / stride 4 / pad 2 transposed convolution to the image, explicit fmaf, then the scaling layer's chain
//
// No float atomics and no split-K: every output element is summed by one thread (or one wave) in one fixed order, so a frame's bits do
// not depend on what shares its launch, and two runs agree bit for bit.
#pragma once
#include "v2v_alex_tile.hpp"

namespace v2v {

// grid (tiles, n), 256 threads; the forward's tiling: a workgroup takes 64 pixels of one image, wave w pixels 16 w .. 16 w + 15 one after
// another, a lane the channels lane, lane + 64, ...  Per pixel, in float64:
//   s0 = sum_c f0_c^2, r0 = sqrt(s0), n0 = r0 + 1e-10 (n1 likewise);  g_c = 2 w_c (f0_c / n0 - f1_c / n1) * (ddist / HW)
//   df0_c = g_c / n0 - f0_c * (sum_k g_k f0_k) / (r0 * n0^2)        the second term is 0 where r0 == 0 (the reference: NaN)
// rounded to float32 once; relu_mask: 0 where f0_c is not > 0 (f0 is a post-ReLU activation: the gradient at the pre-activation).
template <int NC>
__global__ __launch_bounds__(kAlexThreads) void alex_compare_bwd_kernel(const float *__restrict__ f0, const float *__restrict__ f1, const float *__restrict__ w,
                                                                        const float *__restrict__ ddist, int HW, int relu_mask, float *__restrict__ dz)
{
    constexpr int C = NC * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tile = blockIdx.x, img = blockIdx.y;
    double wc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) wc[k] = (double)w[lane + 64 * k];
    const double sc = (double)ddist[img] / (double)HW;
    for (int i = 0; i < kAlexCmpPix / 4; ++i) {
        const int p = tile * kAlexCmpPix + wave * (kAlexCmpPix / 4) + i;
        if (p >= HW) break;   // uniform over the wave
        const int64_t at = ((int64_t)img * HW + p) * C + lane;
        double x0[NC], x1[NC], s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            x0[k] = (double)f0[at + 64 * k];
            x1[k] = (double)f1[at + 64 * k];
            s0 += x0[k] * x0[k];
            s1 += x1[k] * x1[k];
        }
        s0 = __shfl(alex_wave_sum(s0), 0);
        s1 = __shfl(alex_wave_sum(s1), 0);
        const double r0 = __builtin_sqrt(s0), n0 = r0 + 1e-10, n1 = __builtin_sqrt(s1) + 1e-10;
        double g[NC], dot = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            g[k] = 2.0 * wc[k] * (x0[k] / n0 - x1[k] / n1) * sc;
            dot += g[k] * x0[k];
        }
        dot = __shfl(alex_wave_sum(dot), 0);
        const double second = r0 > 0.0 ? dot / (r0 * (n0 * n0)) : 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            float v = (float)(g[k] / n0 - x0[k] * second);
            if (relu_mask && !(x0[k] > 0.0)) v = 0.0f;
            dz[at + 64 * k] = v;
        }
    }
}

// dx = acc + dtap (dtap may be null), 0 where mask is not > 0 (mask may be null); dtap and mask are [M][Cout] like dx
struct AlexDgradEpilogue {
    const float *dtap, *mask;
    __device__ __forceinline__ void operator()(const AlexConvArgs &a, int m, int ch, float s0, float s1) const
    {
        const int64_t at = (int64_t)m * a.Cout + ch;
        float v0 = s0, v1 = s1;
        if (dtap) {
            v0 += dtap[at];
            v1 += dtap[at + 32];
        }
        if (mask) {
            v0 = mask[at] > 0.0f ? v0 : 0.0f;
            v1 = mask[at + 32] > 0.0f ? v1 : 0.0f;
        }
        a.y[at] = v0;
        a.y[at + 32] = v1;
    }
};

// grid (ceil(M / 128), Cout / 64), 256 threads.  a.x = dy [M][Cin], a.w = the dgrad pack [KS * KS * Cin][Cout] (Cin: the forward's output
// channels, Cout: its input channels), a.y = dx [M][Cout]; a.bias and a.relu are not read.
template <int KS>
__global__ __launch_bounds__(kAlexThreads) void alex_dgrad_kernel(const AlexConvArgs a, const float *__restrict__ dtap, const float *__restrict__ mask)
{
    alex_conv_tile<KS>(a, AlexDgradEpilogue{dtap, mask});
}

// one thread per four channels of an INPUT pixel; total = n * H * W * C / 4.  The windows (oy, ox) that hold pixel (iy, ix) are
// oy in {(iy - 1) / 2, iy / 2} (one of them for iy == 0 and for even iy's lower neighbour out of range), ox likewise: up to four.  The
// pixel takes dy of a window when it is the window's arg-max as torch finds it: scanning row-major, a later value replaces the maximum
// only when strictly larger -- so every value before the pixel must be smaller and none after it larger.  Rows and columns that floor
// mode drops lie in no window and get dtap only.  Then + dtap (may be null), and 0 where the pixel's own value is not > 0 when relu_mask.
__global__ __launch_bounds__(kAlexThreads) void alex_pool_bwd_kernel(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ dtap, int H,
                                                                     int W, int OH, int OW, int C, int relu_mask, int64_t total, float *__restrict__ dx)
{
    const int64_t i = (int64_t)blockIdx.x * kAlexThreads + threadIdx.x;
    if (i >= total) return;
    const int c4 = C / 4;
    const int q = (int)(i % c4);
    int64_t p = i / c4;
    const int ix = (int)(p % W);
    p /= W;
    const int iy = (int)(p % H);
    const int64_t img = p / H;
    const float *xi = x + img * H * W * C + q * 4;
    const float4 v = *reinterpret_cast<const float4 *>(x + i * 4);
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int oy_lo = iy > 0 ? (iy - 1) / 2 : 0, oy_hi = iy / 2 < OH ? iy / 2 : OH - 1;
    const int ox_lo = ix > 0 ? (ix - 1) / 2 : 0, ox_hi = ix / 2 < OW ? ix / 2 : OW - 1;
    for (int oy = oy_lo; oy <= oy_hi; ++oy)
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            const int mine = (iy - 2 * oy) * 3 + (ix - 2 * ox);   // the pixel's place in the window's row-major scan, 0..8
            bool tx = true, ty = true, tz = true, tw = true;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float4 o = *reinterpret_cast<const float4 *>(xi + ((int64_t)(2 * oy + k / 3) * W + 2 * ox + k % 3) * C);
                if (k < mine) {
                    tx = tx && o.x < v.x;
                    ty = ty && o.y < v.y;
                    tz = tz && o.z < v.z;
                    tw = tw && o.w < v.w;
                } else if (k > mine) {
                    tx = tx && !(o.x > v.x);
                    ty = ty && !(o.y > v.y);
                    tz = tz && !(o.z > v.z);
                    tw = tw && !(o.w > v.w);
                }
            }
            const float4 d = *reinterpret_cast<const float4 *>(dy + (((img * OH + oy) * OW + ox) * C) + q * 4);
            acc.x += tx ? d.x : 0.0f;
            acc.y += ty ? d.y : 0.0f;
            acc.z += tz ? d.z : 0.0f;
            acc.w += tw ? d.w : 0.0f;
        }
    if (dtap) {
        const float4 t = *reinterpret_cast<const float4 *>(dtap + i * 4);
        acc.x += t.x;
        acc.y += t.y;
        acc.z += t.z;
        acc.w += t.w;
    }
    if (relu_mask) {
        acc.x = v.x > 0.0f ? acc.x : 0.0f;
        acc.y = v.y > 0.0f ? acc.y : 0.0f;
        acc.z = v.z > 0.0f ? acc.z : 0.0f;
        acc.w = v.w > 0.0f ? acc.w : 0.0f;
    }
    *reinterpret_cast<float4 *>(dx + i * 4) = acc;
}

// stem backward: a workgroup takes 32 x 32 input pixels.  The output pixels (oy, ox) that reach them, 4 oy - 2 + ky = iy with ky in 0..10,
// are the 11 x 11 from (iy0 / 4 - 2, ix0 / 4 - 2) on: their dz is staged in LDS once (zero outside the map), rows of 64 + 4 floats so that
// the b128 reads of 16 lanes fall on distinct banks.  The weights of ONE input channel, [121][64] (the forward's pack), are staged per
// channel.  A wave works on one phase (iy & 3, ix & 3) at a time -- its 64 lanes are the 8 x 8 pixels of the tile with that phase -- so
// that ky, kx and with them the weight address are the same for all lanes: a broadcast read.
constexpr int kAlexSbTile = 32;                       // input pixels per side of a workgroup's tile
constexpr int kAlexSbOut = kAlexSbTile / 4 + 3;       // 11 output rows / columns reach a tile
constexpr int kAlexSbPitch = kAlexBN + 4;             // floats per staged dz pixel

// grid (tiles_x * tiles_y, n), 256 threads.  Per input pixel and input channel c, in this order: ky ascending, kx ascending, then the 64
// output channels as four fmaf chains (o & 3), added as (s0 + s1) + (s2 + s3).  Then in float32: / scale[c]; for a one-channel image the
// three channels are added in channel order; * 2 when normalize; / divisor when it is not 1.
__global__ __launch_bounds__(kAlexThreads) void alex_stem_bwd_kernel(const float *__restrict__ dz, const float *__restrict__ w, const float *__restrict__ scale, int cin,
                                                                     int H, int W, int OH, int OW, int tiles_x, float divisor, int normalize, float *__restrict__ dpred)
{
    __shared__ __attribute__((aligned(16))) float Ds[kAlexSbOut * kAlexSbOut][kAlexSbPitch];
    __shared__ __attribute__((aligned(16))) float Ws[kAlexStemK][kAlexBN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x, img = blockIdx.y;
    const int ix0 = bx * kAlexSbTile, iy0 = by * kAlexSbTile;
    const int ox0 = ix0 / 4 - 2, oy0 = iy0 / 4 - 2;
    const float *src = dz + (int64_t)img * OH * OW * kAlexBN;
    for (int i = tid; i < kAlexSbOut * kAlexSbOut * (kAlexBN / 4); i += kAlexThreads) {
        const int pix = i / (kAlexBN / 4), q = i - pix * (kAlexBN / 4);
        const int oy = oy0 + pix / kAlexSbOut, ox = ox0 + pix % kAlexSbOut;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (oy >= 0 && oy < OH && ox >= 0 && ox < OW) v = *reinterpret_cast<const float4 *>(src + ((int64_t)oy * OW + ox) * kAlexBN + q * 4);
        *reinterpret_cast<float4 *>(&Ds[pix][q * 4]) = v;
    }
    const int la = lane >> 3, lb = lane & 7;          // the lane's pixel of a phase: (iy0 + 4 la + py, ix0 + 4 lb + px)
    float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f};          // cin == 1: the sum over the channels, per phase of this wave
    for (int c = 0; c < 3; ++c) {
        __syncthreads();
        const float4 *wc = reinterpret_cast<const float4 *>(w + (int64_t)c * kAlexStemKP * kAlexBN);
        for (int i = tid; i < kAlexStemK * (kAlexBN / 4); i += kAlexThreads) *reinterpret_cast<float4 *>(&Ws[0][0] + i * 4) = wc[i];
        __syncthreads();
        const float sc = scale[c];
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) {
            const int phase = wave * 4 + ph, py = phase >> 2, px = phase & 3;
            const int ry = (py + 2) & 3, qy = (py + 2) >> 2, rx = (px + 2) & 3, qx = (px + 2) >> 2;
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
            for (int j = 0; j < 3; ++j) {
                const int ky = ry + 4 * j;
                if (ky >= kAlexStemKS) break;   // uniform over the wave
                const int row = la + qy - j + 2;
                for (int jj = 0; jj < 3; ++jj) {
                    const int kx = rx + 4 * jj;
                    if (kx >= kAlexStemKS) break;
                    const int col = lb + qx - jj + 2;
                    const float *d = &Ds[row * kAlexSbOut + col][0];
                    const float *wk = &Ws[ky * kAlexStemKS + kx][0];
#pragma unroll
                    for (int o = 0; o < kAlexBN; o += 4) {
                        const float4 dv = *reinterpret_cast<const float4 *>(d + o), wv = *reinterpret_cast<const float4 *>(wk + o);
                        s0 = __builtin_fmaf(wv.x, dv.x, s0);
                        s1 = __builtin_fmaf(wv.y, dv.y, s1);
                        s2 = __builtin_fmaf(wv.z, dv.z, s2);
                        s3 = __builtin_fmaf(wv.w, dv.w, s3);
                    }
                }
            }
            const float t = ((s0 + s1) + (s2 + s3)) / sc;
            if (cin == 1) {
                tot[ph] = c == 0 ? t : tot[ph] + t;
                if (c < 2) continue;
            }
            float v = cin == 1 ? tot[ph] : t;
            if (normalize) v = 2.0f * v;
            if (divisor != 1.0f) v = v / divisor;
            const int iy = iy0 + 4 * la + py, ix = ix0 + 4 * lb + px;
            if (iy < H && ix < W) dpred[(((int64_t)img * cin + (cin == 1 ? 0 : c)) * H + iy) * W + ix] = v;
        }
    }
}

}  // namespace v2v
