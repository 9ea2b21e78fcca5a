// v2v_gcb.hpp -- NER-Net's global context block with the 1x1 convolution in front of it and the residual behind it, and the
// valid-extent helper of the canvas path.  Kernels only; the C entry points are in v2v_nam_tu.hip.
//
// Replaces, of RecurrentConvLayer_NAM_GCB.forward (model/nernet/submodules.py:747-778 of the reference), per image
//     g = Conv2d(C, C, 1)(x)                                     with bias
//     w = softmax over the pixels of Conv2d(C, 1, 1)(g)           ContextBlock2d, pool 'att'
//     ctx[c] = sum_p g[c, p] * w[p]
//     add = Conv2d(C/4, C, 1)(PReLU(LayerNorm([C/4, 1, 1])(Conv2d(C, C/4, 1)(ctx))))       fusion 'channel_add'
//     out = x + g + add                                           add broadcast over the pixels
// by three launches, all float32 arithmetic on the VALU (1 024 to 16 384 multiply-adds per pixel over at most ~10^5 pixels: too small
// for the matrix cores to matter, and float32 operands keep g exact to the reference's precision):
//
//   gcb_tile_kernel<C, false>   a workgroup owns kGcbPix consecutive pixels of one image: g on them, the mask logit, and the tile's
//                               online-softmax partial  (m = max logit, S = sum e^(l - m), V[c] = sum e^(l - m) g[c])  -> workspace
//   gcb_combine_kernel<C>       one workgroup per image: the partials merged in a fixed order, ctx = V / S, the C -> C/4 -> C MLP -> add
//   gcb_tile_kernel<C, true>    g again (the same instructions in the same order), out = bf16(x + g + add)
//
// g is computed twice instead of being kept: a float32 copy costs 4 C bytes per pixel each way, the second pass 2 C flops per byte of it.
// No atomics: every sum has one order, fixed by the shape alone, so two runs agree bit for bit whatever else the GPU runs.
//
// Layouts.  x, out: [B,H,W,C] bf16 (the canvas).  Only pixels with row < Hv and column < Wv (the valid extent) take part in the
// pooling; x is read as zero outside it, out is written as zero outside it.  w1t: float32 [C][C], w1t[ci][co] = conv_1x1.weight[co, ci]
// (transposed once by the caller: lanes own consecutive co).  workspace: float32 [B][tiles][C + 2] = m, S, V[C]; tiles = ceil(H W / kGcbPix).
// ctx_add: float32 [B][2][C] = ctx | add.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace v2v {

constexpr int kGcbPix = 32;              // pixels per workgroup tile
constexpr int kGcbThreads = 256;
constexpr int kGcbXs = kGcbPix + 4;      // LDS pitch of one input channel's pixels (floats): 16-byte aligned rows, rows 4 banks apart

struct GcbArgs {
    const uint16_t *x;
    const float *w1t, *b1, *wmask, *bmask;          // conv_1x1 (transposed), conv_mask [C] and its one bias
    const float *wa, *ba, *ln_w, *ln_b, *prelu;     // channel_add_conv: [C/4][C], [C/4], LayerNorm weight and bias [C/4], PReLU's one slope
    const float *wb, *bb;                           // [C][C/4], [C]
    float *ws, *ctx_add;
    uint16_t *out;
    int B, H, W, Hv, Wv, tiles;
    float eps;
};

__device__ __forceinline__ float gcb_bf16(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ uint16_t gcb_rne(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }

template <int C, bool APPLY>
__global__ void __launch_bounds__(kGcbThreads) gcb_tile_kernel(const GcbArgs a)
{
    constexpr int PPT = C / 8;                       // pixels per work-item: 256 / C pixel groups x PPT = 32
    __shared__ __attribute__((aligned(16))) float xs[C * kGcbXs];       // [ci][pixel]
    __shared__ float gs[APPLY ? 1 : kGcbPix * C];                        // [pixel][co]
    __shared__ float ls[kGcbPix];
    const int t = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int HW = a.H * a.W, p0 = tile * kGcbPix;
    const uint16_t *xb = a.x + (int64_t)b * HW * C;

    // ---- the tile's pixels, as float32, zero outside the valid extent (and past the image) ---------------------------------------
    {
        const int p = t % kGcbPix, pix = p0 + p;
        const bool ok = pix < HW && pix / a.W < a.Hv && pix % a.W < a.Wv;
        for (int c8 = t / kGcbPix; c8 < C / 8; c8 += kGcbThreads / kGcbPix) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ok) v = *reinterpret_cast<const uint4 *>(xb + (int64_t)pix * C + c8 * 8);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                xs[(c8 * 8 + 2 * i) * kGcbXs + p] = __uint_as_float(w[i] << 16);
                xs[(c8 * 8 + 2 * i + 1) * kGcbXs + p] = __uint_as_float(w[i] & 0xFFFF0000u);
            }
        }
    }
    __syncthreads();

    // ---- g[co] on PPT pixels per work-item: ci ascending, one fma per term ---------------------------------------------------------
    const int co = t % C, pg = t / C;
    float acc[PPT];
    {
        const float bias = a.b1[co];
#pragma unroll
        for (int j = 0; j < PPT; ++j) acc[j] = bias;
    }
#pragma unroll 4
    for (int ci = 0; ci < C; ++ci) {
        const float w = a.w1t[ci * C + co];
        const float4 *xr = reinterpret_cast<const float4 *>(&xs[ci * kGcbXs + pg * PPT]);
#pragma unroll
        for (int j = 0; j < PPT / 4; ++j) {
            const float4 v = xr[j];
            acc[4 * j] = fmaf(w, v.x, acc[4 * j]);
            acc[4 * j + 1] = fmaf(w, v.y, acc[4 * j + 1]);
            acc[4 * j + 2] = fmaf(w, v.z, acc[4 * j + 2]);
            acc[4 * j + 3] = fmaf(w, v.w, acc[4 * j + 3]);
        }
    }

    if constexpr (APPLY) {
        const float add = a.ctx_add[((int64_t)b * 2 + 1) * C + co];
        uint16_t *ob = a.out + (int64_t)b * HW * C;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int p = pg * PPT + j, pix = p0 + p;
            if (pix >= HW) break;
            const bool ok = pix / a.W < a.Hv && pix % a.W < a.Wv;
            ob[(int64_t)pix * C + co] = ok ? gcb_rne(xs[co * kGcbXs + p] + acc[j] + add) : (uint16_t)0;
        }
    } else {
#pragma unroll
        for (int j = 0; j < PPT; ++j) gs[(pg * PPT + j) * C + co] = acc[j];
        __syncthreads();
        // the mask logit of pixel p: wave w takes pixels 8 w .. 8 w + 7, a lane its channels in ascending order, then the butterfly
        const int lane = t & 63, wave = t >> 6;
        const float bm = a.bmask[0];
        for (int k = 0; k < kGcbPix / 4; ++k) {
            const int p = wave * (kGcbPix / 4) + k, pix = p0 + p;
            float s = 0.0f;
            for (int c = lane; c < C; c += 64) s = fmaf(a.wmask[c], gs[p * C + c], s);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            const bool ok = pix < HW && pix / a.W < a.Hv && pix % a.W < a.Wv;
            if (lane == 0) ls[p] = ok ? s + bm : -INFINITY;
        }
        __syncthreads();
        if (t < C) {
            float m = -INFINITY;
            for (int p = 0; p < kGcbPix; ++p) m = fmaxf(m, ls[p]);
            float S = 0.0f, V = 0.0f;
            if (m > -INFINITY) {
                for (int p = 0; p < kGcbPix; ++p) {
                    const float e = expf(ls[p] - m);                  // exp(-inf) = 0 for the pixels left out
                    S += e;
                    V = fmaf(e, gs[p * C + t], V);
                }
            }
            float *w = a.ws + ((int64_t)b * a.tiles + tile) * (C + 2);
            if (t == 0) { w[0] = m; w[1] = S; }
            w[2 + t] = V;
        }
    }
}

template <int C>
__global__ void __launch_bounds__(kGcbThreads) gcb_combine_kernel(const GcbArgs a)
{
    constexpr int G = kGcbThreads / C, R = C / 4;    // G work-items per channel, each over the tiles g, g + G, ...
    __shared__ float red[kGcbThreads], redS[G], ctx[C], hid[R], stat[2];
    const int t = threadIdx.x, b = blockIdx.x, c = t % C, g = t / C;
    const float *ws = a.ws + (int64_t)b * a.tiles * (C + 2);

    float m = -INFINITY;                             // the image's largest logit: a maximum has no order
    for (int i = t; i < a.tiles; i += kGcbThreads) m = fmaxf(m, ws[(int64_t)i * (C + 2)]);
    red[t] = m;
    __syncthreads();
    for (int s = kGcbThreads / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmaxf(red[t], red[t + s]);
        __syncthreads();
    }
    m = red[0];
    __syncthreads();

    float S = 0.0f, V = 0.0f;
    for (int i = g; i < a.tiles; i += G) {
        const float *w = ws + (int64_t)i * (C + 2);
        const float f = w[0] > -INFINITY ? expf(w[0] - m) : 0.0f;
        S = fmaf(w[1], f, S);
        V = fmaf(w[2 + c], f, V);
    }
    red[t] = V;
    if (c == 0) redS[g] = S;
    __syncthreads();
    if (t < C) {
        float Vs = 0.0f, Ss = 0.0f;
        for (int k = 0; k < G; ++k) { Vs += red[k * C + t]; Ss += redS[k]; }
        const float v = Vs / Ss;
        ctx[t] = v;
        a.ctx_add[(int64_t)b * 2 * C + t] = v;
    }
    __syncthreads();
    if (t < R) {
        float h = a.ba[t];
        for (int k = 0; k < C; ++k) h = fmaf(a.wa[t * C + k], ctx[k], h);
        hid[t] = h;
    }
    __syncthreads();
    if (t == 0) {                                    // LayerNorm over the C/4 values: mean and biased variance, two passes
        float mu = 0.0f;
        for (int k = 0; k < R; ++k) mu += hid[k];
        mu /= (float)R;
        float var = 0.0f;
        for (int k = 0; k < R; ++k) { const float d = hid[k] - mu; var = fmaf(d, d, var); }
        stat[0] = mu;
        stat[1] = 1.0f / sqrtf(var / (float)R + a.eps);
    }
    __syncthreads();
    if (t < R) {
        const float y = (hid[t] - stat[0]) * stat[1] * a.ln_w[t] + a.ln_b[t];
        hid[t] = y > 0.0f ? y : a.prelu[0] * y;
    }
    __syncthreads();
    if (t < C) {
        float s = a.bb[t];
        for (int k = 0; k < R; ++k) s = fmaf(a.wb[t * R + k], hid[k], s);
        a.ctx_add[((int64_t)b * 2 + 1) * C + t] = s;
    }
}

// ---- the valid-extent helper ------------------------------------------------------------------------------------------------------------
// In place on an NHWC canvas [B,H,W,*] of `pitch16` 16-byte pieces per pixel: a pixel outside the valid extent Hv x Wv is cleared
// (mode 0), or (mode 1) takes the nearest valid pixel when it lies in row Hv or column Wv -- the first row / column outside -- and is
// cleared elsewhere.  Then the x2 upsampling's unclamped 0.75 in[i] + 0.25 in[i + 1] reads, at the last valid row and column, the value
// the reference's clamped index reads.  Sources are valid pixels, which no work-item writes.
__global__ void __launch_bounds__(256) valid_extent_kernel(uint4 *x, int B, int H, int W, int pitch16, int Hv, int Wv, int replicate)
{
    const int64_t n = (int64_t)B * H * W * pitch16, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t pix = i / pitch16;
    const int piece = (int)(i - pix * pitch16);
    const int xw = (int)(pix % W), y = (int)((pix / W) % H);
    const int64_t b = pix / ((int64_t)H * W);
    if (y < Hv && xw < Wv) return;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (replicate && y <= Hv && xw <= Wv) v = x[((b * H + min(y, Hv - 1)) * W + min(xw, Wv - 1)) * pitch16 + piece];
    x[i] = v;
}

}  // namespace v2v
