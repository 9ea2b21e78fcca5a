// v2v_loss.hpp -- the image losses of training (utils/loss.py:6-69 temporal consistency, model/loss.py l1_loss / l2_loss) as device kernels.
//
// Kernels in this file (launched by the C entry points in v2v_loss_tu.hip):
//   tc_loss_fwd_kernel         one launch for a list of images (outer x inner): warp image0 and clamp(processed0) by the flow, visibility mask,
//                              tc_map, |processed1 - image1| and its square; one partial (tc, l1, l2) per workgroup into a fixed slot
//   loss_reduce_kernel         per image: the partials in a fixed order -> weight * mean
//   tc_loss_bwd_kernel         pointwise, recomputes the warp: d tc / d processed1, dwarp = d tc / d warp(processed0), per-image max |dwarp|
//   warp_absmax_kernel         per-image max |dout| for the stand-alone adjoint
//   warp_adjoint_kernel        scatter of dwarp through the bilinear weights into 64-bit fixed point (integer atomics: order-free)
//   warp_adjoint_finish_kernel fixed point -> float32, clamp mask, and the fixed-order sum of everything that reaches one processed image
//   warp_bilinear_kernel       the warp alone
//
// Image list: image (a, b), a < outer, b < inner, lives at element offset a * so + b * si of image1 / processed1; the temporal term exists
// for b >= tc_first, and image0 / processed0 / flow are addressed with b - tc_first (their base pointers point at the first image that has a
// temporal term; flow strides fso / fsi).  Separate [N,C,H,W] tensors: outer = N, inner = 1, tc_first = 0.  Consecutive steps of a
// [B,T,C,H,W] tensor: outer = B, inner = T, tc_first = L0, processed0 = processed1 + (L0 - 1) * si.
// An image is always cut into ceil(H*W / 256) tiles of 256 pixels, whatever else is in the launch, and its partials are summed in one fixed
// order, so a per-image loss does not depend on how many images share the launch.
//
// Arithmetic is float32 throughout, with the reference's sequence of roundings for the sampling position (normalise to [-1, 1], then
// grid_sample's un-normalisation with align_corners = true) and grid_sample's corner weights (nw, ne, sw, se).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v2v {

constexpr int kLossTile = 256;                  // pixels per workgroup = threads per workgroup
constexpr int kLossFixedBits = 38;              // the largest scattered contribution maps to < 2^38; H*W <= 2^22 of them fit an int64

struct LossArgs {
    const float *image0, *image1, *processed0, *processed1, *flow;
    int64_t inner, so, si, fso, fsi, tc_first, n_img;
    int c, h, w, tiles;
    float alpha, flow_sign, w_tc, w_l1, w_l2;
};

#ifdef V2V_LOSS_KERNELS

// ---- sampling position and corner weights ------------------------------------------------------------------------------------------------
struct Bilin {
    int x0, y0;                                 // north-west corner; -2 when no corner is inside the frame
    float wnw, wne, wsw, wse;
    bool nw, ne, sw, se;                        // corner inside the frame
};

__device__ __forceinline__ Bilin bilin_setup(float fx, float fy, int x, int y, int H, int W)
{
    const float gx = (2.0f * ((float)x + fx)) / (float)(W - 1) - 1.0f;
    const float gy = (2.0f * ((float)y + fy)) / (float)(H - 1) - 1.0f;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1);
    const float iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float x1f = x0f + 1.0f, y1f = y0f + 1.0f;
    Bilin b;
    // a NaN or a position further than one pixel outside fails these comparisons: every corner is outside, nothing is read or scattered
    const bool near = x0f >= -1.0f && x0f <= (float)(W - 1) && y0f >= -1.0f && y0f <= (float)(H - 1);
    b.x0 = near ? (int)x0f : -2;
    b.y0 = near ? (int)y0f : -2;
    b.wnw = (x1f - ix) * (y1f - iy);
    b.wne = (ix - x0f) * (y1f - iy);
    b.wsw = (x1f - ix) * (iy - y0f);
    b.wse = (ix - x0f) * (iy - y0f);
    const bool xl = near && b.x0 >= 0, xr = near && b.x0 + 1 <= W - 1, yt = near && b.y0 >= 0, yb = near && b.y0 + 1 <= H - 1;
    b.nw = xl && yt;
    b.ne = xr && yt;
    b.sw = xl && yb;
    b.se = xr && yb;
    return b;
}

template <bool CLAMP>
__device__ __forceinline__ float bilin_tap(const float *p)
{
    const float v = *p;
    return CLAMP ? fminf(fmaxf(v, 0.0f), 255.0f) : v;
}

// grid_sample's sum: nw, ne, sw, se, corners outside the frame contribute nothing
template <bool CLAMP>
__device__ __forceinline__ float bilin_gather(const float *plane, const Bilin &b, int W)
{
    const float *p = plane + (int64_t)b.y0 * W + b.x0;
    float v = 0.0f;
    if (b.nw) v += bilin_tap<CLAMP>(p) * b.wnw;
    if (b.ne) v += bilin_tap<CLAMP>(p + 1) * b.wne;
    if (b.sw) v += bilin_tap<CLAMP>(p + W) * b.wsw;
    if (b.se) v += bilin_tap<CLAMP>(p + W + 1) * b.wse;
    return v;
}

__device__ __forceinline__ float sgnf(float v) { return (float)(v > 0.0f) - (float)(v < 0.0f); }

// wave64 tree, then the four waves of the workgroup through LDS, in a fixed order; the result is valid in thread 0
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o));
    return v;
}

struct LossIndex {
    int64_t img, off1, off0, foff;              // element offsets of this image in image1 / processed1, image0 / processed0, flow
    int pix, x, y;
    bool valid, tc;
};

__device__ __forceinline__ LossIndex loss_index(const LossArgs &a)
{
    LossIndex i;
    i.img = blockIdx.x / a.tiles;
    const int tile = (int)(blockIdx.x % a.tiles);
    const int64_t oa = i.img / a.inner, ob = i.img % a.inner;
    i.pix = tile * kLossTile + (int)threadIdx.x;
    i.valid = i.pix < a.h * a.w;
    i.y = i.pix / a.w;
    i.x = i.pix - i.y * a.w;
    i.tc = a.w_tc != 0.0f && ob >= a.tc_first;  // uniform over the workgroup
    i.off1 = oa * a.so + ob * a.si;
    i.off0 = oa * a.so + (ob - a.tc_first) * a.si;
    i.foff = oa * a.fso + (ob - a.tc_first) * a.fsi;
    return i;
}

__device__ __forceinline__ Bilin loss_bilin(const LossArgs &a, const LossIndex &i)
{
    const int64_t hw = (int64_t)a.h * a.w;
    return bilin_setup(a.flow_sign * a.flow[i.foff + i.pix], a.flow_sign * a.flow[i.foff + hw + i.pix], i.x, i.y, a.h, a.w);
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLossTile) void tc_loss_fwd_kernel(LossArgs a, float *__restrict__ partials, float *__restrict__ m_i0w,
                                                                float *__restrict__ m_p0w, float *__restrict__ m_vis, float *__restrict__ m_err)
{
    __shared__ float red[3][kLossTile / 64];
    const LossIndex i = loss_index(a);
    const int64_t hw = (int64_t)a.h * a.w;
    const bool l12 = a.w_l1 != 0.0f || a.w_l2 != 0.0f;
    float s_tc = 0.0f, s_l1 = 0.0f, s_l2 = 0.0f;
    if (i.valid) {
        Bilin b;
        if (i.tc) b = loss_bilin(a, i);
        for (int ch = 0; ch < a.c; ++ch) {
            const float p1 = a.processed1[i.off1 + ch * hw + i.pix];
            const float i1 = a.image1[i.off1 + ch * hw + i.pix];
            float i0w = 0.0f, p0w = 0.0f, vis = 0.0f, err = 0.0f;
            if (i.tc) {
                i0w = bilin_gather<false>(a.image0 + i.off0 + ch * hw, b, a.w);
                p0w = bilin_gather<true>(a.processed0 + i.off0 + ch * hw, b, a.w);
                const float di = i1 - i0w;
                vis = expf(-a.alpha * (di * di));
                const float div = fabsf(p1) + fabsf(p0w) + 1e-5f;
                err = vis * fabsf(p1 - p0w) / div;
                s_tc += err;
            }
            if (l12) {
                const float d = p1 - i1;
                s_l1 += fabsf(d);
                s_l2 += d * d;
            }
            const int64_t o = (i.img * a.c + ch) * hw + i.pix;
            if (m_i0w) m_i0w[o] = i0w;
            if (m_p0w) m_p0w[o] = p0w;
            if (m_vis) m_vis[o] = vis;
            if (m_err) m_err[o] = err;
        }
    }
    s_tc = wave_sum(s_tc);
    s_l1 = wave_sum(s_l1);
    s_l2 = wave_sum(s_l2);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = s_tc;
        red[1][wave] = s_l1;
        red[2][wave] = s_l2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float s = red[threadIdx.x][0];
#pragma unroll
        for (int k = 1; k < kLossTile / 64; ++k) s += red[threadIdx.x][k];
        partials[(int64_t)blockIdx.x * 3 + threadIdx.x] = s;
    }
}

// one wave per image; losses [3][n_img] = weight * (sum / (c*h*w)), rows tc, l1, l2
__global__ __launch_bounds__(64) void loss_reduce_kernel(const float *__restrict__ partials, float *__restrict__ losses, int64_t n_img, int tiles, float n_elems,
                                                         float w_tc, float w_l1, float w_l2)
{
    const int64_t img = blockIdx.x;
    const float *p = partials + img * tiles * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float s = 0.0f;
        for (int t = threadIdx.x; t < tiles; t += 64) s += p[(int64_t)t * 3 + k];
        s = wave_sum(s);
        const float wgt = k == 0 ? w_tc : k == 1 ? w_l1 : w_l2;
        if (threadIdx.x == 0) losses[k * n_img + img] = wgt != 0.0f ? wgt * (s / n_elems) : 0.0f;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------------
// the upstream coefficient of one element of a per-image mean: (g * weight) / (c*h*w)
__device__ __forceinline__ float loss_coeff(float g, float wgt, float n_elems) { return (g * wgt) / n_elems; }
__device__ __forceinline__ float l1_term(float k, float p1, float i1) { return k * sgnf(p1 - i1); }
__device__ __forceinline__ float l2_term(float k, float p1, float i1) { return k * (2.0f * (p1 - i1)); }

__global__ __launch_bounds__(kLossTile) void tc_loss_bwd_kernel(LossArgs a, const float *__restrict__ gout, float *__restrict__ dp1, float *__restrict__ dwarp,
                                                                unsigned *__restrict__ maxbits)
{
    const LossIndex i = loss_index(a);
    if (!i.tc) return;
    const int64_t hw = (int64_t)a.h * a.w;
    float mx = 0.0f;
    if (i.valid) {
        const float k = loss_coeff(gout[i.img], a.w_tc, (float)(a.c * hw));
        const Bilin b = loss_bilin(a, i);
        for (int ch = 0; ch < a.c; ++ch) {
            const float p1 = a.processed1[i.off1 + ch * hw + i.pix];
            const float i1 = a.image1[i.off1 + ch * hw + i.pix];
            const float i0w = bilin_gather<false>(a.image0 + i.off0 + ch * hw, b, a.w);
            const float p0w = bilin_gather<true>(a.processed0 + i.off0 + ch * hw, b, a.w);
            const float di = i1 - i0w;
            const float vis = expf(-a.alpha * (di * di));
            const float d = p1 - p0w;
            const float num = vis * fabsf(d);
            const float div = fabsf(p1) + fabsf(p0w) + 1e-5f;
            const float g_abs = (k / div) * vis;                    // d / d |processed1 - warp|
            const float g_div = -(k * num) / (div * div);           // d / d div
            const float sd = sgnf(d);
            const float g1 = g_abs * sd + g_div * sgnf(p1);
            const float gw = g_div * sgnf(p0w) - g_abs * sd;
            const int64_t o = (i.img * a.c + ch) * hw + i.pix;
            dp1[o] = g1;
            dwarp[o] = gw;
            mx = fmaxf(mx, fabsf(gw));
        }
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx > 0.0f) atomicMax(maxbits + i.img, __float_as_uint(mx));   // non-negative floats order like their bits
}

__global__ __launch_bounds__(kLossTile) void warp_absmax_kernel(const float *__restrict__ v, int64_t per_img, unsigned *__restrict__ maxbits)
{
    const int64_t img = blockIdx.y;
    float mx = 0.0f;
    for (int64_t k = (int64_t)blockIdx.x * kLossTile + threadIdx.x; k < per_img; k += (int64_t)gridDim.x * kLossTile) mx = fmaxf(mx, fabsf(v[img * per_img + k]));
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx > 0.0f) atomicMax(maxbits + img, __float_as_uint(mx));
}

// Fixed point of one image: max |v| < 2^(e - 126) for the biased exponent e of the maximum, so v * 2^(164 - e) < 2^38.  The power is
// capped at 127 (a maximum below 2^-89, zero included); an infinite maximum gives 0: the image's gradient is then NaN (finish kernel).
__device__ __forceinline__ int loss_fixed_exp(unsigned mb)
{
    const int e = (int)(mb >> 23);
    return e >= 255 ? 0 : min(kLossFixedBits + 126 - e, 127);
}

__device__ __forceinline__ void fixed_add(unsigned long long *acc, float v, float scale)
{
    const long long q = __float2ll_rn(v * scale);
    if (q != 0) atomicAdd(acc, (unsigned long long)q);
}

// grid: (a.n_img * a.tiles) workgroups over images in the LossArgs numbering when a.flow strides apply (images without a temporal term
// return), or over n plain images when a.inner == 1 and a.tc_first == 0
__global__ __launch_bounds__(kLossTile) void warp_adjoint_kernel(LossArgs a, const float *__restrict__ dwarp, const unsigned *__restrict__ maxbits,
                                                                 unsigned long long *__restrict__ acc)
{
    const LossIndex i = loss_index(a);
    if (!i.tc || !i.valid) return;
    const int64_t hw = (int64_t)a.h * a.w;
    const unsigned mb = maxbits[i.img];
    if (mb == 0 || mb >= 0x7f800000u) return;
    const float scale = __uint_as_float((unsigned)(loss_fixed_exp(mb) + 127) << 23);
    const Bilin b = loss_bilin(a, i);
    if (!(b.nw || b.ne || b.sw || b.se)) return;
    for (int ch = 0; ch < a.c; ++ch) {
        const int64_t o = (i.img * a.c + ch) * hw;
        const float g = dwarp[o + i.pix];
        unsigned long long *p = acc + o + (int64_t)b.y0 * a.w + b.x0;
        if (b.nw) fixed_add(p, g * b.wnw, scale);
        if (b.ne) fixed_add(p + 1, g * b.wne, scale);
        if (b.sw) fixed_add(p + a.w, g * b.wsw, scale);
        if (b.se) fixed_add(p + a.w + 1, g * b.wse, scale);
    }
}

__device__ __forceinline__ float fixed_to_float(unsigned long long v, unsigned mb)
{
    if (mb >= 0x7f800000u) return __uint_as_float(0x7fc00000u);
    return ldexpf((float)(long long)v, -loss_fixed_exp(mb));        // one rounding (int64 -> float32), then an exact power of two
}

// Everything that reaches one processed image, summed in the order autograd accumulates it when the step loop calls l1, l2, temporal
// consistency in that order: what the NEXT step scattered into it (clamp-masked), + its own temporal term, + l2, + l1.
// chain == 0: the scatter goes to dprocessed0 (addressed like processed0) instead and dprocessed1 gets the other three.
__global__ __launch_bounds__(kLossTile) void warp_adjoint_finish_kernel(LossArgs a, const float *__restrict__ gout, int chain, const unsigned long long *__restrict__ acc,
                                                                        const float *__restrict__ dp1, const unsigned *__restrict__ maxbits,
                                                                        float *__restrict__ dprocessed1, float *__restrict__ dprocessed0)
{
    const LossIndex i = loss_index(a);
    if (!i.valid) return;
    const int64_t hw = (int64_t)a.h * a.w;
    const float n_elems = (float)(a.c * hw);
    const int64_t ob = i.img % a.inner;
    const bool have_tc = a.w_tc != 0.0f;
    // chain: image (a, b + 1) scattered into this one
    const bool from_next = chain && have_tc && ob + 1 < a.inner && ob + 1 >= a.tc_first;
    const float k1 = a.w_l1 != 0.0f ? loss_coeff(gout[a.n_img + i.img], a.w_l1, n_elems) : 0.0f;
    const float k2 = a.w_l2 != 0.0f ? loss_coeff(gout[2 * a.n_img + i.img], a.w_l2, n_elems) : 0.0f;
    for (int ch = 0; ch < a.c; ++ch) {
        const int64_t o = (i.img * a.c + ch) * hw + i.pix;
        const float p1 = a.processed1[i.off1 + ch * hw + i.pix];
        float g = 0.0f;
        bool any = false;
        if (from_next) {
            g = fixed_to_float(acc[o + a.c * hw], maxbits[i.img + 1]);
            if (!(p1 >= 0.0f && p1 <= 255.0f)) g = 0.0f;
            any = true;
        }
        if (i.tc) {
            const float t = dp1[o];
            g = any ? g + t : t;
            any = true;
            if (!chain) {
                float g0 = fixed_to_float(acc[o], maxbits[i.img]);
                const float p0 = a.processed0[i.off0 + ch * hw + i.pix];
                if (!(p0 >= 0.0f && p0 <= 255.0f)) g0 = 0.0f;
                dprocessed0[i.off0 + ch * hw + i.pix] = g0;
            }
        }
        if (a.w_l2 != 0.0f) {
            const float t = l2_term(k2, p1, a.image1[i.off1 + ch * hw + i.pix]);
            g = any ? g + t : t;
            any = true;
        }
        if (a.w_l1 != 0.0f) {
            const float t = l1_term(k1, p1, a.image1[i.off1 + ch * hw + i.pix]);
            g = any ? g + t : t;
            any = true;
        }
        dprocessed1[i.off1 + ch * hw + i.pix] = g;
    }
}

// ---- the warp and its adjoint alone: n contiguous [c,h,w] images, flow [n,2,h,w] ------------------------------------------------------
__global__ __launch_bounds__(kLossTile) void warp_bilinear_kernel(LossArgs a, const float *__restrict__ img, float *__restrict__ out)
{
    const LossIndex i = loss_index(a);
    if (!i.valid) return;
    const int64_t hw = (int64_t)a.h * a.w;
    const Bilin b = loss_bilin(a, i);
    for (int ch = 0; ch < a.c; ++ch) {
        const int64_t o = (i.img * a.c + ch) * hw;
        out[o + i.pix] = bilin_gather<false>(img + o, b, a.w);
    }
}

__global__ __launch_bounds__(kLossTile) void warp_adjoint_plain_finish_kernel(const unsigned long long *__restrict__ acc, const unsigned *__restrict__ maxbits,
                                                                              int64_t per_img, int64_t total, float *__restrict__ din)
{
    const int64_t k = (int64_t)blockIdx.x * kLossTile + threadIdx.x;
    if (k < total) din[k] = fixed_to_float(acc[k], maxbits[k / per_img]);
}

#endif  // V2V_LOSS_KERNELS

}  // namespace v2v
