// v2v_hyper.hpp -- HyperE2VID's per-pixel dynamic decoder (model/hyper_model.py:33-60, model/hyper/hyper_dynamic.py) on gfx950.
//
// The layer replaces decoders[0] of the recurrent UNet:  y = relu(DynamicConv(up2(x + skip), atoms(context(events, prev_image)))).
// Kernels in this file (launched by the C entry points in v2v_hyper_tu.hip; the training kernels further down by those in v2v_hyper_train_tu.hip):
//   hyper_context_kernel   cat(events, prev_recs) bilinearly downsampled x1/4 -> bf16 NHWC8 (the head kernel's input layout); for the exact
//                          factor 4 the source coordinate 4 d + 1.5 gives weights 1/2, 1/2 on pixels 4 d + 1, 4 d + 2 of either axis: the
//                          mean of the central 2 x 2 of every 4 x 4 block (checked against the golden's `layer__context`)
//   hyper_context_conv_kernel   context_fusion.conv: 3 x 3, <= 8 -> 32 channels on that layout, float32 FMAs on bf16-rounded operands; any h, w
//                          (the head kernel's 16 x 16 tiles need H and W multiples of 64 at this scale: 192 x 240 gives a 48 x 60 context)
//   hyper_tanh_kernel      element-wise tanh on bf16 (bases_net's first activation; the convolutions' epilogue only knows ReLU)
//   hyper_atoms_kernel     72 pre-activation coefficients (bf16 NHWC, padded to 128) -> tanh -> atoms[p][l][m] = sum_k coeff[m,k] bases[k,l],
//                          float32 [B,h,w,25,6] (tap-major: the six atoms of one tap are 24 consecutive bytes for the kernel below)
//   hyper_dynconv_kernel   the dynamic convolution, below
//   hyper_dynconv_pack_kernel   compositional_coefficients float32 [128, 256 * 6] (column c * 6 + m) -> wp[chunk = cb * 6 + m][128 columns][64 k]
//                          bf16, k <-> channel cb * 64 + k: every 64-wide K chunk is ONE atom over 64 channels
//
// hyper_dynconv_kernel.  For output pixel p:  F[c,m] = sum_l atoms_p[m,l] X[c, p + offset_l]  (5 x 5 window, zero padding), then
// y[o] = relu(bias[o] + sum_{c,m} W[o, c * 6 + m] F[c,m]).  The stock graph unfolds X (25 x the input) and writes F in float32; here
// neither exists: a lane builds F for ITS pixel and 8 channels with float32 FMAs, rounds it to bf16 and holds it in registers as the A
// operand of v_mfma_f32_32x32x16_bf16 -- a lane's A fragment is (row = pixel lane & 31, k = 8 (lane >> 5) .. + 7), i.e. exactly one pixel x
// 8 consecutive channels -- so F never touches LDS or HBM.  One X read (ds_read_b128, 8 channels of one tap) feeds all six atoms: 48
// accumulators, 25 taps, 1200 FMAs per lane and k-step, followed by 6 x 4 MFMAs (6 atoms = 6 K chunks, 4 x 32 output columns).
// Workgroup = 8 rows x 16 columns of pixels, 8 waves: wave (kg, w) owns pixel rows 2 w, 2 w + 1 (32 pixels) x all 128 columns for HALF
// of K -- group kg walks channel blocks 2 it + kg, it = 0, 1 -- and group 1's accumulators meet group 0's through LDS before the epilogue
// (a fixed order: deterministic).  The kernel is bound by the vector FMAs (38.4 k per pixel against 196.6 k matrix-core MACs that cost
// 30 x less per MAC), so two waves per SIMD share the vector unit while one waits for LDS.
// LDS: two halo patches (12 x 20 pixels x 64 channels; pixel stride 144 B = 9 sixteen-byte units, patch-row stride 3,072 B = 0 mod 256: a
// ds_read_b128 is served in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, .. -- 8 pixels of one tile row and the OTHER 8 columns of
// the next -- whose unit indices 9 c are then 16 distinct values mod 16, all 64 banks once, without a swizzle) = 73,728 B, and the tile's
// atoms, 128 pixels x 150 float32 (pixel stride 150 words = 22 mod 64: 32 pixels' 8-byte reads cover the 64 banks once) = 76,800 B.  B fragments come straight from the
// packed weights in global memory (393 KB, L2-resident; 16 bytes per lane and MFMA group).
// Partial tiles (H % 8, W % 16) read zeros and store nothing outside the image.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v2v {

constexpr int kHyCin = 256, kHyCout = 128, kHyAtoms = 6, kHyTaps = 25, kHyCoeff = 72, kHyCoeffPad = 128, kHyBases = 12;
constexpr int kHyAtomElems = kHyAtoms * kHyTaps;                         // 150 float32 per pixel

#if defined(V2V_HYPER_KERNELS) || defined(V2V_HYPER_TRAIN_KERNELS)   // what the forward and the backward kernels share

typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 hy_bf16x8;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float hy_f32x16;
typedef __bf16 hy_hwbf16x2 __attribute__((ext_vector_type(2)));
typedef float hy_f32x2 __attribute__((ext_vector_type(2)));

// float -> bf16, round to nearest even (v_cvt_pk_bf16_f32), two values per instruction
__device__ __forceinline__ uint32_t hy_pack_bf16(float lo, float hi)
{
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(hy_f32x2{lo, hi}, hy_hwbf16x2));
}
__device__ __forceinline__ float hy_bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float hy_bf16_hi(uint32_t u) { return __uint_as_float(u & 0xFFFF0000u); }
// tanh on the hardware exp2 / rcp (1 ulp each; exact saturation: exp2(+inf) -> rcp = 0 -> -1, exp2(-inf) = 0 -> 2 - 1 = 1)
__device__ __forceinline__ float hy_tanh(float v) { return 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -2.8853900817779268f)) - 1.0f; }

// the dynamic convolution's tile and halo patch (forward and backward)
constexpr int kHyTH = 8, kHyTW = 16, kHyPW = kHyTW + 4, kHyPH = kHyTH + 4, kHyNP = kHyPW * kHyPH;   // tile, halo patch (240 pixels)
constexpr int kHyPixB = 144;                                             // bytes per halo pixel: 64 channels + 16 (bank spread)
constexpr int kHyRowB = 3072;                                            // bytes per patch row: 20 pixels (2,880), padded to 0 mod 256
constexpr int kHyPatchB = kHyPH * kHyRowB;                               // 36,864
static_assert(kHyPW * kHyPixB <= kHyRowB && kHyRowB % 256 == 0, "patch row pitch");

#endif
#ifdef V2V_HYPER_KERNELS

// ---- context staging: events [B,C,H,W] float32 (any element strides) | prev [B,H,W] float32 -> bf16 [B,H/4,W/4,8], channels C+1..7 zero ----
__global__ void __launch_bounds__(256) hyper_context_kernel(const float *ev, int64_t sb, int64_t sc, int64_t sh, int64_t sw, const float *prev, uint16_t *dst,
                                                            int B, int C, int H, int W)
{
    const int h = H >> 2, w = W >> 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * h * w) return;
    const int x = (int)(i % w), y = (int)((i / w) % h), b = (int)(i / ((int64_t)w * h));
    const int iy = 4 * y + 1, ix = 4 * x + 1;
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        v[c] = 0.0f;
        if (c < C) {
            const float *p = ev + b * sb + c * sc + iy * sh + ix * sw;
            // the interpolation's own order: the two columns of a row blended first (0.5, 0.5), then the two rows
            v[c] = 0.5f * (0.5f * p[0] + 0.5f * p[sw]) + 0.5f * (0.5f * p[sh] + 0.5f * p[sh + sw]);
        } else if (c == C) {
            const float *p = prev + ((int64_t)b * H + iy) * W + ix;
            v[c] = 0.5f * (0.5f * p[0] + 0.5f * p[1]) + 0.5f * (0.5f * p[W] + 0.5f * p[W + 1]);
        }
    }
    *reinterpret_cast<uint4 *>(dst + i * 8) = make_uint4(hy_pack_bf16(v[0], v[1]), hy_pack_bf16(v[2], v[3]), hy_pack_bf16(v[4], v[5]), hy_pack_bf16(v[6], v[7]));
}

// ---- context_fusion.conv: x8 bf16 [B,h,w,8] -> bf16 [B,h,w,32] = conv3x3(x, pad 1) + bias; weight float32 [32,Cin,3,3] rounded to bf16 as the
// matrix-core layers round theirs.  One work-item per (pixel, 8 output channels): 9 taps x 8 x 8 FMAs; 1728 MACs per pixel at 1/16 of the
// image's pixels -- far too little for a matrix-core tile, and free of the head kernel's 16 x 16 tiling ----
__global__ void __launch_bounds__(256) hyper_context_conv_kernel(const uint16_t *x8, const float *w, const float *bias, uint16_t *out, int B, int h, int wd, int Cin)
{
    __shared__ float wl[9 * 8 * 32];                                      // [tap][c][o], zero for c >= Cin
    for (int i = threadIdx.x; i < 9 * 8 * 32; i += 256) {
        const int o = i & 31, c = (i >> 5) & 7, tap = i >> 8;
        const float v = c < Cin ? w[(o * Cin + c) * 9 + tap] : 0.0f;
        wl[i] = hy_bf16_lo(hy_pack_bf16(v, v));
    }
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int og = (int)(idx & 3);
    const int64_t p = idx >> 2;
    if (p >= (int64_t)B * h * wd) return;
    const int x = (int)(p % wd), y = (int)((p / wd) % h);
    float acc[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[o] = 0.0f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        if ((unsigned)(y + dy) >= (unsigned)h || (unsigned)(x + dx) >= (unsigned)wd) continue;
        const uint4 xv = *reinterpret_cast<const uint4 *>(x8 + (p + dy * wd + dx) * 8);
        const float xf[8] = {hy_bf16_lo(xv.x), hy_bf16_hi(xv.x), hy_bf16_lo(xv.y), hy_bf16_hi(xv.y), hy_bf16_lo(xv.z), hy_bf16_hi(xv.z), hy_bf16_lo(xv.w), hy_bf16_hi(xv.w)};
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int o = 0; o < 8; ++o) acc[o] = fmaf(xf[c], wl[(tap * 8 + c) * 32 + og * 8 + o], acc[o]);
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[o] += bias[og * 8 + o];
    *reinterpret_cast<uint4 *>(out + p * 32 + og * 8) = make_uint4(hy_pack_bf16(acc[0], acc[1]), hy_pack_bf16(acc[2], acc[3]), hy_pack_bf16(acc[4], acc[5]), hy_pack_bf16(acc[6], acc[7]));
}

// ---- element-wise tanh on bf16, 8 values per work-item (out may be x) ----
__global__ void __launch_bounds__(256) hyper_tanh_kernel(const uint16_t *x, uint16_t *out, int64_t n8)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const uint4 u = *reinterpret_cast<const uint4 *>(x + i * 8);
    const uint32_t in[4] = {u.x, u.y, u.z, u.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = hy_pack_bf16(hy_tanh(hy_bf16_lo(in[j])), hy_tanh(hy_bf16_hi(in[j])));
    *reinterpret_cast<uint4 *>(out + i * 8) = make_uint4(o[0], o[1], o[2], o[3]);
}

// ---- atoms: one work-item per (pixel, atom m): 12 coefficients -> tanh -> 25 taps, float32 ----
__global__ void __launch_bounds__(256) hyper_atoms_kernel(const uint16_t *coeff, const float *bases, float *atoms, int64_t M)
{
    __shared__ float bl[kHyBases * kHyTaps];
    for (int i = threadIdx.x; i < kHyBases * kHyTaps; i += 256) bl[i] = bases[i];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * kHyAtoms) return;
    const int64_t p = i / kHyAtoms;
    const int m = (int)(i - p * kHyAtoms);
    float cf[kHyBases];
#pragma unroll
    for (int k = 0; k < kHyBases; ++k) cf[k] = hy_tanh(__uint_as_float((uint32_t)coeff[p * kHyCoeffPad + m * kHyBases + k] << 16));
    for (int l = 0; l < kHyTaps; ++l) {
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < kHyBases; ++k) a = fmaf(cf[k], bl[k * kHyTaps + l], a);
        atoms[p * kHyAtomElems + l * kHyAtoms + m] = a;
    }
}

// ---- weight packing: W [128, 1536] float32, column c * 6 + m -> wp[(cb * 6 + m) * 128 + col][k] bf16, c = cb * 64 + k ----
__global__ void __launch_bounds__(256) hyper_dynconv_pack_kernel(const float *w, uint16_t *wp)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kHyCout * kHyCin * kHyAtoms) return;
    const int k = i & 63, col = (i >> 6) & 127, chunk = i >> 13;
    const int cb = chunk / kHyAtoms, m = chunk - cb * kHyAtoms;
    wp[i] = (uint16_t)hy_pack_bf16(w[(int64_t)col * (kHyCin * kHyAtoms) + (cb * 64 + k) * kHyAtoms + m], 0.0f);
}

// ---- the dynamic convolution ----
constexpr int kHyAtomsOff = 2 * kHyPatchB;                               // 73,728
constexpr int kHyLdsBytes = kHyAtomsOff + kHyTH * kHyTW * kHyAtomElems * 4;   // 150,528
static_assert(64 * 256 * 4 <= kHyLdsBytes, "the K groups' accumulator exchange reuses the patches");

__global__ void __launch_bounds__(512) hyper_dynconv_kernel(const uint16_t *x, const float *atoms, const uint16_t *wp, const float *bias, uint16_t *out,
                                                            int B, int H, int W, int relu)
{
    extern __shared__ __attribute__((aligned(128))) unsigned char hy_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, kg = tid >> 8;
    const int fr = lane & 31, fh = lane >> 5;
    const int tiles_x = (W + kHyTW - 1) / kHyTW, tiles_y = (H + kHyTH - 1) / kHyTH;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, bimg = blockIdx.x / (tiles_x * tiles_y);
    const int y0 = ty * kHyTH, x0 = tx * kHyTW;
    float *const atoms_l = reinterpret_cast<float *>(hy_lds + kHyAtomsOff);
    // the tile's atoms (zeros outside the image)
    for (int i = tid; i < kHyTH * kHyTW * kHyAtomElems; i += 512) {
        const int p = i / kHyAtomElems, j = i - p * kHyAtomElems;
        const int y = y0 + (p >> 4), xx = x0 + (p & 15);
        atoms_l[i] = (y < H && xx < W) ? atoms[(((int64_t)bimg * H + y) * W + xx) * kHyAtomElems + j] : 0.0f;
    }
    hy_f32x16 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[g][r] = 0.0f;
    const int pl = wave * 32 + fr;                                           // this lane's pixel of the tile: row pl >> 4, column pl & 15
    const unsigned char *const my_patch = hy_lds + kg * kHyPatchB + (pl >> 4) * kHyRowB + (pl & 15) * kHyPixB + fh * 16;
    const float *const my_atoms = atoms_l + pl * kHyAtomElems;
    for (int it = 0; it < 2; ++it) {
        if (it) __syncthreads();                                             // every wave is done with the previous patches
        for (int i = tid; i < 2 * kHyNP * 8; i += 512) {                      // both groups' halo patches: channel blocks 2 it, 2 it + 1
            const int buf = i / (kHyNP * 8), r = i - buf * (kHyNP * 8), idx = r >> 3, slot = r & 7;
            const int hy = idx / kHyPW, hx = idx - hy * kHyPW;
            const int iy = y0 + hy - 2, ix = x0 + hx - 2;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                v = *reinterpret_cast<const uint4 *>(x + (((int64_t)bimg * H + iy) * W + ix) * kHyCin + (2 * it + buf) * 64 + slot * 8);
            *reinterpret_cast<uint4 *>(hy_lds + buf * kHyPatchB + hy * kHyRowB + hx * kHyPixB + slot * 16) = v;
        }
        __syncthreads();
        const int cb = 2 * it + kg;
#pragma unroll 1
        for (int ks = 0; ks < 4; ++ks) {                                      // 16 channels per k-step: this lane's 8 are cb * 64 + ks * 16 + fh * 8 ..
            float f[kHyAtoms][8];
#pragma unroll
            for (int m = 0; m < kHyAtoms; ++m)
#pragma unroll
                for (int j = 0; j < 8; ++j) f[m][j] = 0.0f;
            // one window row per trip (5 taps in flight: their 50 operand registers, not 250, beside the 48 + 64 accumulators)
#pragma unroll 1
            for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 5; ++dx) {
                    const int l = dy * 5 + dx;
                    const uint4 xv = *reinterpret_cast<const uint4 *>(my_patch + dy * kHyRowB + dx * kHyPixB + ks * 32);
                    const float2 a01 = *reinterpret_cast<const float2 *>(my_atoms + l * kHyAtoms);
                    const float2 a23 = *reinterpret_cast<const float2 *>(my_atoms + l * kHyAtoms + 2);
                    const float2 a45 = *reinterpret_cast<const float2 *>(my_atoms + l * kHyAtoms + 4);
                    const float a[kHyAtoms] = {a01.x, a01.y, a23.x, a23.y, a45.x, a45.y};
                    const float xf[8] = {hy_bf16_lo(xv.x), hy_bf16_hi(xv.x), hy_bf16_lo(xv.y), hy_bf16_hi(xv.y),
                                         hy_bf16_lo(xv.z), hy_bf16_hi(xv.z), hy_bf16_lo(xv.w), hy_bf16_hi(xv.w)};
#pragma unroll
                    for (int m = 0; m < kHyAtoms; ++m)
#pragma unroll
                        for (int j = 0; j < 8; ++j) f[m][j] = fmaf(a[m], xf[j], f[m][j]);
                }
            }
#pragma unroll
            for (int m = 0; m < kHyAtoms; ++m) {
                const uint4 au = make_uint4(hy_pack_bf16(f[m][0], f[m][1]), hy_pack_bf16(f[m][2], f[m][3]), hy_pack_bf16(f[m][4], f[m][5]),
                                            hy_pack_bf16(f[m][6], f[m][7]));
                const hy_bf16x8 af = __builtin_bit_cast(hy_bf16x8, au);
                const uint16_t *const wrow = wp + ((int64_t)(cb * kHyAtoms + m) * kHyCout + fr) * 64 + ks * 16 + fh * 8;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const hy_bf16x8 bf = *reinterpret_cast<const hy_bf16x8 *>(wrow + g * 32 * 64);
                    acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[g], 0, 0, 0);
                }
            }
        }
    }
    // group 1's half of K meets group 0's through LDS (element e of lane t at [e][t]: conflict-free), then bias (+ ReLU) -> bf16 NHWC
    __syncthreads();
    float *const red = reinterpret_cast<float *>(hy_lds);
    if (kg == 1) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int r = 0; r < 16; ++r) red[(g * 16 + r) * 256 + (tid & 255)] = acc[g][r];
    }
    __syncthreads();
    if (kg == 1) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float bv = bias[g * 32 + fr];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * fh;
            const int y = y0 + wave * 2 + (row >> 4), xx = x0 + (row & 15);
            float v = (acc[g][r] + red[(g * 16 + r) * 256 + tid]) + bv;
            if (relu) v = v > 0.0f ? v : (v != v ? v : 0.0f);
            if (y < H && xx < W) out[(((int64_t)bimg * H + y) * W + xx) * kHyCout + g * 32 + fr] = (uint16_t)hy_pack_bf16(v, v);
        }
    }
}

#endif  // V2V_HYPER_KERNELS

#ifdef V2V_HYPER_TRAIN_KERNELS
// ---- training: the dynamic layer's backward (launchers and C entry points: v2v_hyper_train_tu.hip) ------------------------------------------
// With dz = relu'(dout) (bf16 [M][128], M = B H W pixels):
//   hyper_dynconv_df_kernel      dF[p][c][m] = sum_o dz[p][o] W[o][c * 6 + m]: a [M,128] x [128,1536] GEMM on v_mfma_f32_32x32x16_bf16, written
//                                ONCE as bf16 [M][cb][m][64] (c = cb * 64 + k: the forward's K chunks), so a lane of the kernels below reads one
//                                atom x 8 channels as 16 bytes.  B fragments from the packed W^T stream (hyper_dynconv_pack_t_kernel).
//   hyper_dynconv_datoms_kernel  dAtoms[p][l][m] = sum_c X[p + off_l][c] dF[p][c][m], float32: lane = (pixel, half of the channel blocks), 150
//                                accumulators, the forward's halo patches in LDS; the two halves meet through LDS (fixed order).
//   hyper_dynconv_dx_kernel      dX[q][c] = sum_l sum_m atoms[q - off_l][l][m] dF[q - off_l][c][m]: lane = (pixel, 8 channels), a gather over the
//                                25 pixels whose window holds q; one bf16 rounding at the store.
//   hyper_dynconv_dw_kernel      dW[o][c * 6 + m] = sum_p dz[p][o] F[p][c][m] with F RECOMPUTED (the forward's FMAs in the forward's order, rounded
//                                to bf16 as the forward rounds it) and transposed through LDS so that pixels run along K of
//                                v_mfma_f32_16x16x32_bf16; grid = 16-channel chunk x pixel split, float32 partials [S][128][1536] summed in split
//                                order by hyper_sum_partials_kernel.  db through hyper_bias_partials_kernel and the same sum.
// BatchNorm on batch statistics (bases_net.1 / .4; z = the convolution's bf16 output [M][Cs], Cs = 64 or 128 with 72 valid columns):
//   hyper_bn_stats_kernel (two passes: mean, then the centred squares; sums carried in float64, fixed tree) / hyper_bn_apply_kernel /
//   hyper_bn_bwd_reduce_kernel (sum dpre, sum dpre xhat) / hyper_bn_bwd_apply_kernel; hyper_atoms_bwd_kernel is the atoms' adjoint.
// No atomics anywhere: every sum has one fixed order.
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float hy_f32x4;

constexpr int kHyFCols = kHyCin * kHyAtoms;                               // 1536 feature columns

__device__ __forceinline__ void hy_unpack8(const uint4 v, float (&f)[8])
{
    f[0] = hy_bf16_lo(v.x); f[1] = hy_bf16_hi(v.x); f[2] = hy_bf16_lo(v.y); f[3] = hy_bf16_hi(v.y);
    f[4] = hy_bf16_lo(v.z); f[5] = hy_bf16_hi(v.z); f[6] = hy_bf16_lo(v.w); f[7] = hy_bf16_hi(v.w);
}

// ---- W [128][1536] float32 (column c * 6 + m) -> wt[n = cb * 384 + m * 64 + k][o] bf16, c = cb * 64 + k ----
__global__ void __launch_bounds__(256) hyper_dynconv_pack_t_kernel(const float *w, uint16_t *wt)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kHyCout * kHyFCols) return;
    const int o = i & 127, n = i >> 7;
    const int cb = n / 384, r = n - cb * 384, m = r >> 6, k = r & 63;
    wt[i] = (uint16_t)hy_pack_bf16(w[(int64_t)o * kHyFCols + (cb * 64 + k) * kHyAtoms + m], 0.0f);
}

// ---- dF: 32 pixels per workgroup, 4 waves x 12 column tiles of 32 ----
__global__ void __launch_bounds__(256) hyper_dynconv_df_kernel(const uint16_t *dz, const uint16_t *wt, uint16_t *dF, int64_t M)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const int64_t p0 = (int64_t)blockIdx.x * 32, pa = p0 + fr;
    hy_bf16x8 a[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (pa < M) v = *reinterpret_cast<const uint4 *>(dz + pa * kHyCout + ks * 16 + fh * 8);
        a[ks] = __builtin_bit_cast(hy_bf16x8, v);
    }
#pragma unroll 1
    for (int nt = wave; nt < kHyFCols / 32; nt += 4) {
        hy_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const uint16_t *const wrow = wt + (int64_t)(nt * 32 + fr) * kHyCout + fh * 8;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const hy_bf16x8 bf = *reinterpret_cast<const hy_bf16x8 *>(wrow + ks * 16);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks], bf, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t p = p0 + (r & 3) + 8 * (r >> 2) + 4 * fh;
            if (p < M) dF[p * kHyFCols + nt * 32 + fr] = (uint16_t)hy_pack_bf16(acc[r], acc[r]);
        }
    }
}

// one channel block's halo patch of x (zeros outside the image) into LDS, by `nthreads` work-items
__device__ __forceinline__ void hy_load_patch(unsigned char *patch, const uint16_t *x, int bimg, int H, int W, int y0, int x0, int cb, int t, int nthreads)
{
    for (int i = t; i < kHyNP * 8; i += nthreads) {
        const int idx = i >> 3, slot = i & 7;
        const int hy = idx / kHyPW, hx = idx - hy * kHyPW;
        const int iy = y0 + hy - 2, ix = x0 + hx - 2;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
            v = *reinterpret_cast<const uint4 *>(x + (((int64_t)bimg * H + iy) * W + ix) * kHyCin + cb * 64 + slot * 8);
        *reinterpret_cast<uint4 *>(patch + hy * kHyRowB + hx * kHyPixB + slot * 16) = v;
    }
}

// ---- dAtoms: tile 8 x 16 pixels, 256 work-items = (pixel, half hf); half hf walks channel blocks hf, hf + 2 ----
constexpr int kHyDaLdsBytes = kHyTH * kHyTW * kHyAtomElems * 4;          // 76,800: the exchange (the two patches, 73,728 B, fit inside)
static_assert(2 * kHyPatchB <= kHyDaLdsBytes, "the halves' exchange reuses the patches");

__global__ void __launch_bounds__(256) hyper_dynconv_datoms_kernel(const uint16_t *x, const uint16_t *dF, float *datoms, int B, int H, int W)
{
    extern __shared__ __attribute__((aligned(128))) unsigned char hy_lds[];
    const int tid = threadIdx.x, pl = tid & 127, hf = tid >> 7;
    const int tiles_x = (W + kHyTW - 1) / kHyTW, tiles_y = (H + kHyTH - 1) / kHyTH;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, bimg = blockIdx.x / (tiles_x * tiles_y);
    const int y0 = ty * kHyTH, x0 = tx * kHyTW;
    const int y = y0 + (pl >> 4), xx = x0 + (pl & 15);
    const bool inside = y < H && xx < W;
    const int64_t p = ((int64_t)bimg * H + y) * W + xx;
    float acc[kHyTaps][kHyAtoms];
#pragma unroll
    for (int l = 0; l < kHyTaps; ++l)
#pragma unroll
        for (int m = 0; m < kHyAtoms; ++m) acc[l][m] = 0.0f;
    const unsigned char *const my_patch = hy_lds + hf * kHyPatchB + (pl >> 4) * kHyRowB + (pl & 15) * kHyPixB;
    for (int it = 0; it < 2; ++it) {
        if (it) __syncthreads();
        hy_load_patch(hy_lds + hf * kHyPatchB, x, bimg, H, W, y0, x0, 2 * it + hf, pl, 128);
        __syncthreads();
        const int cb = 2 * it + hf;
#pragma unroll 1
        for (int cg = 0; cg < 8; ++cg) {
            float d[kHyAtoms][8];
#pragma unroll
            for (int m = 0; m < kHyAtoms; ++m) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (inside) v = *reinterpret_cast<const uint4 *>(dF + p * kHyFCols + cb * 384 + m * 64 + cg * 8);
                hy_unpack8(v, d[m]);
            }
#pragma unroll
            for (int l = 0; l < kHyTaps; ++l) {
                float xf[8];
                hy_unpack8(*reinterpret_cast<const uint4 *>(my_patch + (l / 5) * kHyRowB + (l % 5) * kHyPixB + cg * 16), xf);
#pragma unroll
                for (int m = 0; m < kHyAtoms; ++m)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[l][m] = fmaf(xf[j], d[m][j], acc[l][m]);
            }
        }
    }
    __syncthreads();
    float *const red = reinterpret_cast<float *>(hy_lds);
    if (hf == 1) {
#pragma unroll
        for (int l = 0; l < kHyTaps; ++l)
#pragma unroll
            for (int m = 0; m < kHyAtoms; ++m) red[(l * kHyAtoms + m) * 128 + pl] = acc[l][m];
    }
    __syncthreads();
    if (hf == 1 || !inside) return;
#pragma unroll
    for (int l = 0; l < kHyTaps; ++l)
#pragma unroll
        for (int m = 0; m < kHyAtoms; ++m) datoms[p * kHyAtomElems + l * kHyAtoms + m] = acc[l][m] + red[(l * kHyAtoms + m) * 128 + pl];
}

// ---- dX: 8 pixels x 32 channel groups per workgroup ----
__global__ void __launch_bounds__(256) hyper_dynconv_dx_kernel(const float *atoms, const uint16_t *dF, uint16_t *dx, int B, int H, int W)
{
    const int tid = threadIdx.x, cg = tid & 31;
    const int64_t q = (int64_t)blockIdx.x * 8 + (tid >> 5);
    if (q >= (int64_t)B * H * W) return;
    const int xq = (int)(q % W), yq = (int)((q / W) % H);
    const int cb = cg >> 3, k8 = (cg & 7) * 8;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
#pragma unroll
    for (int l = 0; l < kHyTaps; ++l) {
        const int oy = l / 5 - 2, ox = l % 5 - 2;                             // p + (oy, ox) = q
        if ((unsigned)(yq - oy) >= (unsigned)H || (unsigned)(xq - ox) >= (unsigned)W) continue;
        const int64_t p = q - (int64_t)oy * W - ox;
        const float *const ap = atoms + p * kHyAtomElems + l * kHyAtoms;
        const uint16_t *const dp = dF + p * kHyFCols + cb * 384 + k8;
#pragma unroll
        for (int m = 0; m < kHyAtoms; ++m) {
            float d[8];
            hy_unpack8(*reinterpret_cast<const uint4 *>(dp + m * 64), d);
            const float a = ap[m];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(a, d[j], acc[j]);
        }
    }
    *reinterpret_cast<uint4 *>(dx + q * kHyCin + cg * 8) = make_uint4(hy_pack_bf16(acc[0], acc[1]), hy_pack_bf16(acc[2], acc[3]), hy_pack_bf16(acc[4], acc[5]),
                                                                      hy_pack_bf16(acc[6], acc[7]));
}

// ---- dW: workgroup = (16-channel chunk, pixel split); per tile: patch + dz^T into LDS, F built and transposed, 48 MFMAs per wave ----
constexpr int kHyWPixB = 48;                                             // 16 channels (32 B) + 16 (bank spread)
constexpr int kHyWRowB = kHyPW * kHyWPixB;                               // 960
constexpr int kHyWPatchB = kHyPH * kHyWRowB;                             // 11,520
constexpr int kHyWPitch = 128 + 8;                                       // bf16 elements per row of dz^T / F^T (272 B: 16-byte aligned, bank spread)
constexpr int kHyWDzOff = kHyWPatchB;                                    // dz^T [128 o][136]
constexpr int kHyWFtOff = kHyWDzOff + 128 * kHyWPitch * 2;               // F^T [6 m * 16 channels][136]
constexpr int kHyWLdsBytes = kHyWFtOff + 96 * kHyWPitch * 2;             // 72,448

__global__ void __launch_bounds__(256) hyper_dynconv_dw_kernel(const uint16_t *dz, const uint16_t *x, const float *atoms, float *part, int B, int H, int W, int S)
{
    extern __shared__ __attribute__((aligned(128))) unsigned char hy_lds[];
    uint16_t *const dzt = reinterpret_cast<uint16_t *>(hy_lds + kHyWDzOff);
    uint16_t *const ft = reinterpret_cast<uint16_t *>(hy_lds + kHyWFtOff);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5, r16 = lane & 15, fg = lane >> 4;
    const int c0 = blockIdx.x * 16, s = blockIdx.y;
    const int tiles_x = (W + kHyTW - 1) / kHyTW, tiles_y = (H + kHyTH - 1) / kHyTH, tiles = B * tiles_x * tiles_y;
    hy_f32x4 acc[2][kHyAtoms];
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
        for (int m = 0; m < kHyAtoms; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[ob][m][r] = 0.0f;
    const int pl = wave * 32 + fr;                                           // this lane's pixel of the tile when it builds F
#pragma unroll 1
    for (int t = s; t < tiles; t += S) {
        const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, bimg = t / (tiles_x * tiles_y);
        const int y0 = ty * kHyTH, x0 = tx * kHyTW;
        __syncthreads();                                                     // the previous tile's MFMAs are done with dz^T / F^T
        for (int i = tid; i < kHyNP * 2; i += 256) {                          // halo patch, 16 channels
            const int idx = i >> 1, slot = i & 1;
            const int hy = idx / kHyPW, hx = idx - hy * kHyPW;
            const int iy = y0 + hy - 2, ix = x0 + hx - 2;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                v = *reinterpret_cast<const uint4 *>(x + (((int64_t)bimg * H + iy) * W + ix) * kHyCin + c0 + slot * 8);
            *reinterpret_cast<uint4 *>(hy_lds + hy * kHyWRowB + hx * kHyWPixB + slot * 16) = v;
        }
        for (int i = tid; i < 128 * 16; i += 256) {                           // dz tile -> dz^T (zeros outside the image)
            const int pp = i >> 4, og = i & 15;
            const int y = y0 + (pp >> 4), xx = x0 + (pp & 15);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (y < H && xx < W) v = *reinterpret_cast<const uint4 *>(dz + (((int64_t)bimg * H + y) * W + xx) * kHyCout + og * 8);
            const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dzt[(og * 8 + 2 * j) * kHyWPitch + pp] = (uint16_t)(u[j] & 0xFFFFu);
                dzt[(og * 8 + 2 * j + 1) * kHyWPitch + pp] = (uint16_t)(u[j] >> 16);
            }
        }
        __syncthreads();
        {   // F for (pixel pl, channels c0 + fh * 8 ..): the forward's FMAs in the forward's order, rounded as the forward rounds
            const int y = y0 + (pl >> 4), xx = x0 + (pl & 15);
            const bool inside = y < H && xx < W;
            const float *const my_atoms = atoms + (((int64_t)bimg * H + y) * W + xx) * kHyAtomElems;
            const unsigned char *const my_patch = hy_lds + (pl >> 4) * kHyWRowB + (pl & 15) * kHyWPixB + fh * 16;
            float f[kHyAtoms][8];
#pragma unroll
            for (int m = 0; m < kHyAtoms; ++m)
#pragma unroll
                for (int j = 0; j < 8; ++j) f[m][j] = 0.0f;
#pragma unroll 1
            for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 5; ++dx) {
                    const int l = dy * 5 + dx;
                    float xf[8];
                    hy_unpack8(*reinterpret_cast<const uint4 *>(my_patch + dy * kHyWRowB + dx * kHyWPixB), xf);
                    float a[kHyAtoms];
#pragma unroll
                    for (int m = 0; m < kHyAtoms; ++m) a[m] = inside ? my_atoms[l * kHyAtoms + m] : 0.0f;
#pragma unroll
                    for (int m = 0; m < kHyAtoms; ++m)
#pragma unroll
                        for (int j = 0; j < 8; ++j) f[m][j] = fmaf(a[m], xf[j], f[m][j]);
                }
            }
#pragma unroll
            for (int m = 0; m < kHyAtoms; ++m)
#pragma unroll
                for (int j = 0; j < 8; ++j) ft[(m * 16 + fh * 8 + j) * kHyWPitch + pl] = (uint16_t)hy_pack_bf16(f[m][j], f[m][j]);
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {                                      // K = 32 pixels per step; A rows = output channels, B columns = channels
            hy_bf16x8 af[2];
#pragma unroll
            for (int ob = 0; ob < 2; ++ob)
                af[ob] = *reinterpret_cast<const hy_bf16x8 *>(dzt + ((wave * 2 + ob) * 16 + r16) * kHyWPitch + kk * 32 + fg * 8);
#pragma unroll
            for (int m = 0; m < kHyAtoms; ++m) {
                const hy_bf16x8 bf = *reinterpret_cast<const hy_bf16x8 *>(ft + (m * 16 + r16) * kHyWPitch + kk * 32 + fg * 8);
#pragma unroll
                for (int ob = 0; ob < 2; ++ob) acc[ob][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ob], bf, acc[ob][m], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
        for (int m = 0; m < kHyAtoms; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = (wave * 2 + ob) * 16 + 4 * fg + r;
                part[((int64_t)s * kHyCout + o) * kHyFCols + (c0 + r16) * kHyAtoms + m] = acc[ob][m][r];
            }
}

// db partials: split s sums its pixels p = s, s + S, .. in that order; one work-item per output channel
__global__ void __launch_bounds__(128) hyper_bias_partials_kernel(const uint16_t *dz, float *part, int64_t M, int S)
{
    const int o = threadIdx.x, s = blockIdx.x;
    float a = 0.0f;
    for (int64_t p = s; p < M; p += S) a += __uint_as_float((uint32_t)dz[p * kHyCout + o] << 16);
    part[s * kHyCout + o] = a;
}

// out[i] = part[0][i] + part[1][i] + .. in split order
__global__ void __launch_bounds__(256) hyper_sum_partials_kernel(const float *part, float *out, int64_t n, int S)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float a = part[i];
    for (int s = 1; s < S; ++s) a += part[(int64_t)s * n + i];
    out[i] = a;
}

// ---- BatchNorm on batch statistics.  One workgroup per 8 channels; work-item t walks rows t, t + 256, ..; the 256 partial sums meet in a
// fixed tree.  Sums in float64 (M * Cs is small: these kernels are launch-bound), results float32. ----
__device__ __forceinline__ void hy_tree8(double (&v)[8], double *sh, int tid)
{
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[j * 256 + tid] = v[j];
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (tid < step) {
#pragma unroll
            for (int j = 0; j < 8; ++j) sh[j * 256 + tid] += sh[j * 256 + tid + step];
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = sh[j * 256];
    __syncthreads();
}

__global__ void __launch_bounds__(256) hyper_bn_stats_kernel(const uint16_t *z, int64_t M, int Cs, float eps, float *mean, float *var, float *rstd)
{
    __shared__ double sh[8 * 256];
    const int tid = threadIdx.x, c0 = blockIdx.x * 8;
    double a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = 0.0;
    for (int64_t p = tid; p < M; p += 256) {
        float f[8];
        hy_unpack8(*reinterpret_cast<const uint4 *>(z + p * Cs + c0), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += (double)f[j];
    }
    hy_tree8(a, sh, tid);
    double mu[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { mu[j] = a[j] / (double)M; q[j] = 0.0; }
    for (int64_t p = tid; p < M; p += 256) {
        float f[8];
        hy_unpack8(*reinterpret_cast<const uint4 *>(z + p * Cs + c0), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) { const double d = (double)f[j] - mu[j]; q[j] += d * d; }
    }
    hy_tree8(q, sh, tid);
    if (tid < 8) {
        const float v = (float)(q[tid] / (double)M);
        mean[c0 + tid] = (float)mu[tid];
        var[c0 + tid] = v;
        rstd[c0 + tid] = (float)(1.0 / sqrt((double)v + (double)eps));
    }
}

// y = gamma (z - mean) rstd + beta [-> tanh] -> bf16; columns >= Cv are written as zeros.  One work-item per (row, 8 channels)
__global__ void __launch_bounds__(256) hyper_bn_apply_kernel(const uint16_t *z, const float *mean, const float *rstd, const float *gamma, const float *beta,
                                                             int64_t M, int Cs, int Cv, int tanh_out, uint16_t *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int groups = Cs >> 3;
    if (i >= M * groups) return;
    const int64_t p = i / groups;
    const int c0 = (int)(i - p * groups) * 8;
    float f[8], y[8];
    hy_unpack8(*reinterpret_cast<const uint4 *>(z + p * Cs + c0), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        y[j] = 0.0f;
        if (c < Cv) {
            const float v = gamma[c] * ((f[j] - mean[c]) * rstd[c]) + beta[c];
            y[j] = tanh_out ? hy_tanh(v) : v;
        }
    }
    *reinterpret_cast<uint4 *>(out + p * Cs + c0) = make_uint4(hy_pack_bf16(y[0], y[1]), hy_pack_bf16(y[2], y[3]), hy_pack_bf16(y[4], y[5]), hy_pack_bf16(y[6], y[7]));
}

// dpre of one element: dy [* (1 - y^2), y = tanh(gamma xhat + beta) recomputed]; xhat = (z - mean) rstd
__device__ __forceinline__ float hy_bn_dpre(float dy, float xhat, float g, float b, int tanh_out)
{
    if (!tanh_out) return dy;
    const float y = hy_tanh(g * xhat + b);
    return dy * (1.0f - y * y);
}

__device__ __forceinline__ void hy_load_dy8(const void *dy, int dy_f32, int64_t off, float (&d)[8])
{
    if (dy_f32) {
        const float4 lo = *reinterpret_cast<const float4 *>(static_cast<const float *>(dy) + off);
        const float4 hi = *reinterpret_cast<const float4 *>(static_cast<const float *>(dy) + off + 4);
        d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w; d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
    } else {
        hy_unpack8(*reinterpret_cast<const uint4 *>(static_cast<const uint16_t *>(dy) + off), d);
    }
}

// sums[0][c] = sum dpre (dbeta), sums[1][c] = sum dpre xhat (dgamma); columns >= Cv: zero.  With sums_in (= that result) the second pass:
// sums[0][c] = sum dz over the rows, dz in float32 BEFORE its bf16 rounding -- the bias gradient of the convolution in front, which is zero
// in exact arithmetic (summing the rounded dz would leave bf16 noise there, this leaves float32's)
__global__ void __launch_bounds__(256) hyper_bn_bwd_reduce_kernel(const void *dy, int dy_f32, const uint16_t *z, const float *mean, const float *rstd,
                                                                  const float *gamma, const float *beta, const float *sums_in, int64_t M, int Cs, int Cv,
                                                                  int tanh_out, float *sums)
{
    __shared__ double sh[8 * 256];
    const int tid = threadIdx.x, c0 = blockIdx.x * 8;
    double sb[8], sg[8];
    float mu[8], rs[8], g[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool ok = c0 + j < Cv;
        sb[j] = sg[j] = 0.0;
        mu[j] = mean[c0 + j]; rs[j] = rstd[c0 + j];
        g[j] = ok ? gamma[c0 + j] : 0.0f; b[j] = ok ? beta[c0 + j] : 0.0f;
    }
    const float inv_m = 1.0f / (float)M;
    float s0[8], s1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s0[j] = sums_in ? sums_in[c0 + j] * inv_m : 0.0f; s1[j] = sums_in ? sums_in[Cs + c0 + j] * inv_m : 0.0f; }
    for (int64_t p = tid; p < M; p += 256) {
        float f[8], d[8];
        hy_unpack8(*reinterpret_cast<const uint4 *>(z + p * Cs + c0), f);
        hy_load_dy8(dy, dy_f32, p * Cs + c0, d);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float xh = (f[j] - mu[j]) * rs[j];
            const float dp = hy_bn_dpre(d[j], xh, g[j], b[j], tanh_out);
            if (sums_in) {
                sb[j] += (double)((g[j] * rs[j]) * ((dp - s0[j]) - xh * s1[j]));
            } else {
                sb[j] += (double)dp;
                sg[j] += (double)dp * (double)xh;
            }
        }
    }
    hy_tree8(sb, sh, tid);
    hy_tree8(sg, sh, tid);
    if (tid < 8) {
        const bool ok = c0 + tid < Cv;
        sums[c0 + tid] = ok ? (float)sb[tid] : 0.0f;
        sums[Cs + c0 + tid] = ok ? (float)sg[tid] : 0.0f;
    }
}

// dz = gamma rstd (dpre - sum_dpre / M - xhat sum_dpre_xhat / M) -> bf16; columns >= Cv: zero
__global__ void __launch_bounds__(256) hyper_bn_bwd_apply_kernel(const void *dy, int dy_f32, const uint16_t *z, const float *mean, const float *rstd,
                                                                 const float *gamma, const float *beta, const float *sums, int64_t M, int Cs, int Cv,
                                                                 int tanh_out, uint16_t *dzout)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int groups = Cs >> 3;
    if (i >= M * groups) return;
    const int64_t p = i / groups;
    const int c0 = (int)(i - p * groups) * 8;
    float f[8], d[8], o[8];
    hy_unpack8(*reinterpret_cast<const uint4 *>(z + p * Cs + c0), f);
    hy_load_dy8(dy, dy_f32, p * Cs + c0, d);
    const float inv_m = 1.0f / (float)M;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        o[j] = 0.0f;
        if (c < Cv) {
            const float xh = (f[j] - mean[c]) * rstd[c];
            const float dp = hy_bn_dpre(d[j], xh, gamma[c], beta[c], tanh_out);
            o[j] = (gamma[c] * rstd[c]) * ((dp - sums[c] * inv_m) - xh * (sums[Cs + c] * inv_m));
        }
    }
    *reinterpret_cast<uint4 *>(dzout + p * Cs + c0) = make_uint4(hy_pack_bf16(o[0], o[1]), hy_pack_bf16(o[2], o[3]), hy_pack_bf16(o[4], o[5]), hy_pack_bf16(o[6], o[7]));
}

// ---- atoms backward: dpre[p][m * 12 + k] = (1 - c^2) sum_l dAtoms[p][l][m] bases[k][l], c = tanh(pre) recomputed; float32 [M][128], columns
// 72..127 zero.  One work-item per (pixel, j): j < 6 an atom, j = 6, 7 the padding's two halves ----
__global__ void __launch_bounds__(256) hyper_atoms_bwd_kernel(const float *datoms, const uint16_t *pre, const float *bases, float *dpre, int64_t M)
{
    __shared__ float bl[kHyBases * kHyTaps];
    for (int i = threadIdx.x; i < kHyBases * kHyTaps; i += 256) bl[i] = bases[i];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * 8) return;
    const int64_t p = i >> 3;
    const int m = (int)(i & 7);
    if (m >= kHyAtoms) {
        float *const o = dpre + p * kHyCoeffPad + kHyCoeff + (m - kHyAtoms) * 28;
        for (int j = 0; j < 28; ++j) o[j] = 0.0f;
        return;
    }
    float g[kHyBases];
#pragma unroll
    for (int k = 0; k < kHyBases; ++k) g[k] = 0.0f;
    for (int l = 0; l < kHyTaps; ++l) {
        const float da = datoms[p * kHyAtomElems + l * kHyAtoms + m];
#pragma unroll
        for (int k = 0; k < kHyBases; ++k) g[k] = fmaf(da, bl[k * kHyTaps + l], g[k]);
    }
#pragma unroll
    for (int k = 0; k < kHyBases; ++k) {
        const float c = hy_tanh(__uint_as_float((uint32_t)pre[p * kHyCoeffPad + m * kHyBases + k] << 16));
        dpre[p * kHyCoeffPad + m * kHyBases + k] = (1.0f - c * c) * g[k];
    }
}

#endif  // V2V_HYPER_TRAIN_KERNELS

}  // namespace v2v
