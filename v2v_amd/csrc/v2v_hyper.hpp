// v2v_hyper.hpp -- HyperE2VID's per-pixel dynamic decoder (model/hyper_model.py:33-60, model/hyper/hyper_dynamic.py) on gfx950.
//
// The layer replaces decoders[0] of the recurrent UNet:  y = relu(DynamicConv(up2(x + skip), atoms(context(events, prev_image)))).
// Kernels in this file (launchers in v2v_hyper_tu.hip; this header alone, without V2V_HYPER_KERNELS, only declares the launchers):
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

hipError_t launch_hyper_context(const float *ev, int64_t sb, int64_t sc, int64_t sh, int64_t sw, const float *prev, uint16_t *dst, int B, int C, int H, int W,
                                hipStream_t s);
hipError_t launch_hyper_context_conv(const uint16_t *x8, const float *w, const float *bias, uint16_t *out, int B, int h, int wd, int Cin, hipStream_t s);
hipError_t launch_hyper_tanh(const uint16_t *x, uint16_t *out, int64_t n8, hipStream_t s);
hipError_t launch_hyper_atoms(const uint16_t *coeff, const float *bases, float *atoms, int64_t M, hipStream_t s);
hipError_t launch_hyper_dynconv_pack(const float *w, uint16_t *wp, hipStream_t s);
hipError_t launch_hyper_dynconv(const uint16_t *x, const float *atoms, const uint16_t *wp, const float *bias, uint16_t *out, int B, int H, int W, int relu,
                                hipStream_t s);

#ifdef V2V_HYPER_KERNELS

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
constexpr int kHyTH = 8, kHyTW = 16, kHyPW = kHyTW + 4, kHyPH = kHyTH + 4, kHyNP = kHyPW * kHyPH;   // tile, halo patch (240 pixels)
constexpr int kHyPixB = 144;                                             // bytes per halo pixel: 64 channels + 16 (bank spread)
constexpr int kHyRowB = 3072;                                            // bytes per patch row: 20 pixels (2,880), padded to 0 mod 256
constexpr int kHyPatchB = kHyPH * kHyRowB;                               // 36,864
constexpr int kHyAtomsOff = 2 * kHyPatchB;                               // 73,728
constexpr int kHyLdsBytes = kHyAtomsOff + kHyTH * kHyTW * kHyAtomElems * 4;   // 150,528
static_assert(kHyPW * kHyPixB <= kHyRowB && kHyRowB % 256 == 0, "patch row pitch");
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

}  // namespace v2v
