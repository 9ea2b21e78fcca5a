// v2v_esim.hpp -- fused ESIM frame-pair simulator + voxel binning for gfx950 (MI355X).
//
// Replaces, for a whole batch of clips in ONE launch:
//   data/v2v_core_esim.py:26-69   EventEmulator.video_to_voxel   (per-pixel potential, threshold crossing)
//   data/v2v_datasets.py:399-400  reshape(L,Tb,fpb,H,W).sum(2)   (V2V_BIN_SUM)
//   utils/event_utils.py:692-728  temporal-bilinear voxel bins    (V2V_BIN_BILINEAR, pseudo-events at ts=k)
//
// Mapping to the hardware (HBM-bound on paper: pointwise in space, sequential scan in time, zero reuse; measured
// VALU-bound at ~21 vector instructions per pixel and frame pair -- see DESIGN.md section 4.1):
//   * one work-item owns VEC=4 horizontally adjacent pixels of one clip and streams the clip's N frames
//     through registers: per-pixel state (float64 potential, previous log value, hot-pixel noise, bin
//     accumulators) never leaves the register file, so HBM traffic is exactly "read every input byte
//     once, write every voxel byte once".
//   * a wave reads one contiguous 1 KiB segment per frame (global_load_dwordx4 per lane, fp32 input); a register
//     ring of kDepth frames is reloaded right after each slot is consumed (unconditional, clamped loads so the
//     compiler can count them: s_waitcnt vmcnt(kDepth-1)), keeping ~kDepth KiB per wave in flight.
//   * the 256-entry log-intensity table (NumPy's bits, golden G1) lives in LDS; integer-valued input
//     costs one ds_read per sample instead of a float64 pow+log.
//   * np.floor_divide's exact result for a >= 0, b > 0 is the true floor of the real quotient; it is obtained
//     without a division and without a per-pixel branch: q = floor(u), u = a * inv_low(b), and a rare (wave-level) +1
//     fix-up found by one sign-exact fma residual; q == 0 exactly when a < b, so the reference's where() masks fall out.
//     The residual and its compare run only behind a SCREEN on bits the step already has: with |u| < 2^20 the estimate
//     can be short only if the top 24 bits of u's low word are all ones (lemma and proof: DESIGN.md section 4.2), so the
//     hot path of a 4-pixel step is an unsigned max over four low words and one compare against a wave-uniform scalar
//     (3 cheap vector instructions) where it ran 4 v_fma_f64 + 4 v_cmp_nlt_f64 + 3 s_or_b64.  A wave is PARANOID -- the
//     scalar is 0, the full check runs in every step, same arithmetic -- when (1) the clip's parameters do not bound the
//     quotient, (max(C+,C-) + 7.0 + 4.0625 (base_std + hot_std)) / min(C+,C-) >= 2^20 (bit 1 of the clip's flag word), or
//     (2) a float32 frame value left the log table (sticky from that frame on, set by pix_logs' slow path).  Replayed
//     noise fields (arbitrary host deviates) keep the full check at compile time.
//   * symmetric thresholds (C+ == C-, wave-uniform per clip) take a loop specialised without the per-lane
//     threshold selection; noise-free launches (V2V_FLAG_NO_NOISE) take kernels without the noise adds.
//   * per-clip ON/OFF totals: lane-local counters -> wave reduction -> one 64-bit atomic per wave.
// No MFMA (nothing here is a contraction), no cross-workgroup communication, no collectives.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "v2v_common.hpp"

namespace v2v {

// Log-intensity tables in device memory (initialised with NumPy's bits, golden G1; re-pinnable through
// v2v_lut_set).  Each workgroup copies the one it needs into LDS.
#include "v2v_luts.inc"
static __device__ double g_lut_esim64[256] = {V2V_LUT_ESIM64_VALUES};
static __device__ float g_lut_esim32[256] = {V2V_LUT_ESIM32_VALUES};
static const double kLutEsim64[256] = {V2V_LUT_ESIM64_VALUES};
static const float kLutEsim32[256] = {V2V_LUT_ESIM32_VALUES};

// float32 content that is not an integer in 0..255: the reference's float32 expression (v2v_core_esim.py:3-4,33-34).
// Out of line: the pow/log bodies (~1.5k instructions per inlined copy, 8 copies per kernel) only bloat the time loop.
#ifndef V2V_SLOWPATH_ATTR
#define V2V_SLOWPATH_ATTR __attribute__((noinline))
#endif
__device__ V2V_SLOWPATH_ATTR float log_generic_f32(float v)
{
    const float lin = powf(v / 255.0f, 2.2f) * 255.0f;
    return logf(0.001f + lin / 255.0f);
}

// Log intensity of the VEC pixels of one raw vector.
//  u8 : one LDS lookup per pixel (float64 table).
//  f32: values that are integers in 0..255 take the float32 table (bitwise NumPy's float32 result); anything
//       else -- detected with a convert/round-trip compare, one wave-level test per vector -- is recomputed with
//       the reference's float32 expression (v2v_core_esim.py:3-4,33-34).  Device powf/logf are within 1-2 ulp
//       of NumPy's float32 kernels, hence the 1e-5 count-flip tolerance stated for non-integer content.
// LDS table entries: uint8 input -> the float64 log value; float32 input -> {float32 log value, (float)index}: the index
// comes back with the value in one ds_read_b64, so the validity test needs no convert (4 of ~100 VALU slots per step)
template <int IN> struct LutEntry { using type = double; };
template <> struct LutEntry<kInF32> { using type = float2; };

template <int IN, int VEC>
__device__ __forceinline__ void pix_logs(const Raw<IN, VEC> &r, const typename LutEntry<IN>::type *lut,
                                         typename LutT<IN>::type (&out)[VEC], uint32_t &screen_min)
{
    using ent_t = typename LutEntry<IN>::type;
    // table entry by BYTE offset: shift + mask (two full-rate VALU ops) instead of a bit-field extract and a
    // shift-add (two half-rate ones) per pixel
    auto at = [&](uint32_t byte_off) { return *reinterpret_cast<const ent_t *>(reinterpret_cast<const unsigned char *>(lut) + byte_off); };
    constexpr uint32_t kSh = 3u, kMask = 255u << kSh;
    if constexpr (IN == kInU8) {
        if constexpr (VEC == 4) {
            out[0] = at((r.v << kSh) & kMask);
            out[1] = at((r.v >> (8u - kSh)) & kMask);
            out[2] = at((r.v >> (16u - kSh)) & kMask);
            out[3] = at((r.v >> (24u - kSh)) & kMask);
        } else if constexpr (VEC == 2) {
            const uint32_t v = r.v;
            out[0] = at((v << kSh) & kMask);
            out[1] = at((v >> (8u - kSh)) & kMask);
        } else {
            out[0] = lut[r.v];
        }
    } else {
        unsigned long long bad = 0;                            // wave-level mask (SGPR pair): any lane, any pixel
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float v = raw_f32<VEC>(r, j);
            // v + 2^20 puts an integer v in 0..255 into mantissa bits 3..10 (ulp = 1/8): masked, that IS the byte offset of the
            // 8-byte table entry -- one cheap add and one and, no convert, no shift; the bits are always a valid offset, and the
            // index that comes back with the entry exposes every other input (non-integer, negative, > 255, NaN)
            const uint32_t b = __float_as_uint(v + 1048576.0f);
            const float2 e = at(b & kMask);
            out[j] = e.x;
            bad |= __ballot(e.y != v);                         // e.y = (float)(b & 255): non-integer, negative, > 255, NaN
        }
        if (__builtin_expect(bad != 0, 0)) {                   // scalar test; lanes with clean pixels skip the bodies below
            screen_min = 0u;                                   // sticky, wave-uniform: from here on a log difference is not bounded by the table's spread
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float v = raw_f32<VEC>(r, j);
                if ((float)((__float_as_uint(v + 1048576.0f) >> 3) & 255u) != v) out[j] = log_generic_f32(v);
            }
        }
    }
}

// NOISE  : false -> the caller guarantees base_noise_std == 0 and hot_pixel_fraction == 0 for every clip
//          (V2V_FLAG_NO_NOISE); the noise adds, their registers and the Gaussian generator disappear.
// OUT64  : true  -> float64 accumulators and output, accumulated exactly like NumPy (product rounded, then
//                   added): bit-exact against the reference's float64 result.
//          false -> float32 output.  Integer counts (SUM mode) stay exact; weighted/noisy values are
//                   accumulated with float32 fma and agree with the float64 result to ~1e-6 relative.
// EXT    : put_noise_external (v2v_core_esim.py:46-49 vs :60-65): the noise goes into the voxel, not into the potential.
//          Compile-time: as a run-time flag the compiler turned both uses into selects over speculated float64 adds and
//          converts (~28 of 213 VALU instructions per 4-pixel step of the noise-on launch, SQ_INSTS_VALU).
// The GENERAL device-noise instances (4 pixels per work-item, float32 grid, thresholds unknown to the host -- per-clip device
// parameters as the dataset draws them, data/v2v_datasets.py:368-386) carry ONE time loop, the by-polarity one: it is exact for
// C+ == C- too, and without the second (symmetric) loop the kernel fits 128 VGPRs = 4 waves per SIMD.
template <int VEC, int RNG, bool NOISE, bool OUT64, bool EXT, bool SYMONLY>
constexpr bool esim_asym4() { return V2V_ESIM_ASYM4 && NOISE && RNG == kRngPhilox && VEC == 4 && !OUT64 && !EXT && !SYMONLY; }

// The quotient screen of the step: with u = p * inv_low(C) and |u| < 2^20, the reciprocal estimate trunc(u) is
// short of floor(|p| / C) only if the top 24 bits of u's low word are all ones, so the step looks at that word and runs the residual
// fma + compare of the fix-up only in the rare wave that passes (2^-24 per pixel and step for a random quotient).  The premise
// |u| < 2^20 follows from the clip's parameters: |p| <= max(C+, C-) + kScreenLogSpread + kScreenGaussMax * (base_std + hot_std).
// NOISE_FREE: the screen in the instances without the noise path too (their bound is evaluated per work-item).
#ifndef V2V_ESIM_SCREEN
#define V2V_ESIM_SCREEN 1
#endif
#ifndef V2V_ESIM_SCREEN_NOISE_FREE
#define V2V_ESIM_SCREEN_NOISE_FREE 1
#endif
constexpr double kScreenLogSpread = 7.0;       // >= log(1.001) - log(0.001) = 6.909: the spread of both log tables
constexpr double kScreenGaussMax = 4.0625;     // >= 4.009, the largest entry of the Gaussian table (v2v_rng.hpp)
constexpr uint32_t kScreenLowWord = 0xFFFFFF00u;
// copysign(1.0, x) for the rare fix-up, with the zero low word made on the spot: as a plain constant the compiler kept the pair in
// registers across the whole time loop, which the float32 4-pixel instances at 128 VGPRs paid with scratch
__device__ __forceinline__ double signed_one(double x)
{
    uint32_t lo;
    asm volatile("v_mov_b32 %0, 0" : "=v"(lo));
    return __hiloint2double((int)(((uint32_t)__double2hiint(x) & 0x80000000u) | 0x3ff00000u), (int)lo);
}
__device__ __forceinline__ double quotient_bound_num(double c_pos, double c_neg, double base_std, double hot_std)
{
    const double noise = kScreenGaussMax * (base_std + hot_std);
    const double reach = fmax(c_pos, c_neg) + kScreenLogSpread;
    return reach + noise;
}

// FIDX   : the clip's frames are read through a per-clip index row (EsimArgs::frame_index, copied to LDS) and clips start at
//          EsimArgs::clip_offsets -- the dataset's pause-index gather folded into the loads (instances: uint8 input, SUM bins, device noise).
template <int IN, int VEC, int BIN, int RNG, bool NOISE, bool OUT64, bool EXT = false, bool SYMONLY = false, bool FIDX = false>
__global__ void __launch_bounds__(kBlock, (SYMONLY || esim_asym4<VEC, RNG, NOISE, OUT64, EXT, SYMONLY>()) ? 4 : V2V_MIN_WAVES) esim_voxel_kernel(const EsimArgs a)
{
    static_assert(!FIDX || BIN == kBinSum, "the frame index row uses the dynamic LDS region the bilinear tables live in");
    constexpr bool ASYM4 = esim_asym4<VEC, RNG, NOISE, OUT64, EXT, SYMONLY>();
    // SYMONLY (V2V_FLAG_SYMMETRIC: the caller guarantees C+ == C- for every clip): compiled without the asymmetric loop, which fits
    // 128 VGPRs = 4 waves per SIMD (-4.6 % on the headline, same box); a clip that breaks the guarantee gets NaN planes (loud, never
    // a wrong count)
    // F32W4 (the float32 instances at 4 waves per SIMD): 4 frames in flight like everyone else.  They ran a 2-frame ring as long as the
    // 4-frame one cost 128 VGPRs + 32..48 bytes of scratch; with the lane addresses below as 32-bit offsets on a scalar base it fits
    // (112..125 VGPRs, no scratch) and is worth 2 % on the headline (profiles/esim_ring4/)
    // (uint8 frames are 4 bytes per lane and frame: their ring stays kDepth deep -- with 2 in flight config 4's shape lost 20 %)
    // (1 pixel per work-item: 8 frames in flight -- at 3 waves per SIMD a step is short and 4 frames of look-ahead do not cover the
    // memory latency; -2 % at the training shape, same box)
    constexpr bool F32W4 = (SYMONLY || ASYM4) && IN == kInF32;
    constexpr int kRing = F32W4 ? V2V_ESIM_F32_RING : VEC == 1 ? 8 : kDepth;
    static_assert(NOISE || !EXT, "external noise needs the noise path");
    using lut_t = typename LutT<IN>::type;
    using acc_t = typename std::conditional<OUT64, double, float>::type;
    // float32 bilinear accumulation of 4 pixels: v_pk_fma_f32 on pixel pairs (4 instead of 8 fma per step); the planes
    // stay in consecutive registers for the 16-byte stores
    constexpr bool PK = !OUT64 && BIN == kBinBilinear && VEC == 4;
    extern __shared__ __align__(16) unsigned char s_raw[];
    using ent_t = typename LutEntry<IN>::type;
    constexpr bool ICDF = NOISE && RNG == kRngPhilox;
    // the Gaussian generator's table is a STATIC LDS array in the instances that draw device-native noise: its address is a
    // compile-time constant, so the reads need no base add (-1.7 % against carving it out of the dynamic region, same box)
    float *s_icdf = nullptr;
    if constexpr (ICDF) { __shared__ __align__(16) float s_icdf_static[kIcdfEntries]; s_icdf = s_icdf_static; }
    // the log table and {threshold, low-biased reciprocal} of the ON and the OFF side (16 bytes each: the asymmetric step
    // selects by polarity with ONE 16-byte LDS read per pixel, address = sign bit >> 27, instead of four v_cndmask at 4 cycles
    // each) are static too; only the K- and Tb-sized bilinear tables live in the dynamic region
    __shared__ __align__(16) ent_t s_lut[256];
    __shared__ __align__(16) double s_thr[4];
    // The writer's value histogram (a.stats: the consumer's normalize_batch_voxel needs the 1 % / 99 % k-th values of every sample;
    // SUM-mode integer grids only): +-1 are counted per wave with one ballot each into scalar registers, |v| >= 2 by LDS atomics under
    // a wave-level branch, zeros not at all (derived from the element count) -- 3 compares per stored voxel instead of a 157 MB pass.
    constexpr bool STATS = BIN == kBinSum && !OUT64 && !EXT;
    __shared__ unsigned int s_hist[STATS ? kStatBins : 1];
    // (kernel-argument tests go through readfirstlane: as plain bools the compiler kept them as lane masks and re-materialised them
    // with a v_cndmask + v_cmp pair in every step of the time loop)
    const bool want_stats = STATS && __builtin_amdgcn_readfirstlane((int)(a.stats != nullptr)) != 0;
    uint32_t st_p1 = 0, st_m1 = 0;                                          // wave totals of +1 / -1 (scalar registers)
    acc_t *s_w = reinterpret_cast<acc_t *>(s_raw);         // BILINEAR: {lower-bin weight, upper-bin weight} of pair k at s_w[2k], s_w[2k + 1] (one LDS read per step)
    int *s_kb = reinterpret_cast<int *>(s_w + 2 * a.K);    // [Tb] first pair index of each bin segment

    // ---- workgroup prologue: tables into LDS
    const int clip = blockIdx.x / a.blocks_per_clip;
    const int blk = blockIdx.x - clip * a.blocks_per_clip;
    const uint32_t p0 = (uint32_t)(blk * kBlock + threadIdx.x) * VEC;
    // ONCE: what is uniform over the clip -- the parameter checks, SYMONLY's promise, the reciprocal threshold -- is worked out once per
    // workgroup, by the few lanes that fill s_thr, and handed to the work-items as one LDS flag word and one 16-byte LDS read; the
    // bilinear tables then need a single barrier.  Every work-item used to run a float64 division (~30 vector instructions) and ten
    // float64 compares on these wave-uniform values: -2.1 % on the headline, -2.0 % on its uint8 twin (profiles/esim_setup/).
    // (Not in the noise-free instances: memory-bound, they measured 0.8 % SLOWER with it on the same box and keep the per-lane form.)
    constexpr bool ONCE = NOISE;
    const double *pp = a.params + (int64_t)clip * a.params_stride;
    double c_pos, c_neg, base_std = 0.0, hot_frac = 0.0, hot_std = 0.0;
    uint64_t seed_;
    uint32_t clip_id;
    auto read_clip = [&]() {                                   // the clip's parameters and keys (wave-uniform)
        c_pos = pp[0];
        c_neg = pp[1];
        if constexpr (NOISE) { base_std = pp[2]; hot_frac = pp[3]; hot_std = pp[4]; }
        seed_ = a.clip_keys ? a.clip_keys[2 * clip] : a.seed;
        clip_id = a.clip_keys ? (uint32_t)a.clip_keys[2 * clip + 1] : (uint32_t)(a.clip_id0 + (uint64_t)clip);
    };
    if constexpr (ONCE) read_clip();                           // before anything is written: scalar loads
    if constexpr (ICDF) icdf_to_lds(s_icdf);
    __shared__ int s_bad;                                      // ONCE: the clip's flag word
    if constexpr (ONCE) {
        if (threadIdx.x < 5) {
            // parameters the arithmetic below is not exact for (host lists are checked by the callers; a DEVICE-resident [B,5] table -- the
            // loaders' per-sample draws -- only here): thresholds outside [1e-9, 1e30] (the floor-divide estimate needs |potential| / C < 2^40;
            // zero, negative and NaN thresholds have no meaning in the reference either), negative or non-finite noise parameters; and
            // SYMONLY's promise C+ == C-.  The clip comes out as NaN planes + the statistics' flag word (see poison_clip below).
            const double c = threadIdx.x == 0 ? c_pos : threadIdx.x == 1 ? c_neg : threadIdx.x == 2 ? base_std : threadIdx.x == 3 ? hot_frac : hot_std;
            bool ok = c >= (threadIdx.x < 2 ? 1e-9 : 0.0) && c <= 1e30;
            if constexpr (SYMONLY) ok = ok && c_pos == c_neg;
            const bool any_bad = __builtin_amdgcn_ballot_w64(!ok) != 0;
            if (threadIdx.x < 2) {
                s_thr[2 * threadIdx.x] = c;
                s_thr[2 * threadIdx.x + 1] = (1.0 / c) * 0x1.ffffffffffffcp-1;   // 1/C biased down by 2^-50 so that floor(|p| * inv) never exceeds the true quotient (one-sided correction)
            }
            // bit 1: the clip's parameters do not bound the floor-divide quotient below 2^20, the premise of the low-word screen in the
            // step (kScreen*: after a reset |potential| < C, it starts in [-C-, C+), a table-valued log difference is at most kScreenLogSpread
            // and a deviate of the Gaussian table at most kScreenGaussMax; the product by 2^20 is exact).  Such a clip runs the full check
            // in every step: slower, the same arithmetic.  NaN parameters fail the compare too, and are poison by bit 0 anyway
            const bool unbounded = !(quotient_bound_num(c_pos, c_neg, base_std, hot_std) < 0x1p20 * fmin(c_pos, c_neg));
            if (threadIdx.x == 0) s_bad = (int)any_bad | (unbounded ? 2 : 0);
        }
    } else if (threadIdx.x < 2) {
        const double c = pp[threadIdx.x];
        s_thr[2 * threadIdx.x] = c;
        s_thr[2 * threadIdx.x + 1] = (1.0 / c) * 0x1.ffffffffffffcp-1;       // same expression as inv_pos below
    }
    if constexpr (IN == kInU8) s_lut[threadIdx.x] = g_lut_esim64[threadIdx.x];
    else s_lut[threadIdx.x] = make_float2(g_lut_esim32[threadIdx.x], (float)threadIdx.x);
    if constexpr (STATS) {
        if (want_stats) for (int i = threadIdx.x; i < kStatBins; i += kBlock) s_hist[i] = 0;
    }
    int *s_fidx = reinterpret_cast<int *>(s_raw);              // FIDX: [K + 1] stored-frame numbers of this clip
    int fidx_bad = 0;                                          // this work-item saw an index / a clip extent out of bounds
    if constexpr (FIDX) {
        const int cb = blockIdx.x / a.blocks_per_clip;
        const int32_t *row = a.frame_index + (int64_t)cb * (a.K + 1);
        const int stored = a.stored_frames ? a.stored_frames[cb] : 0x7FFFFFFF;
        for (int i = threadIdx.x; i <= a.K; i += kBlock) {
            const int f = row[i];
            fidx_bad |= (int)(stored < 1 || (unsigned)f >= (unsigned)stored);   // negative or >= stored (the reference's gather cannot, v2v_datasets.py:286-311); a negative stored count is poison whatever frames_elems says
            s_fidx[i] = f;
        }
        if (a.stored_frames && a.frames_elems > 0 && threadIdx.x == 0) {
            const int64_t off = a.clip_offsets[cb];
            fidx_bad |= (int)(stored < 1 || off < 0 || off + (int64_t)(stored - 1) * a.frame_stride + a.HW > a.frames_elems);
        }
    }
    auto foff = [&](int f) -> int64_t {                        // element offset of simulator frame f inside the clip
        if constexpr (FIDX) return (int64_t)s_fidx[f] * a.frame_stride;
        else return (int64_t)f * a.frame_stride;
    };
    if constexpr (BIN == kBinBilinear) {
        // Pair k contributes to bins seg(k) and seg(k)+1 with the float64 weights of event_utils.py:715-719:
        // t_norm = (k - 0)/((K-1) - 0)*(Tb-1), w_b = max(0, 1 - |t_norm - b|); every other bin's weight is exactly 0.
        auto t_of = [&](int k) { return ((double)k - 0.0) / ((double)(a.K - 1) - 0.0) * (double)(a.Tb - 1); };
        auto seg_of = [&](double t_norm) {
            int b0 = (int)floor(t_norm);
            if (b0 > a.Tb - 2) b0 = a.Tb - 2;
            return b0 < 0 ? 0 : b0;
        };
        if constexpr (ONCE) {
            // s_kb[b] = first pair of segment b.  The loop below writes entries 1 .. Tb - 2, each exactly once (seg() runs from 0 at k = 0
            // to Tb - 2 at k = K - 1 without decreasing); the two it never reaches are set here: no initialising pass, no barrier in between
            if (threadIdx.x == 0) { s_kb[0] = 0x7FFFFFFF; s_kb[a.Tb - 1] = 0x7FFFFFFF; }
        } else {
            for (int b = threadIdx.x; b < a.Tb; b += kBlock) s_kb[b] = 0x7FFFFFFF;
            __syncthreads();
        }
        for (int k = threadIdx.x; k < a.K; k += kBlock) {
            const double t_norm = t_of(k);
            const int b0 = seg_of(t_norm);
            const double wl = 1.0 - fabs(t_norm - (double)b0);
            const double wh = 1.0 - fabs(t_norm - (double)(b0 + 1));
            s_w[2 * k] = (acc_t)(wl > 0.0 ? wl : 0.0);
            s_w[2 * k + 1] = (acc_t)(wh > 0.0 ? wh : 0.0);
            const int bprev = k > 0 ? seg_of(t_of(k - 1)) : 0;
            for (int b = bprev + 1; b <= b0; ++b) s_kb[b] = k;          // seg() is non-decreasing in k
        }
    }
    bool clip_bad = false;
    if constexpr (FIDX) clip_bad = __syncthreads_or(fidx_bad) != 0;       // every workgroup of the clip stages the same row: all agree
    else __syncthreads();

    if (p0 >= (uint32_t)a.HW) return;
    // output planes may be padded (row pitch >= W, plane size >= pitch * H: the consumer's x16 padding written in place); the
    // VEC pixels of a work-item share a row (VEC == 4 needs W % 4 == 0), and a plane is stored a handful of times per clip
    const int64_t pix_off = (a.out_pitch == a.W) ? (int64_t)p0 : (int64_t)(p0 / (uint32_t)a.W) * a.out_pitch + (p0 % (uint32_t)a.W);

    // a clip whose inputs break a promise (parameters outside their domain; V2V_FLAG_SYMMETRIC with C+ != C-; a frame index outside the
    // clip): NaN planes + the statistics' kStatBad word -- loud, never a wrong count, never an out-of-bounds read
    auto poison_clip = [&]() {
        using pacc_t = typename std::conditional<OUT64, double, float>::type;
        pacc_t bad[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) bad[j] = (pacc_t)__builtin_nanf("");
        const int64_t planes = (BIN == kBinSum) ? (a.K / a.fpb) : a.Tb;
        for (int64_t pl = 0; pl < planes; ++pl) store_vec<VEC, pacc_t>(a.out, (int64_t)clip * planes * a.out_plane + pl * a.out_plane + pix_off, bad);
        if constexpr (BIN == kBinSum && !OUT64 && !EXT) {
            if (a.stats != nullptr && p0 == 0) atomicExch(&a.stats[(int64_t)clip * kStatWords + kStatBad], 1u);
        }
    };
    if constexpr (FIDX) {
        if (clip_bad) { poison_clip(); return; }                       // workgroup-uniform
    }

    // symmetric clips keep the threshold and its (slightly low) reciprocal in VGPRs; asymmetric ones read s_thr by polarity.
    // 1/C biased down by 2^-50 so that floor(|p| * inv) never exceeds the true quotient (one-sided correction)
    double pos, inv_pos;
    // SCREEN: the step finds the rare floor-divide fix-up on the low word of the quotient estimate (see kScreen* above).  Replayed noise
    // fields are arbitrary host float64 deviates, which no table bounds: those instances keep the full check in every step.
    // screen_min: the smallest low word that sends a wave into the fix-up's check -- one wave-uniform scalar register.  kScreenLowWord
    // normally; 0 in a PARANOID wave, which then runs the full check in every step (slower, the same arithmetic): the clip's parameters
    // do not bound the quotient, or (sticky, set by pix_logs' slow path) a frame value left the log table
    constexpr bool SCREEN = V2V_ESIM_SCREEN && RNG != kRngReplay && (NOISE || V2V_ESIM_SCREEN_NOISE_FREE);
    uint32_t screen_min = kScreenLowWord;
    if constexpr (ONCE) {
        const int flags = __builtin_amdgcn_readfirstlane(s_bad);       // clip-uniform: bit 0 poison, bit 1 quotient not bounded
        if ((flags & 1) != 0) { poison_clip(); return; }
        if constexpr (SCREEN) screen_min = (flags & 2) != 0 ? 0u : kScreenLowWord;
        pos = s_thr[0];                                                // the same bits by the same expression, computed once
        inv_pos = s_thr[1];
    } else {
        read_clip();
        pos = c_pos;
        inv_pos = (1.0 / pos) * 0x1.ffffffffffffcp-1;
        // (the per-lane form of the checks the ONCE instances make while they fill s_thr; clip-uniform branch)
        if (!(c_pos >= 1e-9 && c_pos <= 1e30 && c_neg >= 1e-9 && c_neg <= 1e30)) { poison_clip(); return; }
        if constexpr (SCREEN) {
            const bool unbounded = !(quotient_bound_num(c_pos, c_neg, 0.0, 0.0) < 0x1p20 * fmin(c_pos, c_neg));
            screen_min = __builtin_amdgcn_readfirstlane((int)unbounded) != 0 ? 0u : kScreenLowWord;
        }
    }
    asm volatile("" : "+v"(pos), "+v"(inv_pos));
    // F32W4: addresses = a wave-uniform part (clip, frame / plane: scalar registers) + the lane's own 32-bit byte offset (the C entry
    // bounds H*W and the plane size), so that no 64-bit lane address lives across the time loop (docs/experiments, "scalar-base
    // addresses": timing-neutral by itself; here it is wanted for its registers -- 4 to 6 per instance, what the 4-frame ring was short of)
    uint32_t lane_in = p0 * (uint32_t)(IN == kInF32 ? 4 : 1), lane_out = (uint32_t)pix_off * (uint32_t)sizeof(acc_t);
    const int64_t in_base = (FIDX ? a.clip_offsets[clip] : (int64_t)clip * a.clip_stride) + (F32W4 ? 0 : p0);
    auto load_frame = [&](int f) {
        if constexpr (F32W4) return load_raw_at<IN, VEC>(a.frames, in_base + foff(f), lane_in);
        else return load_raw<IN, VEC>(a.frames, in_base + foff(f));
    };
    auto store_plane = [&](int64_t uniform_off, const acc_t (&v)[VEC]) {       // uniform_off: element offset of the plane (clip, bin)
        if constexpr (F32W4) store_vec_at<VEC, acc_t>(a.out, uniform_off, lane_out, v);
        else store_vec<VEC, acc_t>(a.out, uniform_off + pix_off, v);
    };

    // ---- per-pixel state
    double pot[VEC];
    double hot[NOISE ? VEC : 1];
    {
        double u0[VEC];
        if constexpr (RNG == kRngPhilox) {
            field_uniform53<VEC>(seed_, clip_id, kFieldPotInit, kStreamEsim, p0, u0);
        } else if constexpr (RNG == kRngReplay) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) u0[j] = a.u_init[(int64_t)clip * a.HW + p0 + j];
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) u0[j] = 0.5;
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const double scaled = u0[j] * (c_pos + c_neg);
            pot[j] = scaled - c_neg;                                   // v2v_core_esim.py:29
        }
        if constexpr (NOISE) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) hot[j] = 0.0;
            if constexpr (RNG == kRngPhilox) {
                if (hot_frac > 0.0) {                                  // uniform: skipping is exact (u >= 0)
                    double u1[VEC];
                    field_uniform53<VEC>(seed_, clip_id, kFieldHotMask, kStreamEsim, p0, u1);
                    bool mine = false;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) mine = mine || (u1[j] < hot_frac);
                    // the Gaussian field of the hot pixels (a Philox-10 block + table lookups) only in waves that own one: with the
                    // reference's hot_pixel_fraction of 1e-3 that is one wave in four; the others keep hot = 0 exactly as before
                    if (__builtin_amdgcn_ballot_w64(mine) != 0) {
                        float gh[VEC], gh_unused[VEC];
                        field_gauss_pairs<VEC>(seed_, clip_id, kFieldHotGauss, kStreamEsim, p0, s_icdf, gh, gh_unused);
#pragma unroll
                        for (int j = 0; j < VEC; ++j) hot[j] = (u1[j] < hot_frac) ? hot_std * (double)gh[j] : 0.0;   // :37-39
                    }
                }
            } else if constexpr (RNG == kRngReplay) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int64_t o = (int64_t)clip * a.HW + p0 + j;
                    hot[j] = (a.u_hot[o] < hot_frac) ? hot_std * a.g_hot[o] : 0.0;
                }
            }
        }
    }

    lut_t lprev[VEC];
    {
        const Raw<IN, VEC> r0 = load_frame(0);
        pix_logs<IN, VEC>(r0, s_lut, lprev, screen_min);
    }

    // ---- binning state
    acc_t acc_lo[VEC], acc_hi[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { acc_lo[j] = 0; acc_hi[j] = 0; }
    // plane of the lower bin leaves the accumulators, the upper bin becomes the lower one
    auto flush_lower = [&](int seg) {
        store_plane(((int64_t)clip * a.Tb + seg) * a.out_plane, acc_lo);
#pragma unroll
        for (int j = 0; j < VEC; ++j) { acc_lo[j] = acc_hi[j]; acc_hi[j] = 0; }
    };
    int cur_seg = 0;          // BILINEAR: bin index acc_lo belongs to (wave-uniform)
    int next_k = 0x7FFFFFFF;  // BILINEAR: first pair of segment cur_seg+1 (wave-uniform, kept scalar)
    if constexpr (BIN == kBinBilinear) {
        if (a.Tb >= 3) next_k = __builtin_amdgcn_readfirstlane(s_kb[1]);
    }
    int sub = 0, plane = 0;   // SUM: pairs accumulated into the current plane, plane index
    const int64_t planes_per_clip = (BIN == kBinSum) ? (a.K / a.fpb) : a.Tb;
    const int64_t out_base = (int64_t)clip * planes_per_clip * a.out_plane;        // wave-uniform
    uint32_t n_all = 0, n_off = 0;
    const bool want_counts = a.counts != nullptr;

    const bool has_base = __builtin_amdgcn_readfirstlane((int)(base_std != 0.0)) != 0;   // per clip: a scalar branch
    // base-noise normals of the odd pair of each (even, odd) couple of time steps: one Philox block and four
    // table-inversion deviate pairs (the two 16-bit halves of a word, v2v_rng.hpp) feed 4 pixels x 2 steps; drawn at the even step, consumed at the odd one
    float g_pend[NOISE ? VEC : 1];
#pragma unroll
    for (int j = 0; j < (NOISE ? VEC : 1); ++j) g_pend[j] = 0.0f;
    // 1 pixel per work-item (small batches): the four lanes of a pixel quad need the SAME Philox block every other step and use
    // one word of it each.  Instead of four identical blocks per couple of steps, lane j of the quad computes the block of couple
    // c0 + j once per 8 steps and a 4x4 transpose inside the quad (two DPP quad_perm exchanges) hands every lane its own word of
    // all four blocks: a quarter of the Philox work, bit-identical fields.  Needs whole quads (H*W % 4 == 0; else the plain path).
    uint32_t gw0 = 0, gw1 = 0, gw2 = 0, gw3 = 0;
    const bool share_quads = VEC == 1 && (a.HW & 3) == 0;

    // SYM (compile-time tag): C+ == C- for this clip (wave-uniform), so no per-lane threshold selection.
    // PAR (compile-time tag): k & 1 -- the time loop is unrolled by an even factor from an even k.
    // 1 pixel per work-item: log intensity of the frame the NEXT step consumes, looked up one step ahead (see the step)
    lut_t ln_pre[VEC];
    auto step = [&](auto sym_tag, auto hot_tag, auto par_tag, int k, const Raw<IN, VEC> &raw, const Raw<IN, VEC> &raw_next) __attribute__((always_inline)) {
        constexpr bool SYM = decltype(sym_tag)::value;
        constexpr bool HOT = decltype(hot_tag)::value;     // false: no work-item of this WAVE owns a hot pixel -> no hot-pixel add
        constexpr int PAR = decltype(par_tag)::value;
        if constexpr (BIN == kBinBilinear) {
            while (k >= next_k) {                                      // scalar compare; rarely taken
                flush_lower(cur_seg);
                ++cur_seg;
                next_k = (cur_seg + 1 <= a.Tb - 2) ? __builtin_amdgcn_readfirstlane(s_kb[cur_seg + 1]) : 0x7FFFFFFF;
            }
        }
        // 1 pixel per work-item (small batches, 3 waves per SIMD, a wave issues in order): this step's log intensity was looked up during
        // the previous step and the next step's lookup is issued here, so that its LDS round trip runs under a whole step instead of
        // parking the wave in front of the potential update; with 4 pixels the lookups' registers would be live across the step for nothing
        lut_t ln[VEC];
        if constexpr (VEC == 1) {
            ln[0] = ln_pre[0];
            pix_logs<IN, VEC>(raw_next, s_lut, ln_pre, screen_min);
        }
        double base[NOISE ? VEC : 1];
        if constexpr (NOISE) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) base[j] = 0.0;
            if constexpr (RNG == kRngPhilox) {
                // (internal noise: no `base_std != 0` branch -- 0 * g is +-0 and p + (+-0) is p bit for bit, because p = pot + d is never
                // -0.0; the branch cost four register clears per step.  External noise adds to the voxel, where -0.0 occurs: branch kept)
                if (!EXT || has_base) {
                    float g[VEC];
                    if constexpr (PAR == 0) {
                        if (VEC == 1 && share_quads) {
                            if ((k & 7) == 0) {                                // wave-uniform: a new period of four couples
                                const uint32_t lq = p0 & 3u;
                                const u32x4 w = philox4x32<kNoiseRounds>(p0 >> 2, kFieldBase0 + (uint32_t)(k >> 1) + lq, clip_id, kStreamEsim,
                                                                        (uint32_t)seed_, (uint32_t)(seed_ >> 32));
                                uint32_t w0 = w.x, w1 = w.y, w2 = w.z, w3 = w.w;   // lane r of the quad: words of couple c0 + r
                                const bool odd = (lq & 1u) != 0, upper = (lq & 2u) != 0;
                                auto xchg = [](uint32_t v, auto ctrl_tag) {
                                    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, decltype(ctrl_tag)::value, 0xF, 0xF, true);
                                };
                                // 2x2 blocks between lanes l and l ^ 1 (quad_perm [1,0,3,2] = 0xB1), then between l and l ^ 2 ([2,3,0,1] = 0x4E)
                                { const uint32_t y = xchg(odd ? w0 : w1, std::integral_constant<int, 0xB1>{}); if (odd) w0 = y; else w1 = y; }
                                { const uint32_t y = xchg(odd ? w2 : w3, std::integral_constant<int, 0xB1>{}); if (odd) w2 = y; else w3 = y; }
                                { const uint32_t y = xchg(upper ? w0 : w2, std::integral_constant<int, 0x4E>{}); if (upper) w0 = y; else w2 = y; }
                                { const uint32_t y = xchg(upper ? w1 : w3, std::integral_constant<int, 0x4E>{}); if (upper) w1 = y; else w3 = y; }
                                gw0 = w0; gw1 = w1; gw2 = w2; gw3 = w3;            // this pixel's word for couples c0 .. c0 + 3
                            }
                            // the couple's word is always gw0: the four words rotate by one after each use (plain moves the unrolled loop
                            // renames away).  NOT `sel == 0 ? gw0 : sel == 1 ? gw1 : ...`: the compiler turned that chain over the by-reference
                            // captures into a run-time index into the lambda's closure object, which pinned the closure and every captured
                            // local -- the whole argument struct included -- to scratch memory (560 bytes, 2,262 scratch instructions in the
                            // <float32, 1 pixel, SUM, device noise> instance of round 4; tests/test_kernel_resources.py refuses any scratch now)
                            const uint32_t word = gw0;
                            gw0 = gw1; gw1 = gw2; gw2 = gw3; gw3 = word;
                            icdf_pair(word, s_icdf, g[0], g_pend[0]);
                        } else
                        field_gauss_pairs<VEC, kNoiseRounds>(seed_, clip_id, kFieldBase0 + (uint32_t)(k >> 1), kStreamEsim, p0, s_icdf, g, g_pend);
                    } else {
#pragma unroll
                        for (int j = 0; j < VEC; ++j) g[j] = g_pend[j];
                    }
#pragma unroll
                    for (int j = 0; j < VEC; ++j) base[j] = base_std * (double)g[j];   // :44
                }
            } else if constexpr (RNG == kRngReplay) {
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    base[j] = base_std * a.g_base[((int64_t)clip * a.K + k) * a.HW + p0 + j];
            }
        }
        acc_t wl = 1, wh = 0;
        if constexpr (BIN == kBinBilinear) {
            typedef acc_t w2_t __attribute__((ext_vector_type(2)));
            const w2_t w2 = *reinterpret_cast<const w2_t *>(s_w + 2 * k);
            wl = w2.x;
            wh = w2.y;
        }

        if constexpr (VEC != 1) pix_logs<IN, VEC>(raw, s_lut, ln, screen_min);

        // Branch-free per pixel: q = np.floor_divide(|p|, C) is 0 exactly when |p| < C, so the reference's
        // `where(p >= C+ ...)` / `where(p <= -C- ...)` masks (v2v_core_esim.py:51-55) need no separate test,
        // and `p -= q*C` with q = 0 leaves p untouched bit for bit.  The VEC pixels are independent chains.
        // Phase A: new potential, polarity, reciprocal quotient estimate and its sign-exact fma residual.
        double mag[VEC], thr[VEC], q[VEC], r[VEC];
        unsigned long long fix = 0;                                    // wave-level mask in an SGPR pair (no per-lane bool)
        uint32_t ulo = 0;                                              // SCREEN: largest low word of the VEC quotient estimates
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const lut_t d = ln[j] - lprev[j];                          // difference in the input's precision (:42)
            lprev[j] = ln[j];
            double p = pot[j] + (double)d;                             // :43
            // :48-49.  (Skipping the hot-pixel add for waves without a hot pixel is exact -- x + (+0.0) is x unless x is -0.0,
            // which a round-to-nearest sum with the never-negative-zero log difference cannot be -- but the scalar branch
            // costs more than the four adds: +2.5 % on the same box, round 2.)
            if constexpr (NOISE && !EXT) { p = p + base[j]; if constexpr (HOT) p = p + hot[j]; }
            // The whole chain in SIGNED form: trunc, the rounded product, the fma and the subtraction are odd functions under
            // round-to-nearest, so q = sign(p) * floor(|p| / C), the residual and the new potential come out with p's sign and the
            // magnitudes of the unsigned form bit for bit -- no sign extraction for the arithmetic, no sign re-insertion into the
            // potential and the count (round 5: -3 vector instructions per pixel-step with C+ == C-, -2 otherwise).  An exact-zero
            // residual is +0.0 here (as in NumPy's `potential += neg * C`) where the unsigned form gave -0.0 for negative p:
            // invisible either way, pot + d is the same sum for both (d is never -0.0).
            double inv;
            if constexpr (SYM) { thr[j] = pos; inv = inv_pos; }
            else {                                                     // {C, 1/C} of the polarity: one 16-byte LDS read at (sign bit) * 16
                const double2 ti = *reinterpret_cast<const double2 *>(reinterpret_cast<const unsigned char *>(s_thr) + (((uint32_t)__double2hiint(p) >> 27) & 16u));
                thr[j] = ti.x;
                inv = ti.y;
            }
            mag[j] = p;
            // inv is biased low, so the estimate never exceeds the true quotient in magnitude; it is short by one only when
            // |p|/C sits within ~1e-15 above an integer -- and then (or for a NaN potential) |r| < C fails
            const double u = p * inv;
            q[j] = trunc(u);
            if constexpr (SCREEN) {
                // ... and then, with |u| < 2^20, the top 24 bits of u's low word are all ones: the residual and its compare wait for
                // the rare branch, the hot path keeps an unsigned maximum over the work-item's pixels
                const uint32_t lo = (uint32_t)__double2loint(u);
                ulo = j == 0 ? lo : (lo > ulo ? lo : ulo);
            } else {
                r[j] = __builtin_fma(-q[j], thr[j], p);
                fix |= __ballot(!(fabs(r[j]) < thr[j]));
            }
        }
        if constexpr (SCREEN) fix = __ballot(ulo >= screen_min);
        if (__builtin_expect(fix != 0, 0)) {                                // rare: exact multiples, NaN; a paranoid wave in every step
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                if constexpr (SCREEN) r[j] = __builtin_fma(-q[j], thr[j], mag[j]);   // here, pixel by pixel: one residual live at a time
                if (fabs(r[j]) >= thr[j]) q[j] += signed_one(r[j]);
                // NaN potential: NumPy's compares are false -> no events.  INFINITE potential (a +-inf or overflowing frame value): the compare
                // passes and np.floor_divide(inf, C) is NaN (fmod(inf, C)), so the reference counts NaN in this step and the potential is NaN
                // from then on (v2v_core_esim.py:51-58) -- q = NaN reproduces both through q * C and the accumulate
                else if (!(fabs(r[j]) < thr[j])) q[j] = __builtin_isinf(mag[j]) ? __builtin_nan("") : 0.0;
            }
        }
        // Phase B: reset the potential (v2v_core_esim.py:57-58), signed count, binning.
        float qabs[VEC];
        float vfs[PK ? VEC : 1];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const double qt = q[j] * thr[j];
            const double m2 = mag[j] - qt;                             // product rounded, then subtracted (no fma)
            pot[j] = m2;
            // (F32W4, at their 128-VGPR budget: the reset stays in its own step.  Without the residual's compare in front of it the compiler
            // sank it into the next step, which keeps q and the old potential of all four pixels live across the branch and spilled)
            if constexpr (SCREEN && F32W4) asm volatile("" : "+v"(pot[j]));
            if constexpr (OUT64) {
                double vox = q[j];
                qabs[j] = __builtin_fabsf((float)q[j]);
                if constexpr (EXT) { vox = vox + base[j]; vox = vox + hot[j]; }   // :64-65
                if constexpr (BIN == kBinBilinear) {
                    const double cl = vox * wl, ch = vox * wh;         // bincount adds ps*w (no fma)
                    acc_lo[j] = acc_lo[j] + cl;
                    acc_hi[j] = acc_hi[j] + ch;
                } else {
                    acc_lo[j] = acc_lo[j] + vox;
                }
            } else {
                const float qf = (float)q[j];
                qabs[j] = __builtin_fabsf(qf);
                float vf = qf;
                if constexpr (EXT) { double vox = (double)vf; vox = vox + base[j]; vox = vox + hot[j]; vf = (float)vox; }
                if constexpr (PK) {
                    vfs[j] = vf;
                } else if constexpr (BIN == kBinBilinear) {
                    acc_lo[j] = __builtin_fmaf(vf, wl, acc_lo[j]);
                    acc_hi[j] = __builtin_fmaf(vf, wh, acc_hi[j]);
                } else {
                    acc_lo[j] = acc_lo[j] + vf;
                }
            }
        }
        if constexpr (PK) {
#pragma unroll
            for (int j = 0; j < VEC; j += 2) {
                const f32x2 v2 = f32x2{vfs[j], vfs[j + 1]};
                const f32x2 lo = pk_fma(v2, pk_splat((float)wl), f32x2{(float)acc_lo[j], (float)acc_lo[j + 1]});
                const f32x2 hi = pk_fma(v2, pk_splat((float)wh), f32x2{(float)acc_hi[j], (float)acc_hi[j + 1]});
                acc_lo[j] = lo.x; acc_lo[j + 1] = lo.y; acc_hi[j] = hi.x; acc_hi[j + 1] = hi.y;
            }
        }
        const unsigned long long *cp = a.counts;                       // the kernel argument (a scalar register pair), re-tested in every step: as a
        asm("" : "+s"(cp));                                            // bool hoisted out of the loop it lived as a lane mask and cost a v_cndmask +
        if (cp != nullptr) {                                           // v_cmp per step.  Wave-uniform
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const uint32_t n = (uint32_t)qabs[j];
                n_all += n;
                n_off += q[j] < 0.0 ? n : 0u;
            }
        }
        if constexpr (BIN == kBinSum) {
            if (++sub == a.fpb) {                                      // wave-uniform
                store_plane(out_base + (int64_t)plane * a.out_plane, acc_lo);
                if constexpr (STATS) {
                    if (want_stats) {                                  // wave-uniform
#pragma unroll
                        for (int j = 0; j < VEC; ++j) {
                            const float v = (float)acc_lo[j];
                            st_p1 += (uint32_t)__popcll(__ballot(v == 1.0f));
                            st_m1 += (uint32_t)__popcll(__ballot(v == -1.0f));
                            if (__builtin_fabsf(v) >= 2.0f) {              // exec-masked region; skipped by the wave when no lane is in
                                const int iv = (int)v;                     // saturating convert; the clamp keeps hot pixels in the overflow bins
                                atomicAdd(&s_hist[(iv < -kStatMax - 1 ? -kStatMax - 1 : iv > kStatMax + 1 ? kStatMax + 1 : iv) + kStatZero], 1u);
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc_lo[j] = 0;
                sub = 0;
                ++plane;
            }
        }
    };

    // ---- time loop: ring of kDepth frames in registers; each slot is reloaded right after it is consumed, so
    //      kDepth-1 loads (x 1 KiB per wave for fp32 input) stay in flight behind the arithmetic.  Loads are
    //      UNCONDITIONAL (frame index clamped to the last frame) so the compiler can count them and wait with
    //      vmcnt(kDepth-1) instead of vmcnt(0); the kDepth clamped re-reads at the end of a clip hit in cache.
    auto tail = [&](auto sym_tag, auto hot_tag, int k0, const Raw<IN, VEC> (&ring)[kRing]) {
        // up to kRing-1 remaining steps, with compile-time slot index (and parity)
        static_for(std::make_integer_sequence<int, kRing - 1>{}, [&](auto u_tag) {
            constexpr int u = decltype(u_tag)::value;
            if (k0 + u < a.K) step(sym_tag, hot_tag, std::integral_constant<int, (u & 1)>{}, k0 + u, ring[u], ring[u + 1]);
        });
    };
    auto run_hot = [&](auto sym_tag, auto hot_tag) {
        static_assert(kRing % 2 == 0, "the time loop must be unrolled by an even factor (noise pairs)");
        Raw<IN, VEC> ring[kRing];
#pragma unroll
        for (int u = 0; u < kRing; ++u) {
            const int f = (1 + u <= a.K) ? 1 + u : a.K;
            ring[u] = load_frame(f);
        }
        if constexpr (VEC == 1) pix_logs<IN, VEC>(ring[0], s_lut, ln_pre, screen_min);
        int k0 = 0;
        for (; k0 + kRing <= a.K; k0 += kRing) {
            static_for(std::make_integer_sequence<int, kRing>{}, [&](auto u_tag) {
                constexpr int u = decltype(u_tag)::value;
                const int k = k0 + u;
                step(sym_tag, hot_tag, std::integral_constant<int, (u & 1)>{}, k, ring[u], ring[(u + 1) % kRing]);
                const int fn = k + 1 + kRing;
                ring[u] = load_frame(fn <= a.K ? fn : a.K);
            });
        }
        tail(sym_tag, hot_tag, k0, ring);
    };
    // Hot pixels are 0.1 % of the pixels (hot_pixel_fraction <= 1e-3 in the reference's defaults and in the dataset's draws):
    // 3 of 4 waves own none, and for them `p + hot` adds +0.0 to a sum that is never -0.0 (a round-to-nearest sum with the
    // never-negative-zero log difference), i.e. nothing.  The choice is made ONCE per wave and clip -- two copies of the time loop
    // in the device-noise instances -- not per step (round 2 measured a per-step scalar branch: +2.5 %, worse than the adds).
    // (not in the general float32 bilinear instance: the second loop copy costs it 2 spilled registers at its 128-VGPR budget and
    // measured no gain there)
    constexpr bool HOT_SPLIT = NOISE && !EXT && RNG == kRngPhilox && !OUT64 && !(ASYM4 && IN == kInF32 && BIN == kBinBilinear);
    bool wave_has_hot = true;
    if constexpr (HOT_SPLIT) {
        bool mine = false;
#pragma unroll
        for (int j = 0; j < VEC; ++j) mine = mine || (hot[j] != 0.0);
        wave_has_hot = __builtin_amdgcn_ballot_w64(mine) != 0;
    }
    auto run = [&](auto sym_tag) {
        if constexpr (HOT_SPLIT) {
            if (wave_has_hot) run_hot(sym_tag, std::true_type{});
            else run_hot(sym_tag, std::false_type{});
        } else {
            run_hot(sym_tag, std::true_type{});
        }
    };
    if constexpr (SYMONLY) {
        static_assert(!SYMONLY || ONCE, "the flag word carries the C+ == C- promise");   // a broken one poisoned the clip above
        run(std::true_type{});
    } else if constexpr (ASYM4) {
        run(std::false_type{});
    } else {
        if (c_pos == c_neg) run(std::true_type{});                     // wave-uniform (per clip)
        else run(std::false_type{});
    }

    // ---- epilogue
    if constexpr (BIN == kBinBilinear) {
        flush_lower(cur_seg);
        if (cur_seg + 1 < a.Tb) flush_lower(cur_seg + 1);
        for (int b = cur_seg + 2; b < a.Tb; ++b) flush_lower(b);       // zeros by now
    }
    if constexpr (STATS) {
        if (want_stats) {
            // lanes past the end of the clip left above; a wave that is still here has its lane 0.  Finished waves do not hold the barrier.
            if ((threadIdx.x & 63) == 0) {
                if (st_p1) atomicAdd(&s_hist[kStatZero + 1], st_p1);
                if (st_m1) atomicAdd(&s_hist[kStatZero - 1], st_m1);
            }
            __syncthreads();
            // only the work-items that own pixels are still here (the last workgroup of a clip may be partly empty): stride by their number
            const int left = (a.HW - blk * kBlock * VEC + VEC - 1) / VEC, n_act = left < kBlock ? left : kBlock;
            unsigned int *gs = a.stats + (int64_t)clip * kStatWords;
            for (int i = threadIdx.x; i < kStatBins; i += n_act)
                if (s_hist[i]) atomicAdd(&gs[i], s_hist[i]);
        }
    }
    const uint32_t n_on = n_all - n_off;
    if (want_counts) {
        // wave64 reduction over the lanes that own pixels, then one 64-bit atomic per wave and polarity
        unsigned long long on = n_on, off = n_off;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const unsigned long long o1 = __shfl_down(on, s, 64);
            const unsigned long long o2 = __shfl_down(off, s, 64);
            const int src = (int)(threadIdx.x & 63) + s;
            const bool src_active = src < 64 && (uint32_t)((blk * kBlock + (threadIdx.x & ~63) + src)) * VEC < (uint32_t)a.HW;
            if (src_active) { on += o1; off += o2; }
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&a.counts[2 * clip], on);
            atomicAdd(&a.counts[2 * clip + 1], off);
        }
    }
}

}  // namespace v2v
