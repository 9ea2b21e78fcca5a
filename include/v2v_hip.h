/*
 * v2v_hip.h -- C ABI of libv2v_hip.so: the MI355X (gfx950) video -> event-count -> voxel-grid hot path.
 *
 * This is the drop-in boundary for the one accelerated path of HYLZ-2019/V2V (reference paths below are
 * relative to the reference checkout).  Every entry point replaces a Python/NumPy function of the
 * reference; a reference maintainer binds it with a ctypes stub (INTEGRATION.md shows each one).
 *
 * Conventions
 *   - All buffer arguments are DEVICE pointers owned by the caller (PyTorch tensors on the host side).
 *     The library never allocates, frees or retains caller-visible memory.
 *   - Every call is asynchronous on the caller's HIP stream (`stream` is a hipStream_t passed as void*;
 *     NULL = the default stream) and never synchronises.
 *   - Return value: 0 (V2V_OK) or a negative v2v_status.  No exceptions, no aborts.  A human-readable
 *     message for the last failure on the calling thread is available from v2v_last_error(): one slot per
 *     thread for every entry point of the library, whichever family it belongs to.
 *   - No global mutable state except the log-intensity tables (v2v_lut_set) and the per-thread error slot.
 *   - There is NO CPU implementation behind this ABI.  Without a GPU every compute entry point
 *     returns V2V_ERR_HIP.
 */
#ifndef V2V_HIP_H
#define V2V_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: every device-native (V2V_RNG_PHILOX) random stream differs from ABI 1 for the same (seed, clip id): Gaussians by
 *    table inversion (was Box-Muller), Philox4x32-7 for per-step fields, two time steps per Gaussian field id; the v2e
 *    shot-noise sampler and its fields changed again in round 3; v2v_v2e_workspace_bytes and v2v_postops_workspace_bytes
 *    grew; v2v_lut_set acts on the current device only (a single-process multi-GPU host calls it once per device).  The
 *    front-end's `gray_first` was RE-MAPPED: 1 now selects OpenCV 4.x's 15-bit BGR2GRAY weights (3735 / 19235 / 9798, >> 15);
 *    the 14-bit OpenCV 2.x/3.x form that ABI 1 ran for gray_first = 1 moved to gray_first = 2 -- an ABI-1 caller passing 1 gets
 *    different gray values on some colours, with no error.  A client must re-query workspace sizes and cannot replay ABI-1
 *    native noise.  Replay-mode (V2V_RNG_REPLAY) results are unchanged.
 * 3: v2v_esim_extras grew two trailing fields (stored_frames, frames_elems: the bounds of the frame_index gather).  Every function
 *    signature and every result of ABI 2 is unchanged; a caller that fills v2v_esim_extras must be recompiled (or zero the struct at
 *    its new size): an ABI-2 struct is 16 bytes shorter.
 * 6: nine new entry points, the 16-channel layer family (FireNet): v2v_convgru16_*, v2v_resblock16_*, v2v_conv_head16_*.  Every signature and
 *    result of ABI 5 is unchanged. */
#define V2V_ABI_VERSION 6

typedef enum v2v_status {
    V2V_OK = 0,
    V2V_ERR_NULL = -1,   /* a required pointer is NULL                                              */
    V2V_ERR_SHAPE = -2,  /* B,N,H,W out of range, N < 2, strides smaller than the extent            */
    V2V_ERR_BINS = -3,   /* SUM: (N-1) % (num_bins*frames_per_bin) != 0  (v2v_datasets.py:365)      */
    V2V_ERR_DTYPE = -4,  /* unsupported in/out dtype                                                */
    V2V_ERR_MODE = -5,   /* unknown rng / bin mode, or replay fields missing in replay mode         */
    V2V_ERR_ALIGN = -6,  /* pointer not aligned for its element type                                */
    V2V_ERR_HIP = -7,    /* HIP runtime error (launch failed, no device); see v2v_last_error()      */
    V2V_ERR_PARAM = -8   /* invalid scalar parameter                                                */
} v2v_status;

typedef enum v2v_dtype { V2V_U8 = 0, V2V_F32 = 1, V2V_F64 = 2, V2V_BF16 = 3 /* consumer-side entry points only */ } v2v_dtype;

/* Where the simulator's random fields come from (reference: global np.random, v2v_core_esim.py:29,37,38,44) */
typedef enum v2v_rng_mode {
    V2V_RNG_NONE = 0,   /* deterministic debug mode: u_init = 0.5, no hot pixels, all Gaussians 0      */
    V2V_RNG_PHILOX = 1, /* device-native counter RNG keyed by (seed, clip_id, field, pixel): results   */
                        /* do not depend on batch size or on how the batch is sharded over GPUs        */
    V2V_RNG_REPLAY = 2, /* caller supplies the fields (e.g. drawn from np.random in the reference's    */
                        /* order): bit-exact replay of a reference run                                 */
    V2V_RNG_PHILOX_FAST = 3 /* accepted as an alias of V2V_RNG_PHILOX.  The round-1 variant on the hardware         */
                        /* transcendental units (not reproducible on a CPU) is gone: the exact generator is as  */
                        /* fast.  Gaussians are drawn by TABLE INVERSION: each 16-bit half n of a Philox4x32    */
                        /* word is one deviate, sign = n >> 15, magnitude = table[(n >> 2) & 0x1FFF] = float32  */
                        /* Phi^-1(1/2 + (i + 1/2) / 2^14) (8192 entries, 2^14 distinct values, |g| <= 4.009:    */
                        /* tails end at 4 sigma; variance 0.99992).  Philox4x32-7 for per-time-step fields, -10 */
                        /* for per-clip fields.  ABI 2 changed every native stream (see V2V_ABI_VERSION).       */
} v2v_rng_mode;

typedef enum v2v_bin_mode {
    V2V_BIN_SUM = 0,      /* v2v_datasets.py:399-400: out[B,L,Tb,H,W], each bin = sum of frames_per_bin pairs.  */
                          /* num_bins = N-1, frames_per_bin = 1 gives EventEmulator.video_to_voxel's [N-1,H,W]. */
    V2V_BIN_BILINEAR = 1  /* utils/event_utils.py:692-728 weights on pseudo-events at ts = 0..K-1: out[B,Tb,H,W] */
} v2v_bin_mode;

#define V2V_FLAG_NOISE_EXTERNAL 0x1u /* put_noise_external (v2v_core_esim.py:46,62-65) */
#define V2V_FLAG_NO_NOISE 0x2u       /* caller guarantees base_noise_std == 0 and hot_pixel_fraction == 0 for every  */
                                     /* clip: selects the kernel without the noise adds (same results, fewer ops)  */
#define V2V_FLAG_SYMMETRIC 0x4u      /* caller guarantees pos_thres == neg_thres for every clip (EventEmulator's own */
                                     /* defaults): instances without the asymmetric loop at 4 waves per SIMD; same   */
                                     /* results; a clip that breaks the guarantee comes out as NaN.  A hint: ignored */
                                     /* where no such instance exists (float64 output, replay, external noise ...)   */
#define V2V_FLAG_MAP_4PX 0x8u        /* work-item mapping: by default 4 pixels per work-item when the layout allows  */
#define V2V_FLAG_MAP_1PX 0x10u       /* it AND the batch gives more than one such wave per SIMD, else 2 pixels, and 1 */
#define V2V_FLAG_MAP_2PX 0x20u       /* pixel below half a wave per SIMD; these three pin the choice (4PX / 2PX still */
                                     /* need the aligned layout).  Results do not depend on the mapping; tests use   */
                                     /* them to cover all three families of instances                                */

/* Replay fields, all float64 device arrays, one set per clip (clip-major). */
typedef struct v2v_esim_replay {
    const double *u_init; /* [B,H*W]     rand  #1: potential init        (v2v_core_esim.py:29) */
    const double *u_hot;  /* [B,H*W]     rand  #2: hot-pixel mask        (:37)                 */
    const double *g_hot;  /* [B,H*W]     randn #1: hot-pixel noise       (:38)                 */
    const double *g_base; /* [B,N-1,H*W] randn per frame pair            (:44)                 */
} v2v_esim_replay;

/* ---- library info / errors ---------------------------------------------------------------------- */
int v2v_version(void);                 /* V2V_ABI_VERSION the library was built with */
const char *v2v_last_error(void);      /* message of the last failure on this thread ("" if none) */
int v2v_device_count(void);            /* number of visible HIP devices, 0 if none (never fails) */

/* ---- log-intensity tables (replaces reverse_gamma_correction + np.log, v2v_core_esim.py:3-4,33-34) --
 * lut64[v] / lut32[v] = the reference's log image value for integer intensity v computed in float64 /
 * float32.  The library ships NumPy's values (golden G1); set lets a deployment re-pin them.
 * `which`: 0 = ESIM float64, 1 = ESIM float32, 2 = v2e lin_log float32.  Host pointers, 256 entries. */
int v2v_lut_get(int which, void *dst_host);
int v2v_lut_set(int which, const void *src_host);     /* the CURRENT device's table; call once per device a process drives */

/* ---- fused ESIM simulator + voxel binning ---------------------------------------------------------
 * Replaces EventEmulator.video_to_voxel (data/v2v_core_esim.py:26-69) fused with the binning of
 * WebvidDatasetV2.imgs_to_voxels (data/v2v_datasets.py:399-400) or the temporal-bilinear binning of
 * utils/event_utils.py:events_to_voxel (:692-728), for a whole batch of clips in one launch.
 *
 * frames        [B,N,H,W] grayscale (HWC with C=1), dtype V2V_U8 or V2V_F32; rows contiguous;
 *               clip_stride / frame_stride in ELEMENTS (>= N*H*W / >= H*W).
 * params        device float64: {pos_thres, neg_thres, base_noise_std, hot_pixel_fraction, hot_pixel_std}
 *               per clip; params_stride = 5 for [B,5], 0 to broadcast one set.  The table lives on the device, so it is checked
 *               there: a clip whose thresholds are outside [1e-9, 1e30] (the exact floor-divide needs |potential| / C < 2^40;
 *               zero, negative, NaN have no meaning in the reference either) or whose noise parameters are negative or not finite
 *               comes out as NaN planes (+ the flag word of `stats`); the other clips of the call are unaffected.
 * seed,clip_id0 Philox key and the GLOBAL id of clip 0 of this call (clip b uses clip_id0 + b).
 * replay        required iff rng_mode == V2V_RNG_REPLAY.
 * out_voxel     SUM: [B,L,Tb,H,W], L = (N-1)/(Tb*fpb); BILINEAR: [B,Tb,H,W]; dtype V2V_F32 or V2V_F64.
 * out_counts    optional int64 [B,2]: total ON / OFF events per clip (ADDED to the buffer: zero it first).
 */
int v2v_esim_voxel_hip(const void *frames, int in_dtype, int64_t B, int64_t N, int64_t H, int64_t W,
                       int64_t clip_stride, int64_t frame_stride, const double *params, int64_t params_stride,
                       uint32_t flags, int rng_mode, uint64_t seed, uint64_t clip_id0,
                       const v2v_esim_replay *replay, int bin_mode, int num_bins, int frames_per_bin,
                       void *out_voxel, int out_dtype, int64_t *out_counts, void *stream);

/* Same, with an optional per-clip RNG key: clip_keys = device uint64 [B,2] = {seed, clip id} of every clip (NULL ->
 * seed / clip_id0 + b).  Lets a collate step simulate independently-seeded samples in ONE launch with exactly the
 * result each sample gets when simulated alone (v2v_amd.datasets.SimulatingCollator). */
int v2v_esim_voxel_keyed_hip(const void *frames, int in_dtype, int64_t B, int64_t N, int64_t H, int64_t W,
                             int64_t clip_stride, int64_t frame_stride, const double *params, int64_t params_stride,
                             uint32_t flags, int rng_mode, uint64_t seed, uint64_t clip_id0, const uint64_t *clip_keys,
                             const v2v_esim_replay *replay, int bin_mode, int num_bins, int frames_per_bin,
                             void *out_voxel, int out_dtype, int64_t *out_counts, void *stream);

/* Same, writing the voxel planes into a PADDED layout: rows of out_row_pitch >= W elements, planes of out_plane_size >=
 * out_row_pitch*(H-1)+W elements -- e.g. the H,W -> multiples-of-16 padding of forward_sequence (model/train_utils.py:322-326)
 * written by the simulator itself instead of a later copy.  Only the H x W interior of every plane is written: the caller
 * zeroes the padding once (it is never touched again). */
int v2v_esim_voxel_padded_hip(const void *frames, int in_dtype, int64_t B, int64_t N, int64_t H, int64_t W,
                              int64_t clip_stride, int64_t frame_stride, const double *params, int64_t params_stride,
                              uint32_t flags, int rng_mode, uint64_t seed, uint64_t clip_id0, const uint64_t *clip_keys,
                              const v2v_esim_replay *replay, int bin_mode, int num_bins, int frames_per_bin,
                              void *out_voxel, int out_dtype, int64_t out_row_pitch, int64_t out_plane_size, int64_t *out_counts, void *stream);

/* Algorithmic HBM bytes of one v2v_esim_voxel_hip call (input read once + output written once);
 * the figure bench.py's roofline is computed from.  Returns a negative v2v_status on bad arguments. */
int64_t v2v_esim_voxel_bytes(int in_dtype, int64_t B, int64_t N, int64_t H, int64_t W, int bin_mode,
                             int num_bins, int frames_per_bin, int out_dtype);

/* ---- synthetic clips (bench / tests input) --------------------------------------
 * Fills frames[B,N,H,W] (V2V_U8 or V2V_F32, integer-valued 0..255) with a per-clip low-frequency pattern
 * translating at a per-clip velocity in [-3,3] px/frame plus N(0,4) pixel noise; clip b is a pure function
 * of (seed, clip_id0 + b), independent of B. */
int v2v_synth_clips_hip(void *frames, int dtype, int64_t B, int64_t N, int64_t H, int64_t W, uint64_t seed,
                        uint64_t clip_id0, void *stream);

/* Segmented form: the voxel grids of consecutive image intervals in ONE launch -- what TestH5Dataset.__getitem__
 * (data/testh5.py:111-119) does with one make_voxel call per image.  seg_offsets = device int64 [n_segments+1]
 * ascending event offsets (the h5 `event_idx` attributes); grid f is built from events [seg[f], seg[f+1]) with that
 * interval's own first/last timestamp; out_voxel float64 [n_segments,num_bins,H,W]. */
int v2v_events_to_voxel_segmented_hip(const double *ts, const int64_t *xs, const int64_t *ys, const double *ps, int64_t n,
                                      const int64_t *seg_offsets, int64_t n_segments, int mode, int num_bins, int64_t H, int64_t W,
                                      double *out_voxel, uint64_t *dropped, void *stream);

/* ---- v2e-derived DVS model fused with voxel binning (BASELINE config 3) -----------------------------------
 * Replaces video_to_voxel (data/v2v_core_v2e.py:556-581) around EventEmulator.generate_events (:401-553): lin-log
 * table, intensity-dependent IIR low-pass, leak current, per-pixel random ON/OFF thresholds, Poisson shot noise,
 * refractory cap (intended semantics min(count, int(dt/refractory)); the reference's own line raises TypeError).
 * `params` is a HOST struct (the arguments of the reference's video_to_voxel, same for every clip of the call).
 * uint8_wrap = 1 reproduces the reference's uint8 wrap in (frame+20)/275 for uint8 input (v2v_core_v2e.py:184-190).
 * rng_mode: V2V_RNG_PHILOX (device-native fields; needs `workspace` of v2v_v2e_workspace_bytes() when
 * shot_noise_rate_hz > 0) or V2V_RNG_REPLAY (fields drawn by NumPy in the reference's order: bit-exact replay).
 * The native shot-noise sampler inverts the Poisson law up to 64 events per pixel, frame and polarity: shot_noise_rate_hz <= 32 fps
 * (16 expected events; the reference's default is 0.1), V2V_ERR_PARAM beyond -- REPLAY takes np.random.poisson's counts at any rate.
 * Output / binning / counts exactly as v2v_esim_voxel_hip. */
typedef enum v2v_v2e_threshold_model {
    V2V_V2E_PN_RELATED = 0,                  /* "pn_related"                    */
    V2V_V2E_SPATIAL_INDEPENDENT = 1,          /* "spatial_independent"           */
    V2V_V2E_SPATIAL_TEMPORAL_INDEPENDENT = 2  /* "spatial_temporal_independent"  */
} v2v_v2e_threshold_model;
typedef struct v2v_v2e_params {
    double fps;
    int threshold_model;
    double thres_mean_mean, thres_mean_std, thres_diff_mean, thres_diff_std;
    double cutoff_hz, leak_rate_hz, refractory_period_s, shot_noise_rate_hz, leak_jitter_fraction, noise_rate_cov_decades;
    int uint8_wrap;
} v2v_v2e_params;
typedef struct v2v_v2e_replay {   /* device pointers */
    const double *pos_thres, *neg_thres; /* clipped thresholds: [B,H*W] (stride 0) or [B,N-1,H*W] (temporal model)      */
    int64_t thres_frame_stride;          /* 0, or H*W for spatial_temporal_independent                                  */
    const float *noise_rate;             /* [B,H*W]  exp(ln10*cov*randn) as NumPy computed it (float32)                 */
    const double *leak_randn;            /* [B,N-1,H*W] or NULL when leak_rate_hz == 0                                  */
    const int64_t *shot_pos, *shot_neg;  /* [B,N-1,H*W] Poisson counts or NULL when shot_noise_rate_hz == 0             */
} v2v_v2e_replay;
int64_t v2v_v2e_workspace_bytes(int64_t B, int64_t N);
int v2v_v2e_voxel_hip(const void *frames, int in_dtype, int64_t B, int64_t N, int64_t H, int64_t W, int64_t clip_stride,
                      int64_t frame_stride, const v2v_v2e_params *params, int rng_mode, uint64_t seed, uint64_t clip_id0,
                      const v2v_v2e_replay *replay, int bin_mode, int num_bins, int frames_per_bin, void *out_voxel,
                      int out_dtype, int64_t *out_counts, void *workspace, void *stream);

/* ---- event list -> voxel grid -------------------------------------------------------------------------
 * Replaces TestH5Dataset.make_voxel (data/testh5.py:60-90; same function at scripts/visualize_esim_sample.py:
 * 113-135) and events_to_voxel (utils/event_utils.py:692-728, temporal_bilinear=True).
 * ts float64 seconds (ascending), xs/ys int64 pixel coordinates, ps float64 (make_voxel modes: 0/1 polarity
 * flags, mapped to -1/+1 like the reference; BILINEAR mode: signed weights used as they are).
 * out_voxel float64 [num_bins,H,W] is zeroed by the call (an empty list gives zeros, testh5.py:63-64).
 * dropped   uint64 device word: number of events outside the sensor / bin range (NumPy would raise IndexError).
 * Interpolated sums use float64 atomics: per-event terms are NumPy's bits, summation order is not. */
typedef enum v2v_event_mode {
    V2V_EV_MAKE_VOXEL_DISCRETE = 0, /* testh5.py:71-74  */
    V2V_EV_MAKE_VOXEL_INTERP = 1,   /* testh5.py:75-81  */
    V2V_EV_BILINEAR = 2             /* event_utils.py:713-727 */
} v2v_event_mode;
int v2v_events_to_voxel_hip(const double *ts, const int64_t *xs, const int64_t *ys, const double *ps, int64_t n, int mode,
                            int num_bins, int64_t H, int64_t W, double *out_voxel, uint64_t *dropped, void *stream);

/* ---- decode-side front-end ("next" row) ----------------------------------------------------
 * Replaces the per-frame host loop of WebvidDatasetV2.read_video (data/v2v_datasets.py:191-224: [cvtColor BGR2GRAY]
 * -> crop -> cv2.resize INTER_LINEAR -> [flip] -> shake crop) and the pause-index gather + gray extraction of
 * __getitem__ (:311-316) for frames that are already decoded and on the device.
 * src [T,Hs,Ws,Cs] uint8 (Cs = 3 BGR or 1); frame_idx [N] int32 = decoded frame shown by each simulator frame;
 * shake_di/dj [T] int32 (>= 0) or NULL; out_gray [N,crop,crop] uint8 (simulator input); out_imgs [N,crop,crop,C]
 * uint8 or NULL.  gray_first: color_mode 'gray' (cvtColor BGR2GRAY before the resize) = 1 with the 15-bit weights of
 * OpenCV >= 4.0 (3735/19235/9798, +2^14, >> 15: what an unpinned opencv-python installs), 2 with the 14-bit weights of
 * OpenCV 2.x/3.x (1868/9617/4899, +2^13, >> 14); 0 with Cs == 3: 'gray_in_bgr_out' (resize BGR, gray = bgr_to_gray,
 * v2v_datasets.py:19-22).
 * PARITY UNPINNED against OpenCV (absent here): bit-exact against the restatement of the OpenCV 4.x 8-bit algorithms in
 * oracle/frontend_oracle.py. */
int v2v_frontend_hip(const uint8_t *src, int64_t T, int64_t Hs, int64_t Ws, int64_t Cs, int64_t min_i, int64_t min_j,
                     int64_t crop_before, int64_t need_h, int64_t need_w, int64_t crop, int flip, int gray_first,
                     const int32_t *frame_idx, int64_t N, const int32_t *shake_di, const int32_t *shake_dj, uint8_t *out_imgs,
                     uint8_t *out_gray, void *stream);

/* Batch form: src [B,T,Hs,Ws,Cs], frame_idx [B,N], clip_table device int32 [B,4] = {min_i, min_j, crop_before, flip}
 * per clip (no shake: the resize target is crop x crop); outputs [B,N,crop,crop(,C)].  One launch for the batch.
 * max_crop_before: upper bound of the table's crop_before column if the host knows it (sizes the LDS tile of the
 * gray-only path; clips above it still produce the same bytes through a slower path), 0 = bounded by the frame only.
 * The tables live on the device and are not validated by this call: whatever they hold is CLAMPED into bounds on the device (frame
 * numbers into [0, T), crop_before into [1, min(Hs, Ws)], the corner so that the rectangle lies inside the frame) -- a clamped crop,
 * never an out-of-bounds read; the Python wrappers validate host tables and raise.
 * `src` may also be DEVICE-ACCESSIBLE PAGE-LOCKED HOST memory (hipHostMalloc / torch pin_memory: mapped, same address on the device):
 * the kernel's staging loads then read each clip's crop rectangle straight over PCIe -- no copy of the whole frames (BASELINE config 4's
 * stream: 69 MB instead of 885 MB per 8 x 40 frames of 720p).  Every other pointer is device memory. */
int v2v_frontend_batch_hip(const uint8_t *src, int64_t B, int64_t T, int64_t Hs, int64_t Ws, int64_t Cs, const int32_t *clip_table,
                           int64_t max_crop_before, int64_t crop, int gray_first, const int32_t *frame_idx, int64_t N,
                           uint8_t *out_imgs, uint8_t *out_gray, void *stream);

/* ---- voxel post-ops of the consumer ("next" row) ------------------------------------------------
 * Replaces normalize_batch_voxel (model/train_utils.py:147-166: per-sample torch.kthvalue at int(0.01*M) / int(0.99*M),
 * clamp(min=1), where(v > 0, v/pos_max, v/neg_max)) fused with the zero padding of H,W to multiples of `pad_to`
 * (model/train_utils.py:322-326).  voxel float32 [B,planes,H,W] (planes = T*C); out float32 [B,planes,Hp,Wp].
 * The k-th values are exact (3-pass radix select); workspace of v2v_postops_workspace_bytes(B) needed iff normalize.
 * B <= 65535 samples per call for every post-op entry point (one grid row per sample; V2V_ERR_SHAPE beyond). */
int64_t v2v_postops_workspace_bytes(int64_t B);
int v2v_normalize_pad_hip(const float *voxel, int64_t B, int64_t planes, int64_t H, int64_t W, int normalize, int pad_to,
                          float *out, void *workspace, void *stream);

/* Same with (a) an input that is already padded -- planes of H_in x W_in >= H x W, pads zero, as v2v_esim_voxel_padded_hip
 * writes them; out may then alias voxel (in-place normalise) -- and (b) a choice of the k-th value method:
 *   V2V_NORM_NONE   pad only
 *   V2V_NORM_RADIX  exact 3-pass radix select, any float32 content (unpadded input only): 3 + 1 reads, 1 write
 *   V2V_NORM_COUNT  exact counting select for INTEGER-valued voxels with |v| <= 255 (the SUM-mode grids V2V trains on, without
 *                   external noise): 1 + 1 reads, 1 write; a sample holding any other value comes out as NaN (loud, no fallback) */
typedef enum v2v_norm_method { V2V_NORM_NONE = 0, V2V_NORM_RADIX = 1, V2V_NORM_COUNT = 2 } v2v_norm_method;
int v2v_normalize_pad_ex_hip(const float *voxel, int64_t B, int64_t planes, int64_t H, int64_t W, int64_t H_in, int64_t W_in, int method,
                             int pad_to, float *out, void *workspace, void *stream);

/* float32 twin: replaces events_to_voxel_torch (utils/event_utils.py:466-507; only caller data/dataset.py:328).
 * ts/ps float32, out float32 [num_bins,H,W]; discrete != 0 selects the `temporal_bilinear=False` branch (:502-505). */
int v2v_events_to_voxel_f32_hip(const float *ts, const int64_t *xs, const int64_t *ys, const float *ps, int64_t n, int discrete,
                                int num_bins, int64_t H, int64_t W, float *out_voxel, uint64_t *dropped, void *stream);

/* Segmented form of the float32 twin: every "between frames" voxel grid of a Monash-format sequence in ONE launch.
 * Replaces the per-index loop of scripts/esim_to_voxel.py:29-36 over DynamicH5Dataset.__getitem__ (data/dataset.py:176-199,
 * 419-427): events [seg[f], seg[f+1]) form grid f; ts float64 as stored in the file -- (ts - ts[seg[f]]).astype(float32) is
 * applied per interval on the device (:194); ps float32 already in {-1,+1} (:385); intervals with fewer than `min_events`
 * events stay zero (:189-190 uses 3).  out_voxel float32 [n_segments, num_bins, H, W]. */
int v2v_events_to_voxel_f32_segmented_hip(const double *ts, const int64_t *xs, const int64_t *ys, const float *ps, int64_t n,
                                          const int64_t *seg_offsets, int64_t n_segments, int min_events, int discrete, int num_bins,
                                          int64_t H, int64_t W, float *out_voxel, uint64_t *dropped, void *stream);

/* ---- consumer side, SURVEY §8f rank 4: the recurrent encoders' ConvLSTM step as one matrix-core kernel --------------------
 * Replaces ConvLSTM.forward (model/submodules.py:179-235): Gates = Conv2d(2C -> 4C, 3x3, pad 1) over cat(x, h_prev), chunk
 * into in/remember/out/cell gates (:218), sigmoid x3 + tanh (:221-226), cell = remember*c_prev + in*cell_gate (:229),
 * hidden = out*tanh(cell) (:230).  bf16 operands, fp32 accumulation and fp32 cell state (a precision choice of THIS kernel:
 * the tests state the tolerance against the fp32 module).  Activations are NHWC: x, h_prev, h_state [B,H,W,C] bf16;
 * c_prev, c_state [B,H,W,C] fp32; h_nchw (optional) the same hidden state as [B,C,H,W] in h_nchw_dtype (V2V_F32 or V2V_BF16: the
 * dtype the module's input had, :202-203) for the stock layers downstream.
 * h_prev == NULL and c_prev == NULL mean the zero state (prev_state=None, :196-209).  c_state may alias c_prev; h_state must
 * not alias h_prev.  tile_rows: pixels per workgroup tile, 64, 128 or 256; 0 = pick by image size.
 * Requirements (else V2V_ERR_SHAPE): C % 64 == 0, (H*W) % 4 == 0.  Any B*H*W: the last pixel tile of a launch may be partial (its rows
 * past the end read zeros and are not stored), so real-data frame sizes (180x240, 260x346 padded to multiples of 16) run at batch 1. */
int v2v_convlstm_packed_bytes(int64_t C, uint64_t *bytes);   /* size of the packed weight buffer: 4C*2C*9 bf16 */
/* gates_weight: the module's Gates.weight, fp32 [4C, 2C, 3, 3] on the device -> packed bf16 (once per weight update) */
int v2v_convlstm_pack_weights_hip(const float *gates_weight, int64_t C, void *packed, void *stream);
int v2v_convlstm_step_hip(const void *x, const void *h_prev, const float *c_prev, const void *packed, const float *gates_bias,
                          int64_t B, int64_t H, int64_t W, int64_t C, void *h_state, float *c_state, void *h_nchw, int h_nchw_dtype, int tile_rows,
                          void *stream);
/* The other recurrent cell, ConvGRU.forward (model/submodules.py:260-278), as TWO launches on the same main loop (the candidate reads
 * h * reset through a 3x3 window, so it cannot share a tile's accumulators with the gates):
 *   gates:      u = sigmoid(update_gate(cat(x, h))), r = sigmoid(reset_gate(cat(x, h)))  ->  u_ws fp32 [B,H,W,C], hr_ws = rne_bf16(h_f32 * r) bf16
 *   candidate:  o = tanh(out_gate(cat(x, hr)));  h'_f32 = h_f32 * (1 - u) + o * u  ->  h_state_f32 fp32 and its bf16 copy h_state
 * bf16 operands, fp32 accumulation, and the hidden state carried in fp32 (h_prev_f32 / h_state_f32) beside the bf16 copy the convolutions
 * read (h_prev / h_state): a precision choice of THIS kernel, as the LSTM's fp32 cell state is.  All NHWC [B,H,W,C]; h_nchw (optional) as
 * in v2v_convlstm_step_hip.  h_prev == NULL and h_prev_f32 == NULL (together) mean the zero state.  The caller owns the u_ws (B*H*W*C
 * floats) and hr_ws (B*H*W*C bf16) workspaces; the library allocates nothing.  h_state_f32 may alias h_prev_f32; h_state / hr_ws must
 * not alias x, h_prev or each other.  gates_bias = update_gate.bias | reset_gate.bias [2C], out_bias = out_gate.bias [C].
 * tile_gates / tile_cand: kernel instance codes 1..5 (pixels x columns per workgroup; gates 64x128, 128x128, 128x256, 256x256, 64x256 K-split;
 * candidate 128x64, 128x128 K-split, 128x256, 256x256, 64x128 K-split), 0 = pick by shape; a code whose columns do not divide C (gates: 2C
 * per 64 / 128 channels) is V2V_ERR_PARAM.  Shape rules are the ConvLSTM step's (else V2V_ERR_SHAPE): C % 64 == 0, (H*W) % 4 == 0, any B*H*W. */
int v2v_convgru_packed_bytes(int64_t C, uint64_t *gates_bytes, uint64_t *cand_bytes);   /* 2C*2C*9 and C*2C*9 bf16 */
/* the module's update_gate.weight, reset_gate.weight, out_gate.weight, fp32 [C, 2C, 3, 3] each on the device -> the two packed bf16 streams */
int v2v_convgru_pack_weights_hip(const float *update_weight, const float *reset_weight, const float *out_weight, int64_t C, void *packed_gates,
                                 void *packed_cand, void *stream);
int v2v_convgru_step_hip(const void *x, const void *h_prev, const float *h_prev_f32, const void *packed_gates, const void *packed_cand,
                         const float *gates_bias, const float *out_bias, int64_t B, int64_t H, int64_t W, int64_t C, float *u_ws, void *hr_ws,
                         void *h_state, float *h_state_f32, void *h_nchw, int h_nchw_dtype, int tile_gates, int tile_cand, void *stream);
/* The 16-channel layer family (FireNet, model/model.py:264-311; kernels in v2v_amd/csrc/v2v_narrow.hpp).  All activations NHWC bf16
 * [B,H,W,16], bf16 operands, fp32 accumulation on the matrix cores, ANY B, H, W >= 1 (tensors below 2^31 elements, else V2V_ERR_SHAPE).
 * Each layer is ONE launch that runs two dependent 3x3 convolutions through LDS on 16 x 16 pixel tiles; the intermediate never reaches
 * memory.  Asynchronous on `stream`, nothing is allocated.  x / h_prev / packed / out need 16-byte alignment (V2V_ERR_ALIGN).
 *
 * ConvGRU(16, 16, 3) step (model/submodules.py:260-278): the precision contract of v2v_convgru_step_hip -- u in fp32,
 * hr = rne_bf16(h_f32 * r), h'_f32 = h_f32 (1 - u) + tanh(.) u stored as fp32 (h_state_f32) and as its bf16 RNE copy (h_state), plus the
 * optional [B,16,H,W] copy h_nchw in h_nchw_dtype -- without the u / hr workspaces.  h_prev == NULL and h_prev_f32 == NULL (together): the zero
 * state.  gates_bias = update_gate.bias | reset_gate.bias [32], out_bias = out_gate.bias [16].  h_state must not alias h_prev or x, and
 * h_state_f32 must not alias h_prev_f32 (neighbouring tiles read both). */
int64_t v2v_convgru16_packed_elems(void);                                         /* bf16 elements of the packed stream (3 * 16 * 32 * 9) */
/* update_gate.weight, reset_gate.weight, out_gate.weight: fp32 [16, 32, 3, 3] each on the device */
int v2v_convgru16_pack_weights_hip(const float *update_weight, const float *reset_weight, const float *out_weight, void *packed, void *stream);
int v2v_convgru16_step_hip(const void *x, const void *h_prev, const float *h_prev_f32, const void *packed, const float *gates_bias,
                           const float *out_bias, int64_t B, int64_t H, int64_t W, void *h_state, float *h_state_f32, void *h_nchw,
                           int h_nchw_dtype, void *stream);
/* ResidualBlock(16, 16) (model/submodules.py:143-177, norm=None): out = relu(conv2(relu(conv1(x) + b1)) + b2 + x), one rounding to bf16.
 * w1 / w2: conv1.weight / conv2.weight fp32 [16, 16, 3, 3].  out must not alias x. */
int64_t v2v_resblock16_packed_elems(void);
int v2v_resblock16_pack_weights_hip(const float *w1, const float *w2, void *packed, void *stream);
int v2v_resblock16_nhwc_hip(const void *x, const void *packed, const float *b1, const float *b2, int64_t B, int64_t H, int64_t W, void *out,
                            void *stream);
/* The head ConvLayer(Cin <= 8, 16, 3, padding 1): x8 [B,H,W,8] bf16 (v2v_to_nhwc8_bf16[_scaled]_hip) -> [relu](conv3x3 + bias) [B,H,W,16] bf16.
 * weight: fp32 [16, Cin, 3, 3]. */
int64_t v2v_conv_head16_packed_elems(void);
int v2v_conv_head16_pack_weights_hip(const float *weight, int64_t Cin, void *packed, void *stream);
int v2v_conv_head16_nhwc_hip(const void *x8, const void *packed, const float *bias, int relu, int64_t B, int64_t H, int64_t W, void *out,
                             void *stream);
/* The residual blocks of the same encoder (ResidualBlock.forward, model/submodules.py:143-177, norm=None as E2VID instantiates
 * it at model/unet.py:48): a 3x3, stride-1, pad-1 convolution on the matrix cores with the same tiles and pipeline as the
 * ConvLSTM step -- out = [relu]( conv(x) + bias [+ residual] ), x [B,H,W,Cin] / residual, out [B,H,W,Cout] bf16 NHWC,
 * weight = the module's conv weight fp32 [Cout,Cin,3,3] packed once by v2v_conv3x3_pack_weights_hip (Cout*Cin*9 bf16).
 * Two calls make a block: conv1 with relu, conv2 with residual = the block's input and relu.
 * Requirements (else V2V_ERR_SHAPE): Cin % 64 == 0, Cout % 256 == 0 (or 128 / 64 / 32), (H*W) % 4 == 0 (any B*H*W: a partial last
 * tile); tile_rows: 32, 64, 128 or 256 pixels per workgroup, the first two for Cout % 256 == 0 only; 0 = the largest tile that
 * still fills the CUs;
 * out must not alias x (neighbouring tiles read x); it may alias residual. */
int v2v_conv3x3_pack_weights_hip(const float *weight, int64_t Cin, int64_t Cout, void *packed, void *stream);   /* = conv_pack, ks 3 */
int v2v_conv3x3_nhwc_hip(const void *x, const void *packed, const float *bias, const void *residual, int relu, int64_t B, int64_t H,
                         int64_t W, int64_t Cin, int64_t Cout, void *out, int tile_rows, void *stream);

/* The general form: the encoder / decoder convolutions around those blocks (ConvLayer, model/submodules.py:10-50 as built at
 * model/unet.py:34-60, 83-87: 5x5, stride 2 in the encoders, stride 1 after the bilinear upsampling in the decoders, ReLU).
 * ks = 3 or 5 (pad ks/2), stride 1 or 2; x [B,Hin,Win,Cin] -> out [B,Hout,Wout,Cout] with Hout = (Hin-1)/stride + 1; Cin % 64 == 0;
 * Cout a multiple of 256, or 128 / 64 / 32; (Hout*Wout) % 4 == 0, any B*Hout*Wout; weight fp32 [Cout,Cin,ks,ks].
 * Cin = 32 with Cout 64 / 128 (the UNet's first encoder, model/unet.py:34-44 with base 32) packs two taps per 64-wide K chunk.
 * tile_rows 16 = halo tiles (a 16x16 pixel patch staged once per channel chunk with its halo; stride 1, H and W multiples of
 * 16, Cout 32 / 64, or 128 for 3x3): what 0 picks for the 5x5 decoders with 32 / 64 output channels. */
int64_t v2v_conv_packed_elems(int64_t Cin, int64_t Cout, int ks);      /* bf16 elements of the packed stream; -1: shape not taken */
int v2v_conv_pack_weights_hip(const float *weight, int64_t Cin, int64_t Cout, int ks, void *packed, void *stream);
int v2v_conv_nhwc_hip(const void *x, const void *packed, const float *bias, const void *residual, int relu, int64_t B, int64_t Hin,
                      int64_t Win, int64_t Cin, int64_t Cout, int ks, int stride, void *out, int tile_rows, void *stream);

/* The bilinear x2 upsampling in front of a decoder convolution (UpsampleConvLayer.forward, model/submodules.py:86-87:
 * f.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)) with the sum skip connection that feeds it
 * (skip_sum, model/model_util.py:14, applied at model/unet.py:304) folded in: out = up2(x [+ skip]); x / skip [B,H,W,C], out
 * [B,2H,2W,C], all bf16 NHWC; skip may be NULL; the sum is rounded to bf16 before the interpolation, as the stock bf16 add is.
 * C % 8 == 0, 16-byte aligned buffers, out must not alias an input. */
int v2v_upsample2x_nhwc_hip(const void *x, const void *skip, int64_t B, int64_t H, int64_t W, int64_t C, void *out, void *stream);

/* The head of the recurrent UNet: ConvLayer(num_bins, base_num_channels = 32, kernel_size 5, stride 1, padding 2, relu)
 * (model/unet.py:77-78 / :265-266, ConvLayer.forward model/submodules.py:25-33) -- few input channels (<= 8: the voxel bins),
 * 32 output channels.  x8 = the input as bf16 NHWC with the channels padded to 8 (v2v_to_nhwc8_bf16_hip makes it from a float32
 * [B,C,H,W] tensor of any element strides); weight fp32 [32,Cin,ks,ks] packed once (v2v_conv_head_packed_elems(ks) bf16
 * elements); out bf16 [B,H,W,32] = [relu](conv + bias).  ks 3 or 5 (pad ks/2), H and W multiples of 16. */
int64_t v2v_conv_head_packed_elems(int ks);
int v2v_conv_head_pack_weights_hip(const float *weight, int64_t Cin, int ks, void *packed, void *stream);
int v2v_to_nhwc8_bf16_hip(const float *src, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, int64_t B, int64_t C,
                          int64_t H, int64_t W, void *dst, void *stream);
/* the same conversion with normalize_batch_voxel's scaling folded into the read (model/train_utils.py:162-166): scales float32 [B,2] =
 * {neg_max, pos_max} (v2v_voxel_scales_hip), x -> where(x > 0, x / pos_max, x / neg_max) before the bf16 rounding; NULL = no scaling */
int v2v_to_nhwc8_bf16_scaled_hip(const float *src, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, int64_t B, int64_t C,
                                 int64_t H, int64_t W, const float *scales, void *dst, void *stream);
int v2v_conv_head_nhwc_hip(const void *x8, const void *packed, const float *bias, int relu, int64_t B, int64_t H, int64_t W, int ks, void *out, void *stream);

/* The prediction layer: ConvLayer(base_num_channels, out, kernel_size=1, activation=None) (model/unet.py:58-64) applied to
 * skip_sum(x, head) (model/unet.py:307): out[m][o] = bias[o] + sum_c w[o][c] * (x[m][c] + skip[m][c]); x / skip [M, C] bf16
 * (NHWC with M = B*H*W; skip may be NULL; the sum is rounded to bf16 first, the weights to bf16, as bf16 autocast does), weight
 * fp32 [Cout, C], out [M, Cout] fp32 or bf16 (out_dtype) -- for Cout = 1 that is the NCHW image.  C a power of two in 8..512,
 * Cout 1..3. */
int v2v_conv1x1_nhwc_hip(const void *x, const void *skip, const float *weight, const float *bias, int64_t M, int64_t C, int64_t Cout,
                         void *out, int out_dtype, void *stream);

/* fp32 or bf16 [B,C,H,W] (src_dtype V2V_F32 / V2V_BF16) -> bf16 [B,H,W,C] (relu != 0: through max(x,0), the activation in front of the recurrent block,
 * model/submodules.py:267-271 RecurrentConvLayer = ConvLayer(relu) -> ConvLSTM).  C % 64 == 0 and (H*W) % 64 == 0. */
int v2v_nchw_to_nhwc_bf16_hip(const void *src, int src_dtype, int64_t B, int64_t C, int64_t H, int64_t W, int relu, void *dst, void *stream);

/* ---- Backward passes of the recurrent UNet (training: v2v_amd.unet.E2VIDRecurrent(trainable=True)) ---------------------------------
 * All NHWC; activation gradients bf16, cell-state gradients and parameter gradients fp32; bf16 MFMA operands with fp32 accumulation.
 * Caller-owned memory (a *_workspace_bytes query where a scratch slab is needed), no allocation, no synchronisation.  No float atomics:
 * every result is bitwise reproducible from run to run.
 *
 * ConvLSTM step backward (gate order i, r, o, g as in model/submodules.py:ConvLSTM): the 3x3 gate GEMM recomputed from the SAVED x,
 * h_prev (may be NULL: zero state), c_prev (may be NULL) with the forward's packed weights and bias; dh fp32 [B,H,W,C], dc fp32 (NULL:
 * zero) -> dgates bf16 [B,H,W,4C] (gradient of the pre-activation gates) and dc_prev fp32 [B,H,W,C].  Same shape limits as the step. */
int v2v_convlstm_step_bwd_hip(const void *x, const void *h_prev, const float *c_prev, const void *packed, const float *bias, const float *dh,
                              const float *dc, int64_t B, int64_t H, int64_t W, int64_t C, void *dgates, float *dc_prev, void *stream);
/* ReLU backward from the saved post-ReLU output: out = y > 0 ? dy : 0 on [M, C] bf16 (y NULL: a copy); C % 8 == 0. */
int v2v_relu_bwd_nhwc_hip(const void *dy, const void *y, int64_t M, int64_t C, void *out, void *stream);
/* Data gradient of a ks x ks convolution (pad ks/2) with weight fp32 [Cout,Cin,ks,ks]: dx [B,Hin,Win,Cin] = the stride-1 convolution of
 * dy [B,Hin/stride,Win/stride,Cout] (stride 2: spread onto the input grid, zeros between) with the flipped, transposed weights, on the
 * forward convolution kernel -- so Cout -> Cin must be a shape v2v_conv_nhwc_hip takes.  The weights are packed once per update
 * (scratch: Cin*Cout*ks*ks floats); residual (may be NULL) [B,Hin,Win,Cin] bf16 is added before the one bf16 rounding. */
int64_t v2v_conv_dgrad_packed_elems(int64_t Cin, int64_t Cout, int ks);
int v2v_conv_dgrad_pack_weights_hip(const float *weight, int64_t Cin, int64_t Cout, int ks, float *scratch, void *packed, void *stream);
int64_t v2v_conv_dgrad_workspace_bytes(int64_t B, int64_t Hin, int64_t Win, int64_t Cin, int64_t Cout, int stride);
int v2v_conv_dgrad_nhwc_hip(const void *dy, const void *packed, const void *residual, int64_t B, int64_t Hin, int64_t Win, int64_t Cin, int64_t Cout,
                            int ks, int stride, void *workspace, void *dx, void *stream);
/* Weight and bias gradient of a ks x ks convolution (ks 1, 3 or 5, pad ks/2, stride 1 or 2): dy [B,Ho,Wo,Cout] bf16 (Cout % 32 == 0),
 * input x1 [B,Hin,Win,C1] | x2 [B,Hin,Win,C2] bf16 (x2 may be NULL: zeros; the ConvLSTM's cat(x, h_prev) without the copy) ->
 * dw fp32 [Cout, Cin_out, ks, ks] (the first Cin_out <= C1 + C2 input channels: the head's 8-channel padded input), db fp32 [Cout]
 * (may be NULL).  An MFMA GEMM with K = the output pixels, split into slabs and summed in a fixed order. */
int64_t v2v_conv_wgrad_workspace_bytes(int64_t B, int64_t Ho, int64_t Wo, int64_t Cin, int64_t Cout, int ks);
int v2v_conv_wgrad_nhwc_hip(const void *dy, const void *x1, int64_t C1, const void *x2, int64_t C2, int64_t Cin_out, int64_t B, int64_t Hin, int64_t Win,
                            int64_t Cout, int ks, int stride, void *workspace, float *dw, float *db, void *stream);
/* Adjoint of v2v_upsample2x_nhwc_hip: dout [B,2H,2W,C] bf16 -> dx [B,H,W,C] bf16 (fp32 sums; the gradient of x and of the skip). */
int v2v_upsample2x_bwd_nhwc_hip(const void *dout, int64_t B, int64_t H, int64_t W, int64_t C, void *dx, void *stream);
/* Backward of the prediction layer (v2v_conv1x1_nhwc_hip with Cout = 1): dy [M] fp32 -> dx [M,C] bf16 = dy * bf16(w) (the gradient of
 * x and of the skip), dw [C] = sum dy * bf16(x + skip), db [1] = sum dy (fp32).  C a power of two in 8..128. */
int64_t v2v_conv1x1_bwd_workspace_bytes(int64_t M, int64_t C);
int v2v_conv1x1_bwd_nhwc_hip(const float *dy, const void *x, const void *skip, const float *weight, int64_t M, int64_t C, void *dx, float *dw, float *db,
                             void *workspace, void *stream);

/* normalize_batch_voxel's per-sample k-th values gathered BY THE SIMULATOR'S WRITER (model/train_utils.py:147-166):
 * v2v_esim_voxel_stats_hip = v2v_esim_voxel_padded_hip + `stats`, uint32 [B][V2V_VOXEL_STATS_WORDS] (zeroed here, then accumulated by
 * the launch): word 256 + v counts the voxels of clip b equal to the integer v in -255..255 except v = 0 (left 0: the reader derives
 * it from the element count), words 0 / 512 the voxels below -255 / above 255 (hot pixels), word 513 != 0 flags a clip whose planes
 * are not counts.  SUM mode, float32 grid, no V2V_FLAG_NOISE_EXTERNAL (anything else: V2V_ERR_MODE).
 * v2v_voxel_scales_hip: scales[b] = {neg_max, pos_max} = {clamp(-kthvalue(1 %), min=1), clamp(kthvalue(99 %), min=1)} (:153-160; ranks
 * int(0.01*M), int(0.99*M), 1-based, M = elems_per_sample = the sample's voxel count WITHOUT padding) from those statistics, exact;
 * NaN when a rank falls into an overflow word or the clip is flagged.
 * v2v_voxel_apply_scales_hip: out = where(voxel > 0, voxel / pos_max, voxel / neg_max) (:162-166; IEEE division) [+ zero padding of H, W to
 * multiples of pad_to]; voxel [B,planes,H_in,W_in] (interior H x W valid), out [B,planes,Hp,Wp]; out == voxel allowed when the layouts
 * agree; scales NULL = copy / pad only.  A consumer that scales while it reads (v2v_to_nhwc8_bf16_scaled_hip) needs no such pass. */
#define V2V_VOXEL_STATS_WORDS 516
/* Optional extras of one simulator launch (v2v_esim_voxel_ex_hip = v2v_esim_voxel_padded_hip + this; NULL fields are off):
 *   stats         as v2v_esim_voxel_stats_hip.
 *   frame_index   int32 [B, N]: simulator frame f of clip b is STORED frame frame_index[b*N + f] -- the reference's pause-index gather
 *                 (data/v2v_datasets.py:286-311: all_imgs = stack(raw_imgs[i] for i in img_idxes)) folded into the kernel's loads, so a
 *                 clip whose video pauses is stored (and crosses PCIe) once per DECODED frame; results are those of the gathered clip.
 *   clip_offsets  int64 [B]: clip b starts at element clip_offsets[b] of `frames` (clips of different stored lengths packed back to
 *                 back); `clip_stride` then only states the alignment every offset keeps (in elements, e.g. 16).  Comes with frame_index.
 *   stored_frames int32 [B] (with frame_index; NULL = the caller vouches for the rows): clip b holds stored_frames[b] frames.  The launch
 *                 checks every row while it stages it through LDS: a clip whose row names a frame outside [0, stored_frames[b]) is NOT
 *                 read -- its planes come out NaN and, with `stats`, its flag word (513) is set, so v2v_voxel_scales_hip hands out NaN
 *                 scales for it -- the same loud failure as a broken V2V_FLAG_SYMMETRIC promise; the other clips are unaffected.  (The
 *                 reference's gather, a Python list index at data/v2v_datasets.py:311, raises IndexError there.)
 *   frames_elems  int64 (with stored_frames; 0 = not stated): elements in `frames`.  A clip with clip_offsets[b] < 0 or
 *                 clip_offsets[b] + (stored_frames[b]-1)*frame_stride + H*W > frames_elems is poisoned the same way.
 * Indexed launches: uint8 clips, SUM bins, device-native noise, float32 grid, none of the NO_NOISE / NOISE_EXTERNAL / SYMMETRIC flags
 * (V2V_ERR_MODE otherwise).  The index rows live on the device, so their check cannot return a status code without a synchronisation:
 * it is reported through the data (NaN planes / the flag word), never by reading out of bounds. */
typedef struct v2v_esim_extras {
    uint32_t *stats;
    const int32_t *frame_index;
    const int64_t *clip_offsets;
    const int32_t *stored_frames;
    int64_t frames_elems;
} v2v_esim_extras;
int v2v_esim_voxel_ex_hip(const void *frames, int in_dtype, int64_t B, int64_t N, int64_t H, int64_t W,
                          int64_t clip_stride, int64_t frame_stride, const double *params, int64_t params_stride,
                          uint32_t flags, int rng_mode, uint64_t seed, uint64_t clip_id0, const uint64_t *clip_keys,
                          const v2v_esim_replay *replay, int bin_mode, int num_bins, int frames_per_bin,
                          void *out_voxel, int out_dtype, int64_t out_row_pitch, int64_t out_plane_size, int64_t *out_counts,
                          const v2v_esim_extras *extras, void *stream);
int v2v_esim_voxel_stats_hip(const void *frames, int in_dtype, int64_t B, int64_t N, int64_t H, int64_t W,
                             int64_t clip_stride, int64_t frame_stride, const double *params, int64_t params_stride,
                             uint32_t flags, int rng_mode, uint64_t seed, uint64_t clip_id0, const uint64_t *clip_keys,
                             const v2v_esim_replay *replay, int bin_mode, int num_bins, int frames_per_bin,
                             void *out_voxel, int out_dtype, int64_t out_row_pitch, int64_t out_plane_size, int64_t *out_counts, uint32_t *stats,
                             void *stream);
int v2v_voxel_scales_hip(const uint32_t *stats, int64_t B, int64_t elems_per_sample, float *scales, void *stream);
int v2v_voxel_apply_scales_hip(const float *voxel, int64_t B, int64_t planes, int64_t H, int64_t W, int64_t H_in, int64_t W_in, int pad_to,
                               const float *scales, float *out, void *stream);
/* The same scales by selection over a FINISHED tensor (what v2v_normalize_pad_ex_hip does before it scales): method V2V_NORM_RADIX (any
 * float32 content, unpadded input) or V2V_NORM_COUNT (integer-valued, padded input allowed); workspace of v2v_postops_workspace_bytes(B). */
int v2v_voxel_scales_select_hip(const float *voxel, int64_t B, int64_t planes, int64_t H, int64_t W, int64_t H_in, int64_t W_in, int method,
                                float *scales, void *workspace, void *stream);

/* The `frame` tensor of a batch from the uint8 clips already in HBM (WebvidDatasetV2.__getitem__, data/v2v_datasets.py:329-338, 352:
 * frame[l] = float(all_imgs[idx_l]).permute(2,0,1) / 255): out[b,l,c,y,x] = float(src[b, pick[l], y, x, c]) / 255.0f (IEEE division:
 * torch's CPU values bit for bit).  src uint8 [B, *, H, W, C] with element strides clip_stride / frame_stride; pick = L device int32
 * frame indices (NULL: frames 0..L-1); out float32 [B,L,C,H,W] contiguous.  C >= 1. */
int v2v_clip_frames_f32_hip(const void *src, int64_t clip_stride, int64_t frame_stride, const int32_t *pick, int64_t B, int64_t L, int64_t H,
                            int64_t W, int64_t C, float *out, void *stream);
/* the same for packed clips (v2v_esim_extras): clip b starts at clip_offsets[b] (NULL: b * clip_stride; with offsets clip_stride states
 * their common alignment) and picks frame pick[b * pick_stride + l] (pick_stride 0: one row of picks for every clip) */
int v2v_clip_frames_f32_ex_hip(const void *src, int64_t clip_stride, const int64_t *clip_offsets, int64_t frame_stride, const int32_t *pick,
                               int64_t pick_stride, int64_t B, int64_t L, int64_t H, int64_t W, int64_t C, float *out, void *stream);
/* the same with the gather's bounds (ABI 3, round 5; what the loader calls): stored_frames int32 [B] = frames clip b holds, src_elems =
 * bytes in `src` (0: not stated).  A picked frame outside [0, stored_frames[b]), or one that does not fit `src`, is not read: its output
 * frame is NaN -- like v2v_esim_extras.stored_frames for the simulator (the picks live on the device: no status code without a
 * synchronisation).  stored_frames NULL = v2v_clip_frames_f32_ex_hip (the caller vouches for the picks).  Any B: more than 65,535
 * output frames go out as several launches of whole clips on `stream`; L <= 65535. */
int v2v_clip_frames_f32_bounded_hip(const void *src, int64_t clip_stride, const int64_t *clip_offsets, int64_t frame_stride, const int32_t *pick,
                                    int64_t pick_stride, const int32_t *stored_frames, int64_t src_elems, int64_t B, int64_t L, int64_t H, int64_t W,
                                    int64_t C, float *out, void *stream);

/* ---- the plain UNet (EVFlowNet, model/unet.py:313-352): stem, concat skips, a trainable prediction of 1..3 outputs -------------------
 * Stem = UNet.encoders[0]: x8 bf16 [B,H,W,8] (what v2v_to_nhwc8_bf16[_scaled]_hip makes) -> out bf16 [B,H/2,W/2,64] =
 * [relu](conv3x3(x, stride 2, pad 1) + bias); weight float32 [64, Cin <= 8, 3, 3] packed once; H, W multiples of 16. */
int64_t v2v_conv_stem_packed_elems(void);
int v2v_conv_stem_pack_weights_hip(const float *weight, int64_t Cin, void *packed, void *stream);
int v2v_conv_stem_nhwc_hip(const void *x8, const void *packed, const float *bias, int relu, int64_t B, int64_t H, int64_t W, void *out, void *stream);
/* Concat skip in front of a decoder: out bf16 [B,2H,2W,C1+C2] = cat(up2(x [B,H,W,C1]), up2(skip [B,H,W,C2])) along the channels, i.e. the
 * bilinear x2 upsampling (align_corners = false) of cat(x, skip) without ever writing that tensor; the arithmetic of the sum-skip upsampling
 * entry above, per channel.  C1, C2 multiples of 8; skip NULL with C2 = 0 gives that entry's result without a skip, bit for bit. */
int v2v_upsample2x_cat_nhwc_hip(const void *x, int64_t C1, const void *skip, int64_t C2, int64_t B, int64_t H, int64_t W, void *out, void *stream);
/* Its adjoint for one channel slice: dout bf16 [B,2H,2W,Ctot], channels [c0, c0 + C) -> dx bf16 [B,H,W,C] (fp32 sums, gather form, no
 * atomics).  c0 = 0 and C = Ctot gives the sum-skip adjoint's result bit for bit. */
int v2v_upsample2x_cat_bwd_nhwc_hip(const void *dout, int64_t B, int64_t H, int64_t W, int64_t Ctot, int64_t c0, int64_t C, void *dx, void *stream);
/* Backward of the prediction layer for Cout = 1..3: dy fp32 [M,Cout] -> dx bf16 [M,C] = sum_o dy[m][o] * bf16(w[o][c]) (one rounding),
 * dw fp32 [Cout,C], db fp32 [Cout] by fixed-order slab sums (bitwise reproducible).  C a power of two in 8..128; skip may be NULL. */
int64_t v2v_conv1x1_bwd_cout_workspace_bytes(int64_t M, int64_t C, int64_t Cout);
int v2v_conv1x1_bwd_cout_nhwc_hip(const float *dy, const void *x, const void *skip, const float *weight, int64_t M, int64_t C, int64_t Cout, void *dx,
                                  float *dw, float *db, void *workspace, void *stream);
/* The convolution entry with its automatic tile chosen as for a batch of B_like images (0: B): a batch that folds T time steps of B_like
 * images runs the instance a single step would, so every image comes out bit-identical to the per-step launch. */
int v2v_conv_nhwc_like_hip(const void *x, const void *packed, const float *bias, const void *residual, int relu, int64_t B, int64_t Hin, int64_t Win,
                           int64_t Cin, int64_t Cout, int ks, int stride, void *out, int64_t B_like, void *stream);

/* ---- HyperE2VID's per-pixel dynamic decoder (model/hyper_model.py:33-60, model/hyper/hyper_dynamic.py), inference ------------------------
 * Context staging (ConvolutionalContextFusion.forward up to its convolution): cat(events [B,C,H,W] float32 of any element strides, prev
 * [B,1,H,W] float32 contiguous) bilinearly downsampled by 4 (align_corners = false: the mean of the central 2 x 2 of every 4 x 4 block)
 * -> dst bf16 [B,H/4,W/4,8], channels C + 1 .. 7 zero: the input layout of v2v_conv_head_nhwc_hip.  1 <= C <= 7, H and W multiples of 4. */
int v2v_hyper_context_hip(const float *events, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, const float *prev, int64_t B,
                          int64_t C, int64_t H, int64_t W, void *dst, void *stream);
/* context_fusion.conv on that layout: x8 bf16 [B,h,w,8] -> out bf16 [B,h,w,32] = conv3x3(x, pad 1) + bias; weight float32 [32,Cin,3,3] (rounded
 * to bf16 while it is read), 1 <= Cin <= 8, any h, w >= 1 (the head entry above needs multiples of 16). */
int v2v_hyper_context_conv_hip(const void *x8, const float *weight, const float *bias, int64_t B, int64_t h, int64_t w, int64_t Cin, void *out, void *stream);
/* Element-wise tanh on n bf16 values (bases_net's first activation); n % 8 == 0, out may be x. */
int v2v_tanh_bf16_hip(const void *x, int64_t n, void *out, void *stream);
/* Atoms (DynamicAtomGeneration.forward's tanh + einsum): coeff bf16 [M,128] = the 72 pre-activation coefficients of a pixel (index
 * m * 12 + k; columns 72..127 ignored), bases float32 [12,25] -> atoms float32 [M,25,6]: atoms[p][l][m] = sum_k tanh(coeff[p][m*12+k]) * bases[k][l]. */
int v2v_hyper_atoms_hip(const void *coeff, const float *bases, int64_t M, float *atoms, void *stream);
/* The dynamic convolution (DynamicConv.forward + bias [+ ReLU]) without the unfolded tensor: x bf16 [B,H,W,256], atoms float32 [B,H,W,25,6],
 * out bf16 [B,H,W,128]: out[p][o] = [relu](bias[o] + sum_{c,m} W[o][c*6+m] * bf16(sum_l atoms[p][l][m] * x[p + offset_l][c])) over the
 * zero-padded 5 x 5 window, float32 accumulation.  weight float32 [Cout, Cin * atoms] (compositional_coefficients) is packed once into
 * v2v_hyper_dynconv_packed_elems bf16 elements.  Shapes taken: Cin 256, Cout 128, 6 atoms, ks 5; anything else: -1 / V2V_ERR_SHAPE. */
int64_t v2v_hyper_dynconv_packed_elems(int64_t Cin, int64_t Cout, int atoms, int ks);
int v2v_hyper_dynconv_pack_weights_hip(const float *weight, int64_t Cin, int64_t Cout, int atoms, void *packed, void *stream);
int v2v_hyper_dynconv_nhwc_hip(const void *x, const float *atoms, const void *packed, const float *bias, int relu, int64_t B, int64_t H, int64_t W,
                               int64_t Cin, int64_t Cout, int n_atoms, int ks, void *out, void *stream);

/* ---- the dynamic decoder's backward (training; v2v_amd/train.py DynamicUpsampleFn).  No atomics: two runs give equal bits.  Errors go to
 * v2v_last_error() like everyone's; v2v_hyper_train_last_error() is a DEPRECATED ALIAS that returns v2v_last_error() (ABI 6 first shipped
 * these entry points with a slot of their own; the symbol stays so that a client linked against that build keeps working). -----------
 * With dz = relu'(dout) bf16 [M = B*H*W][128], x = the upsampled input bf16 [B,H,W,256], atoms float32 [B,H,W,25,6]:
 *   pack_t   compositional_coefficients float32 [128,1536] -> the transposed bf16 stream of df (128 * 1536 elements)
 *   df       dF[p][c][m] = sum_o dz[p][o] W[o][c*6+m], stored bf16 as [M][c / 64][m][c % 64] (1536 per pixel), one rounding
 *   datoms   dAtoms[p][l][m] = sum_c x[p + offset_l][c] dF[p][c][m], float32 [M,25,6], zero padding as the forward
 *   dx       dX[q][c] = sum_l sum_m atoms[q - offset_l][l][m] dF[q - offset_l][c][m], bf16 [B,H,W,256], one rounding
 *   wgrad    dW[o][c*6+m] = sum_p dz[p][o] bf16(F[p][c][m]) with F recomputed as the forward computes it, db[o] = sum_p dz[p][o]; float32;
 *            workspace of v2v_hyper_dynconv_wgrad_workspace_bytes (16-byte aligned; -1: shape not taken)
 * Any B, H, W >= 1 with B*H*W*1536 below 2^33. */
const char *v2v_hyper_train_last_error(void);        /* deprecated: the same text as v2v_last_error() */
int v2v_hyper_dynconv_pack_t_hip(const float *weight, void *packed_t, void *stream);
int v2v_hyper_dynconv_df_hip(const void *dz, const void *packed_t, int64_t M, void *dF, void *stream);
int v2v_hyper_dynconv_datoms_hip(const void *x, const void *dF, int64_t B, int64_t H, int64_t W, float *datoms, void *stream);
int v2v_hyper_dynconv_dx_hip(const float *atoms, const void *dF, int64_t B, int64_t H, int64_t W, void *dx, void *stream);
int64_t v2v_hyper_dynconv_wgrad_workspace_bytes(int64_t B, int64_t H, int64_t W);
int v2v_hyper_dynconv_wgrad_hip(const void *dz, const void *x, const float *atoms, int64_t B, int64_t H, int64_t W, void *workspace, float *dw, float *db,
                                void *stream);
/* BatchNorm on batch statistics over the M rows of z bf16 [M][Cs] (Cs % 8 == 0; columns >= Cv are padding: outputs and gradients zero).
 *   stats   mean, biased variance and rstd = 1 / sqrt(var + eps) per column (float32 [Cs] each; two passes, sums carried in float64)
 *   apply   out = gamma (z - mean) rstd + beta [-> tanh], bf16 [M][Cs]
 *   bwd     dy (bf16, or float32 with dy_is_f32) -> sums float32 [4][Cs] = (dbeta, dgamma, sum over the rows of dz before its rounding, unused)
 *           and dz bf16 [M][Cs] = gamma rstd (dpre - dbeta / M - xhat dgamma / M), dpre = dy [(1 - tanh(gamma xhat + beta)^2) with tanh_out]
 * atoms_bwd: dpre[p][m*12+k] = (1 - tanh(pre[p][m*12+k])^2) sum_l datoms[p][l][m] bases[k][l], float32 [M][128], columns 72..127 zero. */
int v2v_hyper_bn_stats_hip(const void *z, int64_t M, int64_t Cs, float eps, float *mean, float *var, float *rstd, void *stream);
int v2v_hyper_bn_apply_hip(const void *z, const float *mean, const float *rstd, const float *gamma, const float *beta, int64_t M, int64_t Cs, int64_t Cv,
                           int tanh_out, void *out, void *stream);
int v2v_hyper_bn_bwd_hip(const void *dy, int dy_is_f32, const void *z, const float *mean, const float *rstd, const float *gamma, const float *beta, int64_t M,
                         int64_t Cs, int64_t Cv, int tanh_out, float *sums, void *dz, void *stream);
int v2v_hyper_atoms_bwd_hip(const float *datoms, const void *pre, const float *bases, int64_t M, float *dpre, void *stream);

/* ---- the image losses of training (utils/loss.py:6-69 temporal consistency; model/loss.py l1_loss, l2_loss), float32 ----------------------
 * One call serves a list of images (a, b), a < outer, b < inner: image1 / processed1 of image (a, b) start at element a * img_stride_outer +
 * b * img_stride_inner and are contiguous [c,h,w]; the temporal term exists for b >= tc_first, and image0 / processed0 / flow ([2,h,w],
 * strides flow_stride_*) are addressed with b - tc_first: their base pointers point at the first image that has a temporal term.  Separate
 * [N,C,H,W] tensors: outer = N, inner = 1, tc_first = 0.  Steps of a [B,T,C,H,W] tensor: outer = B, inner = T, tc_first = L0, processed0 =
 * processed1 + (L0 - 1) * img_stride_inner.  The flow is multiplied by flow_sign (the reference's classes pass -flow).
 *   warp(img)[y,x] = bilinear sample at (x + flow_x, y + flow_y) through grid_sample's normalise / un-normalise roundings, zero outside
 *   tc = mean_chw( exp(-alpha (image1 - warp(image0))^2) |processed1 - w| / (|processed1| + |w| + 1e-5) ),  w = warp(clamp(processed0, 0, 255))
 *   l1 = mean_chw |processed1 - image1|,  l2 = mean_chw (processed1 - image1)^2
 * losses float32 [3][outer*inner] = weight * mean, rows tc, l1, l2; a zero weight skips that loss (row 0), and with w_tc == 0 image0,
 * processed0 and flow may be NULL.  The four map outputs are optional (NULL), dense [outer*inner,c,h,w], zero where there is no temporal term.
 * An image's sum does not depend on what else is in the launch.  h, w >= 2, h*w <= 2^22.
 * v2v_tc_loss_workspace_bytes(outer*inner, c, h, w, backward): bytes of workspace for the forward (0) or the backward / adjoint (1) call. */
int64_t v2v_tc_loss_workspace_bytes(int64_t n_img, int64_t c, int64_t h, int64_t w, int backward);
int v2v_tc_loss_fwd_hip(const float *image0, const float *image1, const float *processed0, const float *processed1, const float *flow, int64_t outer,
                        int64_t inner, int64_t img_stride_outer, int64_t img_stride_inner, int64_t flow_stride_outer, int64_t flow_stride_inner,
                        int64_t tc_first, int64_t c, int64_t h, int64_t w, float alpha, float flow_sign, float w_tc, float w_l1, float w_l2, float *losses,
                        float *image0_warped, float *processed0_warped, float *visibility_mask, float *error_map, void *workspace, void *stream);
/* Gradient of sum(gout * losses), gout float32 [3][outer*inner], to the processed images; frames and flow get none.  dprocessed1 (addressed
 * like processed1) = the pointwise terms; the temporal term's gradient to processed0 is the bilinear adjoint of d tc / d w, accumulated in
 * 64-bit fixed point with integer atomics (bitwise reproducible; no float atomics), then clamp-masked.  chain = 0: it goes to dprocessed0
 * (addressed like processed0).  chain = 1: processed0 of image (a, b) is processed1 of image (a, b - 1), and dprocessed1 of that image
 * receives it, summed in a fixed order: scatter of the next step + own temporal term + l2 + l1; dprocessed0 is not used. */
int v2v_tc_loss_bwd_hip(const float *image0, const float *image1, const float *processed0, const float *processed1, const float *flow, int64_t outer,
                        int64_t inner, int64_t img_stride_outer, int64_t img_stride_inner, int64_t flow_stride_outer, int64_t flow_stride_inner,
                        int64_t tc_first, int64_t c, int64_t h, int64_t w, float alpha, float flow_sign, float w_tc, float w_l1, float w_l2, const float *gout,
                        int chain, float *dprocessed1, float *dprocessed0, void *workspace, void *stream);
/* The warp alone and its adjoint: img / out / dout / din float32 [n,c,h,w] contiguous, flow [n,2,h,w]; the adjoint's workspace is the
 * backward one of v2v_tc_loss_workspace_bytes. */
int v2v_warp_bilinear_hip(const float *img, const float *flow, int64_t n, int64_t c, int64_t h, int64_t w, float *out, void *stream);
int v2v_warp_bilinear_adjoint_hip(const float *dout, const float *flow, int64_t n, int64_t c, int64_t h, int64_t w, float *din, void *workspace, void *stream);

/* ---- the LPIPS-VGG perceptual loss (PerceptualSimilarity PNetLin, model/loss.py:95-119): what is not a 64..512-channel convolution --------
 * Activations and their gradients are bf16 NHWC (16-byte aligned), everything else float32.  Every reduction has a fixed order and there
 * are no float atomics; a sample's result does not depend on what else is in the launch.
 * Stem: x [B,Cin,H,W] (Cin 1 or 3; one channel stands for three equal ones; x_dtype V2V_F32 or V2V_BF16), weight [64,3,3,3], bias [64],
 * shift / scale [3] -> out [B,H,W,64] = relu(conv3x3(s) + bias), s = ((normalize ? 2x - 1 : x) - shift_c) / scale_c inside the image and 0
 * outside (the zero padding comes AFTER the scaling layer).  Any H, W >= 1.
 * Stem backward: dz [B,H,W,64] (ReLU-masked) -> dpred float32 [B,Cin,H,W] = (normalize ? 2 : 1) / scale_c * the transposed convolution
 * 64 -> 3 in float32, the three channels summed when Cin is 1. */
int v2v_lpips_stem_hip(const void *x, int x_dtype, int64_t B, int64_t Cin, int64_t H, int64_t W, const float *weight, const float *bias, const float *shift,
                       const float *scale, int normalize, void *out, void *stream);
int v2v_lpips_stem_bwd_hip(const void *dz, int64_t B, int64_t Cin, int64_t H, int64_t W, const float *weight, const float *scale, int normalize,
                           float *dpred, void *stream);
/* 2x2 max-pool x [B,H,W,C] -> out [B,H/2,W/2,C] (H, W even, C a multiple of 8) and its backward: dx [B,H,W,C] gets dy at the FIRST maximum of
 * each window in row-major order (autograd's rule), plus dtap [B,H,W,C] when that is not NULL -- added in float32, rounded to bf16 once --
 * and is zeroed where x <= 0 when relu_mask is set (x is then the post-ReLU tensor that was pooled). */
int v2v_lpips_pool_hip(const void *x, int64_t B, int64_t H, int64_t W, int64_t C, void *out, void *stream);
int v2v_lpips_pool_bwd_hip(const void *dy, const void *x, const void *dtap, int relu_mask, int64_t B, int64_t H, int64_t W, int64_t C, void *dx, void *stream);
/* Compare: f0, f1 [n_img,HW,Cc] (Cc 64, 128, 256 or 512), w float32 [Cc]; n = f / (sqrt(sum_c f^2) + 1e-10) per pixel.
 * Forward: dist[b] += mean_pixels sum_c w_c (n0_c - n1_c)^2 (dist float32 [n_img] is ACCUMULATED into: zero it before the first tap);
 * workspace: v2v_lpips_compare_workspace_bytes(n_img, HW) bytes, 16-byte aligned.
 * Backward: df0 [n_img,HW,Cc] bf16 from ddist float32 [n_img]: g_c = 2 w_c (n0_c - n1_c) ddist / HW, df0_c = g_c / (r + eps) -
 * f0_c (sum_k g_k f0_k) / (r (r + eps)^2), r = |f0|; at r == 0 the second term is defined as 0 (autograd returns NaN there). */
int64_t v2v_lpips_compare_workspace_bytes(int64_t n_img, int64_t HW);
int v2v_lpips_compare_fwd_hip(const void *f0, const void *f1, const float *w, int64_t n_img, int64_t HW, int64_t Cc, float *dist, void *workspace, void *stream);
int v2v_lpips_compare_bwd_hip(const void *f0, const void *f1, const float *w, const float *ddist, int64_t n_img, int64_t HW, int64_t Cc, void *df0, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* V2V_HIP_H */
