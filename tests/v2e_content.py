"""Arbitrary float32 content for the v2e simulator tests (tests/test_v2e_float_content.py): clips that are NOT integers in
0..255, the device-native random source for the NumPy oracle, the launcher's routing rule restated, and the table of GPU cases
that the CPU side checks for sensitivity.  A plain module: no fixtures, nothing collected from here."""
import math

import numpy as np

from oracle import v2v_oracle as O

SEED = 0xA5C3F09E17                 # 40 bits: both halves of the Philox key are in use
CLIP_ID0 = 5
FEATURES = {1: "cutoff", 2: "leak", 4: "shot"}        # bits of the feature mask, as in v2v_amd/csrc/v2v_v2e.hpp
TWO_STEP_CUTOFF = 26.738033171514086                  # float32(dt / tau) takes two values over 31 frame pairs at 24 fps


def v2e_args(model, mask, refractory=0.0, fps=24, cutoff=30.0):
    """The 12 positional arguments of video_to_voxel for a feature mask {1 low-pass, 2 leak, 4 shot noise}."""
    return [fps, model, 0.5, 0.1, 0.0, 0.1, cutoff if mask & 1 else 0, 0.1 if mask & 2 else 0, refractory, 5.0 if mask & 4 else 0, 0.1, 0.1]


def mixed_clip(n, h, w, seed):
    """[n,h,w] float32 in [0, 255]: a smooth integer video plus a uniform fraction in [0, 0.9); a random quarter of the pixels
    is set back to its integer value, so every wave mixes table lanes with recomputed lanes."""
    g = np.random.default_rng(seed)
    whole = O.synth_clip_s1(n, h, w, seed=seed, dtype=np.float32)
    x = np.clip(whole + g.uniform(0.0, 0.9, size=whole.shape), 0, 255).astype(np.float32)
    back = g.random(whole.shape) < 0.25
    x[back] = whole[back]
    return x


def mixed_batch(b, n, h, w, seed):
    return np.stack([mixed_clip(n, h, w, seed + i) for i in range(b)])


# (frame, value) of the odd pixels of degenerate_clip, in the order of their positions
ODD_PIXELS = (((0,), np.nan), ((4,), np.nan), ((3,), np.inf), ((5, 6), np.inf), ((2,), -np.inf), ((6,), -3.0), ((1,), -2.0),
              ((7,), 300.0), ((8,), 1e30), ((3,), 0.5))


def degenerate_positions(h, w):
    """Flat pixel index of each odd pixel: every one in a 4-pixel group (work-item) of its own, spread over the frame, the
    last ones in the last wave of the 4-pixel mapping -- which must be a partly filled one."""
    groups = h * w // 4
    assert h * w % 4 == 0 and groups % 64 != 0 and groups >= 10 * len(ODD_PIXELS)
    pos = [4 * (i * groups // len(ODD_PIXELS)) + (i + 1) % 4 for i in range(len(ODD_PIXELS))]
    assert len({p // 4 for p in pos}) == len(pos) and pos[-1] // 4 >= (groups - 1) // 64 * 64
    return pos


def degenerate_clip(n, h, w, seed):
    """mixed_clip with isolated NaN, +-inf, negative, out-of-range and sub-integer pixels.  Returns (clip, flat positions)."""
    x = mixed_clip(n, h, w, seed)
    flat = x.reshape(n, h * w)
    pos = degenerate_positions(h, w)
    for p, (frames, value) in zip(pos, ODD_PIXELS):
        for f in frames:
            assert f < n
            flat[f, p] = value
    return x, pos


def numpy_oracle(video, args, seed, rng=O.V2ERng, record=None):
    """The NumPy oracle on arbitrary content: the formula for every pixel (no table), NumPy's own warnings silenced."""
    with np.errstate(all="ignore"):
        return O.v2e_video_to_voxel(video, *args, seed=seed, rng=rng, use_lut=False, record=record)


def replay_tensors(record):
    """The fields recorded by the NumPy oracle for ONE clip, as v2e.v2e_voxel_batch's replay dict wants them (no batch axis)."""
    pt, nt = np.stack(record["pos_thres"]), np.stack(record["neg_thres"])
    temporal = pt.shape[0] > 1
    out = {"pos_thres": pt[1:] if temporal else pt[0], "neg_thres": nt[1:] if temporal else nt[0], "noise_rate": record["noise_rate"]}
    if record["leak_randn"]:
        out["leak_randn"] = np.stack(record["leak_randn"])
    out["shot_pos"], out["shot_neg"] = np.stack(record["shot_pos"]).astype(np.int64), np.stack(record["shot_neg"]).astype(np.int64)
    return out


class NativeRng:
    """The device-native random fields behind the NumPy oracle's rng interface, in the oracle's draw order.  Field numbering
    of v2v_amd/csrc/v2v_v2e.hpp: block 0 the static thresholds (the two deviates of a word: first / second normal), block 2
    the leak-rate normal, per frame i block 16 + 8 i (+0 redrawn thresholds, +3 shot uniforms), per couple m of frame pairs
    block 16 + 8 m + 2 the leak jitter (7 Philox rounds, like the shot uniforms); the Poisson sampler is the native float32
    inversion, exp the native expf."""

    def __init__(self, clib, seed, clip_id, h, w, temporal):
        self.c, self.seed, self.clip, self.h, self.w, self.temporal = clib, seed, clip_id, h, w, temporal
        self.n_normal = self.n_randn = self.n_poisson = 0
        self.rounds = clib.noise_rounds()

    def _gauss(self, field, comp, rounds=10):
        g = self.c.philox_gauss_field(self.seed, self.clip, field, self.h * self.w, 1, comp, rounds)
        return g.astype(np.float64).reshape(self.h, self.w)

    def normal(self, loc, scale, shape):
        c = self.n_normal
        self.n_normal += 1
        field = 0
        if self.temporal and c not in (2, 3):       # draws 0, 1: frame 0's, discarded; 2, 3: the initial ones; then two per frame
            field = 16 + 8 * (0 if c < 2 else (c - 4) // 2 + 1)
        return loc + scale * self._gauss(field, c & 1)

    def randn(self, h, w):
        c = self.n_randn
        self.n_randn += 1
        if c == 0:
            return self._gauss(2, 0)
        k = c - 1                                   # leak jitter of frame pair k: member k & 1 of couple k >> 1
        return self._gauss(16 + 8 * (k >> 1) + 2, k & 1, self.rounds)

    def poisson(self, lam):
        c = self.n_poisson
        self.n_poisson += 1
        u = self.c.philox_uniform16_field(self.seed, self.clip, 16 + 8 * (c // 2 + 1) + 3, self.h * self.w, 1, low=c & 1)
        return self.c.poisson_inv_f32(np.asarray(lam, dtype=np.float64).astype(np.float32), u.reshape(self.h, self.w))

    def exp(self, x):
        x = np.asarray(x)
        return self.c.expf_det(x).reshape(x.shape) if x.dtype == np.float32 else np.exp(x)


def takes_specialised(shape, in_dtype, args, *, out64, rng_mode="philox", contiguous=True):
    """launch_v2e's routing rule (v2v_amd/csrc/v2v_v2e_tu.hip, the vec4 test of v2v_v2e_voxel_hip), restated: a
    feature-specialised instance runs iff the launch maps 4 pixels per work-item (H*W, frame stride and clip stride divisible
    by 4), the grid is float32, the fields are Philox's, the thresholds are not redrawn per frame and -- float32 input with a
    low-pass -- float32(dt / tau) is ONE value over the clip.  Everything else takes a run-time-feature instance."""
    b, n, h, w = shape
    assert contiguous                              # frame stride H*W, clip stride N*H*W
    vec4 = (h * w) % 4 == 0
    spec = vec4 and not out64 and rng_mode == "philox" and args[1] != "spatial_temporal_independent"
    if spec and np.dtype(in_dtype) == np.float32 and args[6] > 0:
        spec = len(dt_over_tau_f32(args[0], args[6], n - 1)) == 1
    return spec


def dt_over_tau_f32(fps, cutoff, k):
    i = np.arange(1, k + 1, dtype=np.float64)
    tau = 1 / (math.pi * 2 * cutoff)
    return set(((i / float(fps) - (i - 1) / float(fps)) / tau).astype(np.float32).tolist())


# ---------------------------------------------------------------------------------------------------- the GPU cases
B, N, H, W = 3, 10, 52, 80                          # 4160 pixels: 5 workgroups per clip (the last: 16 lanes of one wave), 2 pre-pass ones
BINS = {"sum": dict(num_bins=3, frames_per_bin=1), "bilinear": dict(num_bins=5, frames_per_bin=1)}


def spec_case(bin_mode, mask):
    """Parameters of the specialised-instance case (bin_mode, feature mask): pn_related for even masks, spatial_independent for
    odd ones; the refractory cap on one low-pass + shot case."""
    model = "spatial_independent" if mask & 1 else "pn_related"
    return v2e_args(model, mask, refractory=1 / 240 if (bin_mode, mask) == ("sum", 5) else 0.0)


SPEC_CASES = [(bm, mask) for bm in ("sum", "bilinear") for mask in range(8)]
REPLAY_SIZES = [(36, 40), (35, 41)]                 # 4 pixels per work-item; 1 pixel per work-item with a scalar tail


def replay_args(model):
    return v2e_args(model, 7, refractory=1 / 240 if model == "spatial_temporal_independent" else 0.0)


def philox_oracle(clib, luts, video, args, bin_mode, uint8_wrap=True, **bins):
    bm = clib.BIN_SUM if bin_mode == "sum" else clib.BIN_BILINEAR
    return clib.v2e_voxel(video, clib.v2e_params(*args, uint8_wrap=uint8_wrap), luts, seed=SEED, clip_id0=CLIP_ID0, bin_mode=bm, **bins)


def replay_oracle(video, args, seed0):
    """NumPy oracle clip by clip (global stream seeded with seed0 + clip): (voxels [B,K,H,W] float64, replay dict with a batch axis)."""
    outs, recs = [], []
    for c in range(video.shape[0]):
        rec = {}
        outs.append(numpy_oracle(video[c], args, seed0 + c, record=rec))
        recs.append(replay_tensors(rec))
    return np.stack(outs), {k: np.stack([r[k] for r in recs]) for k in recs[0]}


def mixed_content_cases(clib, luts):
    """Every GPU case that runs on mixed content, as (id, content, fn): fn(content) is the oracle output the GPU test asserts
    against.  The CPU side runs fn on rounded and on truncated content to show that such a kernel could not pass."""
    cases = []
    video = mixed_batch(B, N, H, W, 100)
    for bm, mask in SPEC_CASES:
        cases.append((f"spec-{bm}-{mask}", video, lambda v, bm=bm, mask=mask: philox_oracle(clib, luts, v, spec_case(bm, mask), bm, **BINS[bm])[0]))
    sti = v2e_args("spatial_temporal_independent", 7)
    cases.append(("runtime-temporal", video, lambda v: philox_oracle(clib, luts, v, sti, "sum", **BINS["sum"])[0]))
    for h, w in REPLAY_SIZES:
        small = mixed_batch(B, N, h, w, 200)
        for model in O.V2E_MODELS:
            cases.append((f"replay-{model}-{h}x{w}", small, lambda v, model=model: replay_oracle(v, replay_args(model), 40)[0]))
    long_clip = mixed_batch(B, 32, H, W, 300)
    for co in (TWO_STEP_CUTOFF, 30.0):
        a = v2e_args("pn_related", 7, cutoff=co)
        cases.append((f"cutoff-{co:.3f}", long_clip, lambda v, a=a: philox_oracle(clib, luts, v, a, "sum", num_bins=31, frames_per_bin=1)[0]))
    return cases
