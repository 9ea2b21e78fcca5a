"""-m gpu: the ESIM step's quotient screen against the oracles, with the bars of tests/test_esim_ring4.py: SUM
voxels and ON/OFF totals bit-exact, float32 bilinear voxels rtol = atol = 1e-5.

The step finds the rare +1 fix-up of its floor-divide estimate on the low word of the estimate and runs the residual fma + compare only
then; a wave whose clip parameters do not bound the quotient below 2^20, or that has met a frame value outside the log table, runs them in
every step ("paranoid").  Cases: the screened instances of every mapping, both inputs, both bin modes, symmetric and by-polarity
thresholds; parameters that break the bound; float32 frames with single off-table pixels in one middle frame (paranoid from that frame
on, and only in the waves that saw one); and clips built so that EVERY step needs the fix-up.

Shapes: 3 clips of N x 8 x 40 (320 pixels: two workgroups per clip in the 1-pixel mapping, the second partly empty; one partly empty
workgroup in the others), N = 9 and 10 frames = 8 and 9 frame pairs (two turns of the 4-frame ring; two turns and a one-step tail);
8 x 160 where the 4-pixel mapping needs its second workgroup; 12 x 12 and 5 x 9 (odd width: only the 1-pixel mapping fits)."""
import warnings

import numpy as np
import pytest

gpu = pytest.mark.gpu
SEED = 20240611
# pos_thres, neg_thres, base_noise_std, hot_pixel_fraction, hot_pixel_std: the reference's default noise, and 5 % hot pixels so that
# waves of both copies of the time loop (with and without a hot pixel) are in every launch
PARAMS = {"sym": [0.2, 0.2, 0.1, 0.05, 0.1], "asym": [0.2, 0.3, 0.1, 0.05, 0.1]}
MODES = [("bilinear", 5, 1), ("sum", 1, 1)]                              # (bin mode, bins, frames per bin)
MAPPINGS = ["4px", "2px", "1px"]
NS = [9, 10]


def _launch(frames, params, mode, tb, fpb, mapping, rng_mode, counts=None, **kw):
    from v2v_amd import esim
    return esim.esim_voxel_batch(frames, params, bin_mode=mode, num_bins=tb, frames_per_bin=fpb, rng_mode=rng_mode, seed=SEED, clip_id0=0,
                                 counts=counts, mapping=mapping, **kw)


def _check(oracle_c, luts, frames, params, mode, tb, fpb, mapping, what, rng_mode="philox", f32_slack=None):
    """The oracle call and the comparison of tests/test_esim_ring4.py.  f32_slack: see test_parameters_that_break_the_bound."""
    import torch
    b = frames.shape[0]
    counts = torch.zeros((b, 2), dtype=torch.int64, device="cuda")
    out = _launch(frames, params, mode, tb, fpb, mapping, rng_mode, counts)
    plain = _launch(frames, params, mode, tb, fpb, mapping, rng_mode)
    torch.cuda.synchronize()
    want, totals = oracle_c.esim_voxel(frames.cpu().numpy(), params, luts, seed=SEED, clip_id0=0,
                                       rng_mode=oracle_c.RNG_PHILOX if rng_mode == "philox" else oracle_c.RNG_NONE,
                                       bin_mode=oracle_c.BIN_SUM if mode == "sum" else oracle_c.BIN_BILINEAR, num_bins=tb, frames_per_bin=fpb)
    got = out.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, what
    if mode == "sum":
        assert np.array_equal(got, want), what
    elif f32_slack is None:
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5, err_msg=what)
    else:
        assert np.all(np.abs(got - want) <= 1e-5 + 1e-5 * np.abs(want) + f32_slack), what
        import torch
        got64 = _launch(frames, params, mode, tb, fpb, mapping, rng_mode, out_dtype=torch.float64).cpu().numpy()
        assert np.array_equal(got64, want), f"{what}: float64 grid"
    assert np.array_equal(counts.cpu().numpy(), totals), f"{what}: ON/OFF totals"
    assert np.array_equal(plain.cpu().numpy().view(np.uint32), out.cpu().numpy().view(np.uint32)), f"{what}: with / without totals"
    return want, totals


def _clips(dtype, b, n, h, w):
    import torch
    from v2v_amd import esim
    if w % 4:                                                              # the device generator writes 4 pixels per work-item
        v = np.random.default_rng(SEED).integers(0, 256, size=(b, n, h, w))
        return torch.from_numpy(v.astype(np.uint8 if dtype == "u8" else np.float32)).cuda()
    return esim.synth_clips(b, n, h, w, dtype={"u8": torch.uint8, "f32": torch.float32}[dtype], seed=SEED, clip_id0=0)


@gpu
@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_screened_instances(oracle_c, luts, dtype, pname):
    """Noise on: both inputs, both bin modes, symmetric and by-polarity thresholds, every mapping, N = 9 and 10."""
    for n in NS:
        frames = _clips(dtype, 3, n, 8, 40)
        for mode, tb, fpb in MODES:
            for mapping in MAPPINGS:
                _check(oracle_c, luts, frames, PARAMS[pname], mode, tb, fpb, mapping, f"{dtype} N={n} {pname} {mode} {mapping}")


@gpu
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_second_workgroup_and_one_pixel_shapes(oracle_c, luts, dtype):
    """8 x 160: the 4-pixel mapping's second workgroup (a quarter full); 12 x 12 and 5 x 9 at N = 9: the 1-pixel mapping (5 x 9 fits no
    other), a partly empty last wave."""
    for pname in PARAMS:
        for mode, tb, fpb in MODES:
            _check(oracle_c, luts, _clips(dtype, 3, 9, 8, 160), PARAMS[pname], mode, tb, fpb, "4px", f"{dtype} 8x160 {pname} {mode}")
            _check(oracle_c, luts, _clips(dtype, 3, 9, 12, 12), PARAMS[pname], mode, tb, fpb, "1px", f"{dtype} 12x12 {pname} {mode}")
            _check(oracle_c, luts, _clips(dtype, 3, 9, 5, 9), PARAMS[pname], mode, tb, fpb, "auto", f"{dtype} 5x9 {pname} {mode}")


@gpu
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_parameters_that_break_the_bound(oracle_c, luts, dtype):
    """C = 1e-6 with base_std = 1.0: quotients reach 1e7 > 2^20, the lemma's premise fails and every wave runs the full check from the
    first step.  Counts stay below 2^24, so the float32 SUM planes are still exact (the bar of tests/test_esim_ring4.py).  The float32
    BILINEAR grid cannot meet that file's rtol = atol = 1e-5 at this size, with or without the screen: a voxel is a float32 fma chain
    over K = N - 1 counts of up to 1e7 of either sign (ulp(1e7) = 1), and each link rounds once, to within 2^-24 of a partial sum that is
    at most the sum of the |counts|.  So the float32 bilinear bar here is 1e-5 + 1e-5 |want| + K 2^-24 sum_k |count_k| (from the number
    format, not from the kernel's output), and the exactness moves to the float64 grid, which must equal the oracle bit for bit."""
    for params in ([1e-6, 1e-6, 1.0, 0.05, 0.1], [1e-6, 2e-6, 1.0, 0.05, 0.1]):
        for n in NS:
            frames = _clips(dtype, 3, n, 8, 40)
            slack = None
            for mode, tb, fpb in reversed(MODES):                          # SUM first: its oracle planes give the bilinear slack
                for mapping in MAPPINGS:
                    want, _ = _check(oracle_c, luts, frames, params, mode, tb, fpb, mapping, f"{dtype} N={n} C={params[:2]} {mode} {mapping}",
                                     f32_slack=slack)
                    assert np.abs(want).max() > float(1 << 20)
                if mode == "sum":                                          # want: [B, K, 1, H, W]
                    slack = ((n - 1) * 2.0 ** -24 * np.abs(want).sum(axis=(1, 2)))[:, None]


# off-table values of one middle frame: non-integer, negative, above 255, overflowing, and the non-finite ones
ODD_VALUES = [100.5, -3.0, 300.0, 1e30, float("nan"), float("inf"), float("-inf")]
ODD_FLAT = [1, 87, 140, 233, 250, 270, 299]                               # flat pixel indices, all inside the first 320 pixels
ODD_CLIP, ODD_FRAME = 1, 5


@gpu
@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("shape", [(8, 40), (8, 160)])
def test_off_table_pixels_in_a_middle_frame(oracle_c, luts, shape, pname):
    """float32 clips; single pixels of frame 5 of clip 1 are 100.5, -3, 300, 1e30, NaN and +-inf.  The waves that own one take the log
    table's slow path there and run the full check from that frame on; the other waves, the other clips and (8 x 160, 4-pixel mapping)
    the second workgroup never do.  Every other pixel: the C oracle on the same clip with those pixels put back on the table.  The
    odd pixels themselves (pixels are independent): the NumPy oracle, which evaluates the reference's float32 expression, on the
    device-native fields -- NaN-aware equality on the SUM planes, as tests/test_hip_parity.py compares degenerate frames."""
    import torch
    from oracle import v2v_oracle as O
    h, w = shape
    n = 10
    params = PARAMS[pname]
    clean = _clips("f32", 3, n, h, w).cpu().numpy()
    video = clean.copy()
    ys, xs = np.divmod(np.array(ODD_FLAT), w)
    video[ODD_CLIP, ODD_FRAME, ys, xs] = np.array(ODD_VALUES, dtype=np.float32)
    odd = np.zeros((3, h, w), dtype=bool)
    odd[ODD_CLIP, ys, xs] = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_odd = O.esim_video_to_voxel(video[ODD_CLIP], *params, rng=O.PhiloxFieldRNG(SEED, ODD_CLIP))[:, ys, xs]      # [K, 7]
    assert np.isnan(want_odd).any()
    frames = torch.from_numpy(video).cuda()
    for mode, tb, fpb in MODES:
        want, _ = oracle_c.esim_voxel(clean, params, luts, seed=SEED, clip_id0=0,
                                      bin_mode=oracle_c.BIN_SUM if mode == "sum" else oracle_c.BIN_BILINEAR, num_bins=tb, frames_per_bin=fpb)
        for mapping in MAPPINGS:
            what = f"{h}x{w} {pname} {mode} {mapping}"
            got = _launch(frames, params, mode, tb, fpb, mapping, "philox").cpu().numpy().astype(np.float64)
            assert got.shape == want.shape, what
            if mode == "sum":                                              # [B, K, 1, H, W]
                keep = np.broadcast_to(~odd[:, None, None], got.shape)
                assert np.array_equal(got[keep], want[keep]), what
                got_odd = got[ODD_CLIP, :, 0][:, ys, xs]
                assert np.array_equal(got_odd, want_odd, equal_nan=True), f"{what}: odd pixels {got_odd} != {want_odd}"
            else:                                                          # [B, Tb, H, W]
                keep = np.broadcast_to(~odd[:, None], got.shape)
                np.testing.assert_allclose(got[keep], want[keep], rtol=1e-5, atol=1e-5, err_msg=what)


@gpu
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_every_step_needs_the_fix_up(oracle_c, luts, dtype):
    """rng mode "none": the potential starts at exactly 0.  Frames alternate between two table values a and b, and C+ is the table
    difference log(b) - log(a) in the input's precision, so the potential reaches +-C exactly in every step: |p| * inv_low(C) is just
    below an integer, the estimate is short by one and only the fix-up gives the event.  A third of the pixels runs in the opposite
    phase, a third is constant.  Symmetric thresholds only: with C+ != C- the potential does not start at 0.  Counts must equal the
    oracle's exactly, and the oracle's must be what the construction says: one event per moving pixel and step."""
    import torch
    a, b, n, h, w = 40, 200, 10, 8, 40
    if dtype == "u8":
        c = float(np.float64(luts["lut64"][b]) - np.float64(luts["lut64"][a]))
    else:
        c = float(np.float32(luts["lut32"][b]) - np.float32(luts["lut32"][a]))
    assert c > 0
    phase = np.arange(h * w).reshape(h, w) % 3                             # 0: a b a b ..., 1: b a b a ..., 2: constant
    t = np.arange(n)[:, None, None]
    clip = np.where(phase == 2, 77, np.where((t + phase) % 2 == 0, a, b))
    video = np.stack([clip, clip[:, ::-1], clip[:, :, ::-1]]).astype(np.uint8 if dtype == "u8" else np.float32)
    frames = torch.from_numpy(video).cuda()
    params = [c, c, 0.0, 0.0, 0.0]
    for mode, tb, fpb in MODES:
        for mapping in MAPPINGS:
            want, totals = _check(oracle_c, luts, frames, params, mode, tb, fpb, mapping, f"{dtype} {mode} {mapping}", rng_mode="none")
            if mode == "sum":
                moving = np.broadcast_to((phase != 2)[None, None, None], want[:1].shape)
                assert set(np.unique(want[:1][moving])) == {1.0, -1.0} and not want[:1][~moving].any()
                assert totals[0, 0] + totals[0, 1] == (n - 1) * int((phase != 2).sum())
