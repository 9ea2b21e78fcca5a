"""-m gpu: the ESIM kernels' workgroup prologue -- the parameter checks, the symmetry promise and the reciprocal threshold worked out once
per workgroup and handed on through LDS (a flag word, one 16-byte read), the bilinear tables behind a single barrier -- against the C oracle
with the bars of tests/test_esim_ring4.py: SUM voxels and ON/OFF totals bit-exact, float32 bilinear voxels rtol = atol = 1e-5, the launch
with and without totals identical bits.  The cases are those of a REORDERED prologue (they also pinned the variants that request frames
and draw the start fields in front of the barrier, docs/experiments/README.md).

Shapes are the smallest at which a reordered prologue can go wrong: 1 x 4 (one lane of one wave), 8 x 36 (72 four-pixel work-items: one
full wave, 8 lanes of a second, two waves without a pixel that still stage their share of the tables and meet the barrier) and 40 x 32
(320 work-items: a second workgroup with one live wave and three empty ones); three clips each."""
import numpy as np
import pytest

gpu = pytest.mark.gpu
SEED = 20240001
SYM = [0.2, 0.2, 0.1, 1e-3, 0.1]          # pos_thres, neg_thres, base_noise_std, hot_pixel_fraction, hot_pixel_std (data/v2v_core_esim.py:8-16)
ASYM = [0.2, 0.3, 0.1, 1e-3, 0.1]
MODES = [("bilinear", 5, 1), ("bilinear", 2, 1), ("sum", 1, 1)]          # (bin mode, bins, frames per bin)
SHAPES = [(1, 4), (8, 36), (40, 32)]
BAD = 513                                  # the statistics' flag word (kStatBad: behind the 513 histogram bins)


def _clips(b, n, h, w, dtype, seed=SEED):
    import torch
    from v2v_amd import esim
    return esim.synth_clips(b, n, h, w, dtype=getattr(torch, dtype), seed=seed, clip_id0=0)


def _check(oracle_c, luts, frames, params, mode, tb, fpb, mapping, what, **kw):
    """One launch with and one without the ON/OFF totals against the oracle; -> the voxels."""
    import torch
    from v2v_amd import esim
    b = frames.shape[0]
    counts = torch.zeros((b, 2), dtype=torch.int64, device="cuda")
    args = dict(bin_mode=mode, num_bins=tb, frames_per_bin=fpb, seed=SEED, clip_id0=0, mapping=mapping, **kw)
    out = esim.esim_voxel_batch(frames, params, counts=counts, **args)
    plain = esim.esim_voxel_batch(frames, params, **args)
    torch.cuda.synchronize()
    want, totals = oracle_c.esim_voxel(frames.cpu().numpy(), params, luts, seed=SEED, clip_id0=0,
                                       bin_mode=oracle_c.BIN_SUM if mode == "sum" else oracle_c.BIN_BILINEAR, num_bins=tb, frames_per_bin=fpb)
    got = out.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, what
    if mode == "sum":
        assert np.array_equal(got, want), what
    else:
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5, err_msg=what)
    assert np.array_equal(counts.cpu().numpy(), totals), f"{what}: ON/OFF totals"
    bits = np.uint32 if out.dtype == torch.float32 else np.uint64
    assert np.array_equal(plain.cpu().numpy().view(bits), out.cpu().numpy().view(bits)), f"{what}: with / without totals"
    return out


@gpu
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_work_items_and_waves_past_the_end_of_a_clip(oracle_c, luts, hw, dtype):
    """Lanes, whole waves and most of a workgroup own no pixel: they stage their share of the tables and meet the barrier all the same."""
    frames = _clips(3, 7, hw[0], hw[1], dtype)
    for mapping in ("4px", "2px", "1px"):
        for pname, params in (("sym", SYM), ("asym", ASYM)):
            for mode, tb, fpb in MODES:
                _check(oracle_c, luts, frames, params, mode, tb, fpb, mapping, f"{hw} {dtype} {mapping} {pname} {mode} tb={tb}")


@gpu
@pytest.mark.parametrize("k", [2, 3, 4, 5, 9])
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_ring_prefill_clamps(oracle_c, luts, k, dtype):
    """Fewer frame pairs than ring slots (4; 8 with one pixel per work-item), one more, and a turn plus one: the ring's first requests
    clamp to the last frame exactly like the ones the time loop issues."""
    frames = _clips(3, k + 1, 8, 36, dtype, seed=SEED + k)
    for mapping in ("4px", "1px"):
        for pname, params in (("sym", SYM), ("asym", ASYM)):
            for mode, tb, fpb in MODES:
                _check(oracle_c, luts, frames, params, mode, tb, fpb, mapping, f"K={k} {dtype} {mapping} {pname} {mode} tb={tb}")


BAD_ROWS = {"zero threshold": [0.0, 0.3, 0.1, 1e-3, 0.1], "negative threshold": [0.2, -0.3, 0.1, 1e-3, 0.1],
            "NaN threshold": [float("nan"), 0.3, 0.1, 1e-3, 0.1], "threshold 1e31": [1e31, 0.3, 0.1, 1e-3, 0.1],
            "negative noise": [0.2, 0.3, -0.1, 1e-3, 0.1]}


@gpu
@pytest.mark.parametrize("case", list(BAD_ROWS))
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_the_flag_word_poisons_its_clip_only(case, dtype):
    """A device-resident [B,5] table with one row outside the domain: that clip is all NaN (SUM with statistics: its flag word set), every
    other clip -- voxels and statistics -- has the bits of the same launch with a good row in its place."""
    import torch
    from v2v_amd import _lib, esim
    frames = _clips(4, 6, 8, 36, dtype)
    rows = [ASYM, BAD_ROWS[case], [0.25, 0.2, 0.05, 1e-3, 0.1], ASYM]
    clean_rows = [ASYM, ASYM, rows[2], ASYM]
    ok = [0, 2, 3]
    dev = lambda r: torch.tensor(r, dtype=torch.float64, device="cuda")   # noqa: E731
    for mapping in ("4px", "1px"):
        for mode, tb in (("bilinear", 5), ("sum", 5)):
            st = [torch.zeros((4, _lib.VOXEL_STATS_WORDS), dtype=torch.int32, device="cuda") if mode == "sum" else None for _ in range(2)]
            clean = esim.esim_voxel_batch(frames, dev(clean_rows), bin_mode=mode, num_bins=tb, seed=SEED, mapping=mapping, stats=st[0])
            out = esim.esim_voxel_batch(frames, dev(rows), bin_mode=mode, num_bins=tb, seed=SEED, mapping=mapping, stats=st[1])
            assert not bool(torch.isnan(clean).any())
            assert bool(torch.isnan(out[1]).all()), f"{case} {mapping} {mode}"
            assert torch.equal(out[ok], clean[ok]), f"{case} {mapping} {mode}: the other clips"
            if mode == "sum":
                assert int(st[1][1, BAD]) != 0 and int(st[0][:, BAD].abs().sum()) == 0
                assert torch.equal(st[1][ok], st[0][ok]), f"{case} {mapping}: the other clips' statistics"


@gpu
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_a_broken_symmetry_promise_poisons_its_clip_only(dtype):
    """A host list with C+ != C- in one row under symmetric=True (the instances compiled without the by-polarity loop)."""
    import torch
    from v2v_amd import _lib, esim
    frames = _clips(4, 6, 8, 36, dtype)
    rows = [SYM, SYM, ASYM, [0.3, 0.3, 0.05, 1e-3, 0.1]]
    clean_rows = [SYM, SYM, SYM, rows[3]]
    ok = [0, 1, 3]
    for mode, tb in (("bilinear", 5), ("sum", 5)):
        st = [torch.zeros((4, _lib.VOXEL_STATS_WORDS), dtype=torch.int32, device="cuda") if mode == "sum" else None for _ in range(2)]
        clean = esim.esim_voxel_batch(frames, clean_rows, bin_mode=mode, num_bins=tb, seed=SEED, mapping="4px", symmetric=True, stats=st[0])
        out = esim.esim_voxel_batch(frames, rows, bin_mode=mode, num_bins=tb, seed=SEED, mapping="4px", symmetric=True, stats=st[1])
        assert not bool(torch.isnan(clean).any())
        assert bool(torch.isnan(out[2]).all()) and torch.equal(out[ok], clean[ok]), mode
        if mode == "sum":
            assert int(st[1][2, BAD]) != 0 and int(st[0][:, BAD].abs().sum()) == 0 and torch.equal(st[1][ok], st[0][ok])


EDGES = {"no hot pixels": [0.2, 0.2, 0.1, 0.0, 0.1], "hot pixels without base noise": [0.2, 0.2, 0.0, 1e-3, 0.1],
         "5 % hot pixels": [0.2, 0.2, 0.1, 0.05, 0.1], "5 % hot pixels, by polarity": [0.2, 0.3, 0.1, 0.05, 0.1],
         "noise-free": [0.2, 0.2, 0.0, 0.0, 0.0], "noise-free, by polarity": [0.2, 0.3, 0.0, 0.0, 0.0]}


@gpu
@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_parameter_edges_that_skip_set_up_branches(oracle_c, luts, edge, dtype):
    """No hot-pixel field at all; hot pixels with a zero base noise; every wave owns a hot pixel (the HOT copy of the time loop); the
    instances without the noise path (no Gaussian table to stage)."""
    frames = _clips(3, 7, 8, 36, dtype)
    for mode, tb, fpb in MODES:
        _check(oracle_c, luts, frames, EDGES[edge], mode, tb, fpb, "4px", f"{edge} {dtype} {mode} tb={tb}")


@gpu
def test_frame_index_launch_keeps_its_order(oracle_c, luts):
    """The indexed launch (its row check and the parameter flag share the barrier): 2 clips x 9 stored frames x 8 x 36 against the oracle on the
    gathered clips, and a row with an index outside its clip -> NaN planes + flag word, the other clip untouched."""
    import torch
    from v2v_amd import _lib, esim
    g = np.random.default_rng(11)
    b, n, h, w, stored = 2, 11, 8, 36, 9
    clips = g.integers(0, 256, (b, stored, h, w), dtype=np.uint8)
    fidx = np.stack([np.sort(np.concatenate([np.arange(stored), g.integers(0, stored, n - stored)])) for _ in range(b)]).astype(np.int32)
    gathered = np.stack([c[i] for c, i in zip(clips, fidx)])
    flat = torch.from_numpy(clips.reshape(-1)).cuda()
    offs = torch.tensor([0, stored * h * w], dtype=torch.int64, device="cuda")
    st_n = torch.full((b,), stored, dtype=torch.int32, device="cuda")
    params = torch.tensor([ASYM, ASYM], dtype=torch.float64, device="cuda")
    keys = torch.tensor([[SEED, 0], [SEED, 1]], dtype=torch.int64, device="cuda")
    want, _ = oracle_c.esim_voxel(gathered, ASYM, luts, seed=SEED, clip_id0=0, bin_mode=oracle_c.BIN_SUM, num_bins=5, frames_per_bin=1)
    bad = fidx.copy()
    bad[1, 4] = stored
    for mapping in ("4px", "2px", "1px"):
        st = torch.zeros((b, _lib.VOXEL_STATS_WORDS), dtype=torch.int32, device="cuda")
        got = esim.esim_voxel_packed(flat, offs, torch.from_numpy(fidx).cuda(), h, w, params, keys, num_bins=5, stats=st, stored_frames=st_n, mapping=mapping)
        assert np.array_equal(got.cpu().numpy().astype(np.float64), want), mapping
        assert int(st[:, BAD].abs().sum()) == 0
        st2 = torch.zeros_like(st)
        out = esim.esim_voxel_packed(flat, offs, torch.from_numpy(bad).cuda(), h, w, params, keys, num_bins=5, stats=st2, stored_frames=st_n, mapping=mapping)
        assert bool(torch.isnan(out[1]).all()) and int(st2[1, BAD]) == 1, mapping
        assert torch.equal(out[0], got[0]) and torch.equal(st2[0], st[0]), mapping


@gpu
def test_replay_fields_and_float64_output(oracle_c, luts):
    """The instances with replayed fields (read from memory) and the float64-output ones, one 8 x 36 clip each."""
    import torch
    from v2v_amd import esim
    h, w, k = 8, 36, 5
    frames = _clips(1, k + 1, h, w, "uint8")
    g = np.random.default_rng(3)
    replay = (g.random((1, h, w)), g.random((1, h, w)), g.standard_normal((1, h, w)), g.standard_normal((1, k, h, w)))
    params = [0.2, 0.3, 0.1, 0.05, 0.1]
    for mode, tb in (("sum", 1), ("bilinear", 5)):
        bm = oracle_c.BIN_SUM if mode == "sum" else oracle_c.BIN_BILINEAR
        want, totals = oracle_c.esim_voxel(frames.cpu().numpy(), params, luts, rng_mode=oracle_c.RNG_REPLAY, replay=replay, bin_mode=bm, num_bins=tb)
        counts = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
        got = esim.esim_voxel_batch(frames, params, bin_mode=mode, num_bins=tb, rng_mode="replay", replay=replay, out_dtype=torch.float64, counts=counts)
        if mode == "sum":
            assert np.array_equal(got.cpu().numpy(), want)
        else:
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
        assert np.array_equal(counts.cpu().numpy(), totals)
    for dtype in ("float32", "uint8"):
        f = _clips(1, k + 1, h, w, dtype)
        for mode, tb, fpb in MODES:
            _check(oracle_c, luts, f, SYM, mode, tb, fpb, "4px", f"float64 output {dtype} {mode} tb={tb}", out_dtype=torch.float64)
