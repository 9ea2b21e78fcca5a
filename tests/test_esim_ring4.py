"""-m gpu: the float32 4-pixel device-noise ESIM instances (symmetric-only and by-polarity) at the edges of their 4-frame register
ring, against the C oracle with the bars of tests/test_hip_fullsize.py: SUM voxels and ON/OFF totals bit-exact, float32 bilinear
voxels rtol = atol = 1e-5.

Shapes: 3 clips of (K + 1) x 8 x 32 float32 = one 64-lane wave of 4-pixel work-items per clip (clip 2 is a second workgroup), with
K frame pairs below the ring (1, 2, 3), at every K mod 4 (4, 5, 7, 9 -> tails of 0, 1, 3, 1 steps) and at two whole turns (8: empty
tail).  mapping="4px" pins the 4-pixel instances (a batch this small would otherwise take the 1-pixel mapping); a host parameter
list with C+ == C- selects the symmetric-only instance, C+ != C- the by-polarity one."""
import numpy as np
import pytest

gpu = pytest.mark.gpu
SEED = 20240001
KS = [1, 2, 3, 4, 5, 7, 8, 9]
# pos_thres, neg_thres, base_noise_std, hot_pixel_fraction, hot_pixel_std: the reference's default noise (data/v2v_core_esim.py:8-16) ...
PARAMS = {"sym": [0.2, 0.2, 0.1, 1e-3, 0.1], "asym": [0.2, 0.3, 0.1, 1e-3, 0.1],
          # ... and 5 % hot pixels: with 256 pixels per wave every wave owns one (1 - 0.95^256) and takes the HOT copy of the time loop,
          # whose hot-pixel deviate is held as float32 and scaled in the step
          "sym_hot": [0.2, 0.2, 0.1, 0.05, 0.1], "asym_hot": [0.2, 0.3, 0.1, 0.05, 0.1]}
MODES = [("bilinear", 5, 1), ("bilinear", 2, 1), ("sum", 1, 1)]          # (bin mode, bins, frames per bin)


def _check(oracle_c, luts, frames, params, mode, tb, fpb, what):
    import torch
    from v2v_amd import esim
    b = frames.shape[0]
    if mode == "bilinear" and frames.shape[1] == 2:
        # one frame pair has no temporal-bilinear grid (dt = 0): the entry point refuses it, as before; K = 1 runs in SUM mode only
        with pytest.raises(AssertionError, match="at least 2 frame pairs"):
            esim.esim_voxel_batch(frames, params, bin_mode=mode, num_bins=tb, seed=SEED, clip_id0=0, mapping="4px")
        return
    counts = torch.zeros((b, 2), dtype=torch.int64, device="cuda")
    out = esim.esim_voxel_batch(frames, params, bin_mode=mode, num_bins=tb, frames_per_bin=fpb, seed=SEED, clip_id0=0, counts=counts, mapping="4px")
    plain = esim.esim_voxel_batch(frames, params, bin_mode=mode, num_bins=tb, frames_per_bin=fpb, seed=SEED, clip_id0=0, mapping="4px")
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
    # the launch without the totals (the benchmark's) computes the same planes bit for bit
    assert np.array_equal(plain.cpu().numpy().view(np.uint32), out.cpu().numpy().view(np.uint32)), f"{what}: with / without totals"


@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("pname", list(PARAMS))
def test_ring_edges(oracle_c, luts, k, pname):
    """K below the ring, every K mod 4, an empty tail; default noise (most waves take the loop copy without hot pixels) and 5 % hot
    pixels (every wave takes the HOT copy)."""
    import torch
    from v2v_amd import esim
    frames = esim.synth_clips(3, k + 1, 8, 32, dtype=torch.float32, seed=SEED, clip_id0=0)
    for mode, tb, fpb in MODES:
        _check(oracle_c, luts, frames, PARAMS[pname], mode, tb, fpb, f"K={k} {pname} {mode} tb={tb}")


@gpu
@pytest.mark.parametrize("pname", list(PARAMS))
def test_one_lane(oracle_c, luts, pname):
    """One clip of 1 x 4 pixels: a single active lane in the only wave."""
    import torch
    from v2v_amd import esim
    for k in KS:
        frames = esim.synth_clips(1, k + 1, 1, 4, dtype=torch.float32, seed=SEED + k, clip_id0=0)
        for mode, tb, fpb in MODES:
            _check(oracle_c, luts, frames, PARAMS[pname], mode, tb, fpb, f"one lane K={k} {pname} {mode} tb={tb}")
