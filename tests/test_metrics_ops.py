"""The evaluation-metric kernels (v2v_amd/csrc/v2v_metrics.hpp) through v2v_amd/metrics.py on the GPU, against the restatements of
tests/metrics_reference.py and golden G33 (tests/golden/g33_metrics.npz).

Bars.  Integer-valued images with divisor 1: the S map and the MSE equal the direct float64 evaluation bit for bit (every moment is exact).
Real-valued images: every S within 1e-9 of G33's float64 map -- a moment's absolute error is at most 49 * 2^-53, divided by B1 >= C1 >=
1e-4 and B2 >= C2 >= 9e-4 that is ~1e-10, with a factor of ten to spare; the mean within 1e-9 + N * 2^-52, N = (H-6)(W-6); the MSE within a
relative 2^-22 of the float64 truth (the float32 subtraction costs at most 2^-23 on a sum of non-negative terms, one bit of margin).
Flow: counts equal, EE sums within a relative H * W * 2^-53 of the float64 sum of the float32 EE, the six ratios equal to the reference's
float32 values where the count is 0 or the case is integer-exact and within float32 summation error H * W * 2^-24 otherwise."""
import functools

import numpy as np
import pytest
import torch

import metrics_reference as MR

pytestmark = pytest.mark.gpu

TX, TY = 32, 8                       # the tile of windows of image_metrics_kernel
EXACT_SIZES = [(7, 7), (7, 40), (40, 7), (8, 9), (45, 31)] + [(TY + 6 + dy, TX + 6 + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


@pytest.fixture(scope="module")
def g33(golden):
    return golden("g33_metrics.npz")


@functools.lru_cache(maxsize=None)
def _exact_pair(T, H, W):
    rng = np.random.default_rng(1000 * H + W + T)
    return rng.integers(0, 16, (T, H, W)).astype(np.float32), rng.integers(0, 16, (T, H, W)).astype(np.float32)


def _mean_bar(n):
    return 1e-9 + n * 2.0 ** -52


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("H,W", EXACT_SIZES)
def test_integer_images_are_bit_exact(H, W, T):
    from v2v_amd import metrics
    x, y = _exact_pair(T, H, W)
    # pred: frames 2*H*W apart inside a larger buffer (a non-zero, non-contiguous frame stride); image: contiguous
    buf = torch.full((T, 2, H, W), 99.0, device="cuda")
    buf[:, 1] = torch.from_numpy(x).cuda()
    pred = buf[:, 1:2]
    assert pred.stride(0) == 2 * H * W
    out, smap = metrics.image_metrics(pred, torch.from_numpy(y).cuda(), divisor=1.0, ssim_map=True)
    assert out.dtype == torch.float64 and out.shape == (T, 2) and smap.shape == (T, H - 6, W - 6) and smap.dtype == torch.float64
    out, smap = out.cpu(), smap.cpu()
    for t in range(T):
        S = MR.ssim_direct64(x[t], y[t], 2.0)
        assert torch.equal(smap[t], torch.from_numpy(S)), f"frame {t}: {int((smap[t] != torch.from_numpy(S)).sum())} of {S.size} windows differ"
        assert float(out[t, 0]) == MR.mse64(x[t], y[t])
        assert abs(float(out[t, 1]) - S.mean()) <= _mean_bar(S.size)
    # the same frames through the other accepted layouts, and a frame stride of 0
    flat = metrics.image_metrics(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), divisor=1.0)
    five = metrics.image_metrics(torch.from_numpy(x).cuda()[None, :, None], torch.from_numpy(y).cuda()[None, :, None], divisor=1.0)
    assert torch.equal(flat.cpu(), out) and torch.equal(five.cpu(), out)
    same = metrics.image_metrics(torch.from_numpy(x[:1]).cuda().expand(T, H, W), torch.from_numpy(y[:1]).cuda().expand(T, H, W), divisor=1.0).cpu()
    assert all(torch.equal(same[t], out[0]) for t in range(T))


@pytest.mark.parametrize("H,W", [(7, 7), (45, 31), (TY + 7, TX + 7)])
def test_equal_images_give_ssim_one_and_mse_zero(H, W):
    from v2v_amd import metrics
    const = torch.stack([torch.full((H, W), v, device="cuda") for v in (0.0, 7.0, 128.0)])
    rnd = torch.from_numpy(MR.image_case("i45x31")[0][:, :H, :W].copy()).cuda() if H <= 45 and W <= 31 else torch.rand((3, H, W), device="cuda") * 255
    for frames in (const, rnd):
        for divisor in (1.0, 255.0):
            out, smap = metrics.image_metrics(frames, frames.clone(), divisor=divisor, ssim_map=True)
            assert torch.equal(out.cpu(), torch.tensor([[0.0, 1.0]] * 3, dtype=torch.float64))
            assert bool((smap == 1.0).all())


@pytest.mark.parametrize("where", ["corner", "last", "tile_boundary"])
def test_one_differing_pixel_touches_exactly_its_windows(where):
    from v2v_amd import metrics
    H, W = 2 * TY + 9, 2 * TX + 11
    py, px = {"corner": (0, 0), "last": (H - 1, W - 1), "tile_boundary": (TY + 2, TX + 3)}[where]
    base = _exact_pair(1, H, W)[0]
    pred = base.copy()
    pred[0, py, px] += 5.0
    out, smap = metrics.image_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(base).cuda(), divisor=1.0, ssim_map=True)
    touched = np.zeros((H - 6, W - 6), dtype=bool)
    touched[max(py - 6, 0):min(py, H - 7) + 1, max(px - 6, 0):min(px, W - 7) + 1] = True
    assert 1 <= touched.sum() <= 49
    assert np.array_equal(smap[0].cpu().numpy() != 1.0, touched)
    assert float(out[0, 0]) == 25.0 / (H * W)
    assert torch.equal(smap[0].cpu(), torch.from_numpy(MR.ssim_direct64(pred[0], base[0], 2.0)))


def _check_real(g33, name, r, out, smap=None):
    pred, image = MR.image_case(name)
    x, y = MR.scaled(pred, 255.0), MR.scaled(image, 255.0)
    T, H, W, _ = MR.IMAGE_CASES[name]
    n = (H - 6) * (W - 6)
    dev_mse = [float(torch.nn.functional.mse_loss(torch.from_numpy(x[t]).cuda(), torch.from_numpy(y[t]).cuda())) for t in range(T)]
    for t in range(T):
        mse, ssim = float(out[t, 0]), float(out[t, 1])
        truth, mse64 = g33[f"{name}__ssim64_r{int(r)}"][t], g33[f"{name}__mse64"][t]
        print(f"{name} r={r} frame {t}: ssim {ssim:.17g} off the truth by {abs(ssim - truth):.2e} (bar {_mean_bar(n):.2e}), off the float32 restatement by "
              f"{abs(ssim - g33[f'{name}__ssim32_r{int(r)}'][t]):.2e}; mse {mse:.17g} off the truth by {abs(mse - mse64) / mse64:.2e} relative "
              f"(bar {2.0 ** -22:.2e}), off F.mse_loss float32 on the CPU by {abs(mse - g33[f'{name}__mse32'][t]) / mse64:.2e}, on the device by "
              f"{abs(mse - dev_mse[t]) / mse64:.2e}")
        if smap is not None:
            d = np.abs(smap[t].cpu().numpy() - g33[f"{name}__S_r{int(r)}"][t]).max()
            print(f"    largest |S - truth| {d:.2e} (bar 1e-9)")
            assert d <= 1e-9
        assert abs(ssim - truth) <= _mean_bar(n)
        assert abs(mse - mse64) <= 2.0 ** -22 * mse64


@pytest.mark.parametrize("r", MR.DATA_RANGES)
@pytest.mark.parametrize("name", MR.SMALL_IMAGE_CASES)
def test_real_valued_images_against_the_float64_truth(g33, name, r):
    from v2v_amd import metrics
    pred, image = (torch.from_numpy(v).cuda() for v in MR.image_case(name))
    out, smap = metrics.image_metrics(pred, image, data_range=r, ssim_map=True)
    _check_real(g33, name, r, out.cpu(), smap)


@pytest.mark.parametrize("name", ["i180x240", "i260x346"])
def test_full_size_frames_against_the_float64_truth(g33, name):
    from v2v_amd import metrics
    pred, image = (torch.from_numpy(v).cuda() for v in MR.image_case(name))
    for r in MR.DATA_RANGES:
        _check_real(g33, name, r, metrics.image_metrics(pred, image, data_range=r).cpu())


# ---- flow ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MR.FLOW_CASES))
def test_flow_counts_sums_and_ratios(g33, name):
    from v2v_amd import metrics
    T, C, H, W, _, exact = MR.FLOW_CASES[name]
    pred, gt, events = (torch.from_numpy(v).cuda() for v in MR.flow_case(name))
    counts, sums = metrics.flow_metrics(pred, gt, events)
    assert counts.dtype == torch.int64 and counts.shape == (T, 6) and sums.dtype == torch.float64 and sums.shape == (T, 2)
    assert np.array_equal(counts.cpu().numpy(), g33[f"{name}__counts"])
    want = g33[f"{name}__ee_sums"]
    err = np.abs(sums.cpu().numpy() - want)
    print(f"{name}: largest relative error of an EE sum {np.max(err / np.maximum(want, 1e-300)):.2e} (bar {H * W * 2.0 ** -53:.2e})")
    assert (err <= H * W * 2.0 ** -53 * want).all()
    if exact:
        assert np.array_equal(sums.cpu().numpy(), want)
    batch = {"frame": torch.zeros((1, T + 1, 1, H, W), device="cuda"), "flow": gt[None], "events": events[None], "sequence_name": [["seq"]],
             "data_source_idx": torch.tensor([2])}
    got = metrics.compute_flow_metrics(pred[None], batch)
    assert list(got) == [f"MVSEC/seq/{k}" for k in MR.FLOW_NAMES]
    ratios, ref = np.array([got[f"MVSEC/seq/{k}"] for k in MR.FLOW_NAMES]).T, g33[f"{name}__ratios"]
    assert all(isinstance(v, float) for k in got for v in got[k]) and ratios.shape == (T, 6)
    assert np.array_equal(ratios.astype(np.float32), ratios), "the values are float32 numbers, as the reference's .item() gives"
    assert np.array_equal(ratios[:, [1, 2, 4, 5]], ref[:, [1, 2, 4, 5]])
    for m in range(2):
        zero = g33[f"{name}__counts"][:, m] == 0
        assert not ratios[zero, 3 * m:3 * m + 3].any()
        if exact:
            assert np.array_equal(ratios[:, 3 * m], ref[:, 3 * m])
        else:
            assert (np.abs(ratios[:, 3 * m] - ref[:, 3 * m]) <= H * W * 2.0 ** -24 * np.abs(ref[:, 3 * m])).all()
    # the raw operator on a batch of one and on frames that lie apart in memory gives the same bits
    c5, s5 = metrics.flow_metrics(pred[None], gt[None], events[None])
    wide = torch.zeros((T, 3, C, H, W), device="cuda")
    wide[:, 1] = events
    c6, s6 = metrics.flow_metrics(pred, gt, wide[:, 1])
    for c, s_ in ((c5, s5), (c6, s6)):
        assert torch.equal(c, counts) and torch.equal(s_.view(torch.int64), sums.view(torch.int64))


def test_nan_pred_and_nan_event_channel():
    from v2v_amd import metrics
    pred, gt, events = (torch.from_numpy(v[:1]).clone() for v in MR.flow_case("f50x47"))
    c0, s0, _ = MR.flow_terms(pred[0], gt[0], events[0])
    valid = torch.logical_not(torch.isnan(gt[0, 0]) | torch.isnan(gt[0, 1]) | ((gt[0, 0] == 0) & (gt[0, 1] == 0)))
    sparse = valid & (events[0].abs().sum(0) > 0)
    # a NaN pred on a valid pixel without events: the dense sum is NaN, the sparse one stays; it counts in neither threshold
    y, x = (int(v[0]) for v in torch.nonzero(valid & ~sparse, as_tuple=True))
    was_gt1, was_gt3 = (float(((pred[0, :, y, x] - gt[0, :, y, x]) ** 2).sum() ** 0.5) > k for k in (1, 3))
    pred[0, 1, y, x] = float("nan")
    counts, sums = (v.cpu().numpy() for v in metrics.flow_metrics(pred.cuda(), gt.cuda(), events.cuda()))
    want = c0.copy()
    want[2] -= was_gt1
    want[3] -= was_gt3
    assert np.array_equal(counts[0], want) and np.array_equal(counts[0, [0, 1, 4, 5]], c0[[0, 1, 4, 5]])
    assert np.isnan(sums[0, 0]) and abs(sums[0, 1] - s0[1]) <= 50 * 47 * 2.0 ** -53 * s0[1]
    batch = {"frame": torch.zeros((1, 2, 1, 50, 47), device="cuda"), "flow": gt[None].cuda(), "events": events[None].cuda(), "sequence_name": [["seq"]],
             "data_source_idx": torch.tensor([2])}
    got = metrics.compute_flow_metrics(pred[None].cuda(), batch)
    assert np.isnan(got["MVSEC/seq/dense_EPE"][0]) and not np.isnan(got["MVSEC/seq/sparse_EPE"][0])
    assert got["MVSEC/seq/dense_1PE"][0] == float(np.float32(want[2]) / np.float32(want[0]))
    # the reference, restated, says the same
    cr, sr, _ = MR.flow_terms(pred[0], gt[0], events[0])
    assert np.array_equal(cr, counts[0]) and np.isnan(sr[0])
    # a NaN event channel makes a sparse pixel not sparse (NaN > 0 is False), whatever the other channels hold
    pred[0, 1, y, x] = 0.0
    ys, xs = (int(v[0]) for v in torch.nonzero(sparse, as_tuple=True))
    events[0, 1, ys, xs] = float("nan")
    counts2, _ = metrics.flow_metrics(pred.cuda(), gt.cuda(), events.cuda())
    cr2, _, _ = MR.flow_terms(pred[0], gt[0], events[0])
    assert np.array_equal(counts2[0].cpu().numpy(), cr2) and cr2[1] == c0[1] - 1 and cr2[0] == c0[0]


# ---- drop-in behaviour ---------------------------------------------------------------------------------------------------------------------
def test_compute_metrics_is_the_raw_operator_frame_by_frame(g33):
    from v2v_amd import metrics
    pred, image = (torch.from_numpy(v).cuda() for v in MR.image_case("i45x31"))
    batch = {"frame": image[None, :, None], "sequence_name": [["boxes_6dof"]], "data_source_idx": torch.tensor([1])}
    raw = metrics.image_metrics(pred, image).cpu()
    got = metrics.compute_metrics(pred[None, :, None], batch)
    assert list(got) == ["IJRR/boxes_6dof/MSE", "IJRR/boxes_6dof/SSIM"]
    assert got["IJRR/boxes_6dof/MSE"] == raw[:, 0].tolist() and got["IJRR/boxes_6dof/SSIM"] == raw[:, 1].tolist()
    assert all(isinstance(v, float) for k in got for v in got[k])
    seen = []

    def lpips_fn(a, b, normalize=False):
        seen.append((a, b, normalize))
        return (a - b).abs().mean().reshape(1, 1, 1, 1)
    got = metrics.compute_metrics(pred[None, :, None], batch, lpips_fn=lpips_fn)
    assert list(got) == ["IJRR/boxes_6dof/MSE", "IJRR/boxes_6dof/LPIPS", "IJRR/boxes_6dof/SSIM"]            # the reference's order
    assert len(seen) == 3 and all(n is True for _, _, n in seen)
    for t, (a, b, _) in enumerate(seen):
        assert torch.equal(a, pred[t][None] / 255) and torch.equal(b, image[t][None] / 255)
        assert got["IJRR/boxes_6dof/LPIPS"][t] == float((a - b).abs().mean())
    assert got["IJRR/boxes_6dof/MSE"] == raw[:, 0].tolist() and got["IJRR/boxes_6dof/SSIM"] == raw[:, 1].tolist()
    with pytest.raises(ValueError, match="Batch size must be 1"):
        metrics.compute_metrics(pred[None, :, None].expand(2, -1, -1, -1, -1), dict(batch, frame=batch["frame"].expand(2, -1, -1, -1, -1)))


def test_operators_enqueue_without_synchronising_and_repeat_bit_for_bit():
    from v2v_amd import metrics
    pred, image = (torch.from_numpy(v).cuda() for v in MR.image_case("i180x240"))
    fp, fg, fe = (torch.from_numpy(v).cuda() for v in MR.flow_case("f180x240"))
    first = (*metrics.image_metrics(pred, image, ssim_map=True), *metrics.flow_metrics(fp, fg, fe))         # warm: the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = (*metrics.image_metrics(pred, image, ssim_map=True), *metrics.flow_metrics(fp, fg, fe))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    empty = metrics.image_metrics(pred[:0], image[:0])
    assert empty.shape == (0, 2) and metrics.flow_metrics(fp[:0], fg[:0], fe[:0])[0].shape == (0, 6)


def test_bad_arguments_raise_value_errors_before_any_launch():
    from v2v_amd import metrics
    z = torch.zeros((2, 1, 9, 9), device="cuda")
    for bad in (z.double(), z[0, 0], z.expand(2, 2, 9, 9), z.cpu(), z[:, :, :6], z[None].expand(2, -1, -1, -1, -1)):
        with pytest.raises(ValueError):
            metrics.image_metrics(bad, bad)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.image_metrics(z, z[:, :, :8])
    f, e = torch.zeros((2, 2, 9, 9), device="cuda"), torch.zeros((2, 5, 9, 9), device="cuda")
    for args in ((f.double(), f, e), (f, f[:, :1], e), (f, f, e[:1]), (f, f, e[:, :, :8]), (f, f, e[:, :0]), (f[0], f[0], e[0])):
        with pytest.raises(ValueError):
            metrics.flow_metrics(*args)
