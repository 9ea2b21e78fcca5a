"""CPU-side checks of the evaluation metrics (v2v_amd/metrics.py, include/v2v_metrics.h) against golden G33 (tests/golden/g33_metrics.npz,
written by tests/golden/make_golden_metrics.py): the restatements the GPU tests lean on (tests/metrics_reference.py) reproduce it, the seeded
inputs hash to what it records, the C entry points validate their arguments (the header against the binding: tests/test_capi_contract.py),
and the wrappers raise without a GPU.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import metrics_reference as MR
from capi_calls import _D, _d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g33(golden):
    return golden("g33_metrics.npz")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from v2v_amd import _lib
    return _lib


def test_golden_holds_the_cases_of_the_issue(g33):
    assert set(MR.SMALL_IMAGE_CASES) == {"i7x7", "i8x9", "i23x70", "i45x31"} and {"i180x240", "i260x346"} <= set(MR.IMAGE_CASES)
    for name, (T, H, W, _) in MR.IMAGE_CASES.items():
        for r in (1, 2):
            assert g33[f"{name}__ssim64_r{r}"].shape == (T,) and g33[f"{name}__ssim32_r{r}"].shape == (T,)
            assert (f"{name}__S_r{r}" in g33) == (name in MR.SMALL_IMAGE_CASES)
        assert g33[f"{name}__mse32"].shape == (T,) and g33[f"{name}__mse64"].shape == (T,)
    for name, (T, C, H, W, _, _) in MR.FLOW_CASES.items():
        counts = g33[f"{name}__counts"]
        assert counts.shape == (T, 6) and g33[f"{name}__ee_sums"].shape == (T, 2) and g33[f"{name}__ratios"].dtype == np.float32
        assert (counts[1] == 0).all(), "frame 1 has no valid pixel"
        if T > 3:
            assert counts[2, 0] == counts[2, 1] > 0, "frame 2 has events everywhere"
            assert counts[3, 0] > 0 and counts[3, 1] == 0, "frame 3 has events nowhere"
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g33_metrics.npz")) < 256 * 1024


@pytest.mark.parametrize("name", sorted(MR.IMAGE_CASES))
def test_seeded_image_inputs_hash_to_the_golden(g33, name):
    assert MR.sha(*MR.image_case(name)) == str(g33[f"{name}__sha"])


@pytest.mark.parametrize("name", sorted(MR.FLOW_CASES))
def test_seeded_flow_inputs_hash_to_the_golden_and_hold_the_special_values(g33, name):
    pred, gt, events = MR.flow_case(name)
    assert MR.sha(pred, gt, events) == str(g33[f"{name}__sha"])
    assert np.isnan(gt[0]).any() and (np.signbit(gt[0]) & (gt[0] == 0)).any() and (~np.signbit(gt[0]) & (gt[0] == 0)).any()


@pytest.mark.parametrize("name", sorted(MR.SMALL_IMAGE_CASES))
@pytest.mark.parametrize("r", MR.DATA_RANGES)
def test_direct_sums_reproduce_the_running_sum_truth(g33, name, r):
    """skimage's algorithm on scipy's running-sum filter (G33) against direct 49-tap sums in the kernels' order: 1e-12"""
    pred, image = MR.image_case(name)
    x, y = MR.scaled(pred, 255.0), MR.scaled(image, 255.0)
    for t in range(pred.shape[0]):
        S = MR.ssim_direct64(x[t], y[t], r)
        want = g33[f"{name}__S_r{int(r)}"][t]
        assert S.shape == want.shape and np.abs(S - want).max() <= 1e-12
        assert abs(S.mean() - g33[f"{name}__ssim64_r{int(r)}"][t]) <= 1e-12
        mean, S2 = MR.ssim_skimage(x[t], y[t], r)
        assert np.array_equal(S2, want) and abs(mean - g33[f"{name}__ssim64_r{int(r)}"][t]) <= 1e-15


@pytest.mark.parametrize("name", ["i180x240", "i260x346"])
def test_full_size_scalars_reproduce(g33, name):
    pred, image = MR.image_case(name)
    x, y = MR.scaled(pred, 255.0), MR.scaled(image, 255.0)
    for t in range(pred.shape[0]):
        for r in MR.DATA_RANGES:
            assert abs(MR.ssim_direct64(x[t], y[t], r).mean() - g33[f"{name}__ssim64_r{int(r)}"][t]) <= 1e-12
            assert abs(MR.ssim_skimage(x[t], y[t], r, np.float32)[0] - g33[f"{name}__ssim32_r{int(r)}"][t]) <= 1e-12
        assert abs(MR.mse64(x[t], y[t]) - g33[f"{name}__mse64"][t]) <= 2.0 ** -22 * g33[f"{name}__mse64"][t]
        assert abs(g33[f"{name}__mse32"][t] - g33[f"{name}__mse64"][t]) <= x[t].size * 2.0 ** -24 * g33[f"{name}__mse64"][t]


@pytest.mark.parametrize("name", sorted(MR.FLOW_CASES))
def test_flow_restatement_equals_the_references_values(g33, name):
    """Counts, the float64 sums of the correctly rounded float32 EE, the N-PE quotients and everything in the integer-exact case: exactly
    G33's.  The reference's float32 EPE goes through torch's CPU sqrt and float32 sum, whose last bits depend on the CPU's vector width and
    the thread count (seen: 2.0921173 on one host, 2.0921175 on another), so off the integer-exact case it is held to the float32
    summation error H*W*2^-24 that the device's ratios are held to."""
    T, _, H, W, _, exact = MR.FLOW_CASES[name]
    pred, gt, events = (torch.from_numpy(v) for v in MR.flow_case(name))
    for t in range(T):
        counts, sums, _ = MR.flow_terms(pred[t], gt[t], events[t])
        assert np.array_equal(counts, g33[f"{name}__counts"][t])
        assert np.array_equal(sums, g33[f"{name}__ee_sums"][t])
        ratios, want = np.array(MR.flow_ratios(pred[t], gt[t], events[t]), dtype=np.float32), g33[f"{name}__ratios"][t]
        assert np.array_equal(ratios[[1, 2, 4, 5]], want[[1, 2, 4, 5]])
        for m in range(2):
            if exact or counts[m] == 0:
                assert ratios[3 * m] == want[3 * m]
            else:
                assert abs(float(ratios[3 * m]) - float(want[3 * m])) <= H * W * 2.0 ** -24 * float(want[3 * m])


@pytest.mark.parametrize("name", sorted(MR.FLOW_CASES))
def test_host_side_ratios_from_golden_counts(g33, name):
    """v2v_amd.metrics.flow_ratios on G33's counts and float64 sums: N-PE exactly the reference's, EPE exactly where the count is 0 or the
    case is integer-exact, within float32 summation error H*W*2^-24 otherwise"""
    from v2v_amd import metrics
    T, _, H, W, _, exact = MR.FLOW_CASES[name]
    got, want = metrics.flow_ratios(g33[f"{name}__counts"], g33[f"{name}__ee_sums"]), g33[f"{name}__ratios"]
    assert got.dtype == np.float32 and got.shape == (T, 6)
    assert np.array_equal(got[:, [1, 2, 4, 5]], want[:, [1, 2, 4, 5]])
    for m in range(2):
        zero = g33[f"{name}__counts"][:, m] == 0
        assert np.array_equal(got[zero, 3 * m], want[zero, 3 * m]) and not got[zero, 3 * m].any()
        if exact:
            assert np.array_equal(got[:, 3 * m], want[:, 3 * m])
        else:
            assert (np.abs(got[:, 3 * m].astype(np.float64) - want[:, 3 * m]) <= H * W * 2.0 ** -24 * np.abs(want[:, 3 * m])).all()


# ---- the C entry points (include/v2v_metrics.h) ------------------------------------------------------------------------------------------
def _img(**kw):
    return [kw.get("pred", _d()), kw.get("ps", 49), kw.get("image", _d(1)), kw.get("is_", 49), kw.get("T", 1), kw.get("H", 7), kw.get("W", 7),
            kw.get("divisor", 255.0), kw.get("data_range", 2.0), kw.get("ws", _d(2)), kw.get("out", _d(3)), kw.get("map", None), None]


def _flow(**kw):
    return [kw.get("pred", _d()), kw.get("ps", 8), kw.get("gt", _d(1)), kw.get("gs", 8), kw.get("events", _d(2)), kw.get("es", 20), kw.get("T", 1),
            kw.get("C", 5), kw.get("H", 2), kw.get("W", 2), kw.get("ws", _d(3)), kw.get("counts", _d(4)), kw.get("sums", _d(5)), None]


def test_image_argument_validation_answers_without_a_gpu(L):
    lib = L.lib()
    f = lib.v2v_image_metrics_hip
    for k in ("pred", "image", "ws", "out"):
        assert f(*_img(**{k: None})) == L.ERR_NULL
    assert lib.v2v_last_error().decode() == "v2v_image_metrics_hip: pred/image/workspace/out is NULL"
    assert f(*_img(H=6)) == L.ERR_SHAPE
    assert lib.v2v_last_error().decode() == "v2v_image_metrics_hip: the 7x7 window needs H >= 7 and W >= 7 (got 6 x 7)"
    assert f(*_img(W=6)) == L.ERR_SHAPE and f(*_img(H=0, W=0)) == L.ERR_SHAPE
    assert f(*_img(T=-1)) == L.ERR_SHAPE and b"T must be >= 0" in lib.v2v_last_error()
    assert f(*_img(ps=-1)) == L.ERR_SHAPE and b"strides" in lib.v2v_last_error()
    assert f(*_img(divisor=0.0)) == L.ERR_PARAM and f(*_img(data_range=0.0)) == L.ERR_PARAM and f(*_img(data_range=float("nan"))) == L.ERR_PARAM
    assert f(*_img(pred=C.c_void_p(_D + 2))) == L.ERR_ALIGN and f(*_img(out=C.c_void_p(_D + 4))) == L.ERR_ALIGN
    assert f(*_img(map=C.c_void_p(_D + 4))) == L.ERR_ALIGN
    assert f(*_img(T=0)) == L.OK and f(*_img(T=0, pred=None, image=None, ws=None, out=None)) == L.OK
    assert f(*_img(T=0, H=6)) == L.ERR_SHAPE
    assert f(*_img(T=1 << 20, H=1 << 14, W=1 << 14)) == L.ERR_SHAPE and b"below 2^31" in lib.v2v_last_error()
    w = lib.v2v_image_metrics_workspace_bytes
    assert w(3, 7, 7) == 3 * 16 and w(1, 7 + 8, 7 + 32) == 4 * 16 and w(2, 260, 346) == 2 * 32 * 11 * 16 and w(0, 7, 7) == 0
    assert w(1, 6, 7) == L.ERR_SHAPE and w(-1, 7, 7) == L.ERR_SHAPE


def test_flow_argument_validation_answers_without_a_gpu(L):
    lib = L.lib()
    f = lib.v2v_flow_metrics_hip
    for k in ("pred", "gt", "events", "ws", "counts", "sums"):
        assert f(*_flow(**{k: None})) == L.ERR_NULL
    assert lib.v2v_last_error().decode() == "v2v_flow_metrics_hip: pred/gt/events/workspace/counts/ee_sums is NULL"
    assert f(*_flow(H=1 << 12, W=1 << 12)) == L.ERR_SHAPE
    assert lib.v2v_last_error().decode() == ("v2v_flow_metrics_hip: need H, W >= 1 and H * W < 2^24, the reference's float32 counts (got 4096 x 4096)")
    assert f(*_flow(H=1 << 40, W=1 << 40)) == L.ERR_SHAPE and f(*_flow(H=0)) == L.ERR_SHAPE
    assert f(*_flow(C=0)) == L.ERR_SHAPE and b"event channels (got 0)" in lib.v2v_last_error()
    assert f(*_flow(T=-1)) == L.ERR_SHAPE and f(*_flow(es=-1)) == L.ERR_SHAPE
    assert f(*_flow(gt=C.c_void_p(_D + 2))) == L.ERR_ALIGN and f(*_flow(counts=C.c_void_p(_D + 4))) == L.ERR_ALIGN
    assert f(*_flow(T=0)) == L.OK and f(*_flow(T=0, C=0)) == L.ERR_SHAPE
    w = lib.v2v_flow_metrics_workspace_bytes
    assert w(2, 260, 346) == 2 * 44 * 64 and w(1, 1, 1) == 64 and w(0, 4, 4) == 0
    assert w(1, 4096, 4096) == L.ERR_SHAPE and w(-1, 4, 4) == L.ERR_SHAPE


def test_wrappers_raise_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from v2v_amd import metrics
    z = torch.zeros((2, 1, 8, 9))
    batch = {"frame": z[None], "flow": torch.zeros((1, 1, 2, 8, 9)), "events": torch.zeros((1, 1, 5, 8, 9)), "sequence_name": [["s"]],
             "data_source_idx": torch.tensor([0])}
    for call in (lambda: metrics.image_metrics(z, z), lambda: metrics.flow_metrics(batch["flow"], batch["flow"], batch["events"]),
                 lambda: metrics.compute_metrics(z[None], batch), lambda: metrics.compute_flow_metrics(batch["flow"], batch)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
