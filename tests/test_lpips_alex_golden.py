"""CPU-side checks of the LPIPS-AlexNet metric (v2v_amd/lpips_alex.py, include/v2v_lpips_alex.h) against golden G34
(tests/golden/g34_lpips_alex.npz, written by tests/golden/make_golden_lpips_alex.py from the reference's PNetLin): the stock restatement the
timing tool and the GPU tests lean on (tests/lpips_alex_stock.py) reproduces it, the module carries the reference's 17 keys, the C entry
points validate their arguments (the header against the binding and the library: tests/test_capi_contract.py), the wrappers raise without
a GPU.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lpips_alex_stock as STOCK
import lpips_alex_weights as LW
from capi_calls import _D, _d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g34(golden):
    return golden("g34_lpips_alex.npz")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from v2v_amd import _lib
    return _lib


def test_golden_holds_the_cases_of_the_issue(g34):
    assert LW.CASES == {"a": (2, 1, 31, 31), "b": (3, 1, 47, 63), "c": (1, 3, 64, 95), "close": (2, 1, 47, 63), "r180": (1, 1, 180, 240),
                        "r260": (1, 1, 260, 346)}
    for name, (T, _, _, _) in LW.CASES.items():
        assert g34[f"{name}__taps64"].shape == (T, 5) and g34[f"{name}__taps64"].dtype == np.float64 and g34[f"{name}__dist64"].shape == (T,)
        assert g34[f"{name}__taps32"].shape == (T, 5) and g34[f"{name}__taps32"].dtype == np.float32 and g34[f"{name}__dist32"].dtype == np.float32
        assert (g34[f"{name}__taps64"] > 0).all()
        assert (f"{name}__pred" in g34) == (name in LW.STORED)
        lo, hi = (0.0035, 0.0045) if name in LW.CLOSE else (0.09, 0.1)
        assert (g34[f"{name}__dist64"] > lo).all() and (g34[f"{name}__dist64"] < hi).all()
    assert sum(g34[k].size for k in LW.LIN_KEYS) == 1152 and all((g34[k] >= 0).all() for k in LW.LIN_KEYS)
    assert [g34[k].shape for k in LW.LIN_KEYS] == [(1, c, 1, 1) for c in LW.CHANNELS]
    # the float32 CPU run's error: a few float32 roundings, nowhere near a bf16 one
    assert 1e-7 < float(g34["e32_tap"]) < 4e-6 and 1e-8 < float(g34["e32_dist"]) < 4e-6
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g34_lpips_alex.npz")) < 512 * 1024


@pytest.mark.parametrize("name", LW.STORED)
def test_seeded_inputs_are_the_stored_ones(g34, name):
    pred, target = LW.case_inputs(name)
    assert np.array_equal(pred, g34[f"{name}__pred"]) and np.array_equal(target, g34[f"{name}__target"])
    assert pred.min() >= 0 and pred.max() <= 1


@pytest.mark.parametrize("name", ["a", "b", "c", "close", "r180"])
def test_stock_restatement_reproduces_the_golden(g34, name):
    """float64: the same operators in the same order, 1e-10 is generous.  float32: both runs are float32 CPU runs of the same operators,
    each within the recorded float32 error of the truth on the machine that made it; four times that error between them leaves room for
    another CPU's vector width and thread count."""
    torch.set_num_threads(4)
    state = LW.golden_state(g34)
    pred, target = (torch.from_numpy(v) for v in LW.case_inputs(name))
    s64 = {k: v.double() for k, v in state.items()}
    for t in range(pred.shape[0]):
        val, res = STOCK.lpips_alex(s64, pred[t].double(), target[t].double(), normalize=True, per_layer=True)
        assert val.shape == (1, 1, 1, 1)
        want_t, want_d = g34[f"{name}__taps64"][t], g34[f"{name}__dist64"][t]
        assert (np.abs(res[0].numpy() - want_t) <= 1e-10 * want_t).all() and abs(float(val) - want_d) <= 1e-10 * want_d
        val, res = STOCK.lpips_alex(state, pred[t], target[t], normalize=True, per_layer=True)
        assert val.dtype == torch.float32
        assert (np.abs(res[0].numpy().astype(np.float64) - g34[f"{name}__taps32"][t]) <= 4 * float(g34["e32_tap"]) * want_t).all()
        assert abs(float(val) - float(g34[f"{name}__dist32"][t])) <= 4 * float(g34["e32_dist"]) * want_d


def test_module_has_the_references_17_keys_and_loads_strict(g34):
    from v2v_amd.lpips_alex import LPIPSAlex
    m = LPIPSAlex()
    assert list(m.state_dict()) == LW.reference_keys() and len(LW.reference_keys()) == 17
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes["net.slice1.0.weight"] == (64, 3, 11, 11) and shapes["net.slice2.3.weight"] == (192, 64, 5, 5)
    assert shapes["net.slice3.6.weight"] == (384, 192, 3, 3) and shapes["net.slice5.10.bias"] == (256,) and shapes["lin1.model.1.weight"] == (1, 192, 1, 1)
    state = LW.golden_state(g34)
    res = m.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.lin3.model[1].weight, state["lin3.model.1.weight"]) and torch.equal(m.scaling_layer.shift, state["scaling_layer.shift"])
    assert not m.training and not m.train().training and not any(p.requires_grad for p in m.parameters())
    with pytest.raises(ValueError):
        LPIPSAlex(net="vgg")
    with pytest.raises(ValueError):
        LPIPSAlex(spatial=True)


def test_tap_sizes():
    from v2v_amd import lpips_alex
    assert lpips_alex.tap_sizes(260, 346) == ((64, 85), (31, 42), (15, 20), (15, 20), (15, 20))
    assert lpips_alex.tap_sizes(180, 240) == ((44, 59), (21, 29), (10, 14), (10, 14), (10, 14))
    assert lpips_alex.tap_sizes(31, 31) == ((7, 7), (3, 3), (1, 1), (1, 1), (1, 1))
    for h, w in ((31, 31), (47, 63), (64, 95), (180, 240)):
        assert lpips_alex.tap_sizes(h, w) == LW.tap_sizes(h, w)
        sizes = [tuple(f.shape[2:]) for f in STOCK.features({k: torch.zeros(s) for k, s in LW.backbone_shapes().items()}, torch.zeros((1, 3, h, w)))]
        assert tuple(sizes) == lpips_alex.tap_sizes(h, w)
    for h, w in ((30, 31), (31, 30), (0, 0)):
        with pytest.raises(ValueError):
            lpips_alex.tap_sizes(h, w)


def test_packing_layouts():
    from v2v_amd import lpips_alex
    w = torch.arange(64 * 3 * 121, dtype=torch.float32).reshape(64, 3, 11, 11)
    p = lpips_alex.pack_stem_weights(w)
    assert p.shape == (3, 122, 64) and not p[:, 121].any() and p[2, 5 * 11 + 7, 9] == w[9, 2, 5, 7]
    w = torch.arange(192 * 64 * 25, dtype=torch.float32).reshape(192, 64, 5, 5)
    p = lpips_alex.pack_conv_weights(w)
    assert p.shape == (25 * 64, 192) and p.is_contiguous() and p[(3 * 5 + 1) * 64 + 17, 100] == w[100, 17, 3, 1]


# ---- the C entry points (include/v2v_lpips_alex.h) ---------------------------------------------------------------------------------------
def _stem(**kw):
    return [kw.get("frames", _d()), kw.get("fs", 961), kw.get("n", 1), kw.get("cin", 1), kw.get("H", 31), kw.get("W", 31), kw.get("divisor", 255.0),
            1, kw.get("shift", _d(1)), _d(2), kw.get("weight", _d(3)), _d(4), kw.get("out", _d(5)), None]


def _conv(**kw):
    return [kw.get("x", _d()), kw.get("weight", _d(1)), kw.get("bias", _d(2)), kw.get("n", 1), kw.get("H", 3), kw.get("W", 3), kw.get("Cin", 64),
            kw.get("Cout", 192), kw.get("ks", 5), 1, kw.get("y", _d(3)), None]


def test_stem_and_conv_argument_validation(L):
    lib = L.lib()
    f = lib.v2v_lpips_alex_stem_hip
    for k in ("frames", "shift", "weight", "out"):
        assert f(*_stem(**{k: None})) == L.ERR_NULL
    assert f(*_stem(H=30)) == L.ERR_SHAPE and b"H and W >= 31" in lib.v2v_last_error()
    assert f(*_stem(W=30)) == L.ERR_SHAPE and f(*_stem(cin=2)) == L.ERR_SHAPE and f(*_stem(n=-1)) == L.ERR_SHAPE and f(*_stem(fs=-1)) == L.ERR_SHAPE
    assert f(*_stem(n=1 << 20, H=1 << 12, W=1 << 12)) == L.ERR_SHAPE and b"below 2^31" in lib.v2v_last_error()
    assert f(*_stem(divisor=0.0)) == L.ERR_PARAM and f(*_stem(divisor=float("inf"))) == L.ERR_PARAM
    assert f(*_stem(out=C.c_void_p(_D + 4))) == L.ERR_ALIGN and f(*_stem(frames=C.c_void_p(_D + 2))) == L.ERR_ALIGN
    assert f(*_stem(n=0)) == L.OK and f(*_stem(n=0, frames=None, out=None)) == L.OK and f(*_stem(n=0, H=30)) == L.ERR_SHAPE
    f = lib.v2v_lpips_alex_conv_hip
    for k in ("x", "weight", "bias", "y"):
        assert f(*_conv(**{k: None})) == L.ERR_NULL
    assert f(*_conv(ks=7)) == L.ERR_SHAPE and f(*_conv(ks=4)) == L.ERR_SHAPE and b"ks must be 3 or 5" in lib.v2v_last_error()
    assert f(*_conv(Cin=48)) == L.ERR_SHAPE and f(*_conv(Cout=96)) == L.ERR_SHAPE and f(*_conv(H=0)) == L.ERR_SHAPE and f(*_conv(n=-1)) == L.ERR_SHAPE
    assert f(*_conv(n=1 << 16, H=1 << 10, W=1 << 10)) == L.ERR_SHAPE
    assert f(*_conv(x=C.c_void_p(_D + 4))) == L.ERR_ALIGN
    assert f(*_conv(n=0)) == L.OK and f(*_conv(n=0, x=None, y=None)) == L.OK


def test_pool_compare_and_sum_argument_validation(L):
    lib = L.lib()
    f = lib.v2v_lpips_alex_pool_hip
    assert f(None, 1, 3, 3, 64, _d(1), None) == L.ERR_NULL and f(_d(), 1, 3, 3, 64, None, None) == L.ERR_NULL
    assert f(_d(), 1, 2, 3, 64, _d(1), None) == L.ERR_SHAPE and f(_d(), 1, 3, 3, 6, _d(1), None) == L.ERR_SHAPE and f(_d(), -1, 3, 3, 64, _d(1), None) == L.ERR_SHAPE
    assert f(C.c_void_p(_D + 4), 1, 3, 3, 64, _d(1), None) == L.ERR_ALIGN and f(_d(), 0, 3, 3, 64, _d(1), None) == L.OK
    w = lib.v2v_lpips_alex_compare_workspace_bytes
    assert w(1, 1) == 8 and w(3, 64) == 24 and w(3, 65) == 48 and w(80, 64 * 85) == 80 * 85 * 8 and w(0, 5) == 0
    assert w(1, 0) == L.ERR_SHAPE and w(-1, 4) == L.ERR_SHAPE and w(70000, 4) == L.ERR_SHAPE
    assert w(0, 0) == L.ERR_SHAPE and b"v2v_lpips_alex_compare_workspace_bytes" in lib.v2v_last_error()
    f = lib.v2v_lpips_alex_compare_hip
    ok = lambda **kw: [kw.get("f0", _d()), kw.get("f1", _d(1)), kw.get("w", _d(2)), kw.get("n", 1), kw.get("HW", 6), kw.get("C", 192), kw.get("tap", 1),   # noqa: E731
                       kw.get("ws", _d(3)), kw.get("taps", _d(4)), None]
    for k in ("f0", "f1", "w", "ws", "taps"):
        assert f(*ok(**{k: None})) == L.ERR_NULL
    assert f(*ok(C=128)) == L.ERR_SHAPE and b"64, 192, 256 or 384" in lib.v2v_last_error()
    assert f(*ok(tap=5)) == L.ERR_SHAPE and f(*ok(tap=-1)) == L.ERR_SHAPE and f(*ok(HW=0)) == L.ERR_SHAPE and f(*ok(n=-1)) == L.ERR_SHAPE
    assert f(*ok(taps=C.c_void_p(_D + 4))) == L.ERR_ALIGN and f(*ok(n=0)) == L.OK
    f = lib.v2v_lpips_alex_sum_hip
    assert f(None, 1, _d(), None) == L.ERR_NULL and f(_d(), 1, None, None) == L.ERR_NULL and f(_d(), -1, _d(1), None) == L.ERR_SHAPE
    assert f(C.c_void_p(_D + 4), 1, _d(1), None) == L.ERR_ALIGN and f(None, 0, None, None) == L.OK


def test_wrappers_raise_without_a_gpu(g34):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from v2v_amd import lpips_alex, metrics
    m = lpips_alex.LPIPSAlex()
    z = torch.zeros((2, 1, 31, 31))
    batch = {"frame": z[None], "sequence_name": [["s"]], "data_source_idx": torch.tensor([0])}
    for call in (lambda: m(z, z), lambda: m.sequence(z, z), lambda: metrics.compute_metrics(z[None], batch, lpips_fn=m),
                 lambda: lpips_alex.pool(torch.zeros((1, 3, 3, 64))), lambda: lpips_alex.tap_sum(torch.zeros((1, 5), dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
