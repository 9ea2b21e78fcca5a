"""CPU-side checks of LPIPS-AlexNet as a training loss (v2v_amd/lpips_alex.py, include/v2v_alex_train.h) against golden G35
(tests/golden/g35_lpips_alex_grad.npz, written by tests/golden/make_golden_lpips_alex_grad.py from the reference's PNetLin with autograd):
the file's layout and the conditions its generator asserted, the stock restatement's float64 autograd (tests/lpips_alex_stock.py, the CPU
cross-check the GPU tests lean on), every entry point's argument validation (the header against the binding table and the library's
symbols: tests/test_capi_contract.py), the dgrad pack, the loss class's error without torchvision.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lpips_alex_grad_cases as GC
import lpips_alex_stock as STOCK
import lpips_alex_weights as LW
from capi_calls import _D, _d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g34(golden):
    return golden("g34_lpips_alex.npz")


@pytest.fixture(scope="module")
def g35(golden):
    return golden("g35_lpips_alex_grad.npz")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from v2v_amd import _lib
    return _lib


def test_golden_holds_the_cases_of_the_issue(g35):
    assert GC.CASES == {"a": (2, 1, 31, 31), "b": (3, 1, 47, 63), "c": (1, 3, 40, 55), "wide": (2, 1, 47, 143), "t128": (1, 1, 128, 128), "close": (1, 1, 31, 47)}
    assert GC.J == {"a": 0, "b": 1, "c": 0, "wide": 20, "t128": 0, "close": 1} and GC.MARGIN == 8
    # what the shapes are there for
    assert LW.tap_sizes(31, 31) == ((7, 7), (3, 3), (1, 1), (1, 1), (1, 1))
    assert LW.tap_sizes(47, 63)[:2] == ((11, 15), (5, 7)) and LW.tap_sizes(47, 143)[:2] == ((11, 35), (5, 17)) and 2 * 5 * 17 == 170
    for name, shape in GC.CASES.items():
        T = shape[0]
        g = g35[f"{name}__grad64"]
        assert g.shape == shape and g.dtype == np.float64 and np.isfinite(g).all()
        assert all(np.abs(g[t]).max() > 0 for t in range(T))
        assert g35[f"{name}__dist64"].shape == (T,) and g35[f"{name}__dist64"].dtype == np.float64 and (g35[f"{name}__dist64"] > 0).all()
        act = g35[f"{name}__active"]
        assert act.shape == (5,) and act.dtype == np.int64
        sizes = [T * c * h * w for c, (h, w) in zip(LW.CHANNELS, LW.tap_sizes(*shape[2:]))]
        assert all(0.2 * s < a < 0.8 * s for a, s in zip(act, sizes)), "about half of the units of a tap are active"
        assert (f"{name}__pred" in g35) == (f"{name}__target" in g35) == (name in GC.STORED)
        if name in GC.STORED:
            pred, target = GC.case_inputs(name)
            assert pred.dtype == np.float32 and np.array_equal(pred, g35[f"{name}__pred"]) and np.array_equal(target, g35[f"{name}__target"])
            assert pred.min() >= 0 and pred.max() <= 1
    assert set(GC.CASES) - set(GC.STORED) == {"t128"}
    # the float32 CPU run's own error: a few float32 roundings
    assert 1e-7 < float(g35["e32_grad"]) < 1e-5
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g35_lpips_alex_grad.npz")) < 640 * 1024
    assert sorted(k for k in g35 if "__" not in k) == ["e32_grad"]


def test_the_draws_differ_and_the_close_case_is_close():
    a0, a1 = GC.case_inputs("b", 0)[0], GC.case_inputs("b", 1)[0]
    assert not np.array_equal(a0, a1)
    pred, target = GC.case_inputs("close")
    assert 0 < np.abs(pred - target).max() < 0.3
    assert np.array_equal(GC.coefficients(3), [0.5, 1.25, 2.0])


def _stock_grad(state, pred, target, dtype):
    """(grad, dist [T], active [5]) of the stock restatement with autograd on  sum_b c_b dist_b"""
    s = {k: v.to(dtype) for k, v in state.items()}
    p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    t = torch.from_numpy(target).to(dtype)
    dist = STOCK.lpips_alex(s, p, t, normalize=True).reshape(-1)
    (torch.from_numpy(GC.coefficients(pred.shape[0])).to(dtype) * dist).sum().backward()
    with torch.no_grad():
        taps = STOCK.features(s, ((2 * p - 1) - s["scaling_layer.shift"]) / s["scaling_layer.scale"])
    return p.grad.numpy(), dist.detach().numpy(), np.array([int((f > 0).sum()) for f in taps], dtype=np.int64)


@pytest.mark.parametrize("name", list(GC.CASES))
def test_stock_restatement_reproduces_the_golden_gradient(g34, g35, name):
    """float64: the same operators in the same order as the reference's, 1e-10 of the largest gradient is generous.  float32: the stock
    run is the kind of run e32_grad was measured on; four times that error leaves room for another CPU's vector width and threads."""
    torch.set_num_threads(4)
    state = LW.golden_state(g34)
    pred, target = GC.case_inputs(name)
    g64 = g35[f"{name}__grad64"]
    scale = np.abs(g64).reshape(g64.shape[0], -1).max(1).reshape(-1, 1, 1, 1)
    grad, dist, active = _stock_grad(state, pred, target, torch.float64)
    assert grad.shape == g64.shape and (np.abs(grad - g64) <= 1e-10 * scale).all()
    assert (np.abs(dist - g35[f"{name}__dist64"]) <= 1e-10 * dist).all()
    assert np.array_equal(active, g35[f"{name}__active"])
    grad32, _, active32 = _stock_grad(state, pred, target, torch.float32)
    assert grad32.dtype == np.float32 and (np.abs(grad32 - g64) <= 4 * float(g35["e32_grad"]) * scale).all()
    assert np.array_equal(active32, active), "conditions (ii) and (iii): no float32 rounding flips a gate"


def test_pack_dgrad_weights_layout():
    from v2v_amd import lpips_alex
    w = torch.arange(192 * 64 * 25, dtype=torch.float32).reshape(192, 64, 5, 5)
    p = lpips_alex.pack_dgrad_weights(w)
    assert p.shape == (25 * 192, 64) and p.is_contiguous() and p.dtype == torch.float32
    for ky, kx, co, ci in ((0, 0, 0, 0), (3, 1, 100, 17), (4, 4, 191, 63), (2, 2, 5, 9), (1, 4, 77, 31)):
        assert p[(ky * 5 + kx) * 192 + co, ci] == w[co, ci, 4 - ky, 4 - kx]
    w = torch.arange(384 * 192 * 9, dtype=torch.float32).reshape(384, 192, 3, 3)
    p = lpips_alex.pack_dgrad_weights(w)
    assert p.shape == (9 * 384, 192) and p[(2 * 3 + 0) * 384 + 300, 150] == w[300, 150, 0, 2]


def test_perceptual_loss_alex_names_what_is_missing(monkeypatch, g34):
    import sys
    from v2v_amd import losses
    monkeypatch.setitem(sys.modules, "torchvision", None)           # `import torchvision` raises ImportError, installed or not
    with pytest.raises(RuntimeError, match="torchvision"):
        losses.perceptual_loss_alex()
    with pytest.raises(ValueError, match="alex"):
        losses.perceptual_loss_alex(net="vgg", state_dict=LW.golden_state(g34), use_gpu=False)
    loss = losses.perceptual_loss_alex(weight=0.25, state_dict=LW.golden_state(g34), use_gpu=False)
    assert loss.weight == 0.25 and list(loss.model.state_dict()) == LW.reference_keys()
    with pytest.raises(ValueError):
        losses.perceptual_loss(net="alex", state_dict={})             # the vgg class stays vgg-only


def test_wrappers_raise_without_a_gpu(g34):
    if torch.cuda.is_available():
        return
    from v2v_amd import lpips_alex
    m = lpips_alex.LPIPSAlex()
    z = torch.zeros((2, 1, 31, 31))
    calls = (lambda: m(z.clone().requires_grad_(True), z), lambda: lpips_alex.compare_bwd(torch.zeros((1, 1, 1, 64)), torch.zeros((1, 1, 1, 64)), torch.zeros(64), torch.zeros(1)),
             lambda: lpips_alex.conv_dgrad(torch.zeros((1, 1, 1, 256)), torch.zeros((9 * 256, 256)), 3), lambda: lpips_alex.pool_bwd(torch.zeros((1, 3, 3, 64)), torch.zeros((1, 1, 1, 64))),
             lambda: lpips_alex.stem_bwd(torch.zeros((1, 7, 7, 64)), torch.zeros((3, 122, 64)), torch.ones(3), 1, 31, 31))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the C entry points (include/v2v_alex_train.h) ------------------------------------------------------------------------------------------
_ODD = C.c_void_p(_D + 4)        # 4-byte but not 16-byte aligned
_OFF = C.c_void_p(_D + 2)        # not even 4-byte aligned


def test_compare_bwd_argument_validation(L):
    lib = L.lib()
    f = lib.v2v_alex_train_compare_bwd_hip
    ok = lambda **kw: [kw.get("f0", _d()), kw.get("f1", _d(1)), kw.get("w", _d(2)), kw.get("ddist", _d(3)), kw.get("n", 1), kw.get("HW", 6), kw.get("C", 192), 1,   # noqa: E731
                       kw.get("dz", _d(4)), None]
    for k in ("f0", "f1", "w", "ddist", "dz"):
        assert f(*ok(**{k: None})) == L.ERR_NULL
        assert f(*ok(**{k: _OFF})) == L.ERR_ALIGN
    assert f(*ok(C=128)) == L.ERR_SHAPE and b"64, 192, 256 or 384" in lib.v2v_last_error()
    assert f(*ok(HW=0)) == L.ERR_SHAPE and f(*ok(n=-1)) == L.ERR_SHAPE and f(*ok(n=65536)) == L.ERR_SHAPE
    assert f(*ok(n=60000, HW=1 << 10)) == L.ERR_SHAPE and b"below 2^31" in lib.v2v_last_error()
    assert f(*ok(n=0)) == L.OK and f(*ok(n=0, f0=None, dz=None)) == L.OK and f(*ok(n=0, C=100)) == L.ERR_SHAPE


def test_conv_dgrad_argument_validation(L):
    lib = L.lib()
    f = lib.v2v_alex_train_conv_dgrad_hip
    ok = lambda **kw: [kw.get("dy", _d()), kw.get("weight", _d(1)), kw.get("dtap", _d(2)), kw.get("mask", _d(3)), kw.get("n", 1), kw.get("H", 3), kw.get("W", 3),   # noqa: E731
                       kw.get("Cin", 64), kw.get("Cout", 192), kw.get("ks", 5), kw.get("dx", _d(4)), None]
    for k in ("dy", "weight", "dx"):
        assert f(*ok(**{k: None})) == L.ERR_NULL
    for k in ("dy", "weight", "dtap", "mask", "dx"):
        assert f(*ok(**{k: _ODD})) == L.ERR_ALIGN, k
    assert f(*ok(ks=7)) == L.ERR_SHAPE and f(*ok(ks=4)) == L.ERR_SHAPE and b"ks must be 3 or 5" in lib.v2v_last_error()
    assert f(*ok(Cin=96)) == L.ERR_SHAPE and f(*ok(Cout=48)) == L.ERR_SHAPE and f(*ok(H=0)) == L.ERR_SHAPE and f(*ok(n=-1)) == L.ERR_SHAPE
    assert f(*ok(n=1 << 16, H=1 << 10, W=1 << 10)) == L.ERR_SHAPE
    assert f(*ok(n=0)) == L.OK and f(*ok(n=0, dy=None, dx=None, dtap=None, mask=None)) == L.OK and f(*ok(n=0, ks=4)) == L.ERR_SHAPE


def test_pool_bwd_argument_validation(L):
    lib = L.lib()
    f = lib.v2v_alex_train_pool_bwd_hip
    ok = lambda **kw: [kw.get("x", _d()), kw.get("dy", _d(1)), kw.get("dtap", _d(2)), kw.get("n", 1), kw.get("H", 3), kw.get("W", 3), kw.get("C", 64), 1,   # noqa: E731
                       kw.get("dx", _d(3)), None]
    for k in ("x", "dy", "dx"):
        assert f(*ok(**{k: None})) == L.ERR_NULL
    for k in ("x", "dy", "dtap", "dx"):
        assert f(*ok(**{k: _ODD})) == L.ERR_ALIGN, k
    assert f(*ok(H=2)) == L.ERR_SHAPE and f(*ok(W=2)) == L.ERR_SHAPE and f(*ok(C=6)) == L.ERR_SHAPE and f(*ok(n=-1)) == L.ERR_SHAPE
    assert f(*ok(n=1 << 16, H=1 << 10, W=1 << 10)) == L.ERR_SHAPE and b"below 2^31" in lib.v2v_last_error()
    assert f(*ok(n=0)) == L.OK and f(*ok(n=0, x=None, dy=None, dx=None)) == L.OK and f(*ok(n=0, H=2)) == L.ERR_SHAPE


def test_stem_bwd_argument_validation(L):
    lib = L.lib()
    f = lib.v2v_alex_train_stem_bwd_hip
    ok = lambda **kw: [kw.get("dz", _d()), kw.get("weight", _d(1)), kw.get("scale", _d(2)), kw.get("n", 1), kw.get("cin", 1), kw.get("H", 31), kw.get("W", 31),   # noqa: E731
                       kw.get("divisor", 255.0), 1, kw.get("dpred", _d(3)), None]
    for k in ("dz", "weight", "scale", "dpred"):
        assert f(*ok(**{k: None})) == L.ERR_NULL
    assert f(*ok(dz=_ODD)) == L.ERR_ALIGN and f(*ok(weight=_ODD)) == L.ERR_ALIGN and f(*ok(scale=_OFF)) == L.ERR_ALIGN and f(*ok(dpred=_OFF)) == L.ERR_ALIGN
    assert f(*ok(H=30)) == L.ERR_SHAPE and b"H and W >= 31" in lib.v2v_last_error()
    assert f(*ok(W=30)) == L.ERR_SHAPE and f(*ok(cin=2)) == L.ERR_SHAPE and f(*ok(n=-1)) == L.ERR_SHAPE and f(*ok(n=65536, H=31, W=31)) == L.ERR_SHAPE
    assert f(*ok(n=1 << 20, H=1 << 12, W=1 << 12)) == L.ERR_SHAPE and b"below 2^31" in lib.v2v_last_error()
    assert f(*ok(divisor=0.0)) == L.ERR_PARAM and f(*ok(divisor=float("inf"))) == L.ERR_PARAM and f(*ok(divisor=float("nan"))) == L.ERR_PARAM
    assert f(*ok(n=0)) == L.OK and f(*ok(n=0, dz=None, dpred=None)) == L.OK and f(*ok(n=0, H=30)) == L.ERR_SHAPE
