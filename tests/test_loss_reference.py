"""CPU-side checks of the image losses: the float64 formulas of tests/loss_reference.py against the reference's formula under
torch.autograd and against golden G29 (both to 1e-12), the C ABI's exports and argument validation without a GPU, the carry-over logic
of the loss classes, and that the wrappers raise without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_inputs as LI
import loss_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NEW = ("v2v_tc_loss_workspace_bytes", "v2v_tc_loss_fwd_hip", "v2v_tc_loss_bwd_hip", "v2v_warp_bilinear_hip", "v2v_warp_bilinear_adjoint_hip")


def stock_warp(img, flow):
    """utils/loss.py:22-42 restated on stock operators."""
    h, w = img.shape[2:]
    xx, yy = torch.meshgrid(torch.arange(w, dtype=img.dtype), torch.arange(h, dtype=img.dtype), indexing="xy")
    gx = 2 * (xx + flow[:, 0]) / (w - 1) - 1
    gy = 2 * (yy + flow[:, 1]) / (h - 1) - 1
    return F.grid_sample(img, torch.stack([gx, gy], dim=3), align_corners=True)


def stock_tc(image0, image1, processed0, processed1, flow, alpha=50.0):
    vis = torch.exp(-alpha * (image1 - stock_warp(image0, flow)) ** 2)
    w = stock_warp(torch.clamp(processed0, 0, 255), flow)
    return (vis * torch.abs(processed1 - w) / (torch.abs(processed1) + torch.abs(w) + 1e-5)).mean(dim=(1, 2, 3))


def close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol, float((a - b).abs().max())


@pytest.fixture(scope="module")
def g29(golden):
    return golden("g29_tc_loss.npz")


@pytest.mark.parametrize("name", sorted(LI.PAIR_SHAPES))
def test_reference_formulas_equal_autograd_in_float64(name):
    t = {k: torch.from_numpy(v).to(F64) for k, v in LI.pair_inputs(name).items()}
    close(R.ref_warp(t["image0"], t["flow01"]), stock_warp(t["image0"], t["flow01"]))
    dout = torch.from_numpy(np.random.default_rng(3).normal(size=t["image0"].shape))
    img = t["image0"].clone().requires_grad_(True)
    close(R.ref_warp_adjoint(dout, t["flow01"]), torch.autograd.grad((stock_warp(img, t["flow01"]) * dout).sum(), img)[0])
    p0, p1 = t["processed0"].clone().requires_grad_(True), t["processed1"].clone().requires_grad_(True)
    loss = stock_tc(t["image0"], t["image1"], p0, p1, t["flow01"])
    gout = torch.from_numpy(np.random.default_rng(4).uniform(0.5, 2.0, loss.shape[0]))
    want0, want1 = torch.autograd.grad((loss * gout).sum(), (p0, p1))
    close(R.ref_tc_maps(*(t[k] for k in LI.KEYS))["loss"], loss.detach())
    got0, got1 = R.ref_tc_grads(*(t[k] for k in LI.KEYS), gout)
    close(got0, want0)
    close(got1, want1)
    assert float(got0.abs().max()) > 0 and float(got1.abs().max()) > 0
    p = t["processed1"].clone().requires_grad_(True)
    for fwd, bwd, stock in ((R.ref_l1, R.ref_l1_grad, lambda a, b: (a - b).abs()), (R.ref_l2, R.ref_l2_grad, lambda a, b: (a - b) ** 2)):
        ls = stock(p, t["image1"]).mean(dim=(1, 2, 3))
        close(fwd(p.detach(), t["image1"]), ls.detach())
        close(bwd(p.detach(), t["image1"], gout), torch.autograd.grad((ls * gout).sum(), p)[0])


@pytest.mark.parametrize("name", sorted(LI.PAIR_SHAPES))
def test_reference_formulas_equal_golden_g29(g29, name):
    t = [torch.from_numpy(LI.pair_inputs(name)[k]) for k in LI.KEYS]
    maps = R.ref_tc_maps(*t)
    for k, v in maps.items():
        close(v, torch.from_numpy(g29[f"{name}__{k}"]))
    d0, d1 = R.ref_tc_grads(*t, torch.ones(t[0].shape[0], dtype=F64))
    close(d0, torch.from_numpy(g29[f"{name}__dprocessed0"]))
    close(d1, torch.from_numpy(g29[f"{name}__dprocessed1"]))


def test_reference_sequence_equals_golden_g29(g29):
    inp = {k: torch.from_numpy(v) for k, v in LI.seq_inputs().items()}
    losses, dpred = R.ref_sequence(inp["pred"], inp["frame"], inp["flow"], LI.SEQ_L0)
    for row, k in enumerate(("tc", "l1", "l2")):
        close(losses[row], torch.from_numpy(g29[f"seq__{k}"]))
    close(dpred, torch.from_numpy(g29["seq__dpred"]))
    assert float(losses[0, :, :LI.SEQ_L0].abs().max()) == 0 and float(losses[0, :, LI.SEQ_L0:].min()) > 0


def test_g29_holds_arrays_only_and_a_nonzero_yardstick(g29):
    z = np.load(os.path.join(ROOT, "tests", "golden", "g29_tc_loss.npz"), allow_pickle=False)
    assert all(z[k].dtype.kind in "fi" for k in z.files)
    errs = [k for k in g29 if k.endswith("__f32_err")]
    assert len(errs) == 7 + 7 + 4
    assert all(g29[k].shape == (2,) and (g29[k] > 0).all() and g29[k][1] <= g29[k][0] for k in errs)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from v2v_amd import _lib
    return _lib


def test_loss_symbols_declared_exported_and_bound(L):
    hdr = open(os.path.join(ROOT, "include", "v2v_hip.h")).read()
    declared = set(re.findall(r"\b(v2v_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.v2v_version() == L.ABI_VERSION == 6


def test_loss_argument_validation_needs_no_gpu(L):
    lib = L.lib()
    d = C.c_void_p(4096)

    def fwd(image0=d, image1=d, processed1=d, losses=d, ws=d, h=8, w=8, w_tc=1.0, c=1, n=2):
        return lib.v2v_tc_loss_fwd_hip(image0, image1, d, processed1, d, n, 1, c * h * w, 0, 2 * h * w, 0, 0, c, h, w, 50.0, 1.0, w_tc, 0.0, 0.0,
                                       losses, None, None, None, None, ws, None)

    def bwd(gout=d, d1=d, d0=d, ws=d, h=8, w=8, chain=0, tc_first=0):
        return lib.v2v_tc_loss_bwd_hip(d, d, d, d, d, 2, 1, h * w, 0, 2 * h * w, 0, tc_first, 1, h, w, 50.0, 1.0, 1.0, 0.0, 0.0, gout, chain, d1, d0, ws, None)

    assert fwd(image1=None) == L.ERR_NULL and fwd(processed1=None) == L.ERR_NULL and fwd(losses=None) == L.ERR_NULL and fwd(ws=None) == L.ERR_NULL
    assert fwd(image0=None) == L.ERR_NULL
    assert b"temporal term" in lib.v2v_last_error()
    assert fwd(h=1) == L.ERR_SHAPE and fwd(w=1) == L.ERR_SHAPE and fwd(c=0) == L.ERR_SHAPE
    assert fwd(h=2048, w=2049) == L.ERR_SHAPE
    assert b"2^22" in lib.v2v_last_error()
    assert fwd(image1=C.c_void_p(4098)) == L.ERR_ALIGN
    assert fwd(n=0) == L.OK and fwd(image0=None, w_tc=0.0, n=0) == L.OK
    assert bwd(gout=None) == L.ERR_NULL and bwd(d1=None) == L.ERR_NULL and bwd(d0=None) == L.ERR_NULL and bwd(ws=None) == L.ERR_NULL
    assert bwd(h=1) == L.ERR_SHAPE and bwd(h=4096, w=1025) == L.ERR_SHAPE
    assert bwd(chain=1) == L.ERR_PARAM
    assert lib.v2v_warp_bilinear_hip(None, d, 1, 1, 8, 8, d, None) == L.ERR_NULL
    assert lib.v2v_warp_bilinear_hip(d, d, 1, 1, 8, 1, C.c_void_p(8192), None) == L.ERR_SHAPE
    assert lib.v2v_warp_bilinear_hip(d, d, 1, 1, 8, 8, d, None) == L.ERR_PARAM
    assert lib.v2v_warp_bilinear_adjoint_hip(d, d, 1, 1, 8, 8, d, None, None) == L.ERR_NULL
    assert lib.v2v_warp_bilinear_adjoint_hip(d, d, 1, 1, 4096, 1025, d, d, None) == L.ERR_SHAPE
    assert lib.v2v_warp_bilinear_adjoint_hip(d, d, 0, 1, 8, 8, d, d, None) == L.OK
    # workspace: forward = one (tc, l1, l2) partial per 256-pixel tile; backward = int64 accumulator + two float32 planes + a word per image
    assert lib.v2v_tc_loss_workspace_bytes(480, 1, 128, 128, 0) == 480 * 64 * 12
    assert lib.v2v_tc_loss_workspace_bytes(480, 1, 128, 128, 1) == 480 * 128 * 128 * 16 + 480 * 4
    assert lib.v2v_tc_loss_workspace_bytes(1, 1, 1, 8, 0) == L.ERR_SHAPE and lib.v2v_tc_loss_workspace_bytes(1, 1, 2048, 2049, 1) == L.ERR_SHAPE
    assert lib.v2v_tc_loss_workspace_bytes(1, 1, 2048, 2048, 1) > 0


def test_loss_classes_keep_the_reference_names_and_carry_over(monkeypatch):
    from v2v_amd import loss_ops, losses
    assert [c.__name__ for c in (losses.l1_loss, losses.l2_loss, losses.temporal_consistency_loss)] == ["l1_loss", "l2_loss", "temporal_consistency_loss"]
    with pytest.raises(AssertionError):
        losses.temporal_consistency_loss(L0=0)
    calls = []

    class Fake:
        @staticmethod
        def apply(*args):
            calls.append(args)
            return torch.arange(6.0).reshape(3, 2)

    monkeypatch.setattr(losses, "PairLossFn", Fake)
    tc = losses.temporal_consistency_loss(weight=0.5, L0=2)
    imgs = [torch.full((2, 1, 4, 4), float(k)) for k in range(8)]
    assert tc(0, imgs[0], imgs[1], imgs[2], reduce_batch=False) == 0 and tc(1, imgs[3], imgs[4], imgs[2], reduce_batch=False) == 0
    assert not calls and tc.image0 is imgs[3] and tc.processed0 is imgs[4]
    out = tc(2, imgs[5], imgs[6], imgs[7], reduce_batch=False)
    assert torch.equal(out, torch.tensor([0.0, 1.0]))
    processed0, processed1, image0, image1, flow, alpha, weights, flow_sign, maps = calls[0]
    assert processed0 is imgs[4] and processed1 is imgs[6] and image0 is imgs[3] and image1 is imgs[5] and flow is imgs[7]
    assert (alpha, weights, flow_sign, maps) == (50.0, (0.5, 0.0, 0.0), -1.0, False)     # the flow is negated inside the kernel
    assert tc.image0 is imgs[5] and tc.processed0 is imgs[6]
    assert float(tc(3, imgs[0], imgs[1], imgs[2])) == 0.5                                   # reduce_batch: the mean over the samples
    assert torch.equal(losses.l1_loss(2.0)(imgs[1], imgs[0], reduce_batch=False), torch.tensor([2.0, 3.0]))
    assert calls[-1][0] is None and calls[-1][6] == (0.0, 2.0, 0.0)
    assert torch.equal(losses.l2_loss()(imgs[1], imgs[0], reduce_batch=False), torch.tensor([4.0, 5.0]))
    assert calls[-1][6] == (0.0, 0.0, 1.0)
    assert loss_ops.MAPS == ("image0_warped_to1", "processed0_warped_to1", "visibility_mask", "error_map")


def test_loss_wrappers_fail_loudly_without_gpu(L):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from v2v_amd import loss_ops, losses
    x, f = torch.zeros((1, 1, 4, 4)), torch.zeros((1, 2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_ops.warp_bilinear(x, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_ops.warp_bilinear_adjoint(x, f, (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_ops.temporal_consistency_loss(x, x, x, x, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.l1_loss()(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_ops.sequence_losses(x[None], x[None], f[None], 1.0, None, 1.0, 1)
