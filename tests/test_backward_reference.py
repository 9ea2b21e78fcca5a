"""tests/backward_reference.py against torch.autograd.grad in float64, on the CPU: the hand-written references of the backward operators
agree with autograd through F.conv2d / F.interpolate / the ConvLSTM step of tests/test_convlstm.py to 1e-12 relative, at two small ragged
shapes each.  With this file the references are a fixed point the GPU tests (tests/test_backward_ops.py) can be exact against."""
import pytest

import backward_reference as R
from test_convlstm import _ref_step

RTOL = 1e-12


def _rand(gen, *shape):
    import torch
    return torch.randn(shape, generator=gen, dtype=torch.float64)


def _close(name, got, want):
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    err, ref = float((got - want).abs().max()), float(want.abs().max())
    assert ref > 0 and err <= RTOL * ref, f"{name}: max error {err:.3e} against max |reference| {ref:.3e}"


def test_relu_bwd():
    import torch
    g = torch.Generator().manual_seed(1)
    for shape in ((1, 3, 5, 7), (2, 8, 3, 1)):
        pre = _rand(g, *shape).requires_grad_()
        pre.data[0, 0, 0, 0] = 0.0                                               # relu'(0) = 0: y > 0 is strict
        y, dy = torch.relu(pre), _rand(g, *shape)
        _close("relu", R.ref_relu_bwd(dy, y.detach()), torch.autograd.grad(y, pre, dy)[0])


@pytest.mark.parametrize("b,cin,cout,ks,stride,hin,win", [(2, 3, 4, 3, 1, 5, 7), (1, 2, 3, 5, 1, 4, 9), (2, 3, 2, 5, 2, 6, 10), (1, 4, 3, 3, 2, 7, 5),
                                                         (1, 2, 2, 5, 2, 1, 3)])
def test_conv_fwd_dgrad_wgrad(b, cin, cout, ks, stride, hin, win):
    """stride 2 on even AND odd inputs (the weight gradient takes both; the device data gradient takes even ones)."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(hin * 100 + win)
    x, w, bias = _rand(g, b, cin, hin, win).requires_grad_(), _rand(g, cout, cin, ks, ks).requires_grad_(), _rand(g, cout).requires_grad_()
    out = F.conv2d(x, w, bias, stride=stride, padding=ks // 2)
    dy, res = _rand(g, *out.shape), _rand(g, b, cin, hin, win)
    dx, dw, db = torch.autograd.grad(out, (x, w, bias), dy)
    _close("fwd", R.ref_conv_fwd(x.detach(), w.detach(), bias.detach(), stride), out.detach())
    _close("dgrad", R.ref_conv_dgrad(dy, w.detach(), stride, hin, win), dx)
    _close("dgrad + residual", R.ref_conv_dgrad(dy, w.detach(), stride, hin, win, residual=res), dx + res)
    got_dw, got_db = R.ref_conv_wgrad(dy, x.detach(), ks, stride)
    _close("dW", got_dw, dw)
    _close("db", got_db, db)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 1, 4), (2, 1, 3, 1), (1, 1, 1, 1)])
def test_upsample2x_bwd(shape):
    """H = 1 / W = 1: both clamped edges fold onto the one row / column."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(sum(shape))
    x = _rand(g, *shape).requires_grad_()
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    dout = _rand(g, *up.shape)
    _close("upsample forward", torch.einsum("jk,bckm,lm->bcjl", R.upsample2x_matrix(shape[2]), x.detach(), R.upsample2x_matrix(shape[3])), up.detach())
    _close("upsample adjoint", R.ref_upsample2x_bwd(dout), torch.autograd.grad(up, x, dout)[0])


@pytest.mark.parametrize("b,c,cout,h,w,with_skip", [(2, 8, 1, 3, 5, True), (1, 16, 3, 7, 1, False), (1, 8, 2, 2, 3, True)])
def test_conv1x1_bwd(b, c, cout, h, w, with_skip):
    """The contract's two roundings are the reference's own; behind them it is the gradient of F.conv2d(bf16(x + skip), bf16(w))."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(b + c + cout)
    x, skip, wt = _rand(g, b, c, h, w), (_rand(g, b, c, h, w) if with_skip else None), _rand(g, cout, c, 1, 1)
    xs = (R.bf16_round(x + skip) if with_skip else x.clone()).requires_grad_()
    wb, bias = R.bf16_round(wt).requires_grad_(), torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(xs, wb, bias)
    dy = _rand(g, *out.shape)
    dx, dw, db = torch.autograd.grad(out, (xs, wb, bias), dy)
    got = R.ref_conv1x1_bwd(dy, x, skip, wt)
    _close("dx", got[0], dx)
    _close("dW", got[1], dw.reshape(cout, c))
    _close("db", got[2], db)
    assert with_skip is False or not torch.equal(xs.detach(), x + skip)         # the rounding is there


@pytest.mark.parametrize("b,c,h,w", [(2, 3, 5, 7), (1, 4, 3, 2)])
@pytest.mark.parametrize("state,with_dc", [(True, True), (False, True), (True, False), (False, False)])
def test_convlstm_step_bwd(monkeypatch, b, c, h, w, state, with_dc):
    """Through _ref_step of tests/test_convlstm.py; the differentiated tensor is the pre-activation gate tensor, i.e. the output of the
    one F.conv2d that _ref_step calls (kept by a pass-through wrapper around it)."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(b * 10 + c)
    x, hp, cp = _rand(g, b, c, h, w), torch.tanh(_rand(g, b, c, h, w)), _rand(g, b, c, h, w).requires_grad_()
    if not state:
        hp, cp = torch.zeros_like(hp), torch.zeros_like(x).requires_grad_()
    wt, bias = _rand(g, 4 * c, 2 * c, 3, 3) * 0.3, _rand(g, 4 * c)
    dh, dc = _rand(g, b, c, h, w), (_rand(g, b, c, h, w) if with_dc else None)
    kept, conv2d = [], F.conv2d

    def keeping_conv2d(*args, **kwargs):
        kept.append(conv2d(*args, **kwargs).detach().requires_grad_())
        return kept[-1]
    monkeypatch.setattr(F, "conv2d", keeping_conv2d)
    hid, cell = _ref_step(x, hp, cp, wt, bias, torch.float64)
    monkeypatch.undo()
    assert len(kept) == 1
    loss = (hid * dh).sum() + ((cell * dc).sum() if with_dc else 0.0)
    want_dgates, want_dcp = torch.autograd.grad(loss, (kept[0], cp))
    got_dgates, got_dcp = R.ref_convlstm_step_bwd(x, hp if state else None, cp.detach() if state else None, wt, bias, dh, dc)
    _close("dgates", got_dgates, want_dgates)
    _close("dc_prev", got_dcp, want_dcp)
