"""NER-Net's global context block with the 1x1 convolution in front of it and the residual behind it, restated with stock PyTorch ops
(RecurrentConvLayer_NAM_GCB.forward and ContextBlock2d with pool 'att' and fusion 'channel_add', model/nernet/submodules.py:365-442,
:768-770 of the reference, written from their formulas), and the weight recipe of the operator tests.  A helper module, not a test:
tests/test_gcb.py, tests/test_gcb_concurrency.py and tools/nam_time.py import it."""
import numpy as np
import torch
import torch.nn.functional as F


def gcb_weights(c, g):
    """the eleven tensors of nhwc_ops.GCB_KEYS in the reference's shapes: uniform +-3 / sqrt(fan_in), biases +-0.5, LayerNorm around (1, 0)"""
    u = lambda *s: torch.rand(s, generator=g) * 2 - 1                                      # noqa: E731
    r = c // 4
    return [u(c, c, 1, 1) * 3 / np.sqrt(c), u(c) * 0.5, u(1, c, 1, 1) * 3 / np.sqrt(c), u(1) * 0.5, u(r, c, 1, 1) * 3 / np.sqrt(c), u(r) * 0.5,
            1 + 0.3 * u(r, 1, 1), 0.3 * u(r, 1, 1), torch.tensor([0.25]), u(c, r, 1, 1) * 3 / np.sqrt(r), u(c) * 0.5]


def gcb_ref(x, ws, dtype, eps=1e-5):
    """x [B,C,H,W] -> (out, ctx, add, g, pooling weights [B,HW]) in `dtype` on the CPU"""
    w1, b1, wm, bm = (t.to(dtype) for t in ws[:4])
    x = x.to(dtype)
    g = F.conv2d(x, w1, b1)
    w = torch.softmax(F.conv2d(g, wm, bm).flatten(1), dim=1)
    ctx = (g.flatten(2) * w[:, None, :]).sum(-1)
    add = mlp_ref(ctx, ws, dtype, eps)
    return x + g + add[:, :, None, None], ctx, add, g, w


def mlp_ref(ctx, ws, dtype, eps=1e-5):
    """channel_add_conv on a pooled context [B,C]: 1x1 convolutions on a 1x1 image are linear layers"""
    wa, ba, lw, lb, pr, wb, bb = (t.to(dtype) for t in ws[4:])
    t = F.layer_norm(F.linear(ctx.to(dtype), wa.flatten(1), ba), (ba.numel(),), lw.flatten(), lb.flatten(), eps)
    return F.linear(F.prelu(t, pr), wb.flatten(1), bb)
