"""Training on the device kernels (trainable=True, v2v_amd/train.py): gradients of every layer and of the whole recurrent UNet against
the stock network's float32 autograd on the GPU.

The tolerance is measured in each test, not chosen: for every gradient tensor g of the package,
    rel(g) = |g - g_fp32| / |g_fp32|  <=  2 x rel(g_bf16) + 1e-3      and      cos(g, g_fp32) >= 0.99,
where g_fp32 is the stock network's float32 gradient and g_bf16 the same stock network's gradient under bf16 autocast (same weights,
same inputs).  The stock network is tools/e2vid_consumer.py:E2VIDShapedConsumer (pinned to the reference's modules by
test_stock_restatement_of_the_network_equals_the_reference_on_cpu) or, per layer, the same formulas in torch.nn.functional."""
import os
import sys

import numpy as np
import pytest

from seeded_weights import load_seeded, seeded_input

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KW = dict(num_bins=5, skip_type="sum", recurrent_block_type="convlstm", num_encoders=3, base_num_channels=32,
          num_residual_blocks=2, use_upsample_conv=True, final_activation="", norm=None)


def _t(seed, *shape, scale=1.0):
    import torch
    return torch.from_numpy(seeded_input(seed, *shape) * scale).cuda()


def _r(seed, *shape):
    """The upstream gradient of a per-layer loss sum(out * r): values bf16 holds exactly, as the L1 loss's sign(pred - target) / N is
    (the package hands bf16 activations between layers, so an upstream gradient reaches it rounded to bf16 either way)."""
    import torch
    return _t(seed, *shape).to(torch.bfloat16).float()


def _cl(x):
    """A channels-last bf16 leaf: the layout the package network passes between its layers."""
    return x.detach().to(__import__("torch").bfloat16).contiguous(memory_format=__import__("torch").channels_last).requires_grad_()


def _check(name, g, g32, g16):
    g, g32, g16 = (v.detach().double().flatten() for v in (g, g32, g16))
    n = float(g32.norm())
    assert n > 0, name
    rel, rel16 = float((g - g32).norm()) / n, float((g16 - g32).norm()) / n
    cos = float(g @ g32) / (float(g.norm()) * n + 1e-300)
    assert rel <= 2 * rel16 + 1e-3 and cos >= 0.99, f"{name}: rel {rel:.3e} vs bf16-autocast {rel16:.3e}, cos {cos:.5f}"
    assert bool(g.isfinite().all()), name


def _stock_grads(fn, leaves, autocast):
    """grads of sum(fn() * R) w.r.t. leaves, fp32 or under bf16 autocast."""
    import torch
    for v in leaves:
        v.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        loss = fn()
    loss.backward()
    return [v.grad.detach().clone() for v in leaves]


def _compare_layer(pkg_loss, pkg_leaves, stock_loss, stock_leaves, names):
    for v in pkg_leaves:
        v.grad = None
    pkg_loss().backward()
    g = [v.grad for v in pkg_leaves]
    g32 = _stock_grads(stock_loss, stock_leaves, False)
    g16 = _stock_grads(stock_loss, stock_leaves, True)
    for n, a, b, c in zip(names, g, g32, g16):
        _check(n, a, b, c)


def _stock_params(conv):
    import torch
    return (torch.nn.Parameter(conv.weight.detach().clone()), torch.nn.Parameter(conv.bias.detach().clone()))


# ---- 1. per layer -------------------------------------------------------------------------------------------------------------
@gpu
def test_head_gradients():
    import torch
    import torch.nn.functional as F
    from v2v_amd.convlstm import ConvLayer
    m = ConvLayer(5, 32, 5, 1, 2, trainable=True).cuda()
    load_seeded(m, 11)
    x = _t(12, 2, 5, 64, 64)
    r = _r(13, 2, 32, 64, 64)
    w, b = _stock_params(m.conv2d)
    _compare_layer(lambda: (m(x).float() * r).sum(), [m.conv2d.weight, m.conv2d.bias],
                   lambda: (F.relu(F.conv2d(x, w, b, padding=2)).float() * r).sum(), [w, b], ["head.w", "head.b"])


@gpu
@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 128), (128, 256)])
def test_encoder_conv_gradients(cin, cout):
    import torch.nn.functional as F
    from v2v_amd.convlstm import ConvLayer
    m = ConvLayer(cin, cout, 5, 2, 2, trainable=True).cuda()
    load_seeded(m, 20 + cin)
    x32 = _t(21, 2, cin, 64, 64).requires_grad_()
    x = _cl(x32)
    r = _r(22, 2, cout, 32, 32)
    w, b = _stock_params(m.conv2d)
    _compare_layer(lambda: (m(x).float() * r).sum(), [x, m.conv2d.weight, m.conv2d.bias],
                   lambda: (F.relu(F.conv2d(x32, w, b, stride=2, padding=2)).float() * r).sum(), [x32, w, b], ["dx", "dw", "db"])


def _stock_lstm(x, state, w, b):
    import torch
    import torch.nn.functional as F
    h, c = state if state is not None else (torch.zeros_like(x), torch.zeros_like(x))
    i, rr, o, g = F.conv2d(torch.cat([x, h], 1), w, b, padding=1).chunk(4, 1)
    c = torch.sigmoid(rr) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


@gpu
@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("ch,size", [(64, 32), (128, 16), (256, 16)])
def test_convlstm_gradients(ch, size, steps):
    from v2v_amd.convlstm import ConvLSTM
    m = ConvLSTM(ch, ch, 3, trainable=True).cuda()
    load_seeded(m, 30 + ch)
    xs32 = [_t(31 + t, 2, ch, size, size).requires_grad_() for t in range(steps)]
    xs = [_cl(v) for v in xs32]
    rh = [_r(41 + t, 2, ch, size, size) for t in range(steps)]
    rc = _r(51, 2, ch, size, size)
    w, b = _stock_params(m.Gates)

    def pkg():
        state, loss = None, 0.0
        for t in range(steps):
            state = m(xs[t], state)
            loss = loss + (state[0].float() * rh[t]).sum()
        return loss + (state[1].float() * rc).sum()

    def stock():
        state, loss = None, 0.0
        for t in range(steps):
            state = _stock_lstm(xs32[t], state, w, b)
            loss = loss + (state[0].float() * rh[t]).sum()
        return loss + (state[1].float() * rc).sum()
    _compare_layer(pkg, xs + [m.Gates.weight, m.Gates.bias], stock, xs32 + [w, b], [f"dx{t}" for t in range(steps)] + ["dw", "db"])


@gpu
def test_residual_block_gradients():
    import torch.nn.functional as F
    from v2v_amd.convlstm import ResidualBlock
    m = ResidualBlock(256, 256, trainable=True).cuda()
    load_seeded(m, 60)
    x32 = _t(61, 2, 256, 16, 16).requires_grad_()
    x = _cl(x32)
    r = _r(62, 2, 256, 16, 16)
    (w1, b1), (w2, b2) = _stock_params(m.conv1), _stock_params(m.conv2)
    stock = lambda: (F.relu(F.conv2d(F.relu(F.conv2d(x32, w1, b1, padding=1)), w2, b2, padding=1) + x32).float() * r).sum()  # noqa: E731
    _compare_layer(lambda: (m(x).float() * r).sum(), [x, m.conv1.weight, m.conv1.bias, m.conv2.weight, m.conv2.bias],
                   stock, [x32, w1, b1, w2, b2], ["dx", "dw1", "db1", "dw2", "db2"])


@gpu
@pytest.mark.parametrize("cin,cout,size", [(256, 128, 16), (128, 64, 32), (64, 32, 32)])
def test_decoder_gradients(cin, cout, size):
    import torch.nn.functional as F
    from v2v_amd.unet import UpsampleConvLayer
    m = UpsampleConvLayer(cin, cout, 5, padding=2, trainable=True).cuda()
    load_seeded(m, 70 + cin)
    x32, s32 = _t(71, 2, cin, size, size).requires_grad_(), _t(72, 2, cin, size, size).requires_grad_()
    x, s = _cl(x32), _cl(s32)
    r = _r(73, 2, cout, 2 * size, 2 * size)
    w, b = _stock_params(m.conv2d)
    stock = lambda: (F.relu(F.conv2d(F.interpolate(x32 + s32, scale_factor=2, mode="bilinear", align_corners=False), w, b, padding=2)).float() * r).sum()  # noqa: E731
    _compare_layer(lambda: (m(x, s).float() * r).sum(), [x, s, m.conv2d.weight, m.conv2d.bias], stock, [x32, s32, w, b], ["dx", "dskip", "dw", "db"])


@gpu
def test_prediction_layer_gradients():
    import torch.nn.functional as F
    from v2v_amd.convlstm import ConvLayer
    m = ConvLayer(32, 1, 1, activation=None, trainable=True).cuda()
    load_seeded(m, 80)
    x32, h32 = _t(81, 2, 32, 64, 64).requires_grad_(), _t(82, 2, 32, 64, 64).requires_grad_()
    x, h = _cl(x32), _cl(h32)
    r = _r(83, 2, 1, 64, 64)
    w, b = _stock_params(m.conv2d)
    _compare_layer(lambda: (m(x, h).float() * r).sum(), [x, h, m.conv2d.weight, m.conv2d.bias],
                   lambda: (F.conv2d(x32 + h32, w, b).float() * r).sum(), [x32, h32, w, b], ["dx", "dhead", "dw", "db"])


# ---- 2.-7. the whole network -----------------------------------------------------------------------------------------------------
def _nets(seed=90):
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    from e2vid_consumer import E2VIDShapedConsumer, reference_to_stock_keys
    from v2v_amd.unet import E2VIDRecurrent
    pkg = E2VIDRecurrent(dict(KW), trainable=True).cuda()
    vals = load_seeded(pkg.unetrecurrent, seed)                       # the reference's UNetRecurrent keys
    stock = E2VIDShapedConsumer(num_bins=5).cuda()
    stock.load_state_dict(reference_to_stock_keys({k: torch.from_numpy(v) for k, v in vals.items()}), strict=True)
    return pkg, stock, reference_to_stock_keys


def _sequence_loss(net, events, target, autocast=False):
    """The per-step loop of model/train_utils.py:339-345 with an L1 loss over all steps."""
    import torch
    net.reset_states()
    loss = 0.0
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        for t in range(events.shape[1]):
            pred = net(events[:, t])
            img = pred["image"] if isinstance(pred, dict) else pred
            loss = loss + torch.nn.functional.l1_loss(img.float(), target[:, t])
    return loss / events.shape[1]


def _target(seed, b, t, h, w):
    import torch
    import torch.nn.functional as F
    z = F.avg_pool2d(_t(seed, b * t, 1, h, w), 9, stride=1, padding=4) * 3
    return (0.5 + 0.25 * torch.tanh(z)).reshape(b, t, 1, h, w)


def _grads_by_reference_key(net):
    return {k.split(".", 1)[1]: p.grad.detach().clone() for k, p in net.named_parameters()}   # drop 'unetrecurrent.'


@gpu
def test_whole_network_gradients_every_parameter():
    pkg, stock, ref2stock = _nets()
    ev = _t(91, 2, 4, 5, 64, 64)
    tgt = _target(92, 2, 4, 64, 64)
    pkg.zero_grad()
    _sequence_loss(pkg, ev, tgt).backward()
    got = _grads_by_reference_key(pkg)
    for p in pkg.parameters():
        assert p.grad is not None and bool(p.grad.isfinite().all())
    stock.zero_grad()
    _sequence_loss(stock, ev, tgt).backward()
    g32 = {k: p.grad.detach().clone() for k, p in stock.named_parameters()}
    stock.zero_grad()
    _sequence_loss(stock, ev, tgt, autocast=True).backward()
    g16 = {k: p.grad.detach().clone() for k, p in stock.named_parameters()}
    stock_keys = list(ref2stock({k: None for k in got}))              # the same order, stock names
    assert len(stock_keys) == len(g32) == len(got)
    for ref_key, stock_key in zip(got, stock_keys):
        _check(ref_key, got[ref_key], g32[stock_key], g16[stock_key])


@gpu
def test_training_shape_loss_and_gradient_norm():
    import torch
    pkg, stock, _ = _nets(seed=93)
    ev = _t(94, 12, 8, 5, 128, 128)
    tgt = _target(95, 12, 8, 128, 128)
    pkg.zero_grad()
    lp = _sequence_loss(pkg, ev, tgt)
    lp.backward()
    np_ = torch.stack([p.grad.norm() for p in pkg.parameters()]).norm()
    res = []
    for ac in (False, True):
        stock.zero_grad()
        ls = _sequence_loss(stock, ev, tgt, autocast=ac)
        ls.backward()
        res.append((ls.detach(), torch.stack([p.grad.norm() for p in stock.parameters()]).norm()))
    (l32, n32), (l16, n16) = res
    _check("loss", lp.detach().reshape(1), l32.reshape(1), l16.reshape(1))
    _check("grad norm", np_.reshape(1), n32.reshape(1), n16.reshape(1))


@gpu
def test_trainable_forward_is_bit_identical_to_inference():
    import torch
    from v2v_amd.unet import E2VIDRecurrent
    pkg, _, _ = _nets(seed=96)
    inf = E2VIDRecurrent(dict(KW)).cuda()
    inf.load_state_dict(pkg.state_dict())
    ev = _t(97, 2, 3, 5, 64, 64)
    pkg.reset_states()
    inf.reset_states()
    for t in range(3):
        a = pkg(ev[:, t])["image"]
        assert a.requires_grad
        with torch.no_grad():
            b = inf(ev[:, t])["image"]
        assert torch.equal(a.detach(), b), t


@gpu
def test_gradients_are_bitwise_reproducible():
    pkg, _, _ = _nets(seed=98)
    ev = _t(99, 2, 3, 5, 64, 64)
    tgt = _target(100, 2, 3, 64, 64)
    runs = []
    for _ in range(2):
        pkg.zero_grad()
        _sequence_loss(pkg, ev, tgt).backward()
        runs.append([p.grad.detach().clone() for p in pkg.parameters()])
    import torch
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@gpu
def test_it_trains_like_stock_bf16():
    import torch
    pkg, stock, _ = _nets(seed=101)
    ev = _t(102, 2, 4, 5, 64, 64)
    tgt = _target(103, 2, 4, 64, 64)

    def train(net, autocast):
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        losses = []
        for _ in range(50):
            opt.zero_grad()
            loss = _sequence_loss(net, ev, tgt, autocast=autocast)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        with torch.no_grad():
            losses.append(float(_sequence_loss(net, ev, tgt, autocast=autocast)))
        return losses
    lp = train(pkg, False)
    ls = train(stock, True)
    assert lp[-1] <= 0.5 * lp[0], lp
    assert lp[-1] <= 1.25 * ls[-1], (lp[-1], ls[-1])


@gpu
def test_reference_loop_with_nan_hooks_and_forward_sequence_rules():
    import torch
    pkg, _, _ = _nets(seed=104)
    seen = []

    def nan_hook(module, inp, output):           # model/train_utils.py:90-113: walks tensors, tuples and dicts
        outs = output if isinstance(output, tuple) else (output,)
        for o in outs:
            vals = o.values() if isinstance(o, dict) else (o if isinstance(o, tuple) else (o,))
            for v in vals:
                if isinstance(v, tuple):
                    v = v[0]
                if v is not None:
                    assert not bool(torch.isnan(v).any()), type(module).__name__
                    seen.append(type(module).__name__)
    hooks = [m.register_forward_hook(nan_hook) for m in pkg.modules()]
    ev = _t(105, 2, 3, 5, 64, 64)
    tgt = _target(106, 2, 3, 64, 64)
    pkg.reset_states()
    pred_imgs = []
    for t in range(3):
        pred = pkg(ev[:, t])
        pred_imgs.append(pred["image"])
    loss = torch.nn.functional.l1_loss(torch.stack(pred_imgs, 1).float(), tgt)
    loss.backward()
    for h in hooks:
        h.remove()
    assert {"ConvLSTM", "ResidualBlock", "UpsampleConvLayer", "ConvLayer", "E2VIDRecurrent"} <= set(seen)
    assert all(p.grad is not None for p in pkg.parameters())
    # forward_sequence under grad: the plain step loop, differentiable; graph=True refuses
    pkg.zero_grad()
    pkg.reset_states()
    out = pkg.forward_sequence(ev, overlap=True)
    torch.nn.functional.l1_loss(out.float(), tgt).backward()
    assert all(p.grad is not None for p in pkg.parameters())
    with pytest.raises(ValueError):
        pkg.forward_sequence(ev, graph=True)
