"""Training EVFlowNet on the device kernels (trainable=True): gradients of its three autograd Functions (VoxelConvFn as the stem, UpConvFn
behind a concat skip, PredFn with 2 outputs) and of all 26 parameters of the network against stock PyTorch's float32 autograd on the GPU, and 20 Adam steps.

The tolerance is tests/test_train_grad.py's, measured in each test rather than chosen: for every gradient tensor g of the package
    rel(g) = |g - g_fp32| / |g_fp32|  <=  2 x rel(g_bf16) + 1e-3      and      cos(g, g_fp32) >= 0.99,      g finite,
g_fp32 = the stock network's float32 gradient, g_bf16 = the same stock network's gradient under bf16 autocast (same weights and inputs).
The stock network is tests/evflow_stock.py (pinned to the reference by tests/test_evflow.py on the CPU).  Every test prints its figures.

Where gradients meet: each encoder output has two readers (the next layer, the decoder's skip).  autograd adds the two bf16 gradients in
bf16, which for TWO operands is the float32 sum rounded once -- the rule of DESIGN 4.10 holds without a twin Function; the whole-network
test below is what decides it."""
import numpy as np
import pytest

from evflow_stock import g25 as load_g25, g25_state, sparse_voxels, stock_flow
from seeded_weights import load_seeded, seeded_input

gpu = pytest.mark.gpu


def _t(seed, *shape, scale=1.0):
    import torch
    return torch.from_numpy(seeded_input(seed, *shape) * scale).cuda()


def _r(seed, *shape):
    """An upstream gradient bf16 holds exactly (the package hands bf16 activations between layers)."""
    import torch
    return _t(seed, *shape).to(torch.bfloat16).float()


def _cl(x):
    import torch
    return x.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_()


def _figures(g, g32, g16):
    g, g32, g16 = (v.detach().double().flatten() for v in (g, g32, g16))
    n = float(g32.norm())
    rel, rel16 = float((g - g32).norm()) / max(n, 1e-300), float((g16 - g32).norm()) / max(n, 1e-300)
    return n, rel, rel16, float(g @ g32) / (float(g.norm()) * n + 1e-300)


def _check(name, g, g32, g16):
    """tests/test_train_grad.py::_check, verbatim in what it asserts; prints the figures first."""
    n, rel, rel16, cos = _figures(g, g32, g16)
    print(f"{name}: rel {rel:.3e} vs bf16-autocast {rel16:.3e}, cos {cos:.5f}")
    assert n > 0, name
    assert rel <= 2 * rel16 + 1e-3 and cos >= 0.99, f"{name}: rel {rel:.3e} vs bf16-autocast {rel16:.3e}, cos {cos:.5f}"
    assert bool(g.detach().isfinite().all()), name


def _stock_grads(fn, leaves, autocast):
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


# ---- per layer ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_stem_gradients():
    import torch.nn.functional as F
    from v2v_amd.convlstm import ConvLayer
    m = ConvLayer(5, 64, 3, 2, 1, trainable=True).cuda()
    load_seeded(m, 111)
    x = _t(112, 2, 5, 64, 64)
    r = _r(113, 2, 64, 32, 32)
    w, b = _stock_params(m.conv2d)
    _compare_layer(lambda: (m(x).float() * r).sum(), [m.conv2d.weight, m.conv2d.bias],
                   lambda: (F.relu(F.conv2d(x, w, b, stride=2, padding=1)).float() * r).sum(), [w, b], ["stem.w", "stem.b"])


@gpu
@pytest.mark.parametrize("c,cout,size", [(512, 256, 8), (256, 128, 16), (128, 64, 16), (64, 32, 32)])
def test_concat_decoder_gradients(c, cout, size):
    """UpConvFn behind a concat skip incl. the input gradients of x and skip; (64 + 64 -> 32) is the transposed 32 -> 128 convolution on the two-taps-per-chunk
    packing at kernel size 3."""
    import torch
    import torch.nn.functional as F
    from v2v_amd.unet import UpsampleConvLayer
    m = UpsampleConvLayer(2 * c, cout, 3, padding=1, trainable=True).cuda()
    load_seeded(m, 170 + c)
    x32, s32 = _t(171, 2, c, size, size).requires_grad_(), _t(172, 2, c, size, size).requires_grad_()
    x, s = _cl(x32), _cl(s32)
    r = _r(173, 2, cout, 2 * size, 2 * size)
    w, b = _stock_params(m.conv2d)
    stock = lambda: (F.relu(F.conv2d(F.interpolate(torch.cat([x32, s32], 1), scale_factor=2, mode="bilinear", align_corners=False), w, b, padding=1)).float() * r).sum()  # noqa: E731
    _compare_layer(lambda: (m(x, s, skip_type="concat").float() * r).sum(), [x, s, m.conv2d.weight, m.conv2d.bias], stock, [x32, s32, w, b],
                   ["dx", "dskip", "dw", "db"])


@gpu
@pytest.mark.parametrize("cout", [2, 3])
def test_prediction_layer_gradients_several_outputs(cout):
    import torch.nn.functional as F
    from v2v_amd.convlstm import ConvLayer
    m = ConvLayer(32, cout, 1, activation=None, trainable=True).cuda()
    load_seeded(m, 180)
    x32 = _t(181, 2, 32, 64, 64).requires_grad_()
    x = _cl(x32)
    r = _r(183, 2, cout, 64, 64)
    w, b = _stock_params(m.conv2d)
    _compare_layer(lambda: (m(x).float() * r).sum(), [x, m.conv2d.weight, m.conv2d.bias],
                   lambda: (F.conv2d(x32, w, b).float() * r).sum(), [x32, w, b], ["dx", "dw", "db"])


# ---- the whole network ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g25():
    return load_g25()


def _nets(g25):
    import torch
    from v2v_amd.unet import EVFlowNet
    vals = g25_state(g25)
    pkg = EVFlowNet(dict(num_bins=5), trainable=True).cuda()
    pkg.load_state_dict({k: torch.from_numpy(v) for k, v in vals.items()}, strict=True)
    stock = {k: torch.from_numpy(v).cuda().requires_grad_() for k, v in vals.items()}
    return pkg, stock


def _target(seed, b, h, w):
    """A smooth seeded flow field of the size of the network's output (std ~0.7)."""
    import torch
    import torch.nn.functional as F
    return 2.0 * torch.tanh(F.avg_pool2d(_t(seed, b, 2, h, w), 9, stride=1, padding=4) * 3)


def _l1(flow, target):
    import torch
    return torch.nn.functional.l1_loss(flow.float(), target)


@gpu
@pytest.mark.parametrize("b,size", [(2, 64), (10, 128)])
def test_whole_network_gradients_every_parameter(g25, b, size):
    import torch
    pkg, stock = _nets(g25)
    ev = torch.from_numpy(sparse_voxels(191, b, 5, size, size)).cuda()
    tgt = _target(192, b, size, size)
    pkg.zero_grad()
    out = pkg(ev)
    assert out["flow"].requires_grad and out["flow"].dtype == torch.float32
    _l1(out["flow"], tgt).backward()
    got = {k: p.grad.detach().clone() for k, p in pkg.named_parameters()}
    assert len(got) == 26 and list(got) == list(stock)
    leaves = list(stock.values())
    g32 = dict(zip(stock, _stock_grads(lambda: _l1(stock_flow(ev, stock), tgt), leaves, False)))
    g16 = dict(zip(stock, _stock_grads(lambda: _l1(stock_flow(ev, stock), tgt), leaves, True)))
    bad = []
    for k in got:
        try:
            _check(k, got[k], g32[k], g16[k])
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


@gpu
def test_trainable_forward_is_bit_identical_to_inference_and_gradients_are_reproducible(g25):
    import torch
    from v2v_amd.unet import EVFlowNet
    pkg, _ = _nets(g25)
    inf = EVFlowNet(dict(num_bins=5)).cuda()
    inf.load_state_dict(pkg.state_dict())
    ev = torch.from_numpy(sparse_voxels(193, 2, 5, 64, 64)).cuda()
    tgt = _target(194, 2, 64, 64)
    with torch.no_grad():
        want = inf(ev)["flow"]
    runs = []
    for _ in range(2):
        pkg.zero_grad()
        flow = pkg(ev)["flow"]
        assert torch.equal(flow.detach(), want)
        _l1(flow, tgt).backward()
        runs.append([p.grad.detach().clone() for p in pkg.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    with pytest.raises(ValueError):
        pkg.forward_sequence(ev[:, None])                               # inference only
    with torch.no_grad():
        assert torch.equal(pkg.forward_sequence(ev[:, None])[:, 0], want)


@gpu
def test_twenty_adam_steps_beside_stock_float32_and_bf16_autocast(g25):
    """lr 1e-4, amsgrad (config/train_v2v_evflow_10k.yaml's optimizer), one fixed batch.  The package's loss after step 20 is below its loss
    at step 1, and its distance from the float32 run's final loss is at most 2 x the bf16-autocast run's distance + 1e-3 of that loss."""
    import torch
    ev = torch.from_numpy(sparse_voxels(195, 2, 5, 64, 64)).cuda()
    tgt = _target(196, 2, 64, 64)

    def train(params, forward, autocast):
        opt = torch.optim.Adam(params, lr=1e-4, amsgrad=True)
        losses = []
        for _ in range(20):
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                loss = _l1(forward(), tgt)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            losses.append(float(_l1(forward(), tgt)))                   # the loss AFTER step 20
        return losses
    pkg, s32 = _nets(g25)
    _, s16 = _nets(g25)
    lp = train(list(pkg.parameters()), lambda: pkg(ev)["flow"], False)
    l32 = train(list(s32.values()), lambda: stock_flow(ev, s32), False)
    l16 = train(list(s16.values()), lambda: stock_flow(ev, s16), True)
    print(f"loss at step 1 / after step 20: package {lp[0]:.5f} / {lp[-1]:.5f}, stock float32 {l32[0]:.5f} / {l32[-1]:.5f}, "
          f"stock bf16 autocast {l16[0]:.5f} / {l16[-1]:.5f}")
    assert lp[-1] < lp[0], lp
    assert abs(lp[-1] - l32[-1]) <= 2 * abs(l16[-1] - l32[-1]) + 1e-3 * l32[-1], (lp[-1], l32[-1], l16[-1])
