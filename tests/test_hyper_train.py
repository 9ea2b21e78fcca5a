"""HyperE2VID training on the device kernels: the dynamic layer (v2v_amd.train.DynamicUpsampleFn) and the whole network against the stock
training-mode restatement (tests/hyper_train_stock.py) on the same weights and inputs.

Criterion per gradient tensor (tests/test_train_grad.py's rule with the cosine bar tied to autocast): rel <= 2 rel_bf16 + 1e-3 and
1 - cos <= max(1e-2, 2 (1 - cos_bf16)), all finite, where rel_bf16 / cos_bf16 are the stock restatement's OWN figures under bf16 autocast
(the unfold formulation) against its float32 gradient.  Figures are printed."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hyper_train_stock as hts  # noqa: E402
from hyper_stock import g26, g26_state, sparse_voxels  # noqa: E402
from seeded_weights import seeded_input  # noqa: E402


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _load(module, state):
    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return module.cuda()


def _check(label, grads, want, yard):
    """grads / want / yard: {name: array}; yard = the autocast run's gradients, or {name: (rel_bf16, cos_bf16)}."""
    bad = []
    for name in want:
        rel, cos = hts.rel_cos(grads[name], want[name])
        rel16, cos16 = yard[name] if isinstance(yard[name], tuple) else hts.rel_cos(yard[name], want[name])
        ok = bool(np.isfinite(np.asarray(grads[name], dtype=np.float64)).all()) and hts.within(rel, cos, rel16, cos16)
        print(f"{label} {name}: rel {rel:.3e} (bf16 autocast {rel16:.3e}), 1 - cos {1 - cos:.3e} (bf16 autocast {1 - cos16:.3e}){'' if ok else '   <-- OUT'}")
        if not ok:
            bad.append(name)
    assert not bad, f"{label}: {bad}"


# ---- the layer -------------------------------------------------------------------------------------------------------------------------------
def _stock_layer_grads(state, inputs, autocast):
    p = hts.to_params(state, torch.float32, "cuda")
    x, ev, prev, gy = (_cuda(a) for a in inputs)
    x.requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = hts.stock_layer_train(x, ev, prev, p, unfold=autocast)
    y.backward(gy.to(y.dtype))
    grads = {"x": x.grad.double().cpu().numpy()}
    grads.update({k: v.grad.double().cpu().numpy() for k, v in p.items() if v.requires_grad})
    stats = {k: v.double().cpu().numpy() for k, v in p.items() if k.endswith(hts.BN_KEYS)}
    return y.detach().double().cpu().numpy(), grads, stats


def _package_layer_grads(state, inputs):
    from v2v_amd.hyper import DynamicUpsampleLayer
    layer = _load(DynamicUpsampleLayer(256, 128, 5, padding=2, in_fuse_channels=6, trainable=True), state).train()
    x, ev, prev, gy = (_cuda(a) for a in inputs)
    x.requires_grad_(True)
    y = layer(x, ev, prev)
    y.backward(gy)
    grads = {"x": x.grad.double().cpu().numpy()}
    grads.update({k: v.grad.double().cpu().numpy() for k, v in layer.named_parameters()})
    stats = {k: v.double().cpu().numpy() for k, v in layer.state_dict().items() if k.endswith(hts.BN_KEYS)}
    return y.detach().double().cpu().numpy(), grads, stats


@pytest.fixture(scope="module")
def layer_g31():
    g = hts.g31()
    state, inputs = hts.g31_state(g), hts.g31_inputs(g)
    return g, _package_layer_grads(state, inputs), _stock_layer_grads(state, inputs, False), _stock_layer_grads(state, inputs, True), (state, inputs)


def test_layer_gradients_at_the_fixture_shape_against_stock_float32(layer_g31):
    _, (y, grads, _), (y32, g32, _), (y16, g16, _), _ = layer_g31
    rel, rel16 = hts.rel_cos(y, y32)[0], hts.rel_cos(y16, y32)[0]
    print(f"layer output: rel {rel:.3e} (bf16 autocast {rel16:.3e})")
    assert rel <= 2 * rel16 + 1e-3
    _check("layer [2,256,6,10]", grads, g32, g16)


def test_layer_gradients_against_the_reference_float64_fixture(layer_g31):
    g, (y, grads, stats), _, _, _ = layer_g31
    rel, rel16 = hts.rel_cos(y, hts.g31_array(g, "y"))[0], float(g["y__bf16_autocast"][0])
    print(f"layer output against G31: rel {rel:.3e} (the reference's bf16 autocast {rel16:.3e})")
    assert rel <= 2 * rel16 + 1e-3
    want, got, yard = {}, {}, {}
    for name in (str(n) for n in g["grad__names"]):
        want[name], got[name] = hts.g31_grad(g, name, grads[name])
        yard[name] = tuple(float(v) for v in g["bf16_autocast__" + name])
    _check("layer against G31", got, want, yard)
    for k in (k for k in g.files if k.startswith("state__")):
        if k.endswith("num_batches_tracked"):
            assert int(stats[k[7:]]) == int(g[k]) == 1


def test_layer_running_statistics_at_the_fixture_shape(layer_g31):
    _, (_, _, stats), (_, _, s32), (_, _, s16), _ = layer_g31
    _check_stats("layer", stats, s32, s16)


def _check_stats(label, stats, s32, s16):
    """Bar: 2 x the stock bf16-autocast run's own distance from float32 + 1e-3 of the value (per tensor, largest element)."""
    for k in s32:
        if k.endswith("num_batches_tracked"):
            assert int(stats[k]) == int(s32[k]), k
            continue
        d, d16 = np.abs(stats[k] - s32[k]), np.abs(s16[k] - s32[k])
        print(f"{label} {k}: max distance {d.max():.3e} (bf16 autocast {d16.max():.3e})")
        assert np.all(d <= 2 * d16.max() + 1e-3 * np.abs(s32[k])), k


def test_layer_gradients_at_16x16():
    g = hts.g31()
    state = hts.g31_state(g)
    inputs = (seeded_input(3201, 2, 256, 8, 8), seeded_input(3202, 2, 5, 64, 64), 0.5 * seeded_input(3203, 2, 1, 64, 64),
              hts.bf16_exact(seeded_input(3204, 2, 128, 16, 16)))
    _, grads, _ = _package_layer_grads(state, inputs)
    _, g32, _ = _stock_layer_grads(state, inputs, False)
    _, g16, _ = _stock_layer_grads(state, inputs, True)
    _check("layer [2,256,8,8]", grads, g32, g16)


def test_layer_gradients_are_bitwise_reproducible(layer_g31):
    _, (y, grads, _), _, _, (state, inputs) = layer_g31
    y2, grads2, _ = _package_layer_grads(state, inputs)
    assert np.array_equal(y, y2)
    for k in grads:
        assert np.array_equal(grads[k], grads2[k]), k


def test_an_inference_only_layer_still_raises_in_training_mode():
    from v2v_amd.hyper import DynamicUpsampleLayer
    layer = DynamicUpsampleLayer(256, 128, 5, padding=2, in_fuse_channels=6).cuda().train()
    x, ev, prev = torch.zeros((1, 256, 2, 2), device="cuda"), torch.zeros((1, 5, 16, 16), device="cuda"), torch.zeros((1, 1, 16, 16), device="cuda")
    with pytest.raises(RuntimeError, match="runs BatchNorm on its running statistics only"):
        layer(x, ev, prev)
    with pytest.raises(RuntimeError, match="inference-only"):
        layer.eval()(x.requires_grad_(True), ev, prev)


# ---- the network ----------------------------------------------------------------------------------------------------------------------------
N, T, HW, BETA = 2, 2, 32, 0.5


def _net_inputs():
    ev = sparse_voxels(3301, N, T, 5, HW, HW)
    gt = np.random.Generator(np.random.PCG64(3302)).random((N, T, 1, HW, HW)).astype(np.float32)
    return _cuda(ev), _cuda(gt)


def _package_net(state, trainable=True):
    from v2v_amd.hyper import HyperE2VID
    return _load(HyperE2VID(dict(hts.KW), trainable=trainable), state)


def _package_loss(net, ev, gt):
    net.reset_states()
    loss = 0.0
    for t in range(T):
        loss = loss + (net(ev[:, t], gt[:, t], BETA)["image"].float() - gt[:, t]).abs().mean()
    return loss


def _stock_loss(p, ev, gt, autocast):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        imgs = hts.stock_train_sequence(ev, gt, BETA, p, unfold=autocast)
    return sum((imgs[:, t].float() - gt[:, t]).abs().mean() for t in range(T))


def _stock_net_grads(state, ev, gt, autocast):
    p = hts.to_params(state, torch.float32, "cuda")
    _stock_loss(p, ev, gt, autocast).backward()
    return ({k: v.grad.double().cpu().numpy() for k, v in p.items() if v.requires_grad},
            {k: v.double().cpu().numpy() for k, v in p.items() if k.endswith(hts.BN_KEYS)})


@pytest.fixture(scope="module")
def net_case():
    state = g26_state(g26())
    ev, gt = _net_inputs()
    net = _package_net(state).train()
    _package_loss(net, ev, gt).backward()
    grads = {k: v.grad.double().cpu().numpy() for k, v in net.named_parameters()}
    stats = {k: v.double().cpu().numpy() for k, v in net.state_dict().items() if k.endswith(hts.BN_KEYS)}
    return state, ev, gt, grads, stats, _stock_net_grads(state, ev, gt, False), _stock_net_grads(state, ev, gt, True)


def test_network_gradients_two_steps_of_bptt(net_case):
    _, _, _, grads, _, (g32, _), (g16, _) = net_case
    assert set(grads) == set(g32)                                        # every parameter of the network
    _check("network", grads, g32, g16)


def test_network_running_statistics_after_two_steps(net_case):
    _, _, _, _, stats, (_, s32), (_, s16) = net_case
    assert len(s32) == 6 and all(int(v) == 2 for k, v in stats.items() if k.endswith("num_batches_tracked"))
    _check_stats("network", stats, s32, s16)


def test_network_gradients_are_bitwise_reproducible(net_case):
    state, ev, gt, grads, _, _, _ = net_case
    net = _package_net(state).train()
    _package_loss(net, ev, gt).backward()
    for k, v in net.named_parameters():
        assert np.array_equal(grads[k], v.grad.double().cpu().numpy()), k


def test_a_trainable_network_in_eval_mode_is_the_inference_network_bit_for_bit(net_case):
    state, ev, _, _, _, _, _ = net_case
    a, b = _package_net(state, True).eval(), _package_net(state, False).eval()
    with torch.no_grad():
        for t in range(T):
            assert torch.equal(a(ev[:, t])["image"], b(ev[:, t])["image"])


def test_training_mode_without_grad_uses_batch_statistics_and_updates_the_running_ones(net_case):
    state, ev, gt, _, stats, _, _ = net_case
    net = _package_net(state).train()
    with torch.no_grad():
        _package_loss(net, ev, gt)
    for k, v in net.state_dict().items():
        if k.endswith(hts.BN_KEYS):
            assert np.array_equal(v.double().cpu().numpy(), stats[k]), k    # the same kernels as under grad


def test_an_inference_only_network_still_raises_in_training_mode(net_case):
    state, ev, _, _, _, _, _ = net_case
    net = _package_net(state, False).train()
    with pytest.raises(RuntimeError, match="inference-only and runs BatchNorm on its running statistics"):
        net(ev[:, 0])
    from v2v_amd.hyper import HyperE2VID
    with pytest.raises(ValueError):
        HyperE2VID(dict(hts.KW, skip_type="concat"), trainable=True)


def test_ten_adam_steps_on_one_batch(net_case):
    """The loss falls, and the final loss is within 2 x the bf16-autocast run's distance from the float32 run's (+ 1e-3 of that loss)."""
    state, ev, gt, _, _, _, _ = net_case

    def adam(params):
        return torch.optim.Adam(params, lr=1e-3, amsgrad=True)

    net = _package_net(state).train()
    opt, ours = adam(net.parameters()), []
    for _ in range(10):
        opt.zero_grad()
        loss = _package_loss(net, ev, gt)
        loss.backward()
        opt.step()
        ours.append(float(loss.detach()))
    finals = []
    for autocast in (False, True):
        p = hts.to_params(state, torch.float32, "cuda")
        opt = adam([v for v in p.values() if v.requires_grad])
        for _ in range(10):
            opt.zero_grad()
            loss = _stock_loss(p, ev, gt, autocast)
            loss.backward()
            opt.step()
        finals.append(float(loss.detach()))
    print(f"ten Adam steps: loss {ours[0]:.5f} -> {ours[-1]:.5f}; stock float32 final {finals[0]:.5f}, bf16 autocast final {finals[1]:.5f}")
    assert ours[-1] < ours[0]
    assert abs(ours[-1] - finals[0]) <= 2 * abs(finals[1] - finals[0]) + 1e-3 * finals[0]


def test_the_layer_backward_does_not_depend_on_what_shares_the_cu(layer_g31):
    """The layer's forward + backward beside a ConvLSTM step on another stream gives the bits of its stand-alone run."""
    from v2v_amd import convlstm as CL
    _, (y, grads, _), _, _, (state, inputs) = layer_g31
    g = torch.Generator().manual_seed(5)
    xx, hp = (torch.randn((12, 64, 64, 64), generator=g).bfloat16().cuda() for _ in range(2))
    cp = torch.randn((12, 64, 64, 64), generator=g).cuda()
    packed = CL.pack_gate_weights((torch.randn((256, 128, 3, 3), generator=g) * 0.02).cuda())
    bias = torch.zeros(256).cuda()
    side = torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(side):
            for _ in range(24):
                CL.convlstm_step(xx, hp, cp, packed, bias, nchw_dtype=None)
        y2, grads2, _ = _package_layer_grads(state, inputs)
        torch.cuda.synchronize()
        assert np.array_equal(y, y2)
        for k in grads:
            assert np.array_equal(grads[k], grads2[k]), k
