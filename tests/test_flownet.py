"""FlowNet (the E2VID+ network: UNetFlow, the recurrent UNet with a 3-channel prediction, model/model.py:111-139, model/unet.py:133-194) and
recurrent_block_type 'convgru' on the device kernels.

  * golden G27 = the reference's FlowNet in float32 on seeded weights, both recurrent block types: per step, image and flow must be within
    2.5x the error of the reference's OWN CPU bf16-autocast run against its float32 self (max and rms; the bar of G25 / G26)
  * tests/convgru_stock.py (the stock-PyTorch restatement) reproduces G27 on the CPU to 1e-5 and is the yardstick where G27 does not reach
  * drop-in behaviour: forward_sequence (with / without overlap, hipGraph) bit-identical to the step loop, states round-trip, real-data sizes
  * training ('convlstm'): every parameter gradient by tests/test_train_grad.py's criterion, bitwise reproducible"""
import numpy as np
import pytest

import convgru_stock as S
from seeded_weights import seeded_input

gpu = pytest.mark.gpu
BAR = 2.5


def _t(seed, *shape):
    import torch
    return torch.from_numpy(seeded_input(seed, *shape)).cuda()


def _torch_state(g, block, device="cpu"):
    import torch
    return {k: torch.from_numpy(v).to(device) for k, v in S.g27_state(g, block).items()}


def _pkg(block, state=None, trainable=False, cls=None):
    import torch
    from v2v_amd.unet import FlowNet
    net = (cls or FlowNet)(S.kwargs(block), trainable=trainable).cuda()
    if state is not None:
        net.load_state_dict(state, strict=True)
    return net if trainable else net.eval()


def _within(name, got, want, bar):
    """(max, rms) of got - want against BAR x the stored / measured bf16-autocast error; prints each figure before it asserts."""
    e = S.err(got, want)
    print(f"{name}: max {e[0]:.3e} rms {e[1]:.3e}  (bf16 autocast: max {bar[0]:.3e} rms {bar[1]:.3e})")
    assert e[0] <= BAR * bar[0] and e[1] <= BAR * bar[1], name


@pytest.mark.parametrize("block", S.BLOCKS)
def test_stock_restatement_equals_the_reference_on_cpu(block):
    import torch
    g = S.g27()
    net = S.StockFlowNet(_torch_state(g, block), block)
    vox = torch.from_numpy(g["net__vox"].astype(np.float32))
    with torch.no_grad():
        for t in range(vox.shape[0]):
            out = net(vox[t])
            assert S.err(out["image"].numpy(), g[f"{block}__image"][t])[0] < 1e-5
            assert S.err(out["flow"].numpy(), g[f"{block}__flow"][t])[0] < 1e-5


def test_golden_is_what_its_generator_says():
    g = S.g27()
    assert np.array_equal(g["net__vox"].astype(np.float32), S.sparse_voxels(int(g["net__vox_seed"]), 3, 2, 5, 64, 64))
    for block in S.BLOCKS:
        assert g[f"{block}__image"].shape == (3, 2, 1, 64, 64) and g[f"{block}__flow"].shape == (3, 2, 2, 64, 64)
        assert (g[f"{block}__bf16_autocast_err_image"] > 0).all() and (g[f"{block}__bf16_autocast_err_flow"] > 0).all()
        assert all(str(k).startswith("unetflow.") for k in g[f"{block}__keys"])
    assert "unetflow.encoders.0.recurrent_block.update_gate.weight" in set(map(str, g["convgru__keys"]))


@pytest.mark.parametrize("block", S.BLOCKS)
def test_keys_and_shapes_are_the_references(block):
    """No GPU: the module tree alone.  Reference checkpoints load with strict=True."""
    from v2v_amd.unet import FlowNet
    g = S.g27()
    sd = FlowNet(S.kwargs(block)).state_dict()
    assert list(sd) == [str(k) for k in g[f"{block}__keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g[f"{block}__shapes"]]


def test_what_is_not_covered_raises():
    from v2v_amd.unet import E2VIDRecurrent, FlowNet, RecurrentConvLayer
    with pytest.raises(ValueError, match="backward"):
        FlowNet(S.kwargs("convgru"), trainable=True)
    with pytest.raises(ValueError, match="backward"):
        E2VIDRecurrent(S.kwargs("convgru"), trainable=True)
    with pytest.raises(ValueError):
        RecurrentConvLayer(64, 64, 5, 2, 2, recurrent_block_type="convrnn")
    with pytest.raises(ValueError):
        FlowNet(S.kwargs("convlstm", final_activation="sigmoid"))
    net = FlowNet(S.kwargs("convgru"))
    assert net.num_bins == 5 and net.num_encoders == 3 and net.states == [None] * 3


@gpu
@pytest.mark.parametrize("block", S.BLOCKS)
def test_network_matches_golden(block):
    import torch
    g = S.g27()
    net = _pkg(block, _torch_state(g, block))
    vox = torch.from_numpy(g["net__vox"].astype(np.float32)).cuda()
    with torch.no_grad():
        net.reset_states()
        for t in range(vox.shape[0]):
            out = net(vox[t])
            assert out["image"].shape == (2, 1, 64, 64) and out["flow"].shape == (2, 2, 64, 64) and out["image"].dtype == torch.float32
            _within(f"{block} step {t} image", out["image"].cpu().numpy(), g[f"{block}__image"][t], g[f"{block}__bf16_autocast_err_image"][t])
            _within(f"{block} step {t} flow", out["flow"].cpu().numpy(), g[f"{block}__flow"][t], g[f"{block}__bf16_autocast_err_flow"][t])


def _sequence(seed, n=2, t=4, h=64, w=64):
    import torch
    return torch.from_numpy(S.sparse_voxels(seed, n, t, 5, h, w)).cuda()


def _step_loop(net, ev):
    import torch
    net.reset_states()
    outs = [net(ev[:, t]) for t in range(ev.shape[1])]
    return torch.stack([o["image"] for o in outs], 1), torch.stack([o["flow"] for o in outs], 1)


def _state_tensors(states):
    out = []
    for st in states:
        out.extend(st if isinstance(st, tuple) else (st,))
    return out


@gpu
@pytest.mark.parametrize("block", S.BLOCKS)
def test_forward_sequence_is_bit_identical_to_the_step_loop(block):
    import torch
    net = _pkg(block, _torch_state(S.g27(), block))
    ev = _sequence(2730)
    with torch.no_grad():
        img, flow = _step_loop(net, ev)
        end = _state_tensors(net.states)
        assert float(img.abs().max()) > 0 and float(flow.abs().max()) > 0
        for kw in (dict(overlap=False), dict(overlap=True), dict(overlap=2)):
            net.reset_states()
            seq = net.forward_sequence(ev, **kw)
            assert seq["image"].shape == (2, 4, 1, 64, 64) and seq["flow"].shape == (2, 4, 2, 64, 64)
            assert torch.equal(seq["image"], img) and torch.equal(seq["flow"], flow), kw
            assert all(torch.equal(a, b) for a, b in zip(_state_tensors(net.states), end)), kw
        # hipGraph: the ConvGRU's state buffers follow the ConvLSTM's convention (fresh tensors per step), so both block types capture
        for _ in range(2):                                                      # capture, then replay
            seq = net.forward_sequence(ev, graph=True)
            assert torch.equal(seq["image"], img) and torch.equal(seq["flow"], flow)
            assert all(torch.equal(a, b) for a, b in zip(_state_tensors(net.states), end))


@gpu
@pytest.mark.parametrize("block", S.BLOCKS)
def test_states_round_trip(block):
    """states (a copy, model/model.py:121-123) assigned back continue bit for bit -- for 'convgru' the float32 master travels with the copy;
    reset_states() gives the zero state again."""
    import torch
    net = _pkg(block, _torch_state(S.g27(), block))
    ev = _sequence(2731)
    with torch.no_grad():
        net.reset_states()
        first = [net(ev[:, t]) for t in range(2)]
        saved = net.states
        assert all(a.data_ptr() != b.data_ptr() for a, b in zip(_state_tensors(saved), _state_tensors(net.unetflow.states)))
        want = [net(ev[:, t]) for t in range(2, 4)]
        net.states = saved
        again = [net(ev[:, t]) for t in range(2, 4)]
        for a, b in zip(want, again):
            assert torch.equal(a["image"], b["image"]) and torch.equal(a["flow"], b["flow"])
        net.reset_states()
        assert net.states == [None] * 3
        redo = [net(ev[:, t]) for t in range(2)]
        for a, b in zip(first, redo):
            assert torch.equal(a["image"], b["image"]) and torch.equal(a["flow"], b["flow"])


@gpu
def test_e2vid_recurrent_with_convgru_matches_stock():
    """E2VIDRecurrent with recurrent_block_type 'convgru' (keys unetrecurrent.*, one output) against the stock restatement in float32,
    within 2.5x the error the stock network itself shows under bf16 autocast (computed here, per step)."""
    import torch
    from seeded_weights import load_seeded
    from v2v_amd.unet import E2VIDRecurrent
    net = E2VIDRecurrent(S.kwargs("convgru", final_activation="")).cuda().eval()     # num_output_channels is set to 1 by the class (:263)
    vals = load_seeded(net, 2740, gain=1.6)
    assert "unetrecurrent.encoders.2.recurrent_block.out_gate.bias" in vals
    p = {k: torch.from_numpy(v).cuda() for k, v in vals.items()}
    ev = _sequence(2741, t=3)
    stock32, stock16 = S.StockRecurrentUNet(p, "unetrecurrent.", "convgru"), S.StockRecurrentUNet(p, "unetrecurrent.", "convgru")
    with torch.no_grad():
        net.reset_states()
        for t in range(3):
            want = stock32(ev[:, t])
            with torch.autocast("cuda", dtype=torch.bfloat16):
                auto = stock16(ev[:, t]).float()
            got = net(ev[:, t])["image"]
            assert got.shape == want.shape == (2, 1, 64, 64)
            bar = S.err(auto.cpu().numpy(), want.cpu().numpy())
            assert bar[0] > 0
            _within(f"E2VIDRecurrent convgru step {t}", got.cpu().numpy(), want.cpu().numpy(), bar)
        net.reset_states()
        seq = net.forward_sequence(ev)
        net.reset_states()
        assert torch.equal(seq, torch.stack([net(ev[:, t])["image"] for t in range(3)], 1))


@gpu
@pytest.mark.parametrize("block", S.BLOCKS)
@pytest.mark.parametrize("size", [(192, 240), (272, 352)])
def test_batch_one_at_real_data_sizes(block, size):
    """180 x 240 and 260 x 346 frames padded to multiples of 16, batch 1: partial last tiles at every level.  Against the stock restatement
    in float32, within 2.5x the error the stock network itself shows under bf16 autocast at that size (computed here)."""
    import torch
    net = _pkg(block, _torch_state(S.g27(), block))
    ev = _sequence(2750, n=1, t=2, h=size[0], w=size[1])
    p = _torch_state(S.g27(), block, "cuda")
    stock32, stock16 = S.StockFlowNet(p, block), S.StockFlowNet(p, block)
    with torch.no_grad():
        net.reset_states()
        for t in range(2):
            out, want = net(ev[:, t]), stock32(ev[:, t])
            with torch.autocast("cuda", dtype=torch.bfloat16):
                auto = stock16(ev[:, t])
            assert out["image"].shape == (1, 1) + size and out["flow"].shape == (1, 2) + size
            for k in ("image", "flow"):
                assert bool(out[k].isfinite().all())
                bar = S.err(auto[k].float().cpu().numpy(), want[k].cpu().numpy())
                assert bar[0] > 0
                _within(f"{block} {size} step {t} {k}", out[k].cpu().numpy(), want[k].cpu().numpy(), bar)


# ---- training, 'convlstm' only --------------------------------------------------------------------------------------------------------
def _flow_loss(net, ev, tgt, autocast=False):
    """The per-step loop with an L1 loss on image plus flow over T steps."""
    import torch
    import torch.nn.functional as F
    net.reset_states()
    loss = 0.0
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        for t in range(ev.shape[1]):
            out = net(ev[:, t])
            loss = loss + F.l1_loss(out["image"].float(), tgt[:, t, 0:1]) + F.l1_loss(out["flow"].float(), tgt[:, t, 1:3])
    return loss / ev.shape[1]


def _target(seed, b, t, h, w):
    import torch
    import torch.nn.functional as F
    z = F.avg_pool2d(_t(seed, b * t, 3, h, w), 9, stride=1, padding=4) * 3
    return (0.25 * torch.tanh(z)).reshape(b, t, 3, h, w)


def _train_pair(seed):
    import torch
    from seeded_weights import load_seeded
    pkg = _pkg("convlstm", trainable=True)
    vals = load_seeded(pkg, seed)
    params = {k: torch.nn.Parameter(torch.from_numpy(v).cuda()) for k, v in vals.items()}
    return pkg, params


@gpu
def test_training_gradients_every_parameter():
    """FlowNet(trainable=True), 'convlstm', T = 3: tests/test_train_grad.py's criterion for every parameter gradient against the stock
    network's float32 autograd -- rel <= 2 x rel(stock bf16 autocast) + 1e-3 and cosine >= 0.99."""
    import torch
    from test_train_grad import _check
    pkg, params = _train_pair(2760)
    ev, tgt = _t(2761, 2, 3, 5, 64, 64), _target(2762, 2, 3, 64, 64)
    pkg.zero_grad()
    _flow_loss(pkg, ev, tgt).backward()
    got = {k: p.grad.detach().clone() for k, p in pkg.named_parameters()}
    assert list(got) == list(params)
    grads = {}
    for autocast in (False, True):
        for p in params.values():
            p.grad = None
        _flow_loss(S.StockFlowNet(params, "convlstm"), ev, tgt, autocast=autocast).backward()
        grads[autocast] = {k: p.grad.detach().clone() for k, p in params.items()}
    for k in got:
        assert bool(got[k].isfinite().all())
        _check(k, got[k], grads[False][k], grads[True][k])


@gpu
def test_training_gradients_are_bitwise_reproducible():
    import torch
    pkg, _ = _train_pair(2770)
    ev, tgt = _t(2771, 2, 3, 5, 64, 64), _target(2772, 2, 3, 64, 64)
    runs = []
    for _ in range(2):
        pkg.zero_grad()
        _flow_loss(pkg, ev, tgt).backward()
        runs.append([p.grad.detach().clone() for p in pkg.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@gpu
def test_trainable_forward_equals_inference_and_graph_needs_no_grad():
    import torch
    g = S.g27()
    state = _torch_state(g, "convlstm")
    train_net, infer_net = _pkg("convlstm", state, trainable=True), _pkg("convlstm", state)
    ev = _sequence(2780, t=2)
    with torch.no_grad():
        a, b = _step_loop(train_net, ev), _step_loop(infer_net, ev)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        train_net.forward_sequence(ev, graph=True)
