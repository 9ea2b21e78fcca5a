"""FireNet (model/model.py:264-311) on the 16-channel device kernels (v2v_amd/csrc/v2v_narrow.hpp): the one-launch ConvGRU step, the
one-launch residual block, the 16-output head, and the network as a drop-in.

  * golden G28 = the reference's FireNet in float32 on seeded weights, two inputs (one odd-sized): per step the image, and the two final
    states, must be within 2.5x the error of the reference's OWN CPU bf16-autocast run against its float32 self (max and rms; the bar of
    G25-G27); the ratios are printed
  * tests/firenet_stock.py (the stock-PyTorch restatement) reproduces G28 on the CPU to 1e-5 and is the yardstick where G28 does not reach
  * raw operators: tests/test_convgru.py's bars for the step (2e-5 against float64 on the same bf16-rounded operands, 2e-2 against the
    float32 module; K is 4x shorter here) and its slow-update sequence at C = 16 (1e-2); tests/test_convlstm.py's 2^-8 relative bar
    against float64 for the bf16 outputs of residual block and head (weights of that file's scale), tests/test_unet_golden.py's
    single-layer bar (3e-2 max, 6e-3 rms) against the stock float32 layer (inputs and weights of that file's scale)
  * shapes: 2 x 8 x 16 (one partial tile), 1 x 19 x 37 (odd pixel count, partial tiles on both axes, several tiles), 1 x 3 x 3 (every
    ring pixel outside the image)"""
import numpy as np
import pytest

import firenet_stock as S
from seeded_weights import seeded_input

gpu = pytest.mark.gpu
BAR = 2.5
TOL_SAME_OPERANDS = 2e-5
TOL_FP32_MODULE = 2e-2
TOL_LAYER = (3e-2, 6e-3)
SHAPES = [(2, 8, 16), (1, 19, 37)]


def _torch_state(g, device="cpu"):
    import torch
    return {k: torch.from_numpy(v).to(device) for k, v in S.g28_state(g).items()}


def _pkg(state=None):
    from v2v_amd.unet import FireNet
    net = FireNet().cuda()
    if state is not None:
        net.load_state_dict(state, strict=True)
    return net.eval()


def _within(name, got, want, bar):
    """(max, rms) of got - want against BAR x the stored / measured bf16-autocast error; prints each figure and ratio before it asserts."""
    e = S.err(got, want)
    print(f"{name}: max {e[0]:.3e} rms {e[1]:.3e}  (bf16 autocast: max {bar[0]:.3e} rms {bar[1]:.3e}; ratios {e[0] / bar[0]:.2f} {e[1] / bar[1]:.2f})")
    assert e[0] <= BAR * bar[0] and e[1] <= BAR * bar[1], name


def _bf16_round(t):
    import torch
    return t.to(torch.bfloat16).to(torch.float32)


# ---- no GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.INPUTS)
def test_stock_restatement_equals_the_reference_on_cpu(name):
    import torch
    g = S.g28()
    net = S.StockFireNet(_torch_state(g))
    vox = torch.from_numpy(S.g28_vox(g, name))
    with torch.no_grad():
        for t in range(vox.shape[0]):
            assert S.err(net(vox[t])["image"].numpy(), g[f"{name}__image"][t])[0] < 1e-5
        for i in range(2):
            assert S.err(net.states[i].numpy(), g[f"{name}__states"][i])[0] < 1e-5


def test_golden_is_what_its_generator_says():
    g = S.g28()
    assert int(g["net__seed"]) == 2801 and float(g["net__gain"]) == 2.5 and int(g["net__vox_seed"]) == 2828
    for name in S.INPUTS:
        t, n, c, h, w = S.SHAPES[name]
        assert g[f"{name}__image"].shape == (t, n, 1, h, w) and g[f"{name}__states"].shape == (2, n, 16, h, w)
        assert g[f"{name}__bf16_autocast_err_image"].shape == (t, 2) and (g[f"{name}__bf16_autocast_err_image"] > 0).all()
        assert g[f"{name}__bf16_autocast_err_states"].shape == (2, 2) and (g[f"{name}__bf16_autocast_err_states"] > 0).all()
        assert float(g[f"{name}__image"].std()) > 0.1
    assert S.SHAPES["b"][-2:] == (19, 37) and (19 * 37) % 2 == 1
    assert len(g["net__keys"]) == 24 and "G2.out_gate.bias" in set(map(str, g["net__keys"]))


def test_keys_and_shapes_are_the_references():
    """No GPU: the module tree alone.  Reference checkpoints load with strict=True."""
    import torch
    from v2v_amd.unet import FireNet
    g = S.g28()
    net = FireNet()
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in g["net__keys"]] and len(sd) == 24
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g["net__shapes"]]
    net.load_state_dict(_torch_state(g), strict=True)
    assert torch.equal(net.G1.update_gate.weight.detach(), _torch_state(g)["G1.update_gate.weight"])
    assert net.num_bins == 5 and net.num_encoders == 0 and net.num_recurrent_units == 2 and net.states == [None, None]
    legacy = FireNet(unet_kwargs=dict(num_bins=3))                               # the reference's legacy override (model/model.py:272-275)
    assert legacy.num_bins == 3 and legacy.head.conv2d.in_channels == 3


def test_what_is_not_covered_raises():
    from v2v_amd import convlstm as CL
    from v2v_amd.unet import FireNet
    with pytest.raises(ValueError, match="backward"):
        FireNet(trainable=True)
    for kw in (dict(base_num_channels=32), dict(kernel_size=5), dict(unet_kwargs=dict(base_num_channels=8)), dict(num_bins=9)):
        with pytest.raises(ValueError):
            FireNet(**kw)
    # every other width keeps raising
    for make in (lambda: CL.ConvLayer(5, 24, 3, padding=1), lambda: CL.ConvLayer(5, 16, 5, padding=2), lambda: CL.ConvLayer(5, 16, 3, stride=2, padding=1),
                 lambda: CL.ConvGRU(16, 16, 5), lambda: CL.ConvGRU(16, 16, 3, trainable=True), lambda: CL.ResidualBlock(16, 16, trainable=True),
                 lambda: CL.ConvLayer(5, 16, 3, padding=1, trainable=True)):
        with pytest.raises(ValueError):
            make()


def test_shape_errors_are_reported_without_a_gpu():
    """Argument checks of the C ABI run before any HIP call."""
    import ctypes as C
    from v2v_amd import _lib
    L = _lib.lib()
    assert L.v2v_convgru16_packed_elems() == 3 * 16 * 32 * 9 and L.v2v_resblock16_packed_elems() == 10 * 512 and L.v2v_conv_head16_packed_elems() == 3 * 512
    bufs = [(C.c_char * 4096)() for _ in range(5)]
    p, q, hs, h32, o32 = (C.cast(b, C.c_void_p) for b in bufs)

    def step(x=p, h=None, hf=None, B=1, H=3, W=5, h_state=hs, h_f32=o32, nchw=None, dt=_lib.F32):
        return L.v2v_convgru16_step_hip(x, h, hf, q, q, q, B, H, W, h_state, h_f32, nchw, dt, None)
    assert step(H=0) == _lib.ERR_SHAPE and step(B=1 << 20, H=1 << 10, W=1 << 10) == _lib.ERR_SHAPE
    assert step(x=None) == _lib.ERR_NULL and step(h_f32=None) == _lib.ERR_NULL
    assert step(h=q, hf=None) == _lib.ERR_NULL                                  # the bf16 state without its fp32 master
    assert step(h_state=p) == _lib.ERR_PARAM and step(h=q, hf=h32, h_state=q) == _lib.ERR_PARAM and step(h=q, hf=h32, h_f32=h32) == _lib.ERR_PARAM
    assert step(x=C.c_void_p(p.value + 2)) == _lib.ERR_ALIGN
    assert step(nchw=q, dt=_lib.U8) == _lib.ERR_DTYPE
    assert L.v2v_convgru16_pack_weights_hip(p, None, p, q, None) == _lib.ERR_NULL
    assert L.v2v_resblock16_nhwc_hip(p, q, q, q, 1, 0, 4, hs, None) == _lib.ERR_SHAPE
    assert L.v2v_resblock16_nhwc_hip(p, q, q, q, 1, 4, 4, p, None) == _lib.ERR_PARAM
    assert L.v2v_resblock16_nhwc_hip(p, q, None, q, 1, 4, 4, hs, None) == _lib.ERR_NULL
    assert L.v2v_resblock16_pack_weights_hip(p, p, C.c_void_p(q.value + 8), None) == _lib.ERR_ALIGN
    assert L.v2v_conv_head16_pack_weights_hip(p, 9, q, None) == _lib.ERR_SHAPE and L.v2v_conv_head16_pack_weights_hip(p, 0, q, None) == _lib.ERR_SHAPE
    assert L.v2v_conv_head16_nhwc_hip(p, q, q, 1, 1, 4, -1, hs, None) == _lib.ERR_SHAPE
    assert L.v2v_conv_head16_nhwc_hip(None, q, q, 1, 1, 4, 4, hs, None) == _lib.ERR_NULL and b"x8/packed" in L.v2v_last_error()


# ---- the raw operators ------------------------------------------------------------------------------------------------------------------
def _gru_case(b, h, w, seed, c=16):
    """tests/test_convgru.py's recipe at C = 16: N(0,1) input, tanh(N(0,1)) state, weights uniform in +-3/sqrt(fan_in), biases in +-0.5."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, c, h, w), generator=g)
    hp = torch.tanh(torch.randn((b, c, h, w), generator=g))
    k = 1.0 / np.sqrt(2 * c * 9)
    ws = [(torch.rand((c, 2 * c, 3, 3), generator=g) * 2 - 1) * k * 3 for _ in range(3)]
    bs = [(torch.rand((c,), generator=g) * 2 - 1) * 0.5 for _ in range(3)]
    return x, hp, ws, bs


def _conv(x, w, b, dtype):
    import torch.nn.functional as F
    return F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), padding=1)


def _ref_gru(x, h, ws, bs, dtype, round_hr=False):
    """The reference's forward (model/submodules.py:272-276) in `dtype` on the CPU; round_hr: h * r rounded to bf16 as the kernel's operand is."""
    import torch
    xh = torch.cat([x, h], 1).to(dtype)
    u, r = torch.sigmoid(_conv(xh, ws[0], bs[0], dtype)), torch.sigmoid(_conv(xh, ws[1], bs[1], dtype))
    hr = h.to(dtype) * r
    if round_hr:
        hr = _bf16_round(hr.float()).to(dtype)
    o = torch.tanh(_conv(torch.cat([x.to(dtype), hr], 1), ws[2], bs[2], dtype))
    return h.to(dtype) * (1 - u) + o * u, hr


def _nhwc(t, dtype=None):
    import torch
    t = t.cuda().permute(0, 2, 3, 1).contiguous()
    return t if dtype is None else t.to(dtype)


def _nchw(t):
    return t.permute(0, 3, 1, 2).cpu()


def _pack_gru(N, ws, bs):
    import torch
    return N.pack_gru16_weights(*(w.cuda() for w in ws)), torch.cat(bs[:2]).cuda(), bs[2].cuda()


@gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("zero_state", [False, True])
def test_convgru16_step_matches_reference_semantics(shape, zero_state):
    import torch
    from v2v_amd import nhwc_ops as N
    b, h, w = shape
    x, hp, ws, bs = _gru_case(b, h, w, seed=sum(shape) + int(zero_state))
    if zero_state:
        hp = torch.zeros_like(hp)
    packed, b_gates, b_out = _pack_gru(N, ws, bs)
    xn, h32 = _nhwc(x, torch.bfloat16), _nhwc(hp)
    args = (None, None) if zero_state else (h32.to(torch.bfloat16), h32)
    h_bf16, h_f32, h_nchw = N.convgru16_step(xn, *args, packed, b_gates, b_out, nchw_dtype=torch.float32)
    torch.cuda.synchronize()
    # float64 on the same bf16-rounded operands (x, the bf16 copy of h in the convolutions, the weights), the fp32 master in the blend, and
    # h * r rounded to bf16 as the candidate's operand.  The one-launch kernel hands out no hr, so (unlike tests/test_convgru.py, which reads
    # the package's own hr) the reference rounds it itself.  Where the float64 h * r lies within 2e-6 relative of a bf16 rounding tie -- the
    # fp32 sigmoid (hardware exp2 / rcp, ~4 ulp) can land on the other side -- either neighbour is a correct rounding; the outputs in the 3x3
    # window of such an element get the bar 2e-5 + one bf16 ulp of that hr times |out_gate weight| (tanh' <= 1, u <= 1), every other output
    # exactly 2e-5.  The window must stay a small part of the tensor.
    xr, hb, wr = _bf16_round(x), _bf16_round(hp), [_bf16_round(v) for v in ws]
    f64 = torch.float64
    xh = torch.cat([xr, hb], 1)
    u, r = torch.sigmoid(_conv(xh, wr[0], bs[0], f64)), torch.sigmoid(_conv(xh, wr[1], bs[1], f64))
    hr64 = hp.double() * r
    hr = _bf16_round(hr64.float()).double()
    ulp = torch.where(hr != 0, torch.exp2(torch.floor(torch.log2(hr.abs().clamp_min(1e-30))) - 7), torch.zeros_like(hr))
    near_tie = (ulp > 0) & ((ulp / 2 - (hr64 - hr).abs()) <= 2e-6 * hr64.abs())
    slack = torch.nn.functional.conv2d(near_tie.double() * ulp, wr[2][:, 16:].abs().double(), padding=1)
    want = hp.double() * (1 - u) + torch.tanh(_conv(torch.cat([xr.double(), hr], 1), wr[2], bs[2], f64)) * u
    got = _nchw(h_f32).double()
    diff = (got - want).abs()
    clear = slack == 0
    figures = {"h": float(diff[clear].max()), "h_near_ties": float(diff.max()), "near_ties": int(near_tie.sum()), "outputs_near_ties": float((~clear).double().mean()),
               "fp32_module": float((got.float() - _ref_gru(x, hp, ws, bs, torch.float32)[0]).abs().max())}
    print(shape, "zero state" if zero_state else "given state", figures)
    assert tuple(h_f32.shape) == (b, h, w, 16) and bool(h_f32.isfinite().all()) and float(h_f32.abs().max()) > 0.1
    assert figures["outputs_near_ties"] < 0.25
    assert figures["h"] <= TOL_SAME_OPERANDS and bool((diff <= TOL_SAME_OPERANDS + slack).all())
    assert torch.equal(h_bf16, h_f32.to(torch.bfloat16))                        # the next step's operand: RNE of the fp32 state
    assert torch.equal(h_nchw, h_f32.permute(0, 3, 1, 2).contiguous())
    assert figures["fp32_module"] <= TOL_FP32_MODULE
    hb16 = N.convgru16_step(xn, *args, packed, b_gates, b_out, nchw_dtype=torch.bfloat16)[2]
    assert torch.equal(hb16, h_f32.permute(0, 3, 1, 2).contiguous().to(torch.bfloat16))
    if zero_state:                                                              # None and an explicit zero state are the same sums
        z = N.convgru16_step(xn, torch.zeros_like(xn), torch.zeros_like(h32), packed, b_gates, b_out)
        assert torch.equal(z[1], h_f32)


@gpu
def test_convgru16_slow_update_sequence_keeps_what_a_bf16_state_loses():
    """tests/test_convgru.py's recipe at C = 16: 2 x 16 x 16, update-gate bias -8, |h0| in [0.5, 0.95], 64 steps of N(0,1) inputs, against
    the fp32 module.  Bar: max |h64 - h64_fp32| < 1e-2."""
    import torch
    from v2v_amd import nhwc_ops as N
    x, hp, ws, bs = _gru_case(2, 16, 16, seed=11)
    bs[0] = torch.full((16,), -8.0)
    g = torch.Generator().manual_seed(3)
    h0 = _bf16_round(torch.sign(torch.randn(hp.shape, generator=g)) * (0.5 + 0.45 * torch.rand(hp.shape, generator=g)))
    packed, b_gates, b_out = _pack_gru(N, ws, bs)
    h32 = _nhwc(h0)
    hb = h32.to(torch.bfloat16)
    ref = h0.clone()
    xs = torch.randn((64,) + tuple(x.shape), generator=g)
    xs_dev = xs.cuda().permute(0, 1, 3, 4, 2).contiguous().to(torch.bfloat16)
    for t in range(64):
        ref = _ref_gru(xs[t], ref, ws, bs, torch.float32)[0]
        hb, h32 = N.convgru16_step(xs_dev[t], hb, h32, packed, b_gates, b_out)
    err = float((_nchw(h32) - ref).abs().max())
    moved = float((ref - h0).abs().mean())
    print(f"slow update, C = 16: max |h64 - h64_fp32| = {err:.3e}, mean |h64_fp32 - h0| = {moved:.3e}")
    assert moved > 1e-3                                                         # the sequence does move the state
    assert err < 1e-2


def _layer_case(b, cin, h, w, seed, gain):
    """N(0,1) input; conv(cin -> 16) and conv(16 -> 16) weights uniform in +-gain / sqrt(fan_in), biases in +-0.5 gain / 3."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, cin, h, w), generator=g)
    mk = lambda ci: ((torch.rand((16, ci, 3, 3), generator=g) * 2 - 1) * (gain / np.sqrt(ci * 9)), (torch.rand((16,), generator=g) * 2 - 1) * 0.5 * gain / 3)  # noqa: E731
    return x, mk(cin), mk(16)


# The two references of a bf16 layer output need inputs of different scale, so each test runs its layer on two recipes:
#   gain 3 (tests/test_convlstm.py::test_conv3x3_matches_reference_semantics' weights, outputs up to ~8): float64 on the same bf16-rounded
#           operands, RELATIVE bar of one bf16 ulp, 2^-8 of |want| + 1 -- large values exercise the accumulation
#   gain 1 (tests/test_unet_golden.py's recipe: N(0,1) inputs, weights in +-1/sqrt(fan_in), "activations O(1)", for which that file states
#           its ABSOLUTE single-layer bar 3e-2 max / 6e-3 rms): the stock float32 layer on unrounded operands.  At gain 3 an absolute 3e-2
#           is below the format: a value in [4, 8) is rounded to bf16 by up to 1.6e-2 and its bf16 residual input by as much again.
def _check_float64(name, got, want64):
    rel = float(((got.double() - want64).abs() / (want64.abs() + 1.0)).max())
    print(f"{name}: rel to float64 on the rounded operands {rel:.3e}")
    assert rel < 2.0 ** -8


def _check_float32_layer(name, got, want32):
    e = S.err(got.numpy(), want32.numpy())
    print(f"{name}: against the float32 layer max {e[0]:.3e} rms {e[1]:.3e} (|want| up to {float(want32.abs().max()):.2f})")
    assert e[0] <= TOL_LAYER[0] and e[1] <= TOL_LAYER[1]


@gpu
@pytest.mark.parametrize("shape", SHAPES + [(1, 3, 3)])
def test_resblock16_matches_reference_semantics(shape):
    import torch
    import torch.nn.functional as F
    from v2v_amd import nhwc_ops as N
    b, h, w = shape
    for gain in (3.0, 1.0):
        x, (w1, b1), (w2, b2) = _layer_case(b, 16, h, w, seed=sum(shape), gain=gain)
        out = N.resblock16_nhwc(_nhwc(x, torch.bfloat16), N.pack_resblock16_weights(w1.cuda(), w2.cuda()), b1.cuda(), b2.cuda())
        got = _nchw(out).float()
        assert tuple(out.shape) == (b, h, w, 16) and float(got.max()) > 0.5
        if gain == 3.0:
            xr = _bf16_round(x).double()
            mid = _bf16_round(torch.relu(F.conv2d(xr, _bf16_round(w1).double(), b1.double(), padding=1)).float()).double()
            _check_float64(f"resblock16 {shape}", got, torch.relu(F.conv2d(mid, _bf16_round(w2).double(), b2.double(), padding=1) + xr))
        else:
            _check_float32_layer(f"resblock16 {shape}", got, F.relu(F.conv2d(F.relu(F.conv2d(x, w1, b1, padding=1)), w2, b2, padding=1) + x))


@gpu
@pytest.mark.parametrize("shape", SHAPES + [(1, 3, 3)])
@pytest.mark.parametrize("cin,relu", [(5, True), (8, False)])
def test_conv_head16_matches_reference_semantics(shape, cin, relu):
    import torch
    import torch.nn.functional as F
    from v2v_amd import nhwc_ops as N
    b, h, w = shape
    act = torch.relu if relu else (lambda v: v)
    for gain in (3.0, 1.0):
        x, (wt, bias), _ = _layer_case(b, cin, h, w, seed=sum(shape) + cin, gain=gain)
        out = N.conv_head16_nhwc(N.to_nhwc8_bf16(x.cuda()), N.pack_head16_weights(wt.cuda()), bias.cuda(), relu=relu)
        got = _nchw(out).float()
        assert tuple(out.shape) == (b, h, w, 16)
        if gain == 3.0:
            _check_float64(f"head16 {shape} cin {cin}", got, act(F.conv2d(_bf16_round(x).double(), _bf16_round(wt).double(), bias.double(), padding=1)))
        else:
            _check_float32_layer(f"head16 {shape} cin {cin}", got, act(F.conv2d(x, wt, bias, padding=1)))


# ---- the network ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", S.INPUTS)
def test_network_matches_golden(name):
    import torch
    g = S.g28()
    net = _pkg(_torch_state(g))                                                 # strict=True load from the golden's recipe
    vox = torch.from_numpy(S.g28_vox(g, name)).cuda()
    with torch.no_grad():
        net.reset_states()
        for t in range(vox.shape[0]):
            img = net(vox[t])["image"]
            assert img.shape == g[f"{name}__image"][t].shape and img.dtype == torch.float32
            _within(f"G28 {name} step {t} image", img.cpu().numpy(), g[f"{name}__image"][t], g[f"{name}__bf16_autocast_err_image"][t])
        for i, st in enumerate(net.states):
            _within(f"G28 {name} final state {i}", st.float().cpu().numpy(), g[f"{name}__states"][i], g[f"{name}__bf16_autocast_err_states"][i])


def _sequence(seed, n=2, t=4, h=19, w=37):
    import torch
    return torch.from_numpy(S.sparse_voxels(seed, n, t, 5, h, w)).cuda()


def _step_loop(net, ev, scales=None):
    import torch
    net.reset_states()
    return torch.stack([net(ev[:, t], scales)["image"] for t in range(ev.shape[1])], 1)


def _masters(net):
    """The state tensors with their float32 masters: what a bit-exact continuation needs."""
    out = []
    for s in net._states:
        out.extend((s, s._v2v_gru[0], s._v2v_gru[1]))
    return out


@gpu
def test_forward_sequence_is_bit_identical_to_the_step_loop():
    import torch
    net = _pkg(_torch_state(S.g28()))
    ev = _sequence(2830)
    with torch.no_grad():
        img = _step_loop(net, ev)
        end = [t.clone() for t in _masters(net)]
        assert img.shape == (2, 4, 1, 19, 37) and float(img.abs().max()) > 0
        net.reset_states()
        seq = net.forward_sequence(ev)
        assert torch.equal(seq, img) and all(torch.equal(a, b) for a, b in zip(_masters(net), end))
        for _ in range(2):                                                      # capture, then replay
            seq = net.forward_sequence(ev, graph=True)
            assert torch.equal(seq, img) and all(torch.equal(a, b) for a, b in zip(_masters(net), end))
        assert len(net.__dict__["_sequence_graphs"]) == 1


@gpu
def test_states_round_trip():
    """states (a copy, model/model.py:288-290) assigned back continue bit for bit -- the float32 masters travel with the copy; a cloned
    float32 state continues from its own values; reset_states() gives the zero state again."""
    import torch
    net = _pkg(_torch_state(S.g28()))
    ev = _sequence(2831)
    with torch.no_grad():
        net.reset_states()
        first = [net(ev[:, t])["image"] for t in range(2)]
        saved = net.states
        assert all(a.data_ptr() != b.data_ptr() for a, b in zip(saved, net._states))
        plain = [s.float().clone() for s in saved]      # before `saved` becomes the live list (the setter keeps the list, as the reference's)
        want = [net(ev[:, t])["image"] for t in range(2, 4)]
        net.states = saved
        again = [net(ev[:, t])["image"] for t in range(2, 4)]
        assert all(torch.equal(a, b) for a, b in zip(want, again))
        # float32 clones carry no master: the step takes them at their own (bf16-valued) float32 values
        net.states = [p.clone() for p in plain]
        a = net(ev[:, 2])["image"]
        net.states = [p.contiguous(memory_format=torch.channels_last) for p in plain]
        b = net(ev[:, 2])["image"]
        assert torch.equal(a, b) and float((a - want[0]).abs().max()) < 3e-2
        net.reset_states()
        assert net.states == [None, None]
        redo = [net(ev[:, t])["image"] for t in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(first, redo))


@gpu
def test_event_scales_equals_normalising_first():
    import torch
    net = _pkg(_torch_state(S.g28()))
    ev = _sequence(2832, t=2)
    scales = torch.tensor([[3.0, 2.0], [1.5, 3.0]], device="cuda")              # (neg_max, pos_max) per sample
    sc = scales[:, None, None, None, None, :]
    normed = torch.where(ev > 0, ev / sc[..., 1], ev / sc[..., 0])
    with torch.no_grad():
        want = _step_loop(net, normed)
        assert torch.equal(_step_loop(net, ev, scales), want)
        net.reset_states()
        assert torch.equal(net.forward_sequence(ev, scales), want)
        assert not torch.equal(_step_loop(net, ev), want)


@gpu
def test_standalone_layers_are_drop_ins():
    """ConvGRU(16, 16, 3), ResidualBlock(16, 16), ConvLayer(5, 16, 3, padding=1): NCHW float32 in -> NCHW float32 out; channels-last
    bfloat16 in -> a channels-last view of the kernel's buffer, same values; a cloned float32 state gives the bits of the carried master."""
    import torch
    from v2v_amd import convlstm as CL
    g = S.g28()
    p = _torch_state(g, "cuda")
    sub = lambda pre: {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}   # noqa: E731
    gru, res, head = CL.ConvGRU(16, 16, 3).cuda().eval(), CL.ResidualBlock(16, 16).cuda().eval(), CL.ConvLayer(5, 16, 3, padding=1).cuda().eval()
    gru.load_state_dict(sub("G1."), strict=True), res.load_state_dict(sub("R1."), strict=True), head.load_state_dict(sub("head."), strict=True)
    xs = torch.relu(torch.from_numpy(seeded_input(2840, 3, 2, 16, 19, 37))).cuda()
    with torch.no_grad():
        s = s_clone = want = None
        for t in range(3):
            s = gru(xs[t], s)
            want = S.stock_gru(xs[t], want, p, "G1")
            assert s.shape == want.shape and s.dtype == torch.float32 and s.is_contiguous()
            assert float((s - want).abs().max()) < TOL_FP32_MODULE
            assert torch.equal(gru(xs[t], s_clone), s)                           # prev_state rebuilt from a float32 clone: same bits
            s_clone = s.clone()
        x_cl = xs[1].to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        s_cl = gru(x_cl, s)
        assert s_cl.dtype == torch.bfloat16 and s_cl.is_contiguous(memory_format=torch.channels_last) and not s_cl.is_contiguous()
        assert torch.equal(s_cl.contiguous(), gru(xs[1].to(torch.bfloat16), s))
        r = res(xs[0])
        assert r.dtype == torch.float32 and r.is_contiguous()
        e = S.err(r.cpu().numpy(), S.stock_resblock(xs[0], p, "R1").cpu().numpy())
        scale = max(1.0, float(r.abs().max()))                                   # G28's weights (gain 2.5): the bar of unit-scale activations, scaled as
        assert e[0] <= TOL_LAYER[0] * scale and e[1] <= TOL_LAYER[1] * scale      # tests/test_convlstm.py::test_residual_block_is_a_drop_in scales its own
        r_cl = res(x_cl)
        assert r_cl.dtype == torch.bfloat16 and r_cl.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(r_cl.contiguous(), res(xs[1].to(torch.bfloat16)))
        vox = torch.from_numpy(S.g28_vox(g, "b")).cuda()[0]
        hd = head(vox)
        assert hd.dtype == torch.float32 and hd.shape == (1, 16, 19, 37)
        e = S.err(hd.cpu().numpy(), torch.relu(torch.nn.functional.conv2d(vox, p["head.conv2d.weight"], p["head.conv2d.bias"], padding=1)).cpu().numpy())
        scale = max(1.0, float(hd.abs().max()))
        assert e[0] <= TOL_LAYER[0] * scale and e[1] <= TOL_LAYER[1] * scale
    with pytest.raises(RuntimeError):
        gru(xs[0], None)                                                         # grad mode: loud, no silent graph break


@gpu
@pytest.mark.parametrize("size", [(180, 240), (260, 346)])
def test_batch_one_at_unpadded_real_data_sizes(size):
    """180 x 240 and 260 x 346, unpadded, batch 1, once each: against StockFireNet in float32, within 2.5x the error the stock network itself
    shows under bf16 autocast at that size (measured here)."""
    import torch
    net = _pkg(_torch_state(S.g28()))
    ev = _sequence(2850, n=1, t=2, h=size[0], w=size[1])
    p = _torch_state(S.g28(), "cuda")
    stock32, stock16 = S.StockFireNet(p), S.StockFireNet(p)
    with torch.no_grad():
        net.reset_states()
        for t in range(2):
            out, want = net(ev[:, t])["image"], stock32(ev[:, t])["image"]
            with torch.autocast("cuda", dtype=torch.bfloat16):
                auto = stock16(ev[:, t])["image"]
            assert out.shape == (1, 1) + size and bool(out.isfinite().all())
            bar = S.err(auto.float().cpu().numpy(), want.cpu().numpy())
            assert bar[0] > 0
            _within(f"{size} step {t} image", out.cpu().numpy(), want.cpu().numpy(), bar)


@gpu
@pytest.mark.parametrize("kind", ["convgru16", "resblock16"])
def test_narrow_caches_serve_no_stale_weights(kind):
    """ConvGRU(16, 16, 3) (one cache entry keyed on six parameters) and ResidualBlock(16, 16) (one stream packed from both weights) on a
    1 x 16 x 8 x 8 channels-last bfloat16 input, the ConvGRU from a non-zero previous state (tests/stale_weights.py)."""
    import torch
    from stale_weights import check_no_stale_weights
    from v2v_amd import convlstm as CL
    x = torch.from_numpy(seeded_input(2860, 1, 16, 8, 8)).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    state = torch.tanh(torch.from_numpy(seeded_input(2861, 1, 16, 8, 8))).cuda()

    def make():
        torch.manual_seed(28)
        return (CL.ConvGRU(16, 16, 3) if kind == "convgru16" else CL.ResidualBlock(16, 16)).cuda().eval()
    check_no_stale_weights(make, *((x, state) if kind == "convgru16" else (x,)))
