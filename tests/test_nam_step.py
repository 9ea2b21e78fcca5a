"""NER-Net's NAM cell on the matrix cores (three launches: M, C, H; v2v_amd/csrc/v2v_nam.hpp, nhwc_ops.nam_step) against the reference's
module semantics (NAM_withoutGCB.forward, model/nernet/submodules.py:585-642), restated with stock PyTorch ops in tests/nam_stock.py.

Tolerances.  The kernels multiply in bf16 and accumulate in fp32; K per output is the ConvGRU step's 2C * 9.
  * against the fp64 evaluation on the SAME bf16-rounded operands: tests/test_convgru.py's TOL_SAME_OPERANDS, 2e-5 absolute, for the five
    fp32 outputs (m', alpha, c', o_pre, h'); h' is evaluated on the package's OWN bf16 c' and m' and fp32 o_pre, so that a rounding flip
    in those does not leak into its figure.  The double sigmoid and exp(sigmoid(.)) <= e pass an accumulator error on with a factor
    below 1 (1/4 * 1/4 and e/4).  Confirmed by nam_stock.nam_emulate (`python tests/nam_stock.py`: bf16 operands, fp32 accumulation in a
    shuffled order 16 products at a time, over the seven shapes with and without state): 0.8e-6 .. 4.7e-6, the worst at 1x256x24x30.
  * against the plain fp32 module on unrounded inputs and states: 2 x the same emulation's worst figure over these shapes (6.6e-3 ..
    1.06e-2, the worst at 5x128x12x10: the rounding of x, m_t, h to bf16 and of c', m' in front of conv_o) = 2.13e-2.
  * the bf16 outputs are the RNE of their fp32 masters, bit for bit.
The cell state is carried in fp32: test_slow_update_sequence_keeps_what_a_bf16_state_loses pins that."""
import functools

import pytest

from nam_stock import SHAPES, bf16_round, nam_case, nam_out, nam_ref

pytestmark = pytest.mark.gpu

TOL_SAME_OPERANDS = 2e-5
TOL_FP32_MODULE = 2.13e-2


def _nhwc(t, dtype=None):
    import torch
    t = t.permute(0, 2, 3, 1).contiguous().cuda()
    return t.to(dtype or torch.bfloat16)


def _nchw(t):
    return t.float().permute(0, 3, 1, 2).cpu()


def _pack(N, ws):
    return N.pack_nam_weights(*(ws[k].cuda() for k in ("conv_x", "conv_h", "conv_m", "conv_o", "conv_last", "lag")))


@functools.lru_cache(maxsize=None)
def _reference(shape, zero_state):
    """the case, its fp64 evaluation on the bf16-rounded operands and the plain fp32 module on the unrounded ones: computed once per
    (shape, state), shared by the tile codes, never written to"""
    import torch
    x, m, h, c, ws = nam_case(*shape, seed=sum(shape) + zero_state)
    if zero_state:
        h = c = None
    want = nam_ref(bf16_round(x), bf16_round(m), None if h is None else bf16_round(h), c, ws, torch.float64)
    return (x, m, h, c, ws), want, nam_ref(x, m, h, c, ws, torch.float32)


@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("zero_state", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_step_matches_reference_semantics(shape, zero_state, tile):
    import torch
    from v2v_amd import nhwc_ops as N
    (x, m, h, c, ws), want, plain = _reference(shape, zero_state)
    got = N.nam_step(_nhwc(x), _nhwc(m), None if h is None else _nhwc(h), None if c is None else _nhwc(c, torch.float32), _pack(N, ws),
                     nchw_dtype=torch.float32, tile=tile, return_workspaces=True)
    torch.cuda.synchronize()
    f64 = torch.float64
    figures = {k: float((_nchw(got[src]).double() - want[k]).abs().max()) for k, src in (("m", "m_f32"), ("alpha", "alpha"), ("c", "c"), ("o_pre", "o_pre"))}
    want_h = nam_out(_nchw(got["o_pre"]), _nchw(got["c_bf16"]), _nchw(got["m"]), ws, f64)          # on the package's OWN operands of launch H
    figures["h"] = float((_nchw(got["h_f32"]).double() - want_h).abs().max())
    figures["fp32_module"] = max(float((_nchw(got[src]) - plain[k]).abs().max()) for k, src in (("m", "m_f32"), ("alpha", "alpha"), ("c", "c"), ("o_pre", "o_pre"),
                                                                                                 ("h", "h_f32")))
    print(shape, "zero state" if zero_state else "with state", "tile", tile, figures)
    for k in ("m", "alpha", "c", "o_pre", "h"):
        assert figures[k] < TOL_SAME_OPERANDS, (k, figures)
    for master, copy in (("h_f32", "h"), ("c", "c_bf16"), ("m_f32", "m")):
        assert torch.equal(got[copy], got[master].to(torch.bfloat16)), copy                         # the next convolutions' operands: RNE of the fp32 values
    assert torch.equal(got["h_nchw"], got["h_f32"].permute(0, 3, 1, 2).contiguous())
    assert figures["fp32_module"] < TOL_FP32_MODULE, figures


def test_zero_state_equals_a_state_of_zeros_and_the_cell_state_updates_in_place():
    import torch
    from v2v_amd import nhwc_ops as N
    x, m, _, _, ws = nam_case(2, 64, 8, 16, seed=5)
    packed, xn, mn = _pack(N, ws), _nhwc(x), _nhwc(m)
    zh, zc = torch.zeros_like(xn), torch.zeros(xn.shape, dtype=torch.float32, device="cuda")
    a = N.nam_step(xn, mn, None, None, packed)                     # K over x only in launch C
    b = N.nam_step(xn, mn, zh, zc, packed, c_out=zc)
    # the same sums in another order: fp32 rounding apart (tests/test_convgru.py's margins) -- 2e-6 on fp32 outputs, one bf16 ulp on bf16 ones
    assert b["c"] is zc and float((a["c"] - b["c"]).abs().max()) < 2e-6 and float((a["h_f32"] - b["h_f32"]).abs().max()) < 2e-6
    assert float((a["h"].float() - b["h"].float()).abs().max()) <= 2.0 ** -8
    assert torch.equal(a["m"], b["m"]) and torch.equal(a["m_f32"], b["m_f32"])                        # launch M does not see the state


def test_two_runs_are_bitwise_equal():
    import torch
    from v2v_amd import nhwc_ops as N
    x, m, h, c, ws = nam_case(3, 128, 12, 10, seed=8)
    args = (_nhwc(x), _nhwc(m), _nhwc(h), _nhwc(c, torch.float32), _pack(N, ws))
    a, b = N.nam_step(*args), N.nam_step(*args)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_slow_update_sequence_keeps_what_a_bf16_state_loses():
    """The ConvGRU test of this name, for c.  NAM's cell state cannot update slowly -- f_t = s(s(.) - alpha i_t) < s(1) = 0.731, so a step
    keeps at most 73 % of c and forgets an old rounding at that rate -- hence the bars: over 12 steps on the package's own h, the fp32-carried
    c stays within TOL_SAME_OPERANDS / (1 - 0.731) < 4 x TOL_SAME_OPERANDS of the fp64 recurrence, while the same recurrence with c rounded
    to bf16 at every step (stock fp32 on the CPU) ends up half a bf16 ulp of c away, more than 20 x as far."""
    import torch
    from v2v_amd import nhwc_ops as N
    b, ch, hh, ww, steps = 1, 64, 8, 8, 12
    x, m, _, c0, ws = nam_case(b, ch, hh, ww, seed=21)
    c0 = 1.0 + 0.5 * c0
    packed, xn, mn = _pack(N, ws), _nhwc(x), _nhwc(m)
    c_dev, h_dev = _nhwc(c0, torch.float32), torch.zeros_like(xn)
    c64, c16 = c0.double(), c0.clone()
    for _ in range(steps):
        h_in = _nchw(h_dev)                                                                           # the package's own h: c is what is followed
        h_dev = N.nam_step(xn, mn, h_dev, c_dev, packed, c_out=c_dev)["h"]
        c64 = nam_ref(bf16_round(x), bf16_round(m), h_in, c64, ws, torch.float64)["c"]
        c16 = bf16_round(nam_ref(bf16_round(x), bf16_round(m), h_in, c16, ws, torch.float32)["c"])
    torch.cuda.synchronize()
    err32, err16 = float((_nchw(c_dev).double() - c64).abs().max()), float((c16.double() - c64).abs().max())
    print("fp32-carried state", err32, "bf16-carried state", err16)
    assert float((c64 - c0).abs().mean()) > 1e-2                                                      # the sequence does move the state
    assert err32 < 4 * TOL_SAME_OPERANDS
    assert err16 > 20 * err32, "the sequence does not tell a bf16 state from an fp32 one"


def test_python_side_refuses_what_the_kernels_do_not_take():
    import torch
    from v2v_amd import nhwc_ops as N
    x, m, h, c, ws = nam_case(1, 64, 6, 6, seed=1)
    packed = _pack(N, ws)
    with pytest.raises(ValueError, match="come together"):
        N.nam_step(_nhwc(x), _nhwc(m), _nhwc(h), None, packed)
    with pytest.raises(ValueError, match=r"\(H\*W\) % 4 == 0"):
        N.nam_step(_nhwc(x[:, :, :5, :5]), _nhwc(m[:, :, :5, :5]), None, None, packed)
    with pytest.raises(ValueError, match="tile must be 0"):
        N.nam_step(_nhwc(x), _nhwc(m), None, None, packed, tile=3)
    with pytest.raises(ValueError, match="conv_h.0.weight"):
        N.pack_nam_weights(*(ws[k].cuda() if k != "conv_h" else ws[k][:8].cuda() for k in ("conv_x", "conv_h", "conv_m", "conv_o", "conv_last", "lag")))
    with pytest.raises(ValueError, match="C must be 64, 128 or 256"):
        w96 = nam_case(1, 96, 2, 2, seed=1)[4]
        N.pack_nam_weights(*(w96[k].cuda() for k in ("conv_x", "conv_h", "conv_m", "conv_o", "conv_last", "lag")))
