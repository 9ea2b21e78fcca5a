"""The three recurrent steps of v2v_amd/nhwc_ops.py, instance by instance, against the float64 formulas of tests/recurrent_reference.py
(themselves held to the older restatements, and their recipes to what they claim, on the CPU by tests/test_recurrent_reference.py):
  * convlstm_step    EPI == 0 of convlstm_step_kernel (v2v_convlstm.hpp), four instances
  * convgru_step     EPI == 3 / 4 (v2v_convgru.hpp), two launches, five gates and five candidate instances
  * convgru16_step   MODE 0 of narrow_two_conv_kernel (v2v_narrow.hpp), one launch
-- the recurrent counterpart of tests/test_backward_ops.py and tests/test_forward_ops.py, whose plumbing this file imports.

Three recipes per step:
  * saturated, dense: every pre-activation is an odd multiple of 128 (integer operands, weights k 256, biases +-128; every sum exact in fp32 in
    any order, on the matrix cores and across K groups).  cl_sigmoid is then exactly 0 or 1 and cl_tanh exactly +-1 (v2v_convlstm.hpp: exp2
    over- or underflows), the step is pure routing and the check is torch.equal: c' everywhere, h' of the LSTM where o = 0 or |c'| >= 128
    (elsewhere it is the hardware tanh of an exact c', held to TOL_SAME_OPERANDS), u, hr, h' (fp32, bf16) and both NCHW copies of the GRU steps
    everywhere.  The GRU's fp32 master is n + d with rne_bf16(master) = n and its bf16 copy is INDEPENDENT integers: u = 0 must return n + d bit
    for bit, and which copy feeds the convolutions, hr and the blend shows in the bits.  The zero state (None) must equal an explicit all-zero
    state, torch.equal.
  * saturated, one tap: each gate's weight is zero except 256 at one tap, at the channel map co -> (7 co + 3 + 5 gate) mod 2C (both halves of
    K).  One launch per tap covers every pixel, border and tile seam; the message names the tap, the gate and the border.  On the zero state
    every tap of the h half must give the sign of the bias alone.
  * real-valued: the recipes of tests/test_convlstm.py, test_convgru.py and test_firenet.py at their own TOL_SAME_OPERANDS (imported), on the
    same instances and shapes, so that the saturated cases do not stand alone: h_bf16 == rne(h_f32), the NCHW copies equal to the transposes,
    for the two-launch GRU hr within one bf16 ulp and the candidate on the package's own u / hr.  The one-launch 16-channel step hands out no
    hr: there h' must lie between the formula's values on the two roundings of every hr whose rounding TOL_SAME_OPERANDS on the reset gate can
    flip (the candidate pre-activation is linear in hr, tanh and the blend monotone), widened by TOL_SAME_OPERANDS -- no slack of its own.

Numeric bounds in this file: TOL_SAME_OPERANDS (2e-5: summation order + hardware exp2 / rcp) and 2^-8 for hr (a bf16 rounding of a value in
[-1, 1]), and none other; everything else is torch.equal.

Instances.  Geometry 5 x C x 6 x 10 = 300 pixels: 4.7 tiles of 64, 2.3 of 128, 1.2 of 256 -- seams inside rows, images ending inside tiles,
the last tile partial.  ConvLSTM: C in {64, 128, 256} x tile_rows in {64, 128, 256, 0}; 0 lets launch_convlstm_step choose by the number of
compute units, which the test cannot see: on an MI355X (256 CUs) 300 / 64 x C / 64 <= 256 makes it the two-K-group instance (internal code
65) at every C, which no pinned value reaches.  ConvGRU: every shipped (gates, candidate) instance at every C it admits; (0, 0) is gates 1 and
candidate 1 (C 64) / 5 (C 128, 256) at this size.  The smallest frames -- 2 x 2 (a 16 x 16 input at the deepest encoder) and 1 x 4 (H = 1,
less than one fragment row of pixels) -- run on the automatic and on one pinned single-K-group instance.  ConvGRU16: a single pixel, 1 x 4, two
images of one full tile, one pixel past a tile seam on both axes, three images of several partial tiles.

Outputs the package allocates itself come from the caching allocator, which likes to hand back the block of the previous, identical result;
_poison fills such blocks with NaN first, and the fp32 state goes into a NaN-filled c_out / h_f32_out, so that an element a kernel does not
write does not pass on stale bits."""
import functools

import pytest
import torch

import recurrent_reference as R
from test_backward_ops import BF16, F32, F64, _assert_equal, _borders, _dev, _host, _ops
from test_convgru import TOL_SAME_OPERANDS as TOL_GRU
from test_convgru import _case as _gru_real_operands
from test_convlstm import TOL_SAME_OPERANDS, _case as _lstm_real_operands
from test_firenet import TOL_SAME_OPERANDS as TOL_GRU16
from test_firenet import _gru_case as _gru16_real_operands

gpu = pytest.mark.gpu
assert TOL_GRU == TOL_SAME_OPERANDS == TOL_GRU16
GEOMETRY, SMALLEST = R.GEOMETRY, R.SMALLEST
STATE = pytest.mark.parametrize("given", [True, False], ids=["state", "zero"])

# (C, (B, H, W), tile_rows)
LSTM = [(c, GEOMETRY, t) for c in R.WIDE_CHANNELS for t in (64, 128, 256, 0)] + [(c, g, t) for c in R.WIDE_CHANNELS for g in SMALLEST for t in (0, 64)]
# (C, (B, H, W), (gates, candidate)); gates 1 64x128, 2 128x128, 3 128x256, 4 256x256, 5 64x256 K-split; candidate 1 128x64, 2 128x128 K-split,
# 3 128x256, 4 256x256, 5 64x128 K-split (v2v_convgru_tu.hip)
GRU_PAIRS = {64: [(1, 1), (2, 1), (0, 0)], 128: [(1, 1), (2, 2), (3, 5), (4, 1), (5, 2), (0, 0)], 256: [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (0, 0)]}
GRU = [(c, GEOMETRY, p) for c in R.WIDE_CHANNELS for p in GRU_PAIRS[c]] + [(c, g, p) for c in R.WIDE_CHANNELS for g in SMALLEST for p in ((0, 0), (1, 1))]
TAP_LSTM_TILES, TAP_GRU_TILES = (0, 64), ((0, 0), (1, 1))


def _inst_id(case):
    c, (b, h, w), tile = case
    return f"C{c}-{b}x{h}x{w}-tile{tile if isinstance(tile, int) else f'{tile[0]}+{tile[1]}'}"


def _shape_id(s):
    return "x".join(map(str, s))


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def _poison(shape):
    """Blocks of the sizes the step's outputs take, filled with NaN and handed back to the caching allocator."""
    blocks = [torch.full(shape, float("nan"), dtype=dt, device="cuda") for dt in (BF16, BF16, F32, F32, F32)]
    del blocks


def _nan_like(t):
    return torch.full(t.shape, float("nan"), dtype=F32, device="cuda")


def _where(geometry, c):
    b, h, w = geometry

    def where(i):
        p = (i[0] * h + i[2]) * w + i[3]
        edge = [n for n, on in (("top", i[2] == 0), ("bottom", i[2] == h - 1), ("left", i[3] == 0), ("right", i[3] == w - 1)) if on]
        return (f"image {i[0]} row {i[2]} column {i[3]} channel {i[1]} of {c}: flat pixel {p} of {b * h * w} (pixel {p % 64} / {p % 128} / {p % 256} of a "
                f"64- / 128- / 256-pixel tile), " + ("on the image border: " + " ".join(edge) if edge else "inside the image"))
    return where


def _on(mask, got, want):
    """got where the mask holds, want elsewhere: torch.equal against want then compares the masked elements alone, with their positions."""
    return torch.where(mask, got, want)


def _max(t):
    return float(t.max()) if t.numel() else 0.0


# ---- ConvLSTM ---------------------------------------------------------------------------------------------------------------------------
def _lstm_device(x, h, c, weight, bias, tile):
    """convlstm_step on NCHW float64 CPU operands (None = zero state), with the fp32 and then the bf16 NCHW copy.
    -> (h_state bf16, c' fp32, h' fp32, h' bf16), NCHW on the CPU."""
    ops = _ops()
    packed, bias = ops.pack_gate_weights(weight.to(F32).cuda()), bias.to(F32).cuda()
    xd, hd, cd = _dev(x, BF16), _dev(h, BF16), _dev(c, F32)
    _poison(xd.shape)
    hs, cs, hn = ops.convlstm_step(xd, hd, cd, packed, bias, nchw_dtype=F32, tile_rows=tile, c_out=_nan_like(xd))
    hs2, cs2, hn16 = ops.convlstm_step(xd, hd, cd, packed, bias, nchw_dtype=BF16, tile_rows=tile)
    torch.cuda.synchronize()
    assert torch.equal(hs2, hs) and torch.equal(cs2, cs), "the dtype of the NCHW copy changed the state"
    return _host(hs), _host(cs), hn.cpu(), hn16.cpu()


def _lstm_args(k):
    return k["x"], k["h"], k["c"], k["weight"], k["bias"]


def _check_lstm_saturated(name, k, got, where):
    hs, cs, hn, hn16 = got
    want_h, want_c, exact = k["want_h"], k["want_c"], k["exact"]
    _assert_equal(f"{name}: c'", cs, want_c, where)
    _assert_equal(f"{name}: h' (fp32 NCHW) where o = 0 or |c'| >= 128", _on(exact, hn, want_h), want_h, where)
    _assert_equal(f"{name}: h' (bf16 state) where o = 0 or |c'| >= 128", _on(exact, hs, want_h.to(BF16)), want_h.to(BF16), where)
    _assert_equal(f"{name}: h' (bf16 NCHW) where o = 0 or |c'| >= 128", _on(exact, hn16, want_h.to(BF16)), want_h.to(BF16), where)
    err = _max((hn.to(F64) - want_h.to(F64)).abs()[~exact])
    print(f"{name}: max |h' - [o] tanh(c')| where o = 1 and |c'| < 128 ({int((~exact).sum())} elements) = {err:.3e}")
    assert err < TOL_SAME_OPERANDS, f"{name}: the hardware tanh of an exact c': {err:.3e}"
    _assert_equal(f"{name}: bf16 state against rne(h' fp32)", hs, hn.to(BF16), where)
    _assert_equal(f"{name}: bf16 NCHW against rne(h' fp32)", hn16, hn.to(BF16), where)


@gpu
@STATE
@pytest.mark.parametrize("case", LSTM, ids=_inst_id)
def test_convlstm_saturated(case, given):
    c, geometry, tile = case
    k = R.case(("lstm", c, geometry, given, None))
    where, name = _where(geometry, c), f"convlstm_step {_inst_id(case)} {'state' if given else 'zero state'}"
    got = _lstm_device(*_lstm_args(k), tile)
    _check_lstm_saturated(name, k, got, where)
    if not given:
        zero = torch.zeros_like(k["x"])
        for what, a, b in zip(("h state", "c'", "h' fp32 NCHW", "h' bf16 NCHW"), got, _lstm_device(k["x"], zero, zero, k["weight"], k["bias"], tile)):
            _assert_equal(f"{name}: {what}, None against an explicit zero state", a, b, where)


@functools.lru_cache(maxsize=4)
def _lstm_real(c, geometry, given):
    x, h, cp, weight, bias = _lstm_real_operands(geometry[0], c, *geometry[1:], seed=c + sum(geometry) + given)
    x, h, weight = (R.bf16_round(t.to(F64)) for t in (x, h, weight))
    args = (x, h if given else None, cp.to(F64) if given else None, weight, bias.to(F64))
    return args, R.ref_lstm_step(*args)


@gpu
@STATE
@pytest.mark.parametrize("case", LSTM, ids=_inst_id)
def test_convlstm_real_valued(case, given):
    c, geometry, tile = case
    args, (want_h, want_c) = _lstm_real(c, geometry, given)
    hs, cs, hn, hn16 = _lstm_device(*args, tile)
    figures = {"c": _max((cs.to(F64) - want_c).abs()), "h": _max((hn.to(F64) - want_h).abs())}
    print(f"convlstm_step {_inst_id(case)} {'state' if given else 'zero state'}: {figures}")
    assert figures["c"] < TOL_SAME_OPERANDS and figures["h"] < TOL_SAME_OPERANDS, figures
    where = _where(geometry, c)
    _assert_equal("bf16 state against rne(h' fp32)", hs, hn.to(BF16), where)
    _assert_equal("bf16 NCHW against rne(h' fp32)", hn16, hn.to(BF16), where)


def _lstm_tap_where(k, tap, got_c, got_h):
    """Names the tap, what each gate reads through it and the border; and the gates whose flip alone gives the value the kernel returned."""
    _, c, (b, h, w), given, _ = k["key"]
    maps = R.tap_channels(c, 4)

    def where(i):
        gates, cp = R.lstm_hard_f64(*_lstm_args(k))[2], R._or_zeros(k["c"], k["x"])
        iy, ix = i[2] + tap[0] - 1, i[3] + tap[1] - 1
        reads = []
        for name, ci in zip(R.LSTM_GATES, maps):
            ch = int(ci[i[1]])
            reads.append(f"{name} <- {'x' if ch < c else 'h'}[{ch % c}]")
        v = [float(g[i]) for g in gates]
        suspects = []
        for n, name in enumerate(R.LSTM_GATES):
            f = list(v)
            f[n] = -f[n] if n == 3 else 1 - f[n]
            cell = float(torch.tensor(f[1] * float(cp[i]) + f[0] * f[3], dtype=F64).to(F32))
            if n == 2:                                                           # the out gate shows in h' alone
                if float(got_c[i]) == float(k["want_c"][i]) and float(got_h[i]) != float(k["want_h"][i]):
                    suspects.append(name)
            elif cell == float(got_c[i]) and cell != float(k["want_c"][i]):
                suspects.append(name)
        return (f"tap (ky {tap[0]}, kx {tap[1]}) of pixel (image {i[0]}, row {i[2]}, column {i[3]}), channel {i[1]}, reads input ({iy}, {ix}), "
                f"{_borders(iy, ix, h, w)}; {', '.join(reads)}; want gates (in, remember, out, cell) = {v}; a flip of {suspects or 'no single gate'} gives the value returned")
    return where


@gpu
@STATE
@pytest.mark.parametrize("c", R.WIDE_CHANNELS)
def test_convlstm_one_tap(c, given):
    for tap in R.TAPS:
        k = R.build_case(("lstm", c, GEOMETRY, given, tap))
        for tile in TAP_LSTM_TILES:
            got = _lstm_device(*_lstm_args(k), tile)
            _check_lstm_saturated(f"convlstm_step C{c} tile {tile} tap {tap}", k, got, _lstm_tap_where(k, tap, got[1], got[2]))


# ---- ConvGRU, two launches ------------------------------------------------------------------------------------------------------------------
def _gru_device(x, h, hm, ws, bs, tiles):
    """convgru_step on NCHW float64 CPU operands (h: the bf16 copy, hm: the fp32 master; None = zero state).
    -> (h' bf16, h' fp32, u, hr, h' fp32 NCHW, h' bf16 NCHW), NCHW on the CPU."""
    ops = _ops()
    packed = ops.pack_gru_weights(*(w.to(F32).cuda() for w in ws))
    b_gates, b_out = torch.cat(bs[:2]).to(F32).cuda(), bs[2].to(F32).cuda()
    xd, hd, md = _dev(x, BF16), _dev(h, BF16), _dev(hm, F32)
    _poison(xd.shape)
    hb, hf, u, hr, hn = ops.convgru_step(xd, hd, md, packed, b_gates, b_out, nchw_dtype=F32, tile_gates=tiles[0], tile_cand=tiles[1], h_f32_out=_nan_like(xd))
    second = ops.convgru_step(xd, hd, md, packed, b_gates, b_out, nchw_dtype=BF16, tile_gates=tiles[0], tile_cand=tiles[1])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(second[:4], (hb, hf, u, hr))), "the dtype of the NCHW copy changed the state"
    return _host(hb), _host(hf), _host(u), _host(hr), hn.cpu(), second[4].cpu()


def _gru_args(k):
    return k["x"], k["h"], k["master"], k["ws"], k["bs"]


def _check_gru_saturated(name, k, got, where, wheres=None):
    hb, hf, u, hr, hn, hn16 = got
    want_h, want_u, want_hr = k["want_h"], k["want_u"], k["want_hr"].to(BF16)
    wu, wr, wo = wheres or (where, where, where)
    _assert_equal(f"{name}: u (update gate)", u, want_u, wu)
    _assert_equal(f"{name}: hr = rne(master x reset gate)", hr, want_hr, wr)
    _assert_equal(f"{name}: h' fp32 (candidate and blend)", hf, want_h, wo)
    _assert_equal(f"{name}: h' bf16", hb, want_h.to(BF16), wo)
    _assert_equal(f"{name}: h' fp32 NCHW", hn, want_h, wo)
    _assert_equal(f"{name}: h' bf16 NCHW", hn16, want_h.to(BF16), wo)


@gpu
@STATE
@pytest.mark.parametrize("case", GRU, ids=_inst_id)
def test_convgru_saturated(case, given):
    c, geometry, tiles = case
    k = R.case(("gru", c, geometry, given, None))
    where, name = _where(geometry, c), f"convgru_step {_inst_id(case)} {'state' if given else 'zero state'}"
    got = _gru_device(*_gru_args(k), tiles)
    _check_gru_saturated(name, k, got, where)
    if not given:
        zero = torch.zeros_like(k["x"])
        for what, a, b in zip(("h' bf16", "h' fp32", "u", "hr", "h' fp32 NCHW", "h' bf16 NCHW"), got, _gru_device(k["x"], zero, zero, k["ws"], k["bs"], tiles)):
            _assert_equal(f"{name}: {what}, None against an explicit zero state", a, b, where)


@functools.lru_cache(maxsize=4)
def _gru_real(c, geometry, given):
    """Operands (bf16-rounded x and weights; the master unrounded, its copy rne(master)) and the formula's u and master x reset gate."""
    make = _gru16_real_operands if c == 16 else lambda b, h, w, seed: _gru_real_operands(b, c, h, w, seed)
    x, hp, ws, bs = make(*geometry, seed=c + sum(geometry) + given)
    x, ws, bs = R.bf16_round(x.to(F64)), [R.bf16_round(w.to(F64)) for w in ws], [b.to(F64) for b in bs]
    hm = hp.to(F64) if given else None
    hc = R.bf16_round(hm) if given else None
    pu, pr = R.gru_gate_preactivations(x, hc, ws, bs)
    return (x, hc, hm, ws, bs), torch.sigmoid(pu), torch.sigmoid(pr)


@gpu
@STATE
@pytest.mark.parametrize("case", GRU, ids=_inst_id)
def test_convgru_real_valued(case, given):
    c, geometry, tiles = case
    args, want_u, want_r = _gru_real(c, geometry, given)
    hb, hf, u, hr, hn, hn16 = _gru_device(*args, tiles)
    hm = R._or_zeros(args[2], args[0])
    figures = {"u": _max((u.to(F64) - want_u).abs()), "hr": _max((hr.to(F64) - hm * want_r).abs())}
    want_h = R.ref_gru_step(*args, u=u.to(F64), hr=hr.to(F64))[0]                # the candidate and the blend on the package's own u / hr
    figures["h"] = _max((hf.to(F64) - want_h).abs())
    print(f"convgru_step {_inst_id(case)} {'state' if given else 'zero state'}: {figures}")
    assert figures["u"] < TOL_SAME_OPERANDS and figures["h"] < TOL_SAME_OPERANDS and figures["hr"] <= 2.0 ** -8, figures
    if not given:
        assert not bool(hr.to(F32).abs().any())
    where = _where(geometry, c)
    _assert_equal("h' bf16 against rne(h' fp32)", hb, hf.to(BF16), where)
    _assert_equal("h' fp32 NCHW against its transpose", hn, hf, where)
    _assert_equal("h' bf16 NCHW against rne(h' fp32)", hn16, hf.to(BF16), where)


def _gru_tap_wheres(k, tap):
    """One describe per output: u names the update gate, hr the reset gate, h' the candidate."""
    _, c, (b, h, w), _, _ = k["key"]
    maps = R.tap_channels(c, 3)

    def make(gate, second):
        def where(i):
            iy, ix = i[2] + tap[0] - 1, i[3] + tap[1] - 1
            ch = int(maps[gate][i[1]])
            src = "x" if ch < c else second
            return (f"{R.GRU_GATES[gate]} gate: tap (ky {tap[0]}, kx {tap[1]}) of pixel (image {i[0]}, row {i[2]}, column {i[3]}), channel {i[1]}, reads "
                    f"{src}[{ch % c}] at ({iy}, {ix}), {_borders(iy, ix, h, w)}")
        return where
    return make(0, "h (bf16 copy)"), make(1, "h (bf16 copy)"), make(2, "hr")


@gpu
@STATE
@pytest.mark.parametrize("c", R.WIDE_CHANNELS)
def test_convgru_one_tap(c, given):
    for tap in R.TAPS:
        k = R.build_case(("gru", c, GEOMETRY, given, tap))
        for tiles in TAP_GRU_TILES:
            _check_gru_saturated(f"convgru_step C{c} tiles {tiles} tap {tap}", k, _gru_device(*_gru_args(k), tiles), None, _gru_tap_wheres(k, tap))


# ---- ConvGRU16, one launch ------------------------------------------------------------------------------------------------------------------
def _gru16_device(x, h, hm, ws, bs):
    """-> (h' bf16, h' fp32, h' fp32 NCHW, h' bf16 NCHW), NCHW on the CPU."""
    ops = _ops()
    packed = ops.pack_gru16_weights(*(w.to(F32).cuda() for w in ws))
    b_gates, b_out = torch.cat(bs[:2]).to(F32).cuda(), bs[2].to(F32).cuda()
    xd, hd, md = _dev(x, BF16), _dev(h, BF16), _dev(hm, F32)
    _poison(xd.shape)
    hb, hf, hn = ops.convgru16_step(xd, hd, md, packed, b_gates, b_out, nchw_dtype=F32)
    second = ops.convgru16_step(xd, hd, md, packed, b_gates, b_out, nchw_dtype=BF16)
    torch.cuda.synchronize()
    assert torch.equal(second[0], hb) and torch.equal(second[1], hf), "the dtype of the NCHW copy changed the state"
    return _host(hb), _host(hf), hn.cpu(), second[2].cpu()


def _check_gru16_saturated(name, k, got, where):
    hb, hf, hn, hn16 = got
    want_h = k["want_h"]
    _assert_equal(f"{name}: h' fp32", hf, want_h, where)
    _assert_equal(f"{name}: h' bf16", hb, want_h.to(BF16), where)
    _assert_equal(f"{name}: h' fp32 NCHW", hn, want_h, where)
    _assert_equal(f"{name}: h' bf16 NCHW", hn16, want_h.to(BF16), where)


def _where16(geometry):
    b, h, w = geometry

    def where(i):
        edge = [n for n, on in (("top", i[2] == 0), ("bottom", i[2] == h - 1), ("left", i[3] == 0), ("right", i[3] == w - 1)) if on]
        return (f"image {i[0]} row {i[2]} column {i[3]} channel {i[1]}: pixel ({i[2] % 16}, {i[3] % 16}) of tile ({i[2] // 16}, {i[3] // 16}), "
                + ("on the image border: " + " ".join(edge) if edge else "inside the image"))
    return where


@gpu
@STATE
@pytest.mark.parametrize("shape", R.GRU16_SHAPES, ids=_shape_id)
def test_convgru16_saturated(shape, given):
    k = R.case(("gru16", 16, shape, given, None))
    where, name = _where16(shape), f"convgru16_step {_shape_id(shape)}"
    got = _gru16_device(*_gru_args(k))
    _check_gru16_saturated(name, k, got, where)
    if not given:
        zero = torch.zeros_like(k["x"])
        for what, a, b in zip(("h' bf16", "h' fp32", "h' fp32 NCHW", "h' bf16 NCHW"), got, _gru16_device(k["x"], zero, zero, k["ws"], k["bs"])):
            _assert_equal(f"{name}: {what}, None against an explicit zero state", a, b, where)


@gpu
@STATE
@pytest.mark.parametrize("shape", R.GRU16_SHAPES, ids=_shape_id)
def test_convgru16_real_valued(shape, given):
    """No hr comes out, so the reference cannot take the package's own.  The kernel's reset gate is held to the bar the update gate is held to
    everywhere, |r - r64| < TOL_SAME_OPERANDS; hr may then be any bf16 between rne(master (r64 - TOL)) and rne(master (r64 + TOL)) -- one value
    except near a rounding tie.  The candidate pre-activation is linear in hr, so it lies between p_min (every such hr at the end its weight's
    sign makes smaller) and p_max; tanh and the blend (u >= 0) are monotone, so h' lies in [h'(p_min), h'(p_max)], which is held to
    TOL_SAME_OPERANDS on both sides.  On the zero state hr = 0 and the interval is a point."""
    args, u, r = _gru_real(16, shape, given)
    x, _, hm, ws, bs = args
    hb, hf, hn, hn16 = _gru16_device(*args)
    hm = R._or_zeros(hm, x)
    a, b = R.bf16_round(hm * (r - TOL_SAME_OPERANDS)), R.bf16_round(hm * (r + TOL_SAME_OPERANDS))
    hr_lo, hr_hi = torch.minimum(a, b), torch.maximum(a, b)
    w_pos, w_neg, none = ws[2][:, 16:].clamp_min(0), ws[2][:, 16:].clamp_max(0), torch.zeros(16, dtype=F64)
    base = R.conv3x3(x, ws[2][:, :16].contiguous(), bs[2])
    p_min = base + R.conv3x3(hr_lo, w_pos, none) + R.conv3x3(hr_hi, w_neg, none)
    p_max = base + R.conv3x3(hr_hi, w_pos, none) + R.conv3x3(hr_lo, w_neg, none)
    h_min, h_max = hm * (1 - u) + torch.tanh(p_min) * u, hm * (1 - u) + torch.tanh(p_max) * u
    got = hf.to(F64)
    figures = {"h": _max(torch.maximum(h_min - got, got - h_max)), "open hr": int((hr_lo != hr_hi).sum()), "widest interval": _max(h_max - h_min)}
    print(f"convgru16_step {_shape_id(shape)} {'state' if given else 'zero state'}: {figures}")
    assert tuple(hf.shape) == (shape[0], 16) + tuple(shape[1:]) and bool(hf.isfinite().all())
    assert figures["h"] < TOL_SAME_OPERANDS, figures
    assert given or figures["open hr"] == 0
    where = _where16(shape)
    _assert_equal("h' bf16 against rne(h' fp32)", hb, hf.to(BF16), where)
    _assert_equal("h' fp32 NCHW against its transpose", hn, hf, where)
    _assert_equal("h' bf16 NCHW against rne(h' fp32)", hn16, hf.to(BF16), where)


@gpu
@STATE
def test_convgru16_one_tap(given):
    """h' alone comes out: a wrong update or reset tap shows through the blend and the candidate (the CPU file shows that the dense cases notice
    every mutant in h'); the message names the tap and what each of the three gates reads through it."""
    b, h, w = R.GRU16_TAP_SHAPE
    maps = R.tap_channels(16, 3)
    for tap in R.TAPS:
        k = R.build_case(("gru16", 16, R.GRU16_TAP_SHAPE, given, tap))
        tile = _where16(R.GRU16_TAP_SHAPE)

        def where(i, tap=tap):
            iy, ix = i[2] + tap[0] - 1, i[3] + tap[1] - 1
            reads = ", ".join(f"{name} <- {'x' if int(ci[i[1]]) < 16 else src}[{int(ci[i[1]]) % 16}]" for name, ci, src in zip(R.GRU_GATES, maps, ("h", "h", "hr")))
            return f"tap (ky {tap[0]}, kx {tap[1]}) reads input ({iy}, {ix}), {_borders(iy, ix, h, w)}; {reads}; {tile(i)}"
        _check_gru16_saturated(f"convgru16_step tap {tap}", k, _gru16_device(*_gru_args(k)), where)


# ---- once per family: batch independence, and the state updated in place between guards --------------------------------------------------------
def _assert_batch_independent(name, run, operands, names):
    """run(*operands) -> tuple of NCHW CPU tensors, on the whole batch and on each image alone: image i alone has the bits it has inside it."""
    whole = run(*operands)
    for i in range(operands[0].shape[0]):
        alone = run(*(None if t is None else t[i:i + 1] for t in operands))
        for what, a, b in zip(names, alone, whole):
            _assert_equal(f"{name}: {what}, image {i} alone against the same image inside the batch", a, b[i:i + 1])


@gpu
def test_convlstm_batch_independent():
    """60 pixels per image on the 128-pixel tile: inside the batch the images sit at other rows of other tiles than alone."""
    (x, h, c, weight, bias), _ = _lstm_real(128, (3, 6, 10), True)
    _assert_batch_independent("convlstm_step", lambda xi, hi, ci: _lstm_device(xi, hi, ci, weight, bias, 128), (x, h, c), ("h state", "c'", "h' fp32 NCHW", "h' bf16 NCHW"))


@gpu
def test_convgru_batch_independent():
    (x, hc, hm, ws, bs), _, _ = _gru_real(128, (3, 6, 10), True)
    _assert_batch_independent("convgru_step", lambda xi, hi, mi: _gru_device(xi, hi, mi, ws, bs, (2, 2)), (x, hc, hm), ("h' bf16", "h' fp32", "u", "hr", "h' fp32 NCHW", "h' bf16 NCHW"))


@gpu
def test_convgru16_batch_independent():
    (x, hc, hm, ws, bs), _, _ = _gru_real(16, (3, 19, 37), True)
    _assert_batch_independent("convgru16_step", lambda xi, hi, mi: _gru16_device(xi, hi, mi, ws, bs), (x, hc, hm), ("h' bf16", "h' fp32", "h' fp32 NCHW", "h' bf16 NCHW"))


SENTINEL, GUARD = 0x7FC12345, 64            # a NaN no arithmetic produces; 64 floats keep the view 256-byte aligned


def _guarded(state):
    """NCHW float64 state -> (buffer, view): the NHWC float32 state as a contiguous view inside a buffer of the sentinel bit pattern."""
    n = state.numel()
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(F32)
    b, c, h, w = state.shape
    view = buf[GUARD:GUARD + n].view(b, h, w, c)
    view.copy_(_dev(state, F32))
    return buf, view


def _assert_guards(name, buf):
    bits = buf.view(torch.int32).cpu()
    assert bool((bits[:GUARD] == SENTINEL).all()), f"{name}: wrote before the state"
    assert bool((bits[-GUARD:] == SENTINEL).all()), f"{name}: wrote past the state"


@gpu
def test_convlstm_in_place_between_guards():
    """c_out = c_prev, a view inside a larger buffer; 300 pixels on the 64-pixel tile: the last tile holds 44.  (convgru16_step takes no output
    buffer: it has no such case.)"""
    (x, h, c, weight, bias), _ = _lstm_real(64, GEOMETRY, True)
    want = _lstm_device(x, h, c, weight, bias, 64)
    ops = _ops()
    buf, view = _guarded(c)
    hs, cs, hn = ops.convlstm_step(_dev(x, BF16), _dev(h, BF16), view, ops.pack_gate_weights(weight.to(F32).cuda()), bias.to(F32).cuda(), tile_rows=64, c_out=view)
    torch.cuda.synchronize()
    assert cs.data_ptr() == view.data_ptr()
    for what, a, b in zip(("h state", "c'", "h' fp32 NCHW"), (_host(hs), _host(view), hn.cpu()), want):
        _assert_equal(f"convlstm_step in place: {what}", a, b, _where(GEOMETRY, 64))
    _assert_guards("convlstm_step", buf)


@gpu
def test_convgru_in_place_between_guards():
    """h_f32_out = h_prev_f32, a view inside a larger buffer; 300 pixels on the 64 x 128 gates and 128 x 64 candidate tiles."""
    (x, hc, hm, ws, bs), _, _ = _gru_real(64, GEOMETRY, True)
    want = _gru_device(x, hc, hm, ws, bs, (1, 1))
    ops = _ops()
    buf, view = _guarded(hm)
    packed = ops.pack_gru_weights(*(w.to(F32).cuda() for w in ws))
    got = ops.convgru_step(_dev(x, BF16), _dev(hc, BF16), view, packed, torch.cat(bs[:2]).to(F32).cuda(), bs[2].to(F32).cuda(), nchw_dtype=F32, tile_gates=1, tile_cand=1,
                           h_f32_out=view)
    torch.cuda.synchronize()
    assert got[1].data_ptr() == view.data_ptr()
    for what, a, b in zip(("h' bf16", "h' fp32", "u", "hr", "h' fp32 NCHW"), tuple(_host(t) for t in (got[0], view, got[2], got[3])) + (got[4].cpu(),), want):
        _assert_equal(f"convgru_step in place: {what}", a, b, _where(GEOMETRY, 64))
    _assert_guards("convgru_step", buf)
