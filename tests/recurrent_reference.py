"""float64 formulas of the three recurrent steps on the CPU, and the saturated cases tests/test_recurrent_ops.py runs on the device (both it
and tests/test_recurrent_reference.py build them through `case` below).

The formulas are the reference modules' (ConvLSTM model/submodules.py:179-235, ConvGRU :260-278) on NCHW float64 tensors:
    LSTM   i, r, o, g = conv3x3(cat(x, h)).chunk(4);  c' = sigmoid(r) c + sigmoid(i) tanh(g);  h' = sigmoid(o) tanh(c')
    GRU    u, r = sigmoid(conv3x3(cat(x, h)));  hr = rne_bf16(h_master r);  h' = h_master (1 - u) + tanh(conv3x3(cat(x, hr))) u
with the device kernels' operand contract: the convolutions read the bf16 copy of h, hr and the blend read the fp32 master, hr is rounded to
bf16 (the candidate convolution's operand).  h / c None is the zero state.

The *_saturated variants are the same steps in their exact regime.  Every pre-activation is a multiple of 128 with 128 <= |p| < 2^24
(asserted): an fp32 sigmoid is then exactly 0 or 1 and an fp32 tanh exactly +-1 (exp2 over- or underflows), and float64's sigmoid(-128) =
2.6e-56 is not -- hence hard gates, sigmoid -> (p > 0), tanh -> sign(p).  The step becomes routing: c' = [r] c + [i] sign(g) rounded to float32
once, h' = [o] tanh(c') which is exactly 0 / +-1 where o = 0 or |c'| >= 128 (the mask the LSTM variant returns), GRU h' = h_master or +-1.

Recipes of the saturated cases (`case`): x and the bf16 h operand integers in -3..3, weights integers in -2..2 times 256 (or, one tap: zero
except 256 at w[co, (7 co + 3 + 5 gate) mod 2C, ky, kx]), biases +-128.  Every sum is then a multiple of 256 below 2 C 9 3 512 <= 2^23 (exact in
fp32 in any order), every pre-activation an odd multiple of 128.  LSTM c: three quarters +-U(200, 1000), the rest N(0, 1), float32 values.  GRU
master: n + d, n in +-{1, 2, 3}, 2^-12 <= |d| <= 2^-10, float32 values, so rne_bf16(master) = n; the bf16 copy is INDEPENDENT integers in -3..3, not the
rounding of the master, so that which copy feeds what shows in the bits."""
import functools
import zlib

import torch
import torch.nn.functional as F

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LSTM_GATES, GRU_GATES = ("in", "remember", "out", "cell"), ("update", "reset", "candidate")


def bf16_round(t):
    """float64 -> the nearest bf16 value (through float32, as the kernels' operand is), as float64."""
    return t.to(F32).to(BF16).to(F64)


def conv3x3(x, w, b):
    return F.conv2d(x, w, b, padding=1)


def _or_zeros(t, like):
    return torch.zeros_like(like) if t is None else t


def lstm_preactivations(x, h, weight, bias):
    """[B, 4C, H, W]: in | remember | out | cell."""
    return conv3x3(torch.cat([x, _or_zeros(h, x)], 1), weight, bias)


def ref_lstm_step(x, h, c, weight, bias):
    """(h', c') in float64."""
    i, r, o, g = lstm_preactivations(x, h, weight, bias).chunk(4, 1)
    cell = torch.sigmoid(r) * _or_zeros(c, x) + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(cell), cell


def gru_gate_preactivations(x, h_copy, ws, bs):
    xh = torch.cat([x, _or_zeros(h_copy, x)], 1)
    return conv3x3(xh, ws[0], bs[0]), conv3x3(xh, ws[1], bs[1])


def ref_gru_step(x, h_copy, h_master, ws, bs, u=None, hr=None):
    """(h', u, hr) in float64; ws, bs = (update, reset, out).  u / hr given: the candidate and the blend on THOSE (a kernel's own workspaces)
    in place of the formulas' -- the returned u and hr are the formulas' either way."""
    pu, pr = gru_gate_preactivations(x, h_copy, ws, bs)
    hm = _or_zeros(h_master, x)
    want_u, want_hr = torch.sigmoid(pu), bf16_round(hm * torch.sigmoid(pr))
    uu, hh = (want_u if u is None else u), (want_hr if hr is None else hr)
    return hm * (1 - uu) + torch.tanh(conv3x3(torch.cat([x, hh], 1), ws[2], bs[2])) * uu, want_u, want_hr


def assert_saturated(name, p):
    a = p.abs()
    assert bool(((a >= 128) & (a < 2.0 ** 24) & (p % 128 == 0)).all()), f"{name}: pre-activations outside the saturated recipe (min |p| {float(a.min())}, max |p| {float(a.max())})"


def lstm_hard_f64(x, h, c, weight, bias):
    """(h', c', (i, r, o, g) as 0 / 1 / +-1) with hard gates, float64, NOT rounded to float32."""
    p = lstm_preactivations(x, h, weight, bias)
    assert_saturated("lstm", p)
    i, r, o, g = p.chunk(4, 1)
    gates = ((i > 0).to(F64), (r > 0).to(F64), (o > 0).to(F64), torch.sign(g))
    cell = gates[1] * _or_zeros(c, x) + gates[0] * gates[3]
    return gates[2] * torch.tanh(cell), cell, gates


def ref_lstm_step_saturated(x, h, c, weight, bias):
    """(h' float32, c' float32, exact): c' rounded to float32 once, h' = [o] tanh(c') on that float32 c'; exact = o == 0 or |c'| >= 128, where h' is
    exactly 0 / +-1."""
    _, cell, gates = lstm_hard_f64(x, h, c, weight, bias)
    cell = cell.to(F32)
    return (gates[2] * torch.tanh(cell.to(F64))).to(F32), cell, (gates[2] == 0) | (cell.abs() >= 128)


def gru_hard_f64(x, h_copy, h_master, ws, bs):
    """(h', u, hr) with hard gates, float64, NOT rounded to float32."""
    pu, pr = gru_gate_preactivations(x, h_copy, ws, bs)
    assert_saturated("gru update", pu)
    assert_saturated("gru reset", pr)
    hm = _or_zeros(h_master, x)
    u, hr = (pu > 0).to(F64), bf16_round(hm * (pr > 0).to(F64))
    po = conv3x3(torch.cat([x, hr], 1), ws[2], bs[2])
    assert_saturated("gru candidate", po)
    return hm * (1 - u) + torch.sign(po) * u, u, hr


def ref_gru_step_saturated(x, h_copy, h_master, ws, bs):
    """(h' float32, u float32, hr -- bf16 values as float64)."""
    h, u, hr = gru_hard_f64(x, h_copy, h_master, ws, bs)
    return h.to(F32), u.to(F32), hr


# ---- the saturated cases ----------------------------------------------------------------------------------------------------------------
GEOMETRY = (5, 6, 10)                       # 300 pixels: 4.7 tiles of 64, 2.3 of 128, 1.2 of 256
SMALLEST = ((1, 2, 2), (1, 1, 4))           # a 16 x 16 input at the deepest encoder; H = 1 (H W % 4 == 0 is the wide kernels' contract)
WIDE_CHANNELS = (64, 128, 256)
GRU16_SHAPES = ((1, 1, 1), (1, 1, 4), (2, 16, 16), (1, 17, 33), (3, 19, 37))
GRU16_TAP_SHAPE = (3, 19, 37)
TAPS = tuple((ky, kx) for ky in range(3) for kx in range(3))
# a key: (family, C, (B, H, W), state given, tap or None); a seed that misses a condition of tests/test_recurrent_reference.py is bumped here
SEED_BUMP = {}


def dense_keys():
    keys = [(f, c, g, given, None) for f in ("lstm", "gru") for c in WIDE_CHANNELS for g in (GEOMETRY,) + SMALLEST for given in (True, False)]
    return keys + [("gru16", 16, g, given, None) for g in GRU16_SHAPES for given in (True, False)]


def tap_keys():
    fams = [(f, c, GEOMETRY) for f in ("lstm", "gru") for c in WIDE_CHANNELS] + [("gru16", 16, GRU16_TAP_SHAPE)]
    return [(f, c, g, given, tap) for f, c, g in fams for given in (True, False) for tap in TAPS]


def tap_channels(c, n_gates):
    """ci[gate][co] = (7 co + 3 + 5 gate) mod 2C: the one input channel output channel co of `gate` reads."""
    return [(7 * torch.arange(c) + 3 + 5 * g) % (2 * c) for g in range(n_gates)]


def _ints(gen, k, *shape):
    return torch.randint(-k, k + 1, shape, generator=gen).to(F64)


def _signs(gen, *shape):
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).to(F64)


def _weights(gen, n_gates, c, tap):
    if tap is None:
        return [_ints(gen, 2, c, 2 * c, 3, 3) * 256 for _ in range(n_gates)]
    ws = [torch.zeros((c, 2 * c, 3, 3), dtype=F64) for _ in range(n_gates)]
    for w, ci in zip(ws, tap_channels(c, n_gates)):
        w[torch.arange(c), ci, tap[0], tap[1]] = 256.0
    return ws


def build_case(key):
    """The operands of one saturated case and its reference outputs, float64 NCHW on the CPU (want_*: the dtypes of the *_saturated formulas).
    h / c / master are generated for a zero-state case too (as `unused_*`: what a kernel must NOT read)."""
    family, c, (b, h, w), given, tap = key
    gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) + SEED_BUMP.get(key, 0))
    n_gates = 4 if family == "lstm" else 3
    shape = (b, c, h, w)
    out = {"key": key, "x": _ints(gen, 3, *shape)}
    hc = _ints(gen, 3, *shape)
    ws, bs = _weights(gen, n_gates, c, tap), [_signs(gen, c) * 128 for _ in range(n_gates)]
    if family == "lstm":
        big = _signs(gen, *shape) * (200 + 800 * torch.rand(shape, generator=gen))
        cp = torch.where(torch.rand(shape, generator=gen) < 0.75, big, torch.randn(shape, generator=gen).to(F64)).to(F32).to(F64)
        out.update(weight=torch.cat(ws), bias=torch.cat(bs), h=hc if given else None, c=cp if given else None, unused_h=hc, unused_c=cp)
        out["want_h"], out["want_c"], out["exact"] = ref_lstm_step_saturated(out["x"], out["h"], out["c"], out["weight"], out["bias"])
    else:
        n = _signs(gen, *shape) * torch.randint(1, 4, shape, generator=gen)
        hm = (n + _signs(gen, *shape) * (2.0 ** -12 + torch.rand(shape, generator=gen) * (2.0 ** -10 - 2.0 ** -12))).to(F32).to(F64)
        assert torch.equal(bf16_round(hm), n)
        out.update(ws=ws, bs=bs, h=hc if given else None, master=hm if given else None, unused_h=hc, unused_master=hm)
        out["want_h"], out["want_u"], out["want_hr"] = ref_gru_step_saturated(out["x"], out["h"], out["master"], ws, bs)
    return out


case = functools.lru_cache(maxsize=4)(build_case)       # the instances of one case follow one another in the GPU file's parameter lists
