"""tests/recurrent_reference.py on the CPU: the float64 formulas against the three older restatements of the same modules, the hard-gate
formulas against the soft ones on every saturated case tests/test_recurrent_ops.py runs, what the saturated recipes rest on (asserted from the
reference alone), and mutants -- wrong steps a kernel could plausibly compute -- each of which must change at least one element of every
saturated case it applies to, so that torch.equal on the device would notice it."""
import pytest
import torch
import torch.nn.functional as F

import recurrent_reference as R
from recurrent_reference import F32, F64

DENSE, TAP = R.dense_keys(), R.tap_keys()


def _id(key):
    family, c, (b, h, w), given, tap = key
    return f"{family}-C{c}-{b}x{h}x{w}-{'state' if given else 'zero'}" + ("" if tap is None else f"-tap{tap[0]}{tap[1]}")


def _close(name, got, want, bound):
    err = float((got - want).abs().max())
    assert err <= bound, f"{name}: max |got - want| = {err:.3e} > {bound:.0e}"


# ---- agreement with the existing references ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 6, 10), (1, 128, 1, 4)])
def test_lstm_formula_equals_the_older_restatements(shape):
    from convgru_stock import stock_lstm
    from test_convlstm import _case, _ref_step
    x, h, c, weight, bias = (t.to(F64) for t in _case(*shape, seed=7))
    got_h, got_c = R.ref_lstm_step(x, h, c, weight, bias)
    for name, (want_h, want_c) in (("test_convlstm._ref_step", _ref_step(x, h, c, weight, bias, F64)),
                                   ("convgru_stock.stock_lstm", stock_lstm(x, (h, c), {"g.Gates.weight": weight, "g.Gates.bias": bias}, "g"))):
        _close(name + " h", got_h, want_h, 1e-12)
        _close(name + " c", got_c, want_c, 1e-12)
    zero = torch.zeros_like(x)
    for got, want in zip(R.ref_lstm_step(x, None, None, weight, bias), _ref_step(x, zero, zero, weight, bias, F64)):
        _close("zero state", got, want, 1e-12)


@pytest.mark.parametrize("shape", [(2, 64, 6, 10), (1, 128, 1, 4), (2, 16, 5, 7)])
def test_gru_formula_equals_the_older_restatements(shape):
    """test_firenet._ref_gru rounds hr as the formula here does; test_convgru._ref_gru and convgru_stock.stock_gru do not, so they are met
    with hr handed in unrounded (h * sigmoid(reset) on the formula's own gate pre-activations) and, rounding or not, on the zero state."""
    from convgru_stock import stock_gru
    from test_convgru import _case, _ref_gru
    from test_firenet import _ref_gru as ref_gru_rounding
    x, h, ws, bs = _case(*shape, seed=9)
    x, h, ws, bs = x.to(F64), h.to(F64), [w.to(F64) for w in ws], [b.to(F64) for b in bs]
    p = {f"g.{n}_gate.{k}": v for n, w, b in zip(("update", "reset", "out"), ws, bs) for k, v in (("weight", w), ("bias", b))}
    got_h, got_u, got_hr = R.ref_gru_step(x, h, h, ws, bs)
    want_h, want_hr = ref_gru_rounding(x, h, ws, bs, F64, round_hr=True)
    _close("test_firenet._ref_gru h", got_h, want_h, 1e-12)
    _close("test_firenet._ref_gru hr", got_hr, want_hr, 1e-12)
    _close("u", got_u, torch.sigmoid(R.conv3x3(torch.cat([x, h], 1), ws[0], bs[0])), 1e-12)
    unrounded = R.ref_gru_step(x, h, h, ws, bs, hr=h * torch.sigmoid(R.gru_gate_preactivations(x, h, ws, bs)[1]))[0]
    _close("test_convgru._ref_gru", unrounded, _ref_gru(x, h, ws, bs, F64), 1e-12)
    _close("convgru_stock.stock_gru", unrounded, stock_gru(x, h, p, "g"), 1e-12)
    zero = R.ref_gru_step(x, None, None, ws, bs)[0]
    _close("zero state, test_convgru._ref_gru", zero, _ref_gru(x, torch.zeros_like(x), ws, bs, F64), 1e-12)
    _close("zero state, convgru_stock.stock_gru", zero, stock_gru(x, None, p, "g"), 1e-12)
    # the copy feeds the convolutions, the master hr and the blend
    copy = R.bf16_round(h)
    mixed = R.ref_gru_step(x, copy, h, ws, bs)
    r = torch.sigmoid(R.conv3x3(torch.cat([x, copy], 1), ws[1], bs[1]))
    _close("hr on the master", mixed[2], R.bf16_round(h * r), 0.0)
    _close("blend on the master", mixed[0], h * (1 - mixed[1]) + torch.tanh(R.conv3x3(torch.cat([x, mixed[2]], 1), ws[2], bs[2])) * mixed[1], 1e-12)


# ---- hard against soft, and what the recipes rest on -------------------------------------------------------------------------------------
def _classes(key, classes):
    """Each class holds >= 10 % of the elements (at least one element below 1024 elements)."""
    for name, m in classes.items():
        share = float(m.to(F64).mean())
        assert int(m.sum()) >= 1 and (m.numel() < 1024 or share >= 0.1), f"{_id(key)}: class '{name}' holds {int(m.sum())} of {m.numel()} elements"
    return {n: round(float(m.to(F64).mean()), 3) for n, m in classes.items()}


@pytest.mark.parametrize("key", DENSE + TAP, ids=_id)
def test_saturated_case_rests_on_what_it_claims(key):
    """The pre-activations (the candidate's included) are multiples of 128 in [128, 2^24) -- asserted inside the hard formulas --, the hard
    formulas equal the soft ones to 1e-30 before the one rounding to float32, and (dense recipe, state given) every routing class is there."""
    k = R.build_case(key)
    family, _, _, given, tap = key
    if family == "lstm":
        args = (k["x"], k["h"], k["c"], k["weight"], k["bias"])
        hard_h, hard_c, gates = R.lstm_hard_f64(*args)
        soft_h, soft_c = R.ref_lstm_step(*args)
        _close("c'", hard_c, soft_c, 1e-30)
        _close("h'", hard_h, soft_h, 1e-30)
        assert torch.equal(k["want_c"], hard_c.to(F32)) and k["want_c"].dtype == F32 and k["want_h"].dtype == F32
        assert torch.equal(k["want_h"][k["exact"]], hard_h.to(F32)[k["exact"]])          # there h' does not depend on the rounding of c'
        assert bool(((k["want_h"].abs() == 1) | (k["want_h"] == 0))[k["exact"]].all())
        if given and tap is None:
            o, big = gates[2] == 1, k["want_c"].abs() >= 128
            print(_id(key), _classes(key, {"o = 0": ~o, "o = 1, |c'| >= 128": o & big, "o = 1, |c'| < 128": o & ~big}))
    else:
        args = (k["x"], k["h"], k["master"], k["ws"], k["bs"])
        hard, soft = R.gru_hard_f64(*args), R.ref_gru_step(*args)
        for name, a, b in zip(("h'", "u", "hr"), hard, soft):
            _close(name, a, b, 1e-30)
        assert torch.equal(k["want_h"].to(F64), hard[0]) and torch.equal(k["want_u"].to(F64), hard[1]) and torch.equal(k["want_hr"], hard[2])
        if tap is None:
            u, hr = k["want_u"] == 1, k["want_hr"] != 0
            classes = {"u = 0": ~u, "u = 1": u}
            if given:
                classes.update({"hr = 0": ~hr, "hr != 0": hr})
                assert torch.equal(k["want_h"][~u].to(F64), k["master"][~u]) and not bool((k["master"] == k["master"].round()).any())
            else:
                assert not bool(hr.any())
            print(_id(key), _classes(key, classes))


# ---- mutants -----------------------------------------------------------------------------------------------------------------------------
def _drop_last_pixels(outs):
    """The last 4 pixels of the tensor (NHWC order: of the last image) not written -- left at zero."""
    res = []
    for t in outs:
        t = t.clone()
        flat = t[-1].reshape(t.shape[1], -1)
        flat[:, -min(4, flat.shape[1]):] = 0
        res.append(t)
    return res


def _shift_centre_tap(w):
    """The centre tap reads one pixel to the right: its weights land on tap (1, 2)."""
    w = w.clone()
    w[:, :, 1, 2] += w[:, :, 1, 1]
    w[:, :, 1, 1] = 0
    return w


def _last_chunk(key):
    """Input channels of the last K chunk the kernel walks: 2C-64..2C-1 with state, C-64..C-1 on the zero state (K over x only); the 16-channel
    step has one chunk whose h half is dropped -- on the zero state that is no change."""
    family, c, _, given, _ = key
    if family == "gru16":
        return slice(16, 32) if given else None
    return slice(2 * c - 64, 2 * c) if given else slice(c - 64, c)


def _drop_chunk(w, chunk):
    w = w.clone()
    w[:, chunk] = 0
    return w


def _lstm_mutants(k):
    x, h, c, weight, bias = k["x"], k["h"], k["c"], k["weight"], k["bias"]
    given, f = k["key"][3], lambda *a: R.ref_lstm_step_saturated(*a)[:2]
    cc = weight.shape[0] // 4
    swap = torch.cat([torch.arange(cc, 2 * cc), torch.arange(cc), torch.arange(2 * cc, 4 * cc)])
    m = {"in / remember gates swapped": f(x, h, c, weight[swap], bias[swap]),
         "the last K chunk dropped": f(x, h, c, _drop_chunk(weight, _last_chunk(k["key"])), bias),
         "one tap shifted by one pixel": f(x, h, c, _shift_centre_tap(weight), bias),
         "the last 4 pixels not written": _drop_last_pixels((k["want_h"], k["want_c"]))}
    if not given:
        m["zero state that still reads h"] = f(x, k["unused_h"], None, weight, bias)
        m["zero state that still reads c"] = f(x, None, k["unused_c"], weight, bias)
    return m, (k["want_h"], k["want_c"])


def _gru_variant(x, hc, hm, ws, bs, cand="hr", hr_from="master", blend_from="master", ring=False):
    """The hard-gate GRU step with one wire moved.  ring: hr is not zero outside the image but what the nearest pixel inside holds (computed
    on a padded ring)."""
    hc, hm = R._or_zeros(hc, x), R._or_zeros(hm, x)
    pu, pr = R.gru_gate_preactivations(x, hc, ws, bs)
    u, r = (pu > 0).to(F64), (pr > 0).to(F64)
    hr = R.bf16_round((hm if hr_from == "master" else hc) * r)
    operand = hr if cand == "hr" else hc
    if ring:
        po = F.conv2d(torch.cat([F.pad(x, (1, 1, 1, 1)), F.pad(operand, (1, 1, 1, 1), mode="replicate")], 1), ws[2], bs[2])
    else:
        po = R.conv3x3(torch.cat([x, operand], 1), ws[2], bs[2])
    return ((hm if blend_from == "master" else hc) * (1 - u) + torch.sign(po) * u).to(F32), u.to(F32), hr


def _gru_mutants(k):
    x, h, hm, ws, bs = k["x"], k["h"], k["master"], k["ws"], k["bs"]
    given, f = k["key"][3], R.ref_gru_step_saturated
    want = (k["want_h"], k["want_u"], k["want_hr"])
    assert all(torch.equal(a, b) for a, b in zip(_gru_variant(x, h, hm, ws, bs), want))     # no wire moved: the reference itself
    m = {"update / reset gates swapped": f(x, h, hm, [ws[1], ws[0], ws[2]], [bs[1], bs[0], bs[2]]),
         "one tap shifted by one pixel (gates)": f(x, h, hm, [_shift_centre_tap(ws[0]), _shift_centre_tap(ws[1]), ws[2]], bs),
         "one tap shifted by one pixel (candidate)": f(x, h, hm, [ws[0], ws[1], _shift_centre_tap(ws[2])], bs),
         "the last 4 pixels not written": _drop_last_pixels(want[:1]) + list(want[1:])}
    chunk = _last_chunk(k["key"])
    if chunk is not None:
        m["the last K chunk dropped (gates)"] = f(x, h, hm, [_drop_chunk(ws[0], chunk), _drop_chunk(ws[1], chunk), ws[2]], bs)
        m["the last K chunk dropped (candidate)"] = f(x, h, hm, [ws[0], ws[1], _drop_chunk(ws[2], chunk)], bs)
    if given:
        m.update({"the candidate reads h in place of hr": _gru_variant(x, h, hm, ws, bs, cand="h"),
                  "hr from the bf16 copy": _gru_variant(x, h, hm, ws, bs, hr_from="copy"),
                  "the blend from the bf16 copy": _gru_variant(x, h, hm, ws, bs, blend_from="copy"),
                  "the convolutions read the master": f(x, R.bf16_round(hm), hm, ws, bs),
                  "hr not zero outside the image": _gru_variant(x, h, hm, ws, bs, ring=True)})
    else:
        m["zero state that still reads h in the convolutions"] = f(x, k["unused_h"], None, ws, bs)
        m["zero state that still reads the master"] = f(x, None, k["unused_master"], ws, bs)
    return m, want


@pytest.mark.parametrize("key", DENSE, ids=_id)
def test_every_mutant_changes_the_case(key):
    k = R.case(key)
    mutants, want = _lstm_mutants(k) if key[0] == "lstm" else _gru_mutants(k)
    missed = [name for name, got in mutants.items() if all(torch.equal(a.to(F64), b.to(F64)) for a, b in zip(got, want))]
    assert not missed, f"{_id(key)}: not noticed: {missed}"
    # the 16-channel step returns h' alone: there a mutant must show in h'
    if key[0] == "gru16":
        missed = [name for name, got in mutants.items() if torch.equal(got[0], want[0])]
        assert not missed, f"{_id(key)}: not noticed in h': {missed}"


def test_one_tap_weights_are_the_channel_map():
    """w[co, (7 co + 3 + 5 gate) mod 2C, ky, kx] = 256 and nothing else; the map reaches both halves of K for every gate."""
    for family, c in (("lstm", 64), ("gru", 128), ("gru16", 16)):
        geometry = R.GRU16_TAP_SHAPE if family == "gru16" else R.GEOMETRY
        k = R.build_case((family, c, geometry, True, (0, 2)))
        ws = list(k["weight"].chunk(4)) if family == "lstm" else k["ws"]
        for g, (w, ci) in enumerate(zip(ws, R.tap_channels(c, len(ws)))):
            assert int((w != 0).sum()) == c and bool((w[torch.arange(c), ci, 0, 2] == 256).all()) and torch.equal(ci, (7 * torch.arange(c) + 3 + 5 * g) % (2 * c))
            assert bool((ci < c).any()) and bool((ci >= c).any())
