"""tests/hyper_reference.py (the float64 formulas tests/test_hyper_ops.py holds the dynamic decoder's kernels to) against tests/hyper_stock.py,
which golden G26 pins to the reference: no GPU.

  * in float64 on unit-normal operands at the ragged size 2 x (9 x 17), roundings off: the formulas and the stock graph are the same
    real-number expressions, bound 1e-12 relative to the largest value (float64 summation order is all that differs)
  * against G26's context / atoms / output of the layer at float32 resolution: 1e-4, the bound of
    tests/test_hyper.py::test_stock_restatement_equals_the_reference_on_cpu
  * the seeded integer operands of the exact GPU cases satisfy what those cases rest on, on the reference alone
"""
import numpy as np
import pytest
import torch

import hyper_reference as R
from hyper_stock import _bn, _conv, err, g26 as load_g26, g26_layer_state, stock_atoms, stock_context, stock_dynconv
from seeded_weights import seeded_input

F64 = torch.float64
B, H, W = 2, 9, 17


def _close(name, got, want, tol=1e-12):
    assert got.shape == want.shape and got.dtype == want.dtype == F64, name
    scale = max(1.0, float(want.abs().max()))
    d = float((got - want).abs().max())
    assert d <= tol * scale, f"{name}: max |formula - stock| = {d:.3e} at max |stock| = {scale:.3e}"


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def test_context_formula_equals_bilinear_quarter_resampling():
    g = torch.Generator().manual_seed(1)
    for c in (1, 5, 7):
        ev, prev = torch.randn((B, c, 4 * H, 4 * W), generator=g, dtype=F64), torch.randn((B, 1, 4 * H, 4 * W), generator=g, dtype=F64)
        got = R.ref_context(ev, prev)
        want = torch.nn.functional.interpolate(torch.cat([ev, prev], 1), scale_factor=0.25, mode="bilinear", align_corners=False)
        _close(f"context C={c}", _nchw(got[..., :c + 1]).contiguous(), want)
        assert tuple(got.shape) == (B, H, W, 8) and float(got[..., c + 1:].abs().max() if c < 7 else 0.0) == 0.0
        # with its convolution: stock_context as a whole
        p = {"context_fusion.conv.weight": torch.randn((32, c + 1, 3, 3), generator=g, dtype=F64), "context_fusion.conv.bias": torch.randn((32,), generator=g, dtype=F64)}
        conv = R.ref_context_conv(got, p["context_fusion.conv.weight"], p["context_fusion.conv.bias"], round_weight=False)
        _close(f"context_conv Cin={c + 1}", _nchw(conv).contiguous(), stock_context(ev, prev, p))


def test_context_conv_formula_ignores_the_padding_channels_and_rounds_the_weight():
    g = torch.Generator().manual_seed(2)
    x8, w, b = torch.randn((B, H, W, 8), generator=g, dtype=F64), torch.randn((32, 6, 3, 3), generator=g, dtype=F64), torch.randn((32,), generator=g, dtype=F64)
    zeroed = x8.clone()
    zeroed[..., 6:] = 0.0
    assert torch.equal(R.ref_context_conv(x8, w, b), R.ref_context_conv(zeroed, w, b))
    assert torch.equal(R.ref_context_conv(x8, w, b), R.ref_context_conv(x8, w.to(torch.bfloat16).to(F64), b, round_weight=False))
    assert not torch.equal(R.ref_context_conv(x8, w, b), R.ref_context_conv(x8, w, b, round_weight=False))


def test_atoms_formula_equals_stock_atoms():
    """stock_atoms = tanh(bn(conv(tanh(bn(conv(ctx)))))) then its einsum with the bases; the formula takes the pre-activation of the last tanh."""
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(s, generator=g, dtype=F64)   # noqa: E731
    net = "dynamic_atom_generation.bases_net."
    p = {"dynamic_atom_generation.bases": rn(12, 25)}
    for i, (cin, cout) in ((0, (32, 64)), (3, (64, 72))):
        p[net + f"{i}.weight"], p[net + f"{i}.bias"] = rn(cout, cin, 3, 3) / (3 * cin ** 0.5), rn(cout)
        p[net + f"{i + 1}.weight"], p[net + f"{i + 1}.bias"] = 1 + 0.1 * rn(cout), rn(cout)
        p[net + f"{i + 1}.running_mean"], p[net + f"{i + 1}.running_var"] = rn(cout), 0.5 + torch.rand((cout,), generator=g, dtype=F64)
    ctx = rn(B, 32, H, W)
    want = stock_atoms(ctx, p)                                               # [B,6,25,h,w]
    pre = _bn(_conv(torch.tanh(_bn(_conv(ctx, p, net + "0"), p, net + "1")), p, net + "3"), p, net + "4")
    assert float(pre.abs().max()) > 1.0                                      # the tanh is not in its linear range only
    padded = torch.cat([pre.permute(0, 2, 3, 1), torch.full((B, H, W, 56), float("nan"), dtype=F64)], 3)
    got = R.ref_atoms(padded, p["dynamic_atom_generation.bases"])            # [B,h,w,25,6]; the NaN columns are never read
    _close("atoms", got.permute(0, 4, 3, 1, 2).contiguous(), want)


def test_dynconv_formula_equals_stock_dynconv_both_ways():
    g = torch.Generator().manual_seed(4)
    x, atoms = torch.randn((B, H, W, 256), generator=g, dtype=F64), torch.randn((B, H, W, 25, 6), generator=g, dtype=F64)
    p = {"dynamic_conv.compositional_coefficients": torch.randn((128, 1536, 1, 1), generator=g, dtype=F64), "dynamic_conv.bias": torch.randn((128,), generator=g, dtype=F64)}
    got = R.ref_dynconv(x, atoms, p["dynamic_conv.compositional_coefficients"], p["dynamic_conv.bias"], relu=False, round_features=False, round_weight=False)
    xs, at = _nchw(x).contiguous(), atoms.permute(0, 4, 3, 1, 2).contiguous()
    for unfold in (False, True):
        _close(f"dynconv unfold={unfold}", _nchw(got).contiguous(), stock_dynconv(xs, at, p, unfold=unfold))
    relu = R.ref_dynconv(x, atoms, p["dynamic_conv.compositional_coefficients"], p["dynamic_conv.bias"], relu=True, round_features=False, round_weight=False)
    assert torch.equal(relu, torch.relu(got)) and float(relu.min()) == 0.0
    # the roundings, switched on, are round-to-nearest-even of F and of W and nothing else
    f = R.ref_features(x, atoms, round_features=False)
    assert torch.equal(R.ref_features(x, atoms), f.to(torch.float32).to(torch.bfloat16).to(F64))
    w16 = p["dynamic_conv.compositional_coefficients"].to(torch.bfloat16).to(F64)
    assert torch.equal(R.ref_dynconv(x, atoms, w16, p["dynamic_conv.bias"], False, round_weight=False),
                       R.ref_dynconv(x, atoms, p["dynamic_conv.compositional_coefficients"], p["dynamic_conv.bias"], False))


def test_pack_formula_is_the_stated_permutation():
    w = torch.arange(128 * 1536, dtype=torch.int64).reshape(128, 1536)
    wp = R.ref_pack(w)
    assert tuple(wp.shape) == (128 * 1536,) and torch.equal(wp.sort().values, w.reshape(-1))
    g = np.random.Generator(np.random.PCG64(5))
    for cb, m, col, k in zip(g.integers(0, 4, 400), g.integers(0, 6, 400), g.integers(0, 128, 400), g.integers(0, 64, 400)):
        assert int(wp[((cb * 6 + m) * 128 + col) * 64 + k]) == int(w[col, (cb * 64 + k) * 6 + m])
    assert int(wp[0]) == 0 and int(wp[1]) == 6 and int(wp[64]) == 1536 and int(wp[128 * 64]) == 1 and int(wp[6 * 128 * 64]) == 64 * 6


def test_bf16_ulp():
    v = torch.tensor([1.0, 1.5, 0.999, 0.5, 256.0, 2.0 ** -126, 2.0 ** -130, 0.0], dtype=F64)
    want = [2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 2.0 ** -8, 2.0, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133]
    assert R.bf16_ulp(v).tolist() == want and R.bf16_ulp(-v).tolist() == want
    one = torch.tensor([1.0], dtype=torch.bfloat16)
    assert float(torch.nextafter(one, one + 1) - one) == 2.0 ** -7


def test_formulas_reproduce_the_golden_layer():
    """G26's DynamicUpsampleLayer (the reference's own float32 outputs) from the formulas alone, roundings off: 1e-4, as hyper_stock is held."""
    g26 = load_g26()
    p = {k: torch.from_numpy(np.asarray(v)).to(F64) if np.asarray(v).dtype.kind == "f" else torch.from_numpy(np.asarray(v)) for k, v in g26_layer_state(g26).items()}
    x, ev, prev = (torch.from_numpy(seeded_input(s, *sh)).to(F64) for s, sh in zip(g26["layer__x_seeds"], ((2, 256, 8, 8), (2, 5, 64, 64), (2, 1, 64, 64))))
    ctx = R.ref_context_conv(R.ref_context(ev, prev), p["context_fusion.conv.weight"], p["context_fusion.conv.bias"], round_weight=False)
    assert err(_nchw(ctx[:1]).numpy(), g26["layer__context"])[0] <= 1e-4
    net = "dynamic_atom_generation.bases_net."
    pre = _bn(_conv(torch.tanh(_bn(_conv(_nchw(ctx), p, net + "0"), p, net + "1")), p, net + "3"), p, net + "4")
    atoms = R.ref_atoms(pre.permute(0, 2, 3, 1), p["dynamic_atom_generation.bases"])
    assert err(atoms[:1].permute(0, 4, 3, 1, 2).numpy(), g26["layer__atoms"])[0] <= 1e-4
    up = torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    y = R.ref_dynconv(up.permute(0, 2, 3, 1), atoms, p["dynamic_conv.compositional_coefficients"], p["dynamic_conv.bias"], relu=True,
                      round_features=False, round_weight=False)
    assert err(_nchw(y).numpy(), g26["layer__y"])[0] <= 1e-4


# ---- the integer recipes of tests/test_hyper_ops.py --------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h,w", R.DYNCONV_SHAPES)
def test_dynconv_integer_recipe(b, h, w):
    x, atoms, wgt, bias, feat, y = R.dynconv_ints_case(b, h, w)
    for name, t, k in (("x", x, 1), ("atoms", atoms, 1), ("W", wgt, 1), ("bias", bias, 8)):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= k, name
    assert abs(float((x != 0).double().mean()) - 0.5) < 0.05 and abs(float((wgt != 0).double().mean()) - 1 / 8) < 0.01
    if (h, w) != (1, 1):
        assert abs(float((atoms != 0).double().mean()) - 2 / 15) < 0.03
    assert 0 < float(feat.abs().max()) <= 25 and torch.equal(feat, feat.round())
    peak, nonzero = float(y.abs().max()), float((y != 0).double().mean())
    print(f"dynconv integer recipe {b} x {h} x {w}: max |F| {float(feat.abs().max()):.0f}, max |y| {peak:.0f}, {nonzero:.1%} of y nonzero, {float((y > 0).double().mean()):.1%} positive")
    assert peak <= 256 and torch.equal(y, y.round()) and torch.equal(R.bf16_round(y), y)
    assert nonzero >= 0.25 and float((y > 0).double().mean()) > 0.1 and float((y < 0).double().mean()) > 0.1   # the ReLU acts, and not everywhere


def test_dynconv_rounding_recipe():
    x, atoms, wgt, bias, feat, y = R.dynconv_rounding_case()
    assert float(x.abs().max()) == 8 and float(atoms.abs().max()) == 4 and torch.equal(feat, feat.round())
    rounded = R.bf16_round(feat)
    share = float((rounded != feat).double().mean())
    tie = (feat.abs() > 256) & (feat.abs() < 512) & (feat.abs() % 2 == 1)                          # bf16 steps by 2 there: every odd integer is a tie
    up, down = int((tie & (rounded.abs() > feat.abs())).sum()), int((tie & (rounded.abs() < feat.abs())).sum())
    print(f"dynconv rounding recipe: max |F| {float(feat.abs().max()):.0f}, {share:.2%} of F change under the bf16 rounding, ties rounded up {up} / down {down}; "
          f"max |y| {float(y.abs().max()):.0f}")
    assert float(feat.abs().max()) > 256 and share >= 0.01 and float(y.abs().max()) < 2 ** 24 and torch.equal(y, y.round())
    assert up > 100 and down > 100 and float((feat > 0).double().mean()) > 0.3 and float((feat < 0).double().mean()) > 0.3
    assert float((x > 0).double().mean()) > 0.3 and float((x < 0).double().mean()) > 0.3
    assert float((R.bf16_round(y) != y).double().mean()) > 0.25                                   # the output's own rounding acts as well
    unrounded = R.ref_dynconv(x, atoms, wgt, bias, relu=False, round_features=False)
    assert float((R.bf16_round(unrounded) != R.bf16_round(y)).double().mean()) > 0.05             # skipping F's rounding would be seen


@pytest.mark.parametrize("cin,b,h,w", R.CONTEXT_CONV_CASES)
def test_context_conv_integer_recipe(cin, b, h, w):
    x8, wgt, bias, want = R.context_conv_ints_case(cin, b, h, w)
    assert (b * h * w * 4) % 256 != 0 and float(x8.abs().max()) <= 2 and float(wgt.abs().max()) <= 2 and float(bias.abs().max()) <= 4
    assert float(want.abs().max()) <= 256 and torch.equal(R.bf16_round(want), want) and float((want != 0).double().mean()) > 0.5
    if cin < 8:
        assert float(x8[..., cin:].abs().max()) > 0
