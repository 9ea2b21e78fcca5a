"""tests/forward_reference.py on the CPU, two jobs.

1. Every formula against the stock PyTorch operator in float64, to 1e-12, at small ragged shapes (2 x 9 x 17; stride 2 at 11 x 19).
2. What the integer recipes of tests/test_forward_ops.py rest on, for EVERY parametrised case of that file, from the reference alone:
     * Q (sum |x| |w| + |bias| + |residual|) < 2^24, Q the quantum of the operands (4: biases k/4; 16: the upsampling weights k/16): every
       partial sum, in any order, is an integer multiple of 1/Q below 2^24 / Q, so fp32 accumulation is exact
     * >= 10 % of the outputs lie above 256 in magnitude or carry a fraction bf16 does not hold: the output rounding is exercised
     * >= 1 % of the outputs are exact ties between two bf16 values
     * with a skip, >= 5 % of x + skip does not fit bf16: the rounding of the sum shows; for resblock16 the two rounding conditions hold
       for the intermediate as well, and its rounding changes the output.
   A recipe that misses a condition at some shape is changed, never the condition.
"""
import pytest
import torch
import torch.nn.functional as F

import forward_reference as R
import test_forward_ops as T
from backward_reference import F64, bf16_round

TOL = 1e-12


def _rand(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def _close(got, want):
    assert got.shape == want.shape and float((got - want).abs().max()) < TOL * max(1.0, float(want.abs().max()))


# ---- 1. the formulas against stock PyTorch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks,stride,h,w", [(3, 1, 9, 17), (5, 1, 9, 17), (3, 2, 11, 19), (5, 2, 11, 19)])
@pytest.mark.parametrize("with_res,relu", [(False, False), (True, True), (True, False), (False, True)])
def test_conv_formula(ks, stride, h, w, with_res, relu):
    x, wt, bias = _rand(1, 2, 6, h, w), _rand(2, 7, 6, ks, ks), _rand(3, 7)
    res = _rand(4, 2, 7, (h - 1) // stride + 1, (w - 1) // stride + 1) if with_res else None
    want = F.conv2d(x, wt, bias, stride=stride, padding=ks // 2)
    want = want + res if with_res else want
    _close(R.ref_conv(x, wt, bias, stride, res, relu), torch.relu(want) if relu else want)


@pytest.mark.parametrize("cin", [1, 5, 8])
@pytest.mark.parametrize("ks,stride,h,w", [(3, 1, 9, 17), (5, 1, 9, 17), (3, 2, 11, 19)])
def test_pad8_conv_formula(cin, ks, stride, h, w):
    """The channels beyond Cin do not count, whatever they hold."""
    x8, wt, bias = _rand(5, 2, 8, h, w), _rand(6, 4, cin, ks, ks), _rand(7, 4)
    _close(R.ref_conv_pad8(x8, wt, bias, stride, True), torch.relu(F.conv2d(x8[:, :cin], wt, bias, stride=stride, padding=ks // 2)))
    assert torch.equal(R.pad8(wt)[:, :cin], wt) and float(R.pad8(wt)[:, cin:].abs().sum()) == 0.0


def test_resblock16_formula():
    """ResidualBlock (model/submodules.py:143-177, norm=None) with the intermediate rounded to bf16 where the kernel keeps it in bf16."""
    x, w1, b1, w2, b2 = _rand(8, 2, 16, 9, 17), _rand(9, 16, 16, 3, 3) * 0.1, _rand(10, 16), _rand(11, 16, 16, 3, 3) * 0.1, _rand(12, 16)
    mid, out = R.ref_resblock16(x, w1, b1, w2, b2)
    want_mid = torch.relu(F.conv2d(x, w1, b1, padding=1))
    _close(mid, want_mid)
    _close(out, torch.relu(F.conv2d(bf16_round(want_mid), w2, b2, padding=1) + x))


@pytest.mark.parametrize("shape", [(2, 3, 9, 17), (1, 2, 1, 1), (1, 2, 9, 1)])
def test_upsample_formulas(shape):
    x, skip = _rand(13, *shape), _rand(14, *shape)
    up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)  # noqa: E731
    _close(R.ref_upsample2x(x), up(x))
    _close(R.ref_upsample2x(x, skip), up(bf16_round(x + skip)))
    _close(R.ref_upsample2x_cat(x, skip[:, :1]), up(torch.cat([x, skip[:, :1]], 1)))
    _close(R.ref_upsample2x_cat(x), up(x))
    w9 = R.ref_upsample2x(torch.eye(2, dtype=F64).view(1, 1, 2, 2))                                              # the weights are 1/16 {9, 3, 3, 1}
    assert torch.equal(w9[0, 0, 1:3, 1:3] * 16, torch.tensor([[10.0, 6.0], [6.0, 10.0]], dtype=F64))


@pytest.mark.parametrize("cout", [1, 2, 3])
def test_conv1x1_formula(cout):
    x, skip, w, bias = _rand(15, 2, 8, 9, 17), _rand(16, 2, 8, 9, 17), _rand(17, cout, 8, 1, 1), _rand(18, cout)
    _close(R.ref_conv1x1(x, skip, w, bias), F.conv2d(bf16_round(x + skip), bf16_round(w), bias))
    _close(R.ref_conv1x1(x, None, w, bias), F.conv2d(x, bf16_round(w), bias))


def test_rounding_predicates():
    v = torch.tensor([0.0, 1.0, 255.0, 257.0, 258.0, 259.0, 300.0, 128.5, 64.25, 64.5, -513.0, -514.0, -512.0, 3.0e38], dtype=F64)
    assert R.ties(v).tolist() == [False, False, False, True, False, True, False, True, True, False, False, True, False, False]
    assert R.rounds(v).tolist() == [False, False, False, True, True, True, True, True, True, False, True, True, True, True]
    assert torch.equal(bf16_round(v[R.ties(v)]), torch.tensor([256.0, 260.0, 128.0, 64.0, -512.0], dtype=F64))  # ties go to the even neighbour


# ---- 2. what the integer recipes rest on ----------------------------------------------------------------------------------------------------
def _check_exact(abs_sum, quantum):
    peak = float(abs_sum.max()) * quantum
    assert peak < 2 ** 24, f"sum of magnitudes x {quantum} reaches {peak}: fp32 accumulation is not exact in every order"


def _check_rounding(name, v):
    """v: the unrounded value of a bf16 output."""
    n, r, t = v.numel(), int(R.rounds(v).sum()), int(R.ties(v).sum())
    print(f"{name}: {n} outputs, {100.0 * r / n:.1f} % above 256 or with a fraction bf16 does not hold, {100.0 * t / n:.1f} % ties, max |v| {float(v.abs().max())}")
    assert r >= 0.10 * n, f"{name}: only {r} of {n} outputs exercise the rounding"
    assert t >= 0.01 * n, f"{name}: only {t} of {n} outputs are ties"


def _check_skip(x, skip):
    """Two integers in -200..200 add up to an odd number above 256 in magnitude -- the sums bf16 does not hold -- 6.5 % of the time: at least
    one element in twenty must be such a sum."""
    s = x + skip
    n, r = s.numel(), int((bf16_round(s) != s).sum())
    print(f"x + skip: {r} of {n} sums do not fit bf16, max |x + skip| {float(s.abs().max())}")
    assert r >= 0.05 * n, f"only {r} of {n} skip sums are rounded"


@pytest.mark.parametrize("case", T.CONV, ids=T.CONV_IDS)
def test_conv_recipe(case):
    x, w, bias, res, want = T.conv_integer_case(case)
    assert torch.equal(bf16_round(x), x) and torch.equal(bf16_round(w), w) and (res is None or torch.equal(bf16_round(res), res))
    _check_exact(R.abs_sum_conv(x, w, bias, case[3], res), 4)
    _check_rounding("conv_nhwc", want)


@pytest.mark.parametrize("case", T.PAD8, ids=T.PAD8_IDS)
def test_pad8_conv_recipe(case):
    x8, w, bias, want = T.pad8_integer_case(case)
    assert torch.equal(bf16_round(x8), x8) and torch.equal(bf16_round(w), w)
    if case[1] < 8:
        assert float(x8[:, case[1]:].abs().max()) > 0                                                             # the padded channels are filled
    _check_exact(R.abs_sum_conv(x8, R.pad8(w), bias, case[3]), 4)
    _check_rounding(case[0], want)


@pytest.mark.parametrize("shape", T.NARROW_SHAPES)
def test_resblock16_recipe(shape):
    x, w1, b1, w2, b2, mid, want = T.resblock16_integer_case(shape)
    _check_exact(R.abs_sum_conv(x, w1, b1), 4)
    _check_exact(R.abs_sum_conv(bf16_round(mid), w2, b2, 1, x), 4)
    _check_rounding("resblock16 mid", mid)
    _check_rounding("resblock16 out", want)
    assert not torch.equal(want.to(torch.bfloat16), R.ref_conv(mid, w2, b2, residual=x, relu=True).to(torch.bfloat16))   # the rounding of mid reaches the output


@pytest.mark.parametrize("case", T.UPSAMPLE)
def test_upsample_recipe(case):
    x, skip, want = T.upsample_integer_case(case)
    _check_exact(R.ref_upsample2x(R.skip_sum(x, skip).abs()), 16)
    if skip is not None:
        _check_skip(x, skip)
    if case[1:3] != (1, 1):                                                                                        # 1 x 1: the output is the input, four times
        _check_rounding("upsample2x", want)


@pytest.mark.parametrize("case", T.UPSAMPLE_CAT)
def test_upsample_cat_recipe(case):
    x, skip, want = T.upsample_cat_integer_case(case)
    _check_exact(R.ref_upsample2x_cat(x.abs(), None if skip is None else skip.abs()), 16)
    _check_rounding("upsample2x_cat", want)


@pytest.mark.parametrize("case", T.CONV1X1, ids=T.CONV1X1_IDS)
def test_conv1x1_recipe(case):
    x, skip, w, bias, want = T.conv1x1_integer_case(case)
    _check_exact(R.ref_conv1x1(R.skip_sum(x, skip).abs(), None, w.abs(), bias.abs()), 4)
    if skip is not None:
        _check_skip(x, skip)
    if case[4] == "bf16":
        _check_rounding("conv1x1", want)
