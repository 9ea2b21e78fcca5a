"""The six kernels of HyperE2VID's dynamic decoder (v2v_amd/csrc/v2v_hyper.hpp) one by one, through their raw operators in v2v_amd/nhwc_ops.py,
against the float64 formulas of tests/hyper_reference.py (themselves held to tests/hyper_stock.py and golden G26 on the CPU by
tests/test_hyper_reference.py).  tests/test_hyper.py checks the layer and the network as a whole, under bars a wrong border row or a swapped
pair of atoms passes; here one wrong element fails.

Bit-exact wherever the arithmetic allows: small-integer operands (exact in bf16) make every product and partial sum an integer below 2^24
(a multiple of 1/4 for the context's 2 x 2 mean), so float32 accumulation is exact in ANY order and the output is the reference, or its one
round-to-nearest-even to bf16 -- torch.equal, no tolerance.  The conditions this rests on are asserted on the reference, here and on the CPU.

Numeric bounds in this file (there are no others), all the project's own:
  * 2^-8:  |got - want| / (|want| + 1) on real-valued operands, bf16 outputs, against float64 on the same rounded operands (tests/test_convlstm.py,
    tests/test_backward_ops.py); for the context's resampling |got - want| / (|want| + 2^-6), the form of test_upsample2x_matches_interpolate
  * TOL_SAME_OPERANDS = 2e-5 absolute per hardware exp2 / rcp activation (tests/test_convlstm.py): on top of the output's half bf16 ulp for
    tanh_bf16_, times sum_k |bases[k, l]| for the atoms (an error of 2e-5 in each of the 12 tanh values, weighted as the sum weights them)
  * 3e-2 max / 6e-3 rms x max(1, |y|max) for the composed layer: the bar of tests/test_hyper.py::test_dynamic_layer_vs_reference, unchanged
Every test with a bound prints its figures before it asserts; DESIGN 4.12 records them.
"""
import functools

import numpy as np
import pytest
import torch

import hyper_reference as R
from hyper_stock import err, g26 as load_g26, g26_layer_state, stock_layer
from seeded_weights import seeded_input
from test_backward_ops import _assert_equal, _assert_rounding
from test_convlstm import TOL_SAME_OPERANDS

gpu = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
RELU = [False, True]
SHAPE_IDS = [f"{b}x{h}x{w}" for b, h, w in R.DYNCONV_SHAPES]


def _ops():
    from v2v_amd import nhwc_ops
    return nhwc_ops


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 412)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- hyper_context_nhwc8 ---------------------------------------------------------------------------------------------------------------
# (C, B, H, W): B h w = 3, 30, 297 work-items, never a multiple of the 256-wide block; the last is more than one block
CONTEXT_CASES = [(c, b, h, w) for c in (1, 5, 7) for b, h, w in ((3, 4, 4), (2, 12, 20), (3, 36, 44))]
LAYOUTS = ("contiguous", "channels_last", "strided_view")


def _laid_out(ev, layout):
    """The float32 events on the device in one of the three layouts the operator takes (same values, other strides)."""
    ev = ev.to(F32).cuda()
    if layout == "channels_last":
        return ev.contiguous(memory_format=torch.channels_last)
    if layout == "strided_view":                                             # a window of a larger tensor, in H and in W
        b, c, h, w = ev.shape
        big = torch.full((b, c, h + 3, w + 5), 99.0, dtype=F32, device="cuda")
        big[:, :, 2:2 + h, 1:1 + w] = ev
        view = big[:, :, 2:2 + h, 1:1 + w]
        assert not view.is_contiguous() and view.stride(2) == w + 5
        return view
    return ev


@gpu
@pytest.mark.parametrize("c,b,h,w", CONTEXT_CASES)
def test_context_exact_on_integers_in_every_layout(c, b, h, w):
    """Integers in -8..8: the 2 x 2 mean is a multiple of 1/4 of magnitude <= 8, at most 6 significant bits -- exact in float32 and in bf16."""
    ops = _ops()
    g = _gen(c, b, h, w)
    ev, prev = torch.randint(-8, 9, (b, c, h, w), generator=g).to(F64), torch.randint(-8, 9, (b, 1, h, w), generator=g).to(F64)
    want64 = R.ref_context(ev, prev)
    want = want64.to(BF16)
    assert (b * (h // 4) * (w // 4)) % 256 != 0 and torch.equal(want.to(F64), want64) and float((want64[..., :c + 1] != 0).double().mean()) > 0.5
    for layout in LAYOUTS:
        got = ops.hyper_context_nhwc8(_laid_out(ev, layout), prev.to(F32).cuda()).cpu()
        _assert_equal(f"context [{layout}]", got, want, lambda i: f"(image, y, x, channel) of the 1/4-scale output; C = {c}")
        assert int(_bits(got[..., c + 1:]).ne(0).sum()) == 0, f"padding channels {c + 1}..7 are not +0 [{layout}]"


@gpu
@pytest.mark.parametrize("c,b,h,w", CONTEXT_CASES)
def test_context_within_one_ulp_on_normal_values(c, b, h, w):
    ops = _ops()
    g = _gen(c, b, h, w, 1)
    ev, prev = torch.randn((b, c, h, w), generator=g), torch.randn((b, 1, h, w), generator=g)
    want = R.ref_context(ev, prev)
    worst = 0.0
    for layout in LAYOUTS:
        got = ops.hyper_context_nhwc8(_laid_out(ev, layout), prev.cuda()).cpu()
        worst = max(worst, float(((got.to(F64) - want).abs() / (want.abs() + 2.0 ** -6)).max()))
        assert int(_bits(got[..., c + 1:]).ne(0).sum()) == 0
    print(f"context C={c} {b} x {h} x {w}: max |got - want| / (|want| + 2^-6) = {worst:.3e} (bound 2^-8 = {2.0 ** -8:.3e})")
    assert worst < 2.0 ** -8


# ---- context_conv_nhwc -----------------------------------------------------------------------------------------------------------------
def _context_conv(ops, x8, wgt, bias):
    return ops.context_conv_nhwc(x8.to(BF16).cuda(), wgt.to(F32).cuda(), bias.to(F32).cuda()).cpu()


@gpu
@pytest.mark.parametrize("cin,b,h,w", R.CONTEXT_CONV_CASES)
def test_context_conv_exact_on_integers(cin, b, h, w):
    """x and weight in -2..2, bias in -4..4: 72 products of magnitude <= 4 -- every sum an integer <= 292, asserted <= 256: bf16 holds it."""
    x8, wgt, bias, want = R.context_conv_ints_case(cin, b, h, w)
    assert (b * h * w * 4) % 256 != 0 and float(want.abs().max()) <= 256
    _assert_equal("context_conv", _context_conv(_ops(), x8, wgt, bias), want.to(BF16), lambda i: f"(image, y, x, output channel); Cin = {cin}")


def _border(y, x, h, w):
    out = [n for n, c in (("top", y < 0), ("bottom", y >= h), ("left", x < 0), ("right", x >= w)) if c]
    return "outside the image: " + " ".join(out) if out else "inside the image"


@gpu
def test_context_conv_one_hot_taps_at_corners_edges_and_centre():
    """One input pixel (corner, edge midpoint, centre; alternating images) times one weight tap: the output is the impulse shifted against the
    tap's offset, plus bias -- or bias alone where the shift leaves the image."""
    ops = _ops()
    b, h, w, cin, ci = 2, 5, 7, 6, 4
    wcol = torch.arange(32, dtype=F64) - 13                                   # a distinct weight per output channel
    bias = torch.randint(-4, 5, (32,), generator=_gen(9)).to(F64)
    pixels = [(y, x) for y in (0, h // 2, h - 1) for x in (0, w // 2, w - 1)]
    for n, (qy, qx) in enumerate(pixels):
        bq = n % b
        x8 = torch.zeros((b, h, w, 8), dtype=F64)
        x8[bq, qy, qx, ci] = 1.0
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            wgt = torch.zeros((32, cin, 3, 3), dtype=F64)
            wgt[:, ci, ky, kx] = wcol
            want = bias.view(1, 1, 1, 32).repeat(b, h, w, 1)
            py, px = qy - (ky - 1), qx - (kx - 1)                             # out[p] reads x[p + (ky - 1, kx - 1)]
            where = _border(py, px, h, w)
            if where == "inside the image":
                want[bq, py, px] += wcol
            got = _context_conv(ops, x8, wgt, bias)
            _assert_equal(f"context_conv one-hot: input pixel ({qy},{qx}) of image {bq}, tap (ky {ky}, kx {kx}), shifted impulse at ({py},{px}) {where}",
                          got, want.to(BF16))


@gpu
@pytest.mark.parametrize("cin,b,h,w", R.CONTEXT_CONV_CASES)
def test_context_conv_rounding_on_normal_operands(cin, b, h, w):
    g = _gen(cin, b, h, w, 2)
    x8 = torch.randn((b, h, w, 8), generator=g).to(BF16).to(F64)
    wgt = torch.randn((32, cin, 3, 3), generator=g).to(F64) * (3.0 / (cin * 9) ** 0.5)          # float32 values: the kernel rounds them to bf16 itself
    bias = torch.randn((32,), generator=g).to(F64)
    _assert_rounding(f"context_conv Cin={cin} {b} x {h} x {w}", _context_conv(_ops(), x8, wgt, bias), R.ref_context_conv(x8, wgt, bias))


# ---- tanh_bf16_ ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_tanh_over_all_bf16_bit_patterns():
    """All 65,536 inputs.  The kernel is 2 rcp(1 + exp2(-2 log2(e) x)) - 1 in float32: the hardware exp2 / rcp error is absolute in the result
    (the form cancels near 0), so the bound is the output's half bf16 ulp plus TOL_SAME_OPERANDS.  Measured on an MI355X: at most 8.9e-8 beyond the half ulp (at x = -8.9e-8); 28,160
    of the 65,280 finite inputs are one ulp off the nearest bf16; DESIGN 4.12."""
    ops = _ops()
    bits = torch.arange(65536, dtype=torch.int32)
    x = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(BF16)
    dev = x.clone().cuda()
    out = ops.tanh_bf16_(dev)
    assert out.data_ptr() == dev.data_ptr()                                   # in place
    got = out.cpu()
    nan, inf = x.isnan(), x.isinf()
    assert int(nan.sum()) == 2 * 127 and int(inf.sum()) == 2
    assert torch.equal(got.isnan(), nan), "NaN in <-> NaN out"
    assert torch.equal(got[inf].float(), torch.sign(x[inf].float())), "tanh(+-inf) must be +-1 exactly"
    fin = ~nan & ~inf
    x64 = x[fin].to(F64)
    want = torch.tanh(x64)
    excess = (got[fin].to(F64) - want).abs() - 0.5 * R.bf16_ulp(want)
    at = int(excess.argmax())
    print(f"tanh_bf16_: largest |got - tanh64(x)| beyond half a bf16 ulp of |want|: {float(excess.max()):.3e} at x = {float(x64[at])} "
          f"(bound {TOL_SAME_OPERANDS:.1e}); {int((excess > 0).sum())} of {int(fin.sum())} finite inputs are not the nearest bf16")
    assert float(excess.max()) <= TOL_SAME_OPERANDS
    # one work-item, one partial block, one whole block and a partial one: the same values as in the full run
    start = 0x3E00                                                            # 0.125 .. : away from the saturated range
    for n in (8, 264, 2056):
        part = ops.tanh_bf16_(x[start:start + n].clone().cuda()).cpu()
        assert torch.equal(_bits(part), _bits(got[start:start + n])), n


# ---- hyper_atoms -----------------------------------------------------------------------------------------------------------------------
ATOM_COUNTS = [1, 43, 300]                                                    # M * 6 work-items: 6, 258, 1800 -- never whole blocks


@gpu
@pytest.mark.parametrize("m", ATOM_COUNTS)
def test_atoms_exact_on_saturated_coefficients(m):
    """Coefficients +-64 (exact in bf16): the kernel's tanh is exactly +-1 there (exp2 -> 0 or inf, rcp -> 1 or 0; it holds on an MI355X), as float64's is; integer
    bases in -3..3 make every sum an integer <= 36.  Columns 72..127 of the padded coefficient rows hold NaN: reading one poisons the sum."""
    g = _gen(m, 3)
    coeff = (torch.randint(0, 2, (1, 1, m, R.COEFF_PAD), generator=g).to(F64) * 128 - 64)
    coeff[..., R.N_COEFF:] = float("nan")
    bases = torch.randint(-3, 4, (R.N_BASES, R.N_TAPS), generator=g).to(F64)
    want = R.ref_atoms(coeff, bases)
    assert not bool(want.isnan().any()) and torch.equal(want, want.round()) and float((want != 0).double().mean()) > 0.5
    got = _ops().hyper_atoms(coeff.to(BF16).cuda(), bases.to(F32).cuda()).cpu()
    _assert_equal("atoms", got, want.to(F32), lambda i: f"(.., pixel, tap l, atom m) of {m} pixels")


@gpu
@pytest.mark.parametrize("m", ATOM_COUNTS)
def test_atoms_on_normal_coefficients_and_the_fourier_bessel_bases(m):
    """Coefficients N(0, 1.5) clamped to +-3, bf16; G26's Fourier-Bessel bases.  Measured on an MI355X: max |got - want| 4.3e-7, 0.007 of the bound."""
    g = _gen(m, 4)
    coeff = torch.zeros((1, m, 1, R.COEFF_PAD), dtype=BF16)
    coeff[..., :R.N_COEFF] = torch.randn((1, m, 1, R.N_COEFF), generator=g).mul(1.5).clamp(-3, 3).to(BF16)
    bases = torch.from_numpy(np.asarray(load_g26()["bases"], dtype=np.float32))
    want = R.ref_atoms(coeff.to(F64), bases.to(F64))
    bound = TOL_SAME_OPERANDS * bases.to(F64).abs().sum(0).view(1, 1, 1, R.N_TAPS, 1)
    got = _ops().hyper_atoms(coeff.cuda(), bases.cuda()).cpu()
    diff = (got.to(F64) - want).abs()
    inner = bound.squeeze() > 0
    print(f"atoms, {m} pixels: max |got - want| = {float(diff.max()):.3e}, at most {float((diff / bound.clamp_min(1e-300))[..., inner, :].max()):.3f} of the bound "
          f"2e-5 sum_k |bases[k, l]| (sum_k |bases| up to {float(bound.max() / TOL_SAME_OPERANDS):.2f}; {int((~inner).sum())} taps have all-zero bases: exact zeros)")
    assert got.dtype == F32 and bool((diff <= bound).all())


# ---- pack_dynconv_weights --------------------------------------------------------------------------------------------------------------
@gpu
def test_pack_is_the_stated_permutation_of_the_rne_weights():
    g = _gen(6)
    w = torch.randn((R.COUT, R.CIN * R.N_ATOMS), generator=g)
    w[0, 0], w[0, 1], w[0, 2], w[127, 1535] = float("nan"), float("inf"), float("-inf"), -0.0
    # ties: 1 + 2^-8 -> 1 (even), 1 + 3 2^-8 -> 1 + 2^-6 (even), just above a tie -> up, the negative tie
    w[1, :4] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -(1 + 2.0 ** -8)])
    assert w[1, :4].to(BF16).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -1.0]
    want = R.ref_pack(w.to(BF16))
    got = _ops().pack_dynconv_weights(w.view(R.COUT, -1, 1, 1).cuda()).cpu()
    nan = want.isnan()
    assert got.dtype == BF16 and got.shape == want.shape and int(nan.sum()) == 1 and torch.equal(got.isnan(), nan)
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])                   # bits: infinities, the sign of -0, ties to even


# ---- dynconv_nhwc ----------------------------------------------------------------------------------------------------------------------
def _dynconv(ops, x, atoms, packed, bias, relu):
    """NHWC float64 operands on the CPU (packed / bias: already on the device) -> the kernel's bf16 NHWC output on the CPU."""
    return ops.dynconv_nhwc(x.to(BF16).cuda(), atoms.to(F32).cuda(), packed, bias, relu=relu).cpu()


def _pack(wgt, bias):
    return _ops().pack_dynconv_weights(wgt.to(F32).view(R.COUT, -1, 1, 1).cuda()), bias.to(F32).cuda()


@functools.lru_cache(maxsize=None)
def _packed_ints():
    return _pack(*R.dynconv_weight_ints())


def _want(y, relu):
    """The kernel's contract on the float64 pre-activation y: ReLU, then one round-to-nearest-even to bf16."""
    return (torch.clamp_min(y, 0.0) if relu else y).to(F32).to(BF16)


def _pixel(i):
    return f"(image {i[0]}, row {i[1]}, column {i[2]}: tile row {i[1] // 8} / column {i[2] // 16}, in-tile ({i[1] % 8},{i[2] % 16})), output channel {i[3]}"


@gpu
@pytest.mark.parametrize("relu", RELU)
@pytest.mark.parametrize("b,h,w", R.DYNCONV_SHAPES, ids=SHAPE_IDS)
def test_dynconv_exact_on_integers(b, h, w, relu):
    x, atoms, wgt, bias, feat, y = R.dynconv_ints_case(b, h, w)
    assert float(y.abs().max()) <= 256 and float((y != 0).double().mean()) >= 0.25 and float(feat.abs().max()) > 0
    got = _dynconv(_ops(), x, atoms, *_packed_ints(), relu)
    _assert_equal(f"dynconv {b} x {h} x {w} relu={relu}", got, _want(y, relu), _pixel)


@gpu
@pytest.mark.parametrize("relu", RELU)
def test_dynconv_rounds_the_features_to_nearest_even(relu):
    """|F| up to 428: integers bf16 does not hold.  The reference rounds F to bf16 (RNE) and the integer result once more; equality pins
    that F is rounded to nearest-even before the matrix cores, and nothing else is."""
    x, atoms, wgt, bias, feat, y = R.dynconv_rounding_case()
    assert float((R.bf16_round(feat) != feat).double().mean()) >= 0.01 and float(y.abs().max()) < 2 ** 24
    got = _dynconv(_ops(), x, atoms, *_packed_ints(), relu)
    _assert_equal(f"dynconv F rounding relu={relu}", got, _want(y, relu), _pixel)


@functools.lru_cache(maxsize=None)
def _onehot_weights():
    """W[o, j] = ((7 o + 19 j) mod 257) - 128: distinct over the 128 output channels of every column j, another set for every (c, m);
    integers of magnitude <= 128, bias in -8..8: bf16 holds every expected output."""
    o, j = torch.arange(R.COUT).view(-1, 1), torch.arange(R.CIN * R.N_ATOMS).view(1, -1)
    wgt = (((7 * o + 19 * j) % 257) - 128).to(F64)
    bias = R.dynconv_weight_ints()[1]
    return (wgt, bias) + _pack(wgt, bias)


ONEHOT_CHANNELS = (0, 7, 8, 63, 64, 135, 255)                                 # each 64-channel K block, both 8-channel halves of a k-step
SEAM_PIXELS = ((7, 15), (7, 16), (8, 15), (8, 16))                            # the four pixels around the first tile corner


@gpu
@pytest.mark.parametrize("b,h,w", R.DYNCONV_SHAPES, ids=SHAPE_IDS)
def test_dynconv_one_hot_input_tap_and_atom(b, h, w):
    """x is 1 at one pixel q (the image corners, alternating images; the tile-seam pixels where the image has them) and one channel c.  The
    atoms of every pixel p are one-hot at a tap l(p) and an atom m(p): within the 5 x 5 neighbourhood of q, l(p) is THE tap that makes p read
    q, so every neighbour that lies inside the image must output W[:, c * 6 + m(p)] + bias and every other pixel of the batch bias alone.
    Over the corners (and at once around a seam pixel) l takes all 25 taps, over the 7 channels m(p) takes all 6 atoms at every pixel."""
    ops = _ops()
    wgt, bias, packed, bias_dev = _onehot_weights()
    corners = list(dict.fromkeys([(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]))
    pixels = corners + [q for q in SEAM_PIXELS if (b, h, w) in ((1, 9, 17), (2, 12, 20))]
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    x_dev = torch.zeros((b, h, w, R.CIN), dtype=BF16, device="cuda")
    taps, atoms_seen, launches = set(), set(), 0
    for qi, (qy, qx) in enumerate(pixels):
        bq = qi % b
        near = ((qy - yy).abs() <= 2) & ((qx - xx).abs() <= 2)
        l = torch.where(near, (qy - yy + 2) * 5 + (qx - xx + 2), (3 * yy + 7 * xx + 1) % R.N_TAPS)
        for ci, c in enumerate(ONEHOT_CHANNELS):
            relu = bool((qi + ci) % 2)
            m = (yy * w + xx + ci) % R.N_ATOMS
            atoms = torch.zeros((h * w, R.N_TAPS * R.N_ATOMS), dtype=F32)
            atoms[torch.arange(h * w), (l * R.N_ATOMS + m).reshape(-1)] = 1.0
            atoms = atoms.view(1, h, w, R.N_TAPS, R.N_ATOMS).repeat(b, 1, 1, 1, 1)
            want = bias.view(1, 1, 1, -1).repeat(b, h, w, 1)
            want[bq][near] += wgt[:, c * R.N_ATOMS + m[near]].t()
            x_dev[bq, qy, qx, c] = 1.0
            got = ops.dynconv_nhwc(x_dev, atoms.cuda(), packed, bias_dev, relu=relu).cpu()
            x_dev[bq, qy, qx, c] = 0.0
            launches += 1
            taps.update(int(v) for v in l[near])
            atoms_seen.update(int(v) for v in m[near])
            _assert_equal(f"dynconv one-hot {b} x {h} x {w}: q = ({qy},{qx}) of image {bq}, c = {c}, relu={relu}", got, _want(want, relu),
                          lambda i: _pixel(i) + f"; this pixel's tap l = {int(l[i[1], i[2]])} (offset {R.tap_offset(int(l[i[1], i[2]]))}), atom m = {int(m[i[1], i[2]])}, "
                                                f"{'reads q' if bool(near[i[1], i[2]]) and i[0] == bq else 'does not read q'}")
    assert launches <= 56 and atoms_seen == set(range(R.N_ATOMS))
    assert taps == (set(range(R.N_TAPS)) if h >= 3 and w >= 3 else {12}), sorted(taps)


def _normal_operands(b, h, w):
    """bf16 x ~ N(0, 1), float32 atoms ~ N(0, 1) / 5, bf16 W ~ N(0, 1) / sqrt(1536), bias ~ N(0, 1): unit-normal operands at the fan-in scale
    (25 taps, 1536 columns), so F and y are of order 1 as in the network."""
    g = _gen(b, h, w, 5)
    x = torch.randn((b, h, w, R.CIN), generator=g).to(BF16).to(F64)
    atoms = (torch.randn((b, h, w, R.N_TAPS, R.N_ATOMS), generator=g) / 5).to(F32).to(F64)
    return x, atoms


@functools.lru_cache(maxsize=None)
def _normal_weights():
    g = _gen(8)
    wgt = (torch.randn((R.COUT, R.CIN * R.N_ATOMS), generator=g) / (R.CIN * R.N_ATOMS) ** 0.5).to(BF16).to(F64)
    bias = torch.randn((R.COUT,), generator=g).to(F64)
    return (wgt, bias) + _pack(wgt, bias)


@gpu
@pytest.mark.parametrize("relu", RELU)
def test_dynconv_images_of_a_batch_are_independent_and_runs_repeat(relu):
    ops = _ops()
    b, h, w = 3, 10, 14
    x, atoms = _normal_operands(b, h, w)
    _, _, packed, bias = _normal_weights()
    batched = _dynconv(ops, x, atoms, packed, bias, relu)
    assert torch.equal(_bits(batched), _bits(_dynconv(ops, x, atoms, packed, bias, relu))), "two identical calls differ: the K groups must meet in a fixed order"
    assert float(batched.float().abs().max()) > 1.0
    for i in range(b):
        single = _dynconv(ops, x[i:i + 1], atoms[i:i + 1], packed, bias, relu)
        _assert_equal(f"dynconv image {i} alone vs in the batch, relu={relu}", single, batched[i:i + 1], _pixel)


@gpu
@pytest.mark.parametrize("relu", RELU)
@pytest.mark.parametrize("b,h,w", R.DYNCONV_SHAPES, ids=SHAPE_IDS)
def test_dynconv_rounding_on_normal_operands(b, h, w, relu):
    """Against float64 on the same bf16 x and W and float32 atoms, F rounded to bf16 as the kernel rounds it.  The kernel's float32 F can fall
    on the other side of a bf16 tie than the float64 F (about 8e-5 of the features, float32 emulation on the CPU): one flip moves y by one
    bf16 ulp of F times |W| ~ 2^-7 |F| / 39, some 2e-4 -- a twentieth of the bound at |y| ~ 1.  (With W ~ N(0, 1), |y| ~ 200, the same flip
    is 2e-2 and breaks the bound wherever an output is near 0: the operands have to be at the fan-in scale for the bound to mean anything.)
    Measured on an MI355X: 1.88e-3 (1 x 1 x 1) .. 3.10e-3 (2 x 8 x 16), the output's own bf16 rounding; 0 .. 2.1 % of the outputs above half the bound."""
    x, atoms = _normal_operands(b, h, w)
    wgt, bias, packed, bias_dev = _normal_weights()
    want = R.ref_dynconv(x, atoms, wgt, bias, relu)
    got = _dynconv(_ops(), x, atoms, packed, bias_dev, relu)
    rel = (got.to(F64) - want).abs() / (want.abs() + 1.0)
    print(f"dynconv {b} x {h} x {w} relu={relu}: {float((rel > 2.0 ** -9).double().mean()):.2%} of the outputs above half the bound")
    _assert_rounding(f"dynconv {b} x {h} x {w} relu={relu}", got, want)


# ---- the layer at a size the golden does not cover -------------------------------------------------------------------------------------
@gpu
def test_dynamic_layer_at_partial_tiles_vs_stock_float32():
    """DynamicUpsampleLayer on G26's weights at x 1 x 256 x 6 x 10: the layer runs at 12 x 20 (partial tiles in both directions), the events
    are 48 x 80.  Against hyper_stock.stock_layer in float32 under test_dynamic_layer_vs_reference's bar."""
    from v2v_amd.hyper import DynamicUpsampleLayer
    g26 = load_g26()
    state = g26_layer_state(g26)
    layer = DynamicUpsampleLayer(256, 128, 5, padding=2, in_fuse_channels=6).cuda().eval()
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    x, ev, prev = (torch.from_numpy(seeded_input(s, *sh)).cuda() for s, sh in zip((301, 302, 303), ((1, 256, 6, 10), (1, 5, 48, 80), (1, 1, 48, 80))))
    with torch.no_grad():
        p = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in state.items()}
        want_ctx, want_atoms, want_y = stock_layer(x, ev, prev, p)
        ctx, atoms, y = layer.context(ev, prev), layer.atoms(ev, prev), layer(x, ev, prev)
    assert tuple(y.shape) == (1, 128, 12, 20) and y.dtype == F32
    for name, got, want in (("context", ctx.permute(0, 3, 1, 2), want_ctx), ("atoms", atoms.permute(0, 4, 3, 1, 2), want_atoms), ("output", y, want_y)):
        assert tuple(got.shape) == tuple(want.shape), name
        want = want.cpu().numpy()
        mx, rms = err(got.float().cpu().numpy(), want)
        scale = max(1.0, float(np.abs(want).max()))
        print(f"dynamic layer at 12 x 20, {name} vs stock float32: max {mx:.3e} rms {rms:.3e} (|want|max {float(np.abs(want).max()):.2f}, bar x {scale:.2f})")
        assert mx <= 3e-2 * scale and rms <= 6e-3 * scale, (name, mx, rms, scale)
