"""The forward operators of v2v_amd/nhwc_ops.py that store bfloat16 (kernels: v2v_amd/csrc/v2v_convlstm.hpp and v2v_narrow.hpp), one by one
against the float64 formulas of tests/forward_reference.py (themselves held to the stock PyTorch operators on the CPU by
tests/test_forward_reference.py) -- the forward counterpart of tests/test_backward_ops.py, whose plumbing this file imports.

Three kinds of case per operator:
  * exact on integers: every operand is a small integer (biases k/4), every product and partial sum a multiple of 1/4 below 2^22, so fp32
    accumulation is exact in ANY order -- on the matrix cores, across K groups, in the shuffles.  The bf16 output then equals
    reference.to(bfloat16), ONE round-to-nearest-even, and the check is torch.equal.  A second rounding, a rounding that is missing, a tie
    that goes the wrong way, one wrong (tap, channel) element of K changes at least one element and fails.  The recipes (the ranges of the
    integers) are chosen so that the roundings are exercised; tests/test_forward_reference.py asserts that for every case of this file, on
    the CPU, from the reference alone: sums below 2^24 in units of the quantum, >= 10 % of the outputs above 256 or with a fraction bf16
    does not hold, >= 1 % exact ties.
  * one tap at a time (the convolutions): the weight is zero except at one tap, where it is the channel map co -> ci = (7 co + 3) mod Cin
    with value 1; the output must be the shifted, strided copy of x[ci], zero where the tap lies outside the image.  One launch per tap
    covers every pixel, border and tile seam; the message names the tap and the border.
  * real-valued rounding: unit-normal bf16 operands at the project's bar for bf16 outputs, |got - want| / (|want| + 1) < 2^-8, at the same
    shapes, so that the integer cases do not stand alone.

Numeric bounds in this file: 2^-8 (above) and none other; everything else is torch.equal.

Which conv_nhwc instance runs (launch_conv_nhwc, v2v_convlstm_tu.hip).  The flattened-pixel instances see 5 images of 6 x 10 output
pixels = 300 pixels: 1.2 tiles of 256, 2.3 of 128, 4.7 of 64, 9.4 of 32 -- every seam inside an image, most inside a row, the last tile
partial; stride 2 reads 11 x 19 inputs (once 12 x 20).  A pinned tile_rows names the instance; tile_rows 0 lets the launcher choose by the
number of compute units, which the test cannot see.  On an MI355X (256 CUs), at 300 pixels:
  Cout % 256 == 0:           300 / 64 x (Cout / 256) < 256 -> the 64-pixel x HALF-column tile as two K groups (launch_step_t<1, 2, 3, 1, 2, 2, 1, 2>),
                             which no pinned value reaches; Cin 64 at 3x3 gives it nine K chunks, 5 + 4 on the two groups
  Cout 128 / 64 / 32:        300 / 256 < 256 -> the 128-pixel tile (for 128 columns as two K groups), the same instance as tile_rows 128
  5x5, Cout <= 64, stride 1, H and W multiples of 16: the halo tiles (conv_halo_kernel), the same instance as tile_rows 16
"""
import os

import pytest
import torch

import forward_reference as R
from test_backward_ops import BF16, F32, F64, _assert_equal, _assert_rounding, _borders, _dev, _host, _ints, _normal, _ops, _weights

gpu = pytest.mark.gpu


# ---- operands (CPU only: tests/test_forward_reference.py builds the same cases to assert what the recipes rest on) --------------------------
def _seed(case):
    return sum((i + 1) * int(v) for i, v in enumerate(case) if not isinstance(v, str)) + sum(map(ord, "".join(v for v in case if isinstance(v, str))))


def _quarters(gen, n):
    """Biases k/4, k in -8..8."""
    return torch.randint(-8, 9, (n,), generator=gen).to(F64) / 4


def _real_bias(gen, n):
    """Uniform in -0.5..0.5, float32 values (the kernels read the bias in float32), as float64."""
    return ((torch.rand((n,), generator=gen) * 2 - 1) * 0.5).to(F64)


def _out_hw(hin, win, stride):
    return (hin - 1) // stride + 1, (win - 1) // stride + 1


def _shifted(x, ci, ty, tx, ks, stride):
    """out[b, co, oy, ox] = x[b, ci[co], oy s + ty - pad, ox s + tx - pad], zero where that lies outside the image: what a convolution whose
    only non-zero weights are w[co, ci[co], ty, tx] = 1 computes."""
    b, c, hin, win = x.shape
    pad, (ho, wo) = ks // 2, _out_hw(hin, win, stride)
    xp = torch.zeros((b, c, hin + 2 * pad, win + 2 * pad), dtype=F64)
    xp[:, :, pad:pad + hin, pad:pad + win] = x
    return xp[:, ci, ty:ty + stride * ho:stride, tx:tx + stride * wo:stride].clone()


def _tap_weight(cout, cin, ks, ty, tx):
    """(w [cout, cin, ks, ks], ci [cout]): zero except w[co, ci[co], ty, tx] = 1 with ci[co] = (7 co + 3) mod cin."""
    ci = (7 * torch.arange(cout) + 3) % cin
    w = torch.zeros((cout, cin, ks, ks), dtype=F64)
    w[torch.arange(cout), ci, ty, tx] = 1.0
    return w, ci


def _tap_where(ks, stride, ty, tx, hin, win):
    pad = ks // 2

    def where(i):
        iy, ix = i[2] * stride + ty - pad, i[3] * stride + tx - pad
        return f"tap (ky {ty}, kx {tx}) of output pixel (image {i[0]}, row {i[2]}, column {i[3]}), channel {i[1]}, reads input ({iy}, {ix}), {_borders(iy, ix, hin, win)}"
    return where


# ---- conv_nhwc ---------------------------------------------------------------------------------------------------------------------------
# a case: (cin, cout, ks, stride, tile_rows, B, hin, win, residual, relu)
def _flat_cases(cin, cout, tile, second_stride2=(11, 19)):
    """One kernel instance on the 300-pixel geometry: ks 3 and 5 x stride 1 and 2 x with and without residual x with and without ReLU."""
    out = []
    for ks, stride in ((3, 1), (5, 1), (3, 2), (5, 2)):
        hin, win = (6, 10) if stride == 1 else (11, 19) if ks == 3 else second_stride2
        out += [(cin, cout, ks, stride, tile, 5, hin, win, res, relu) for res in (False, True) for relu in (False, True)]
    return out


CONV = []
for _cin in (64, 128):                                                      # Cout % 256 == 0: pinned 32 / 64 / 128 / 256 and the automatic half-column tile
    for _tile in (32, 64, 128, 256, 0):
        CONV += _flat_cases(_cin, 256, _tile, second_stride2=(12, 20) if (_cin, _tile) == (64, 64) else (11, 19))
CONV += _flat_cases(64, 512, 0) + _flat_cases(128, 512, 64)                # two packed column tiles
for _cout in (128, 64, 32):                                                 # one column tile of 4 / 2 / 1 fragments per wave
    for _cin in (64, 128):
        for _tile in (128, 256, 0):
            CONV += _flat_cases(_cin, _cout, _tile)
for _cout in (64, 128):                                                     # Cin == 32: two taps per K chunk (ks 5: the last half chunk is zero)
    for _tile in (128, 256, 0):
        CONV += _flat_cases(32, _cout, _tile)
HALO = [(64, 32, 3, 16), (128, 128, 3, 16), (192, 64, 5, 16), (64, 32, 5, 0)]      # (cin, cout, ks, tile_rows): pinned, and picked by the launcher
for _cin, _cout, _ks, _tile in HALO:                                        # a patch seam through the image in each direction
    for _b, _h, _w in ((2, 16, 32), (1, 32, 16)):
        CONV += [(_cin, _cout, _ks, 1, _tile, _b, _h, _w, res, relu) for res, relu in ((False, False), (True, True), (True, False), (False, True))]


def _conv_id(c):
    return f"{c[0]}to{c[1]}-k{c[2]}s{c[3]}-t{c[4]}-b{c[5]}-{c[6]}x{c[7]}" + ("-res" if c[8] else "") + ("-relu" if c[9] else "")


CONV_IDS = [_conv_id(c) for c in CONV]
CONV_TAPS = sorted({c[:8] for c in CONV})                                   # one-tap cases: every instance, ks, stride and geometry once
CONV_TAPS_IDS = [_conv_id(c + (False, False)) for c in CONV_TAPS]


def conv_integer_case(case):
    """Activations and residual in -3..3, weights in -2..2, half of each made non-negative; biases k/4 -> (x, w, bias, residual, reference)."""
    cin, cout, ks, stride, _, b, hin, win, with_res, relu = case
    g = torch.Generator().manual_seed(_seed(case))
    x, w, bias = _ints(g, 3, b, cin, hin, win, skew=True), _ints(g, 2, cout, cin, ks, ks, skew=True), _quarters(g, cout)
    res = _ints(g, 3, b, cout, *_out_hw(hin, win, stride), skew=True) if with_res else None
    return x, w, bias, res, R.ref_conv(x, w, bias, stride, res, relu)


def _conv_device(ops, case, x, w, bias, res):
    _, _, ks, stride, tile, _, _, _, _, relu = case
    packed = ops.pack_conv_weights(w.to(F32).cuda())
    return _host(ops.conv_nhwc(_dev(x, BF16), packed, bias.to(F32).cuda(), ks, stride, residual=_dev(res, BF16), relu=relu, tile_rows=tile))


def _conv_where(case):
    _, _, _, stride, tile, _, hin, win, _, _ = case
    ho, wo = _out_hw(hin, win, stride)

    def where(i):
        p = (i[0] * ho + i[2]) * wo + i[3]
        at = f"halo patch ({i[2] // 16}, {i[3] // 16}), pixel ({i[2] % 16}, {i[3] % 16}) of it" if tile == 16 else \
             f"flat pixel {p}" + (f" = row {p % tile} of tile {p // tile}" if tile else "")
        return f"output pixel (image {i[0]}, row {i[2]} of {ho}, column {i[3]} of {wo}), channel {i[1]}, {at}"
    return where


@gpu
@pytest.mark.parametrize("case", CONV, ids=CONV_IDS)
def test_conv_nhwc_exact_on_integers(case):
    ops = _ops()
    x, w, bias, res, want = conv_integer_case(case)
    _assert_equal("out", _conv_device(ops, case, x, w, bias, res), want.to(BF16), _conv_where(case))


@gpu
@pytest.mark.parametrize("case", CONV_TAPS, ids=CONV_TAPS_IDS)
def test_conv_nhwc_one_tap(case):
    ops = _ops()
    cin, cout, ks, stride, tile, b, hin, win = case
    g = torch.Generator().manual_seed(_seed(case) + 1)
    x, bias = _ints(g, 100, b, cin, hin, win), torch.zeros((cout,), dtype=F64)
    for ty in range(ks):
        for tx in range(ks):
            w, ci = _tap_weight(cout, cin, ks, ty, tx)
            got = _conv_device(ops, case + (False, False), x, w, bias, None)
            _assert_equal(f"out for the single tap (ky {ty}, kx {tx})", got, _shifted(x, ci, ty, tx, ks, stride).to(BF16), _tap_where(ks, stride, ty, tx, hin, win))


@gpu
@pytest.mark.parametrize("case", CONV, ids=CONV_IDS)
def test_conv_nhwc_rounding(case):
    ops = _ops()
    cin, cout, ks, stride, _, b, hin, win, with_res, relu = case
    g = torch.Generator().manual_seed(_seed(case) + 2)
    x, w, bias = _normal(g, b, cin, hin, win), _weights(g, cout, cin, ks), _real_bias(g, cout)
    res = _normal(g, b, cout, *_out_hw(hin, win, stride)) if with_res else None
    _assert_rounding("out", _conv_device(ops, case, x, w, bias, res), R.ref_conv(x, w, bias, stride, res, relu))


# ---- the operators on 8 padded input channels: conv_head_nhwc, conv_stem_nhwc, conv_head16_nhwc ----------------------------------------------
# a case: (kind, cin, ks, stride, B, H, W, relu); the output has 32 / 64 / 16 channels
PAD8_COUT = {"head": 32, "stem": 64, "head16": 16}
NARROW_SHAPES = [(2, 8, 16), (1, 19, 37), (1, 3, 3), (1, 17, 33)]          # 3 x 3: every ring pixel outside the image; 17 x 33: one pixel past a tile seam on both axes
PAD8 = [("head", cin, ks, 1, 2, 16, 32, relu) for ks in (3, 5) for cin in (1, 5, 8) for relu in (True, False)] \
    + [("stem", cin, 3, 2, b, h, w, relu) for cin in (5, 8) for b, h, w in ((2, 16, 32), (1, 32, 16)) for relu in (True, False)] \
    + [("head16", cin, 3, 1, b, h, w, relu) for cin in (5, 8) for b, h, w in NARROW_SHAPES for relu in (True, False)]
PAD8_IDS = [f"{c[0]}-cin{c[1]}-k{c[2]}s{c[3]}-b{c[4]}-{c[5]}x{c[6]}" + ("-relu" if c[7] else "") for c in PAD8]
PAD8_TAPS = [c[:7] for c in PAD8 if not c[7]]
PAD8_TAPS_IDS = [i for i, c in zip(PAD8_IDS, PAD8) if not c[7]]


def pad8_integer_case(case):
    """Activations in -15..15 on ALL 8 channels (the padded ones must not reach the output), weights in -8..8, half of each made
    non-negative; biases k/4 -> (x8, w, bias, reference)."""
    kind, cin, ks, stride, b, h, w_, relu = case
    g = torch.Generator().manual_seed(_seed(case))
    x8, w, bias = _ints(g, 15, b, 8, h, w_, skew=True), _ints(g, 8, PAD8_COUT[kind], cin, ks, ks, skew=True), _quarters(g, PAD8_COUT[kind])
    return x8, w, bias, R.ref_conv_pad8(x8, w, bias, stride, relu)


def _pad8_device(ops, case, x8, w, bias):
    kind, _, ks, _, _, _, _, relu = case
    xd, wd, bd = _dev(x8, BF16), w.to(F32).cuda(), bias.to(F32).cuda()
    if kind == "head":
        return _host(ops.conv_head_nhwc(xd, ops.pack_head_weights(wd), bd, ks, relu=relu))
    if kind == "stem":
        return _host(ops.conv_stem_nhwc(xd, ops.pack_stem_weights(wd), bd, relu=relu))
    return _host(ops.conv_head16_nhwc(xd, ops.pack_head16_weights(wd), bd, relu=relu))


def _tile16_where(h, w):
    return lambda i: f"output pixel (image {i[0]}, row {i[2]} of {h}, column {i[3]} of {w}), channel {i[1]}, pixel ({i[2] % 16}, {i[3] % 16}) of tile ({i[2] // 16}, {i[3] // 16})"


@gpu
@pytest.mark.parametrize("case", PAD8, ids=PAD8_IDS)
def test_pad8_conv_exact_on_integers(case):
    ops = _ops()
    x8, w, bias, want = pad8_integer_case(case)
    _assert_equal(case[0], _pad8_device(ops, case, x8, w, bias), want.to(BF16), _tile16_where(*want.shape[2:]))


@gpu
@pytest.mark.parametrize("case", PAD8_TAPS, ids=PAD8_TAPS_IDS)
def test_pad8_conv_one_tap(case):
    ops = _ops()
    kind, cin, ks, stride, b, h, w_ = case
    cout = PAD8_COUT[kind]
    g = torch.Generator().manual_seed(_seed(case) + 1)
    x8, bias = _ints(g, 100, b, 8, h, w_), torch.zeros((cout,), dtype=F64)
    for ty in range(ks):
        for tx in range(ks):
            w, ci = _tap_weight(cout, cin, ks, ty, tx)
            got = _pad8_device(ops, case + (False,), x8, w, bias)
            _assert_equal(f"{kind} for the single tap (ky {ty}, kx {tx})", got, _shifted(x8, ci, ty, tx, ks, stride).to(BF16), _tap_where(ks, stride, ty, tx, h, w_))


@gpu
@pytest.mark.parametrize("case", PAD8, ids=PAD8_IDS)
def test_pad8_conv_rounding(case):
    ops = _ops()
    kind, cin, ks, stride, b, h, w_, relu = case
    g = torch.Generator().manual_seed(_seed(case) + 2)
    x8, w, bias = _normal(g, b, 8, h, w_), _weights(g, PAD8_COUT[kind], cin, ks), _real_bias(g, PAD8_COUT[kind])
    _assert_rounding(kind, _pad8_device(ops, case, x8, w, bias), R.ref_conv_pad8(x8, w, bias, stride, relu))


# ---- resblock16_nhwc ---------------------------------------------------------------------------------------------------------------------
def resblock16_integer_case(shape):
    """x in -7..7 and conv1's weights in -4..4, half of each made non-negative, so that mid passes 256 and its rounding to bf16 shows in the
    output; conv2's weights in -1..1, signed, and biases k/2 -> (x, w1, b1, w2, b2, mid, reference).  (With conv2's weights in -4..4 and
    non-negative halves the output reaches 8e4, an ulp of 512, and 0.1 % of it are ties; with signed -4..4 and biases k/4 about 1 %.  Signed
    -1..1 and k/2 keep it below 1.2e4 and give 3 to 10 % ties at every shape.)  sum |mid| |w2| <= 144 x 4032, every term a multiple of 1/2."""
    b, h, w_ = shape
    g = torch.Generator().manual_seed(_seed(shape) + 16)
    x, w1, w2 = _ints(g, 7, b, 16, h, w_, skew=True), _ints(g, 4, 16, 16, 3, 3, skew=True), _ints(g, 1, 16, 16, 3, 3)
    b1, b2 = _quarters(g, 16) * 2, _quarters(g, 16) * 2
    return (x, w1, b1, w2, b2) + R.ref_resblock16(x, w1, b1, w2, b2)


def _resblock16_device(ops, x, w1, b1, w2, b2):
    packed = ops.pack_resblock16_weights(w1.to(F32).cuda(), w2.to(F32).cuda())
    return _host(ops.resblock16_nhwc(_dev(x, BF16), packed, b1.to(F32).cuda(), b2.to(F32).cuda()))


@gpu
@pytest.mark.parametrize("shape", NARROW_SHAPES)
def test_resblock16_exact_on_integers(shape):
    ops = _ops()
    x, w1, b1, w2, b2, _, want = resblock16_integer_case(shape)
    _assert_equal("resblock16", _resblock16_device(ops, x, w1, b1, w2, b2), want.to(BF16), _tile16_where(*shape[1:]))


@gpu
@pytest.mark.parametrize("shape", NARROW_SHAPES)
@pytest.mark.parametrize("which", ["conv1", "conv2"])
def test_resblock16_one_tap(shape, which):
    """The tapped convolution has one tap and the channel map, the other is the identity (centre tap, co -> co).  b1 is positive, b2 zero:
        conv1 tapped:  out = relu(relu(shift(x)[ci] + b1) + x)
        conv2 tapped:  out = relu(shift(relu(x + b1))[ci] + x), where shift reads ZERO outside the image, not relu(b1): the intermediate on
                       ring pixels outside the image is the second convolution's padding."""
    ops = _ops()
    b, h, w_ = shape
    g = torch.Generator().manual_seed(_seed(shape) + 17)
    x, b1, b2 = _ints(g, 7, b, 16, h, w_), torch.randint(1, 5, (16,), generator=g).to(F64), torch.zeros((16,), dtype=F64)
    ident = torch.zeros((16, 16, 3, 3), dtype=F64)
    ident[torch.arange(16), torch.arange(16), 1, 1] = 1.0
    for ty in range(3):
        for tx in range(3):
            w, ci = _tap_weight(16, 16, 3, ty, tx)
            if which == "conv1":
                want = torch.relu(torch.relu(_shifted(x, ci, ty, tx, 3, 1) + b1.view(1, -1, 1, 1)) + x)
                got = _resblock16_device(ops, x, w, b1, ident, b2)
            else:
                want = torch.relu(_shifted(torch.relu(x + b1.view(1, -1, 1, 1)), ci, ty, tx, 3, 1) + x)
                got = _resblock16_device(ops, x, ident, b1, w, b2)
            assert float(want.abs().max()) < 256                                    # small integers: exact in bf16, intermediate included
            _assert_equal(f"resblock16 with the single tap (ky {ty}, kx {tx}) in {which}", got, want.to(BF16), _tap_where(3, 1, ty, tx, h, w_))


@gpu
@pytest.mark.parametrize("shape", NARROW_SHAPES)
def test_resblock16_rounding(shape):
    ops = _ops()
    b, h, w_ = shape
    g = torch.Generator().manual_seed(_seed(shape) + 18)
    x, w1, w2, b1, b2 = _normal(g, b, 16, h, w_), _weights(g, 16, 16, 3), _weights(g, 16, 16, 3), _real_bias(g, 16), _real_bias(g, 16)
    _assert_rounding("resblock16", _resblock16_device(ops, x, w1, b1, w2, b2), R.ref_resblock16(x, w1, b1, w2, b2)[1])


# ---- upsample2x_nhwc / upsample2x_cat_nhwc --------------------------------------------------------------------------------------------------
UPSAMPLE = [(b, h, w, c, skip) for b, h, w, c in ((2, 5, 7, 64), (1, 1, 1, 8), (1, 9, 1, 256)) for skip in (False, True)]      # (B, H, W, C, with skip)
UPSAMPLE_CAT = [(3, 5, 7, 8, 16), (2, 16, 16, 64, 64), (2, 5, 7, 24, 0)]                                                        # (B, H, W, C1, C2), C2 = 0: no skip


def upsample_integer_case(case):
    """Integers in -200..200: x + skip passes 256, so the sum's rounding to bf16 shows; the outputs are multiples of 1/16 below 2^9."""
    b, h, w, c, with_skip = case
    g = torch.Generator().manual_seed(_seed(case))
    x = _ints(g, 200, b, c, h, w)
    skip = _ints(g, 200, b, c, h, w) if with_skip else None
    return x, skip, R.ref_upsample2x(x, skip)


def upsample_cat_integer_case(case):
    b, h, w, c1, c2 = case
    g = torch.Generator().manual_seed(_seed(case))
    x = _ints(g, 200, b, c1, h, w)
    skip = _ints(g, 200, b, c2, h, w) if c2 else None
    return x, skip, R.ref_upsample2x_cat(x, skip)


def _upsample_where(h, w):
    return lambda i: f"output pixel (row {i[2]} of {2 * h}, column {i[3]} of {2 * w}), image {i[0]}, channel {i[1]}; it reads input rows around {i[2] // 2}, columns around {i[3] // 2}"


@gpu
@pytest.mark.parametrize("case", UPSAMPLE)
def test_upsample2x_exact_on_integers(case):
    """... and the same bits under V2V_UP_RS = 1, 3, 64 (rows per work-item; read by tuning builds only, as tests/test_convlstm.py sets it)."""
    ops = _ops()
    x, skip, want = upsample_integer_case(case)
    xd, sd = _dev(x, BF16), _dev(skip, BF16)
    _assert_equal("up2", _host(ops.upsample2x_nhwc(xd, sd)), want.to(BF16), _upsample_where(case[1], case[2]))
    try:
        for rs in ("1", "3", "64"):
            os.environ["V2V_UP_RS"] = rs
            _assert_equal(f"up2 with V2V_UP_RS={rs}", _host(ops.upsample2x_nhwc(xd, sd)), want.to(BF16), _upsample_where(case[1], case[2]))
    finally:
        os.environ.pop("V2V_UP_RS", None)


@gpu
@pytest.mark.parametrize("case", UPSAMPLE)
def test_upsample2x_rounding(case):
    ops = _ops()
    b, h, w, c, with_skip = case
    g = torch.Generator().manual_seed(_seed(case) + 2)
    x = _normal(g, b, c, h, w)
    skip = _normal(g, b, c, h, w) if with_skip else None
    _assert_rounding("up2", _host(ops.upsample2x_nhwc(_dev(x, BF16), _dev(skip, BF16))), R.ref_upsample2x(x, skip))


@gpu
@pytest.mark.parametrize("case", UPSAMPLE_CAT)
@pytest.mark.parametrize("real", [False, True], ids=["integers", "rounding"])
def test_upsample2x_cat(case, real):
    ops = _ops()
    b, h, w, c1, c2 = case
    if real:
        g = torch.Generator().manual_seed(_seed(case) + 2)
        x = _normal(g, b, c1, h, w)
        skip = _normal(g, b, c2, h, w) if c2 else None
        want = R.ref_upsample2x_cat(x, skip)
    else:
        x, skip, want = upsample_cat_integer_case(case)
    got = _host(ops.upsample2x_cat_nhwc(_dev(x, BF16), _dev(skip, BF16)))
    if real:
        _assert_rounding("up2 cat", got, want)
    else:
        _assert_equal("up2 cat", got, want.to(BF16), _upsample_where(h, w))


# ---- conv1x1_nhwc ------------------------------------------------------------------------------------------------------------------------
# a case: (Cout, C, M, with skip, output type)
CONV1X1 = [(cout, c, m, skip, dt) for cout in (1, 2, 3) for c in (8, 64, 512) for m in (35, 2049) for skip in (False, True) for dt in ("f32", "bf16")]
CONV1X1_IDS = [f"cout{c[0]}-c{c[1]}-m{c[2]}" + ("-skip" if c[3] else "") + "-" + c[4] for c in CONV1X1]


def conv1x1_integer_case(case):
    """x and skip in -256..256 (an eighth of the sums x + skip is odd and above 256: its rounding shows); one image of 1 x M pixels (M is all
    the kernel sees) -> (x, skip, w, bias, reference).  sum |x + skip| |w| <= 512 x 512 x 2 = 5.2e5.
      float32 output: weights in -2..2 on every channel, biases k/4 -- the output IS the sum, every lane and channel counts exactly
      bf16 output:    the same weights on 8 channels per output and zero on the others, integer biases: a dense sum of 512 such products
                      has an ulp of 32 to 64 and next to no ties among 35 outputs; 8 terms stay near 1e3, where 5 to 25 % of the integers are ties"""
    cout, c, m, with_skip, dt = case
    g = torch.Generator().manual_seed(_seed(case[:4]))
    x = _ints(g, 256, 1, c, 1, m)
    skip = _ints(g, 256, 1, c, 1, m) if with_skip else None
    w, bias = _ints(g, 2, cout, c), _quarters(g, cout)
    if dt == "bf16":
        keep = torch.zeros((cout, c), dtype=torch.bool)
        for o in range(cout):
            keep[o, torch.randperm(c, generator=g)[:8]] = True
        w, bias = torch.where(keep, torch.where(w == 0, torch.ones_like(w), w), torch.zeros_like(w)), (bias * 4).round()
    return x, skip, w, bias, R.ref_conv1x1(x, skip, w, bias)


def _conv1x1_device(ops, case, x, skip, w, bias):
    return _host(ops.conv1x1_nhwc(_dev(x, BF16), w.to(F32).cuda(), bias.to(F32).cuda(), skip=_dev(skip, BF16), out_dtype=F32 if case[4] == "f32" else BF16))


@gpu
@pytest.mark.parametrize("case", CONV1X1, ids=CONV1X1_IDS)
def test_conv1x1_exact_on_integers(case):
    """The float32 output is the reference itself, the bf16 output its one rounding."""
    ops = _ops()
    x, skip, w, bias, want = conv1x1_integer_case(case)
    got = _conv1x1_device(ops, case, x, skip, w, bias)
    _assert_equal("conv1x1", got, want.to(F32 if case[4] == "f32" else BF16), lambda i: f"pixel {i[3]} of {case[2]}, output {i[1]}; {case[1] // 8} lanes per pixel")


@gpu
@pytest.mark.parametrize("case", [c for c in CONV1X1 if c[4] == "bf16"], ids=[i for i, c in zip(CONV1X1_IDS, CONV1X1) if c[4] == "bf16"])
def test_conv1x1_rounding(case):
    """The weights are NOT bf16 values here: the kernel rounds them, as the reference does."""
    ops = _ops()
    cout, c, m, with_skip, _ = case
    g = torch.Generator().manual_seed(_seed(case[:4]) + 2)
    x = _normal(g, 1, c, 1, m)
    skip = _normal(g, 1, c, 1, m) if with_skip else None
    w, bias = (torch.randn((cout, c), generator=g) * (3.0 / c ** 0.5)).to(F64), _real_bias(g, cout)
    _assert_rounding("conv1x1", _conv1x1_device(ops, case, x, skip, w, bias), R.ref_conv1x1(x, skip, w, bias))


# ---- batch independence, once per family: image i alone has the bits it has inside the batch (same pinned tile) -------------------------------
def _assert_batch_independent(name, run, *batched):
    """run(*tensors) on the whole batch and on each image alone; tensors: NCHW float64, None passes through."""
    whole = run(*batched)
    for i in range(whole.shape[0]):
        alone = run(*(None if t is None else t[i:i + 1] for t in batched))
        _assert_equal(f"{name}: image {i} alone against the same image inside the batch", alone, whole[i:i + 1])


@gpu
@pytest.mark.parametrize("case", [(64, 256, 3, 1, 64, 3, 6, 10, True, True), (128, 128, 5, 2, 128, 3, 11, 19, True, False), (32, 64, 5, 2, 128, 3, 11, 19, False, True),
                                  (192, 64, 5, 1, 16, 2, 16, 32, True, True)], ids=_conv_id)
def test_conv_nhwc_batch_independent(case):
    """60 pixels per image on 64- and 128-pixel tiles: inside the batch the images sit at other rows of other tiles than alone."""
    ops = _ops()
    cin, cout, ks, stride, _, b, hin, win, _, _ = case
    g = torch.Generator().manual_seed(_seed(case) + 3)
    x, w, bias, res = _normal(g, b, cin, hin, win), _weights(g, cout, cin, ks), _real_bias(g, cout), _normal(g, b, cout, *_out_hw(hin, win, stride))
    _assert_batch_independent("conv_nhwc", lambda xi, ri: _conv_device(ops, case, xi, w, bias, ri), x, res)


@gpu
@pytest.mark.parametrize("case", [("head", 5, 5, 1, 3, 16, 32, True), ("stem", 5, 3, 2, 3, 16, 32, True), ("head16", 5, 3, 1, 3, 19, 37, True)], ids=lambda c: c[0])
def test_pad8_conv_batch_independent(case):
    ops = _ops()
    kind, cin, ks, _, b, h, w_, _ = case
    g = torch.Generator().manual_seed(_seed(case) + 3)
    x8, w, bias = _normal(g, b, 8, h, w_), _weights(g, PAD8_COUT[kind], cin, ks), _real_bias(g, PAD8_COUT[kind])
    _assert_batch_independent(kind, lambda xi: _pad8_device(ops, case, xi, w, bias), x8)


@gpu
def test_resblock16_batch_independent():
    ops = _ops()
    g = torch.Generator().manual_seed(19)
    x, w1, w2, b1, b2 = _normal(g, 3, 16, 19, 37), _weights(g, 16, 16, 3), _weights(g, 16, 16, 3), _real_bias(g, 16), _real_bias(g, 16)
    _assert_batch_independent("resblock16", lambda xi: _resblock16_device(ops, xi, w1, b1, w2, b2), x)


@gpu
@pytest.mark.parametrize("with_skip", [False, True], ids=["plain", "skip"])
def test_upsample2x_batch_independent(with_skip):
    ops = _ops()
    g = torch.Generator().manual_seed(20 + with_skip)
    x = _normal(g, 3, 64, 5, 7)
    skip = _normal(g, 3, 64, 5, 7) if with_skip else None
    _assert_batch_independent("upsample2x", lambda xi, si: _host(ops.upsample2x_nhwc(_dev(xi, BF16), _dev(si, BF16))), x, skip)
    _assert_batch_independent("upsample2x_cat", lambda xi, si: _host(ops.upsample2x_cat_nhwc(_dev(xi, BF16), _dev(si, BF16))), x[:, :8], None if skip is None else skip[:, :16])


@gpu
@pytest.mark.parametrize("out", ["f32", "bf16"])
def test_conv1x1_batch_independent(out):
    """35 pixels per image at 8 lanes per pixel: inside the batch an image's pixels sit in other lanes of other workgroups than alone."""
    ops = _ops()
    g = torch.Generator().manual_seed(22)
    x, skip = _normal(g, 3, 64, 5, 7), _normal(g, 3, 64, 5, 7)
    w, bias = (torch.randn((2, 64), generator=g) * (3.0 / 8)).to(F64), _real_bias(g, 2)
    _assert_batch_independent("conv1x1", lambda xi, si: _conv1x1_device(ops, (2, 64, 35, True, out), xi, si, w, bias), x, skip)
