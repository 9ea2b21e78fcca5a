"""The backward operators of v2v_amd/nhwc_ops.py (kernels: v2v_amd/csrc/v2v_train_tu.hip and the EPI == 2 epilogue of v2v_convlstm.hpp),
one by one against the float64 references of tests/backward_reference.py (themselves checked against autograd on the CPU by
tests/test_backward_reference.py).

Bit-exact wherever the arithmetic allows.  The device: every operand is a small integer -- activations and gradients in -3..3, weights in
-2..2, all exact in bf16.  Every product and every partial sum is then an integer below 2^24 (a multiple of 1/16 for the upsampling
adjoint, whose weights are k/16), so fp32 accumulation is exact in ANY order: on the matrix cores, across the slabs, in the LDS
reductions.  float32 outputs therefore equal the float64 reference exactly and bf16 outputs equal reference.to(bfloat16), one
round-to-nearest-even -- the check is torch.equal, no tolerance.  The data gradients' sums pass 256 in magnitude (asserted), so the rounding
and its ties are exercised.  One wrong border row, a tap off by one, a dropped last pixel of a tile or slab changes at least one element
and fails.

Numeric bounds in this file (there are no others):
  * 2^-8:  |got - want| / (|want| + 1) on unit-normal operands, bf16 outputs, against float64 on the same bf16-rounded operands
  * M 2^-24 sum_p |dy_p| |x_p|:  the worst case of ANY fp32 summation order of M terms, for the float32 parameter gradients
  * A = 16 TOL_SAME_OPERANDS for convlstm_step_bwd (sigmoid / tanh: not integer-exact), derived at test_convlstm_step_bwd
"""
import pytest
import torch

import backward_reference as R
from test_convlstm import TOL_SAME_OPERANDS, _case
from test_train_grad import _cl, _compare_layer, _r, _stock_lstm, _stock_params, _t

gpu = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def _ops():
    from v2v_amd import nhwc_ops
    return nhwc_ops


def _ints(gen, k, *shape, skew=False):
    """Integers in -k..k as float64.  skew: half of them made non-negative, so that sums of products grow past 256 instead of cancelling."""
    v = torch.randint(-k, k + 1, shape, generator=gen)
    if skew:
        v = torch.where(torch.rand(shape, generator=gen) < 0.5, v.abs(), v)
    return v.to(F64)


def _normal(gen, *shape):
    """Unit-normal values bf16 holds exactly, as float64."""
    return torch.randn(shape, generator=gen).to(BF16).to(F64)


def _weights(gen, cout, cin, ks):
    """Unit-normal weights scaled 3 / sqrt(fan_in) (the forward tests' scale), rounded to bf16, as float64."""
    return (torch.randn((cout, cin, ks, ks), generator=gen) * (3.0 / (cin * ks * ks) ** 0.5)).to(BF16).to(F64)


def _dev(t, dtype):
    """NCHW float64 on the CPU -> contiguous NHWC `dtype` on the device (None stays None)."""
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def _host(t):
    """NHWC on the device -> NCHW on the CPU, same dtype."""
    return t.cpu().permute(0, 3, 1, 2)


def _assert_equal(name, got, want, describe=None):
    """torch.equal(got, want), with the first differing element (and what `describe(index)` knows about it) in the message."""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: {tuple(got.shape)} {got.dtype} != {tuple(want.shape)} {want.dtype}"
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = tuple(int(v) for v in bad[0])
    msg = f"{name}: {len(bad)} of {got.numel()} elements differ; first at {first}: got {float(got[first])}, want {float(want[first])}"
    raise AssertionError(msg + ("; " + describe(first) if describe else ""))


def _assert_rounding(name, got, want):
    """The project's criterion for bf16 outputs of real-valued operands: |got - want| / (|want| + 1) < 2^-8."""
    rel = (got.to(F64) - want).abs() / (want.abs() + 1.0)
    err, at = float(rel.max()), tuple(int(v) for v in (rel == rel.max()).nonzero()[0])
    msg = f"{name}: max |got - want| / (|want| + 1) = {err:.3e} (bound 2^-8 = {2.0 ** -8:.3e}) at {at}: got {float(got[at])}, want {float(want[at])}; max |want| = {float(want.abs().max()):.3f}"
    print(msg)
    assert err < 2.0 ** -8, msg


def _assert_summation(name, got, want, m, abs_sum):
    """The worst case of fp32 summation of m terms: |got - want| <= m 2^-24 sum |terms| (abs_sum: that sum, by the reference in float64)."""
    assert got.dtype == F32 and got.shape == want.shape, name
    err, bound = (got.to(F64) - want).abs(), m * 2.0 ** -24 * abs_sum
    ratio = err / bound.clamp_min(1e-300)
    at = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
    msg = (f"{name}: max |got - want| = {float(err.max()):.3e}, at most {float(ratio.max()):.3e} of the bound M 2^-24 sum |dy| |x| (M = {m}), "
           f"there at {at}: got {float(got[at])}, want {float(want[at])}")
    print(msg)
    assert bool((err <= bound).all()), msg


def _borders(iy, ix, hin, win):
    """Which image borders the input position (iy, ix) lies beyond."""
    out = [n for n, c in (("top", iy < 0), ("bottom", iy >= hin), ("left", ix < 0), ("right", ix >= win)) if c]
    return "outside the image: " + " ".join(out) if out else "inside the image"


def _onehot_pixels(b, ho, wo, flat):
    """Output pixels (image, row, column) of the one-hot cases: the four corners of the first image, the last pixel of the tensor and the
    pixels at the given flat indices (around a slab or tile boundary)."""
    pix = {(0, 0, 0), (0, 0, wo - 1), (0, ho - 1, 0), (0, ho - 1, wo - 1), (b - 1, ho - 1, wo - 1)}
    pix.update((p // (ho * wo), p % (ho * wo) // wo, p % wo) for p in flat if 0 <= p < b * ho * wo)
    return sorted(pix)


# ---- relu_bwd_nhwc ---------------------------------------------------------------------------------------------------------------------
# +0, -0, the smallest positive subnormal, the smallest positive normal, 1, -1, the negative subnormal 0x8001
RELU_Y_BITS = (0x0000, 0x8000, 0x0001, 0x0080, 0x3F80, 0xBF80, 0x8001)


@gpu
@pytest.mark.parametrize("m,c", [(35, 8), (2049, 64)])
def test_relu_bwd(m, c):
    """The mask is torch's own y > 0 on the CPU bf16 tensor; dy includes +-inf.  Where the mask holds the output is dy bit for bit, elsewhere 0."""
    ops = _ops()
    g = torch.Generator().manual_seed(m + c)
    bits = torch.tensor(RELU_Y_BITS, dtype=torch.int32)[torch.randint(0, len(RELU_Y_BITS), (m, c), generator=g)]
    y = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(BF16)
    assert all(int((bits == v).sum()) > 0 for v in RELU_Y_BITS)
    dy = _ints(g, 3, m, c)
    dy[torch.rand((m, c), generator=g) < 0.1] = float("inf")
    dy[torch.rand((m, c), generator=g) < 0.1] = float("-inf")
    dy = dy.to(BF16)
    mask = y > 0
    assert int((mask & dy.isinf()).sum()) > 0 and int((~mask & dy.isinf()).sum()) > 0
    assert bool(mask[bits == 0x0001].all()) and bool(mask[bits == 0x0080].all()) and not bool(mask[(bits == 0x8001) | (bits == 0x8000) | (bits == 0)].any())
    want = R.ref_relu_bwd(dy.to(F64), y.to(F64)).to(BF16)
    assert torch.equal(want, torch.where(mask, dy, torch.zeros_like(dy)))          # the reference on these values is the mask itself
    got = ops.relu_bwd_nhwc(dy.cuda(), y.cuda()).cpu()
    _assert_equal("relu_bwd", got, want, lambda i: f"y bits {int(bits[i]):#06x}, dy {float(dy[i])}")
    assert torch.equal(got.view(torch.int16)[mask], dy.view(torch.int16)[mask])
    same = ops.relu_bwd_nhwc(dy.cuda(), None).cpu()                                # y = None: dy unchanged
    assert torch.equal(same.view(torch.int16), dy.view(torch.int16))


# ---- conv_dgrad_nhwc -------------------------------------------------------------------------------------------------------------------
# (cin, cout, ks, stride, B, hin, win, residual) of the FORWARD convolution cin -> cout whose data gradient is taken; the kernel runs the
# transposed convolution cout -> cin
DGRAD = [
    (64, 128, 5, 2, 2, 32, 32, False),      # transposed 128 -> 64 on the launcher-picked halo tile over the stuffed grid
    (64, 128, 5, 2, 1, 12, 20, False),      # 240 stuffed pixels: a partial last tile, not multiples of 16
    (32, 64, 5, 2, 3, 8, 24, False),
    (256, 256, 3, 1, 3, 6, 6, True),        # 108 pixels: less than one tile; the residual block's identity branch
    (128, 256, 3, 1, 1, 10, 14, False),     # the gate convolution of C = 64, 256-column tiles
    (128, 32, 3, 1, 2, 16, 16, False),      # transposed 32 -> 128: two taps per K chunk
    (128, 32, 3, 1, 1, 6, 10, False),
    (64, 32, 5, 1, 1, 16, 32, False),       # transposed 32 -> 64: 25 taps, the last half chunk is zero
    (128, 64, 5, 1, 5, 12, 10, False),
]
DGRAD_IDS = [f"{c[0]}to{c[1]}-k{c[2]}s{c[3]}-b{c[4]}-{c[5]}x{c[6]}" + ("-res" if c[7] else "") for c in DGRAD]


def _dgrad_device(ops, dy, packed, cin, ks, stride, hin, win, res):
    return _host(ops.conv_dgrad_nhwc(_dev(dy, BF16), packed, cin, ks, stride, hin, win, residual=_dev(res, BF16)))


@gpu
@pytest.mark.parametrize("cin,cout,ks,stride,b,hin,win,with_res", DGRAD, ids=DGRAD_IDS)
def test_conv_dgrad_exact_on_integers(cin, cout, ks, stride, b, hin, win, with_res):
    ops = _ops()
    g = torch.Generator().manual_seed(cin + cout + ks + stride + b + hin + win)
    ho, wo = (hin - 1) // stride + 1, (win - 1) // stride + 1
    dy, w = _ints(g, 3, b, cout, ho, wo, skew=True), _ints(g, 2, cout, cin, ks, ks, skew=True)
    res = _ints(g, 3, b, cin, hin, win) if with_res else None
    want = R.ref_conv_dgrad(dy, w, stride, hin, win, residual=res)
    peak = float(want.abs().max())
    assert 256 < peak < 2 ** 24, f"max |sum| {peak}: the bf16 rounding must be exercised and fp32 accumulation exact"
    assert not torch.equal(want.to(BF16).to(F64), want)                            # some sums do round
    packed = ops.pack_dgrad_weights(w.to(F32).cuda())
    pad = ks // 2

    def where(i):
        edge = min(i[2], hin - 1 - i[2], i[3], win - 1 - i[3])
        return f"input pixel (image {i[0]}, row {i[2]}, column {i[3]}) channel {i[1]}, {edge} from the nearest border (pad {pad}), flat pixel {(i[0] * hin + i[2]) * win + i[3]}"
    _assert_equal("dx", _dgrad_device(ops, dy, packed, cin, ks, stride, hin, win, res), want.to(BF16), where)


@gpu
@pytest.mark.parametrize("cin,cout,ks,stride,b,hin,win,with_res", DGRAD, ids=DGRAD_IDS)
def test_conv_dgrad_one_hot(cin, cout, ks, stride, b, hin, win, with_res):
    """dy = 1 at one element: dx is the weights of that output channel placed around the pixel (tap (ky, kx) at input position
    (oy s + ky - pad, ox s + kx - pad)), cut at the image border, zero elsewhere (+ the residual)."""
    ops = _ops()
    g = torch.Generator().manual_seed(cin + cout + ks + stride + b + hin + win + 1)
    ho, wo, pad = (hin - 1) // stride + 1, (win - 1) // stride + 1, ks // 2
    w = _ints(g, 2, cout, cin, ks, ks)
    res = _ints(g, 3, b, cin, hin, win) if with_res else None
    packed = ops.pack_dgrad_weights(w.to(F32).cuda())
    # output pixels whose footprint lies on the last input pixel before a 64- / 128- / 256-pixel tile boundary, and on the first after it
    flat = []
    for q in (63, 64, 127, 128, 255, 256):
        if q < b * hin * win:
            flat.append((q // (hin * win) * ho + q % (hin * win) // win // stride) * wo + q % win // stride)
    for n, (bi, oy, ox) in enumerate(_onehot_pixels(b, ho, wo, flat)):
        co = (n * 37 + 5) % cout
        dy = torch.zeros((b, cout, ho, wo), dtype=F64)
        dy[bi, co, oy, ox] = 1.0
        want = torch.zeros((b, cin, hin, win), dtype=F64)
        for ky in range(ks):
            for kx in range(ks):
                iy, ix = oy * stride + ky - pad, ox * stride + kx - pad
                if 0 <= iy < hin and 0 <= ix < win:
                    want[bi, :, iy, ix] = w[co, :, ky, kx]
        if with_res:
            want = want + res

        def where(i, bi=bi, oy=oy, ox=ox):
            ky, kx = i[2] - oy * stride + pad, i[3] - ox * stride + pad
            tap = f"tap (ky {ky}, kx {kx})" if 0 <= ky < ks and 0 <= kx < ks and i[0] == bi else "outside the footprint"
            cut = [_borders(oy * stride + a - pad, ox * stride + c - pad, hin, win) for a in range(ks) for c in range(ks)]
            return f"{tap} of output pixel (image {bi}, row {oy}, column {ox}); its footprint is cut at: {sorted(set(cut) - {'inside the image'}) or 'no border'}"
        _assert_equal(f"dx for dy one-hot at image {bi}, pixel ({oy}, {ox}), channel {co}",
                      _dgrad_device(ops, dy, packed, cin, ks, stride, hin, win, res), want.to(BF16), where)


@gpu
@pytest.mark.parametrize("cin,cout,ks,stride,b,hin,win,with_res", DGRAD, ids=DGRAD_IDS)
def test_conv_dgrad_rounding(cin, cout, ks, stride, b, hin, win, with_res):
    ops = _ops()
    g = torch.Generator().manual_seed(cin + cout + ks + stride + b + hin + win + 2)
    ho, wo = (hin - 1) // stride + 1, (win - 1) // stride + 1
    dy, w = _normal(g, b, cout, ho, wo), _weights(g, cout, cin, ks)
    res = _normal(g, b, cin, hin, win) if with_res else None
    packed = ops.pack_dgrad_weights(w.to(F32).cuda())
    _assert_rounding("dx", _dgrad_device(ops, dy, packed, cin, ks, stride, hin, win, res), R.ref_conv_dgrad(dy, w, stride, hin, win, residual=res))


# ---- conv_wgrad_nhwc -------------------------------------------------------------------------------------------------------------------
# (c1, c2, cin_out, cout, ks, stride, B, hin, win, x2 given)
WGRAD = [
    (8, 0, 5, 32, 5, 1, 1, 16, 16, False),          # the head: N = 200 columns of which 56 are dead; the padded channels are dropped
    (8, 0, 5, 32, 5, 1, 2, 6, 10, False),
    (8, 0, 5, 64, 3, 2, 1, 16, 16, False),          # the stem
    (64, 64, 128, 256, 3, 1, 1, 10, 14, True),      # the gates: M = 140, not a multiple of 16
    (64, 64, 128, 256, 3, 1, 1, 10, 14, False),     # ... with x2 = None: that half of dW is exactly zero
    (64, 0, 64, 128, 5, 2, 2, 31, 33, False),       # stride 2 on an odd input
    (32, 0, 32, 64, 5, 1, 2, 24, 24, False),        # M = 1152: five slabs of 240 pixels that cut through image rows, the last has 192
    (64, 0, 64, 32, 3, 1, 3, 6, 6, False),
]
WGRAD_IDS = [f"{c[0]}+{c[1]}to{c[3]}-out{c[2]}-k{c[4]}s{c[5]}-b{c[6]}-{c[7]}x{c[8]}" + ("-x2" if c[9] else "") for c in WGRAD]


def _slab_pixels(m, cout, n):
    """Pixels per slab of the weight gradient, as launch_conv_wgrad splits them (v2v_train_tu.hip: wgrad_slabs): about 2048 workgroups in
    all, at least 256 pixels per slab, a multiple of 16."""
    tiles = (n + 127) // 128 * (cout // 32)
    s = max(1, min((2048 + tiles - 1) // tiles, (m + 255) // 256))
    return ((m + s - 1) // s + 15) // 16 * 16


def test_slab_pixels_restate_the_launcher():
    assert _slab_pixels(1152, 64, 25 * 32) == 240 and 1152 - 4 * 240 == 192        # five slabs of 240, the last has 192
    assert _slab_pixels(140, 256, 9 * 128) == 144                                   # one slab, its last MFMA step has 12 live pixels


def _wgrad_device(ops, dy, x, c1, c2, cin_out, ks, stride, with_x2):
    x1 = _dev(x[:, :c1], BF16)
    x2 = _dev(x[:, c1:], BF16) if with_x2 else None
    return tuple(v.cpu() for v in ops.conv_wgrad_nhwc(_dev(dy, BF16), x1, x2, c2, cin_out, ks, stride))


def _wgrad_operands(case, draw):
    """dy [B, Cout, Ho, Wo] and the convolution's input x [B, C1 + C2, hin, win] (x2 = None: that half of x is zero; the head's padded
    channels cin_out .. C1 are filled, and must not reach dW)."""
    c1, c2, cin_out, cout, ks, stride, b, hin, win, with_x2 = case
    ho, wo = (hin - 1) // stride + 1, (win - 1) // stride + 1
    dy, x = draw(b, cout, ho, wo), draw(b, c1 + c2, hin, win)
    if c2 and not with_x2:
        x[:, c1:] = 0.0
    return dy, x, b * ho * wo


@gpu
@pytest.mark.parametrize("case", WGRAD, ids=WGRAD_IDS)
def test_conv_wgrad_exact_on_integers(case):
    ops = _ops()
    c1, c2, cin_out, cout, ks, stride, b, hin, win, with_x2 = case
    g = torch.Generator().manual_seed(sum(case))
    dy, x, m = _wgrad_operands(case, lambda *s: _ints(g, 3, *s))
    want_dw, want_db = R.ref_conv_wgrad(dy, x, ks, stride)
    assert float(R.ref_conv_wgrad(dy.abs(), x.abs(), ks, stride)[0].max()) < 2 ** 24
    dw, db = _wgrad_device(ops, dy, x, c1, c2, cin_out, ks, stride, with_x2)
    _assert_equal("dW", dw, want_dw[:, :cin_out].to(F32), lambda i: f"output channel {i[0]}, input channel {i[1]}, tap (ky {i[2]}, kx {i[3]}); M = {m} pixels")
    _assert_equal("db", db, want_db.to(F32))
    if c2 and not with_x2:
        assert torch.equal(dw[:, c1:], torch.zeros_like(dw[:, c1:])) and bool(want_dw[:, :c1].abs().max() > 0)


@gpu
@pytest.mark.parametrize("case", WGRAD, ids=WGRAD_IDS)
def test_conv_wgrad_one_hot(case):
    """dy non-zero at one output pixel: dW[o, i, ky, kx] = dy[o] x[i, oy s + ky - pad, ox s + kx - pad], zero where the tap falls outside
    the image; db = dy at that pixel."""
    ops = _ops()
    c1, c2, cin_out, cout, ks, stride, b, hin, win, with_x2 = case
    g = torch.Generator().manual_seed(sum(case) + 1)
    _, x, m = _wgrad_operands(case, lambda *s: _ints(g, 3, *s))
    ho, wo, pad = (hin - 1) // stride + 1, (win - 1) // stride + 1, ks // 2
    k_slab = _slab_pixels(m, cout, ks * ks * (c1 + c2))
    last = (m - 1) // k_slab * k_slab                                              # first pixel of the last slab
    for bi, oy, ox in _onehot_pixels(b, ho, wo, (7, 8, 15, 16, k_slab - 1, k_slab, last - 1, last)):
        d = _ints(g, 3, cout)
        d[d == 0] = 1.0                                                            # every output channel is live
        dy = torch.zeros((b, cout, ho, wo), dtype=F64)
        dy[bi, :, oy, ox] = d
        want = torch.zeros((cout, c1 + c2, ks, ks), dtype=F64)
        for ky in range(ks):
            for kx in range(ks):
                iy, ix = oy * stride + ky - pad, ox * stride + kx - pad
                if 0 <= iy < hin and 0 <= ix < win:
                    want[:, :, ky, kx] = d[:, None] * x[bi, None, :, iy, ix]
        dw, db = _wgrad_device(ops, dy, x, c1, c2, cin_out, ks, stride, with_x2)

        def where(i, oy=oy, ox=ox):
            iy, ix = oy * stride + i[2] - pad, ox * stride + i[3] - pad
            return f"tap (ky {i[2]}, kx {i[3]}) reads input ({iy}, {ix}), {_borders(iy, ix, hin, win)}; output channel {i[0]}, input channel {i[1]}"
        name = f"for dy at image {bi}, pixel ({oy}, {ox}) = flat pixel {(bi * ho + oy) * wo + ox} of {m} (slabs of {k_slab})"
        _assert_equal("dW " + name, dw, want[:, :cin_out].to(F32), where)
        _assert_equal("db " + name, db, d.to(F32))


@gpu
@pytest.mark.parametrize("case", WGRAD, ids=WGRAD_IDS)
def test_conv_wgrad_summation(case):
    ops = _ops()
    c1, c2, cin_out, cout, ks, stride, b, hin, win, with_x2 = case
    g = torch.Generator().manual_seed(sum(case) + 2)
    dy, x, m = _wgrad_operands(case, lambda *s: _normal(g, *s))
    want_dw, want_db = R.ref_conv_wgrad(dy, x, ks, stride)
    abs_dw, abs_db = R.ref_conv_wgrad(dy.abs(), x.abs(), ks, stride)
    dw, db = _wgrad_device(ops, dy, x, c1, c2, cin_out, ks, stride, with_x2)
    _assert_summation("dW", dw, want_dw[:, :cin_out], m, abs_dw[:, :cin_out])
    _assert_summation("db", db, want_db, m, abs_db)


# ---- upsample2x_bwd_nhwc / upsample2x_cat_bwd_nhwc ---------------------------------------------------------------------------------------
UPSAMPLE = [(1, 1, 1, 8), (2, 5, 7, 64), (1, 9, 1, 256), (3, 16, 8, 32)]           # (B, H, W, C) of the INPUT of the upsampling
UPSAMPLE_CAT = [(3, 5, 7, 24, 8, 16), (2, 16, 16, 128, 64, 64)]                   # (B, H, W, Ctot, c0, c)


def _upsample_where(h, w):
    return lambda i: f"input pixel (row {i[2]} of {h}, column {i[3]} of {w}), image {i[0]}, channel {i[1]}"


@gpu
@pytest.mark.parametrize("b,h,w,c", UPSAMPLE)
@pytest.mark.parametrize("real", [False, True], ids=["integers", "rounding"])
def test_upsample2x_bwd(b, h, w, c, real):
    """Integers: sums of k/16 multiples of values in -3..3, below 16 in magnitude: exact in fp32 AND in bf16.  H = 1 / W = 1: both clamped
    edges fold onto the one row / column."""
    ops = _ops()
    g = torch.Generator().manual_seed(b + h + w + c + real)
    dout = _normal(g, b, c, 2 * h, 2 * w) if real else _ints(g, 3, b, c, 2 * h, 2 * w)
    want = R.ref_upsample2x_bwd(dout)
    got = _host(ops.upsample2x_bwd_nhwc(_dev(dout, BF16)))
    if real:
        _assert_rounding("dx", got, want)
    else:
        assert torch.equal(want.to(BF16).to(F64), want) and float(want.abs().max()) < 2 ** 24
        _assert_equal("dx", got, want.to(BF16), _upsample_where(h, w))


@gpu
@pytest.mark.parametrize("b,h,w,ctot,c0,c", UPSAMPLE_CAT)
@pytest.mark.parametrize("real", [False, True], ids=["integers", "rounding"])
def test_upsample2x_cat_bwd(b, h, w, ctot, c0, c, real):
    """Against the reference on the channel slice [c0, c0 + c), not against the sibling kernel."""
    ops = _ops()
    g = torch.Generator().manual_seed(b + h + w + ctot + c0 + real)
    dout = _normal(g, b, ctot, 2 * h, 2 * w) if real else _ints(g, 3, b, ctot, 2 * h, 2 * w)
    want = R.ref_upsample2x_bwd(dout)[:, c0:c0 + c]
    got = _host(ops.upsample2x_cat_bwd_nhwc(_dev(dout, BF16), c0, c))
    if real:
        _assert_rounding("dx", got, want)
    else:
        _assert_equal("dx", got, want.to(BF16), _upsample_where(h, w))


# ---- conv1x1_bwd_nhwc / conv1x1_bwd_cout_nhwc --------------------------------------------------------------------------------------------
CONV1X1 = [(1, 35, 64, False), (1, 2049, 32, True), (1, 300, 8, False), (1, 4100, 128, True),           # (Cout, M, C, with skip)
           (2, 35, 64, False), (2, 2049, 32, True), (3, 35, 64, False), (3, 2049, 32, True)]


def _conv1x1_device(ops, dy, x, skip, w):
    """Cout = 1 on conv1x1_bwd_nhwc, Cout = 2, 3 on conv1x1_bwd_cout_nhwc -> (dx NCHW bf16, dW [Cout, C] float32, db [Cout] float32) on the CPU."""
    cout = w.shape[0]
    fn = ops.conv1x1_bwd_nhwc if cout == 1 else ops.conv1x1_bwd_cout_nhwc
    dx, dw, db = fn(_dev(dy, F32), _dev(x, BF16), _dev(skip, BF16), w.to(F32).reshape(cout, -1, 1, 1).cuda())
    return _host(dx), dw.cpu().reshape(cout, -1), db.cpu()


def _conv1x1_operands(cout, m, c, with_skip, draw):
    """dy, x, skip as one image of 1 x M pixels: M is all the kernel sees."""
    return draw(1, cout, 1, m), draw(1, c, 1, m), (draw(1, c, 1, m) if with_skip else None)


@gpu
@pytest.mark.parametrize("cout,m,c,with_skip", CONV1X1)
def test_conv1x1_bwd_exact_on_integers(cout, m, c, with_skip):
    ops = _ops()
    g = torch.Generator().manual_seed(cout + m + c)
    dy, x, skip = _conv1x1_operands(cout, m, c, with_skip, lambda *s: _ints(g, 3, *s))
    w = _ints(g, 2, cout, c)
    want_dx, want_dw, want_db = R.ref_conv1x1_bwd(dy, x, skip, w)
    assert float(R.ref_conv1x1_bwd(dy.abs(), x.abs(), None if skip is None else skip.abs(), w.abs())[1].max()) < 2 ** 24
    dx, dw, db = _conv1x1_device(ops, dy, x, skip, w)
    _assert_equal("dx", dx, want_dx.to(BF16), lambda i: f"pixel {i[3]} of {m}, channel {i[1]}")
    _assert_equal("dW", dw, want_dw.to(F32), lambda i: f"output {i[0]}, channel {i[1]}; M = {m} in slabs of 2048")
    _assert_equal("db", db, want_db.to(F32))


@gpu
@pytest.mark.parametrize("cout,m,c,with_skip", CONV1X1)
def test_conv1x1_bwd_rounding_and_summation(cout, m, c, with_skip):
    """dy is read as float32 (the loss gradient, unrounded); x, skip are bf16 values and the weights are rounded by the kernel."""
    ops = _ops()
    g = torch.Generator().manual_seed(cout + m + c + 1)
    dy, x, skip = _conv1x1_operands(cout, m, c, with_skip, lambda *s: torch.randn(s, generator=g).to(F64))
    x, skip = x.to(BF16).to(F64), (None if skip is None else skip.to(BF16).to(F64))
    w = torch.randn((cout, c), generator=g).to(F64) * (3.0 / c ** 0.5)
    want_dx, want_dw, want_db = R.ref_conv1x1_bwd(dy, x, skip, w)
    xs = x if skip is None else R.bf16_round(x + skip)                            # the operand of the sum
    _, abs_dw, abs_db = R.ref_conv1x1_bwd(dy.abs(), xs.abs(), None, w)
    dx, dw, db = _conv1x1_device(ops, dy, x, skip, w)
    _assert_rounding("dx", dx, want_dx)
    _assert_summation("dW", dw, want_dw, m, abs_dw)
    _assert_summation("db", db, want_db, m, abs_db)


# ---- convlstm_step_bwd -----------------------------------------------------------------------------------------------------------------
LSTM_A = 16 * TOL_SAME_OPERANDS


@gpu
@pytest.mark.parametrize("b,c,h,w", [(1, 64, 6, 6), (3, 64, 10, 14), (1, 128, 8, 24), (2, 256, 8, 8)])
@pytest.mark.parametrize("state,with_dc", [(True, True), (False, True), (True, False), (False, False)], ids=["full", "no-state", "no-dc", "no-state-no-dc"])
def test_convlstm_step_bwd(b, c, h, w, state, with_dc):
    """Sigmoid and tanh: not integer-exact.  |got - want| <= 2^-8 |want| + A for dgates (bf16), <= A for dc_prev (fp32), A = 16 x
    TOL_SAME_OPERANDS = 3.2e-4, from propagating to first order the bound tests/test_convlstm.py grants the forward's h and c on the same
    operands (eps = 2e-5), assumed on every gate and on tanh(c): dc_tot = dc + dh o (1 - tc^2) has |dc_tot| <= 2 and an error of at most
    3 eps; the largest propagation is d_r = dc_tot c_prev r(1-r) with |c_prev| up to about 4.5: 3 eps 4.5 / 4 + 2 x 4.5 eps, roughly
    12 eps; 16 eps leaves a third of margin for the hardware exp and reciprocal.

    Measured on an MI355X, maxima over the 16 cases: dgates |got - want| 3.9e-3 on |dgates| up to 1.63, i.e. at most 3.4e-8 above the bf16
    rounding term 2^-8 |want|; dc_prev |got - want| 7.1e-7 on |dc_prev| up to 1.72."""
    ops = _ops()
    from v2v_amd import convlstm as CL
    x, hp, cp, weight, bias = _case(b, c, h, w, seed=b + c + h + w)
    x, hp, weight = x.to(BF16), hp.to(BF16), weight.to(BF16)
    g = torch.Generator().manual_seed(b + c + h + w + 7)
    dh = torch.rand((b, c, h, w), generator=g) * 2 - 1
    dc = (torch.rand((b, c, h, w), generator=g) * 2 - 1) if with_dc else None
    want_dg, want_dcp = R.ref_convlstm_step_bwd(x.to(F64), hp.to(F64) if state else None, cp.to(F64) if state else None, weight.to(F64), bias.to(F64),
                                                dh.to(F64), None if dc is None else dc.to(F64))
    packed = CL.pack_gate_weights(weight.float().cuda())
    dg, dcp = ops.convlstm_step_bwd(_dev(x, BF16), _dev(hp, BF16) if state else None, _dev(cp, F32) if state else None, packed, bias.cuda(),
                                    _dev(dh, F32), _dev(dc, F32))
    assert dg.dtype == BF16 and dcp.dtype == F32
    err_dg, err_dcp = (_host(dg).to(F64) - want_dg).abs(), (_host(dcp).to(F64) - want_dcp).abs()
    excess = err_dg - 2.0 ** -8 * want_dg.abs()
    msg = (f"convlstm_step_bwd {(b, c, h, w)} state={state} dc={with_dc}: dgates max |got - want| {float(err_dg.max()):.3e}, "
           f"max (|got - want| - 2^-8 |want|) {float(excess.max()):.3e}, dc_prev max |got - want| {float(err_dcp.max()):.3e} (A = {LSTM_A:.1e}); "
           f"max |dgates| {float(want_dg.abs().max()):.3f}, max |dc_prev| {float(want_dcp.abs().max()):.3f}")
    print(msg)
    at = tuple(int(v) for v in (excess == excess.max()).nonzero()[0])
    assert bool((excess <= LSTM_A).all()), f"dgates, worst at (image, gate {at[1] // c} of i r o g channel {at[1] % c}, row, column) = {at}; {msg}"
    assert bool((err_dcp <= LSTM_A).all()), "dc_prev; " + msg
    if not state:
        assert float(want_dg[:, c:2 * c].abs().max()) == 0.0 and torch.equal(dg[..., c:2 * c], torch.zeros_like(dg[..., c:2 * c]))    # d_r = dc_tot c_prev = 0


# ---- whole layers at ragged shapes: the criterion of tests/test_train_grad.py, unchanged ----------------------------------------------------
RAGGED = (3, 24, 40)


@gpu
def test_ragged_encoder_conv_gradients():
    import torch.nn.functional as F
    from v2v_amd.convlstm import ConvLayer
    from seeded_weights import load_seeded
    b, h, w = RAGGED
    m = ConvLayer(64, 128, 5, 2, 2, trainable=True).cuda()
    load_seeded(m, 301)
    x32 = _t(302, b, 64, h, w).requires_grad_()
    x = _cl(x32)
    r = _r(303, b, 128, h // 2, w // 2)
    wt, bs = _stock_params(m.conv2d)
    _compare_layer(lambda: (m(x).float() * r).sum(), [x, m.conv2d.weight, m.conv2d.bias],
                   lambda: (F.relu(F.conv2d(x32, wt, bs, stride=2, padding=2)).float() * r).sum(), [x32, wt, bs], ["dx", "dw", "db"])


@gpu
def test_ragged_decoder_gradients():
    import torch.nn.functional as F
    from v2v_amd.unet import UpsampleConvLayer
    from seeded_weights import load_seeded
    b, h, w = RAGGED
    m = UpsampleConvLayer(128, 64, 5, padding=2, trainable=True).cuda()
    load_seeded(m, 311)
    x32, s32 = _t(312, b, 128, h, w).requires_grad_(), _t(313, b, 128, h, w).requires_grad_()
    x, s = _cl(x32), _cl(s32)
    r = _r(314, b, 64, 2 * h, 2 * w)
    wt, bs = _stock_params(m.conv2d)
    stock = lambda: (F.relu(F.conv2d(F.interpolate(x32 + s32, scale_factor=2, mode="bilinear", align_corners=False), wt, bs, padding=2)).float() * r).sum()  # noqa: E731
    _compare_layer(lambda: (m(x, s).float() * r).sum(), [x, s, m.conv2d.weight, m.conv2d.bias], stock, [x32, s32, wt, bs], ["dx", "dskip", "dw", "db"])


@gpu
def test_ragged_residual_block_gradients():
    import torch.nn.functional as F
    from v2v_amd.convlstm import ResidualBlock
    from seeded_weights import load_seeded
    b, h, w = RAGGED
    m = ResidualBlock(256, 256, trainable=True).cuda()
    load_seeded(m, 321)
    x32 = _t(322, b, 256, h, w).requires_grad_()
    x = _cl(x32)
    r = _r(323, b, 256, h, w)
    (w1, b1), (w2, b2) = _stock_params(m.conv1), _stock_params(m.conv2)
    stock = lambda: (F.relu(F.conv2d(F.relu(F.conv2d(x32, w1, b1, padding=1)), w2, b2, padding=1) + x32).float() * r).sum()  # noqa: E731
    _compare_layer(lambda: (m(x).float() * r).sum(), [x, m.conv1.weight, m.conv1.bias, m.conv2.weight, m.conv2.bias],
                   stock, [x32, w1, b1, w2, b2], ["dx", "dw1", "db1", "dw2", "db2"])


@gpu
def test_ragged_convlstm_gradients():
    from v2v_amd.convlstm import ConvLSTM
    from seeded_weights import load_seeded
    b, h, w = RAGGED
    steps = 2
    m = ConvLSTM(64, 64, 3, trainable=True).cuda()
    load_seeded(m, 331)
    xs32 = [_t(332 + t, b, 64, h, w).requires_grad_() for t in range(steps)]
    xs = [_cl(v) for v in xs32]
    rh = [_r(342 + t, b, 64, h, w) for t in range(steps)]
    rc = _r(351, b, 64, h, w)
    wt, bs = _stock_params(m.Gates)

    def pkg():
        state, loss = None, 0.0
        for t in range(steps):
            state = m(xs[t], state)
            loss = loss + (state[0].float() * rh[t]).sum()
        return loss + (state[1].float() * rc).sum()

    def stock():
        state, loss = None, 0.0
        for t in range(steps):
            state = _stock_lstm(xs32[t], state, wt, bs)
            loss = loss + (state[0].float() * rh[t]).sum()
        return loss + (state[1].float() * rc).sum()
    _compare_layer(pkg, xs + [m.Gates.weight, m.Gates.bias], stock, xs32 + [wt, bs], [f"dx{t}" for t in range(steps)] + ["dw", "db"])


@gpu
def test_ragged_concat_decoder_gradients():
    import torch.nn.functional as F
    from v2v_amd.unet import UpsampleConvLayer
    from seeded_weights import load_seeded
    b, h, w = 1, 16, 48
    m = UpsampleConvLayer(128, 32, 3, padding=1, trainable=True).cuda()
    load_seeded(m, 361)
    x32, s32 = _t(362, b, 64, h, w).requires_grad_(), _t(363, b, 64, h, w).requires_grad_()
    x, s = _cl(x32), _cl(s32)
    r = _r(364, b, 32, 2 * h, 2 * w)
    wt, bs = _stock_params(m.conv2d)
    stock = lambda: (F.relu(F.conv2d(F.interpolate(torch.cat([x32, s32], 1), scale_factor=2, mode="bilinear", align_corners=False), wt, bs, padding=1)).float() * r).sum()  # noqa: E731
    _compare_layer(lambda: (m(x, s, skip_type="concat").float() * r).sum(), [x, s, m.conv2d.weight, m.conv2d.bias], stock, [x32, s32, wt, bs],
                   ["dx", "dskip", "dw", "db"])
