"""The LPIPS kernels (v2v_amd/csrc/v2v_lpips.hpp) one by one against a float64 reference of their own operation, with the method of
tests/test_backward_ops.py: bit-exact wherever the arithmetic allows (small integers, multiples of 1/4, a power-of-two scale), and where
it does not, the bf16 rounding bound 2^-8 or -- for the float32 compare step -- the rule of tests/test_loss_ops.py: max error <= 4 x and
rms <= 2 x the error of the same formula run in float32 on the CPU, measured here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
F64, BF16 = torch.float64, torch.bfloat16
REAL_SHIFT, REAL_SCALE = (-.030, -.088, -.188), (.458, .448, .450)
STEM_SHAPES = [(1, 1, 4, 4), (2, 3, 6, 10), (1, 1, 16, 20)]          # every pixel on the border | 3 channels | two tiles, the last partial


def rng(seed):
    return np.random.default_rng(seed)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def ints(g, lo, hi, shape):
    return torch.from_numpy(g.integers(lo, hi + 1, shape).astype(np.float64))


# ---- 2x2 max-pool -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 2, 64), (3, 6, 10, 128), (2, 4, 4, 512)])
def test_pool_forward_and_backward_equal_float64_bit_for_bit_with_ties(shape):
    from v2v_amd import loss_ops
    g = rng(sum(shape))
    x = ints(g, 0, 3, shape)                                           # four values only: most windows hold a tie
    xr = nchw(x).requires_grad_(True)
    y = F.max_pool2d(xr, 2, 2)
    got = loss_ops.lpips_pool(x.to(BF16).cuda())
    assert got.dtype == BF16 and torch.equal(got.double().cpu(), nhwc(y.detach()))
    dy = ints(g, -3, 3, got.shape)
    y.backward(nchw(dy))
    want = nhwc(xr.grad)
    assert int((want != 0).sum()) > 0
    got_dx = loss_ops.lpips_pool_bwd(dy.to(BF16).cuda(), x.to(BF16).cuda())
    assert torch.equal(got_dx.double().cpu(), want)
    # + the tap's own gradient, in float32 with ONE rounding (128..255 + 128..255 passes 256, where bf16 keeps even integers only), and the mask
    dy = ints(g, 128, 255, got.shape)
    dtap = ints(g, 128, 255, shape)
    xr.grad = None
    F.max_pool2d(xr, 2, 2).backward(nchw(dy))
    total = nhwc(xr.grad) + dtap
    assert float(total.max()) > 256 and bool((total % 2 == 1).any())
    got_sum = loss_ops.lpips_pool_bwd(dy.to(BF16).cuda(), x.to(BF16).cuda(), dtap=dtap.to(BF16).cuda())
    assert torch.equal(got_sum.cpu(), total.to(BF16))
    got_masked = loss_ops.lpips_pool_bwd(dy.to(BF16).cuda(), x.to(BF16).cuda(), dtap=dtap.to(BF16).cuda(), relu_mask=True)
    assert torch.equal(got_masked.cpu(), torch.where(x > 0, total, torch.zeros_like(total)).to(BF16))
    assert bool((x == 0).any())


# ---- stem -------------------------------------------------------------------------------------------------------------------------------
def stem_ref(x, weight, bias, shift, scale, normalize):
    """float64: the scaling layer, then the zero-padded 3x3 convolution, bias, ReLU -> NHWC."""
    if x.shape[1] == 1:
        x = torch.cat([x, x, x], dim=1)
    if normalize:
        x = 2 * x - 1
    s = (x - shift.reshape(1, 3, 1, 1)) / scale.reshape(1, 3, 1, 1)
    return nhwc(F.relu(F.conv2d(s, weight, bias, padding=1)))


def stem_operands(g, shape, exact, shift=(0.0, 0.0, 0.0)):
    x = ints(g, 0, 4, shape) / 4
    if exact:
        weight, bias = ints(g, -2, 2, (64, 3, 3, 3)), ints(g, -2, 2, (64,))
        return x, weight, bias, torch.tensor(shift, dtype=F64), torch.full((3,), 0.5, dtype=F64)
    weight = torch.from_numpy(g.standard_normal((64, 3, 3, 3)).astype(np.float32)).double()
    bias = torch.from_numpy(g.standard_normal(64).astype(np.float32)).double()
    return x, weight, bias, torch.tensor(REAL_SHIFT, dtype=torch.float32).double(), torch.tensor(REAL_SCALE, dtype=torch.float32).double()


def run_stem(x, weight, bias, shift, scale, normalize, dtype=torch.float32):
    from v2v_amd import loss_ops
    return loss_ops.lpips_stem(x.to(dtype).cuda(), weight.float().cuda(), bias.float().cuda(), shift.float().cuda(), scale.float().cuda(), normalize)


@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_forward_equals_float64_bit_for_bit_on_exact_operands(shape):
    g = rng(100 + sum(shape))
    for shift in ((0.0, 0.0, 0.0), (0.25, -0.5, 0.75)):              # a non-zero shift: padding before the scaling would put -shift / scale there
        for normalize in (False, True):
            ops = stem_operands(g, shape, True, shift)
            want = stem_ref(*ops, normalize)
            assert float(want.max()) > 0
            got = run_stem(*ops, normalize)
            assert got.dtype == BF16 and tuple(got.shape) == (shape[0], shape[2], shape[3], 64)
            assert torch.equal(got.cpu(), want.to(BF16)), (shift, normalize)
    got16 = run_stem(*ops, True, dtype=BF16)                           # multiples of 1/4: exact in bf16, so a bf16 image gives the same bits
    assert torch.equal(got16, got)


@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_forward_within_the_bf16_rounding_bound_on_real_operands(shape):
    g = rng(200 + sum(shape))
    ops = stem_operands(g, shape, False)
    for normalize in (False, True):
        want = stem_ref(*ops, normalize)
        got = run_stem(*ops, normalize).double().cpu()
        err = float(((got - want).abs() / (want.abs() + 1)).max())
        print(f"stem {shape} normalize={normalize}: max |got - want| / (|want| + 1) = {err:.2e} (bound 2^-8 = {2 ** -8:.2e})")
        assert err < 2 ** -8
    # the real shift is not zero: a kernel that pads BEFORE the scaling layer is off by |shift / scale| * |w| ~ 0.1 .. 1 on the border
    padded_first = nhwc(F.relu(F.conv2d(F.pad((torch.cat([ops[0]] * 3, 1) if shape[1] == 1 else ops[0]), (1, 1, 1, 1)).sub(ops[3].reshape(1, 3, 1, 1))
                                        .div(ops[4].reshape(1, 3, 1, 1)), ops[1], ops[2])))
    assert float(((padded_first - stem_ref(*ops, False)).abs() / (stem_ref(*ops, False).abs() + 1)).max()) > 2 ** -6


@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_backward_equals_float64_exactly_on_integers(shape):
    from v2v_amd import loss_ops
    g = rng(300 + sum(shape))
    x, weight, bias, shift, scale = stem_operands(g, shape, True)
    b, cin, h, w = shape
    dz = ints(g, -2, 2, (b, h, w, 64))
    for normalize, factor in ((True, 4.0), (False, 2.0)):            # (2 if normalize else 1) / 0.5
        xr = x.clone().requires_grad_(True)
        x3 = torch.cat([xr, xr, xr], dim=1) if cin == 1 else xr
        s = ((2 * x3 - 1 if normalize else x3) - shift.reshape(1, 3, 1, 1)) / scale.reshape(1, 3, 1, 1)
        F.conv2d(s, weight, bias, padding=1).backward(nchw(dz))
        want = xr.grad
        assert torch.equal(want, factor * (F.conv_transpose2d(nchw(dz), weight, padding=1) if cin == 3
                                           else F.conv_transpose2d(nchw(dz), weight, padding=1).sum(1, keepdim=True)))
        got = loss_ops.lpips_stem_bwd(dz.to(BF16).cuda(), weight.float().cuda(), scale.float().cuda(), cin, normalize)
        assert got.dtype == torch.float32 and tuple(got.shape) == shape
        assert torch.equal(got.double().cpu(), want), normalize
    assert float(want.abs().max()) > 0


# ---- compare ------------------------------------------------------------------------------------------------------------------------------
def compare_ref(f0, f1, w, ddist, dtype):
    """The formulas of the issue in `dtype` on the CPU: (dist [B], df0 [B,H,W,Cc]); f0, f1 [B,H,W,Cc], w [Cc], ddist [B].  The second term of
    df0 is 0 where |f0| == 0."""
    f0, f1, w, ddist = (t.to(dtype) for t in (f0, f1, w, ddist))
    eps = torch.tensor(1e-10, dtype=dtype)
    hw = f0.shape[1] * f0.shape[2]
    r = torch.sqrt((f0 ** 2).sum(-1, keepdim=True))
    n0, n1 = f0 / (r + eps), f1 / (torch.sqrt((f1 ** 2).sum(-1, keepdim=True)) + eps)
    dist = (w * (n0 - n1) ** 2).sum(-1).mean((1, 2))
    gq = 2 * w * (n0 - n1) * (ddist.reshape(-1, 1, 1, 1) / hw)
    second = f0 * (gq * f0).sum(-1, keepdim=True) / (r * (r + eps) ** 2)
    return dist, gq / (r + eps) - torch.where(r > 0, second, torch.zeros_like(second))


def compare_operands(cc, hw, zero_pixel=False):
    h, w = {4: (2, 2), 48: (6, 8), 1024: (32, 32)}[hw]
    g = rng(cc + hw)
    f0, f1 = (torch.from_numpy(np.maximum(3 * g.standard_normal((2, h, w, cc)), 0).astype(np.float32)).to(BF16) for _ in range(2))
    if zero_pixel:
        f0[1, 0, 1, :] = 0
    wl = torch.from_numpy(g.uniform(0.05, 1.0, cc).astype(np.float32))
    return f0, f1, wl, torch.tensor([1.0, 2.0])


@pytest.mark.parametrize("cc", [64, 512])
@pytest.mark.parametrize("hw", [4, 48, 1024])
def test_compare_forward_and_backward_within_the_float32_yardstick(cc, hw):
    from v2v_amd import loss_ops
    f0, f1, w, ddist = compare_operands(cc, hw)
    want_d, want_g = compare_ref(f0, f1, w, ddist, F64)
    if hw == 48:                                                       # the closed form IS the gradient of the forward formula
        leaf = f0.double().requires_grad_(True)
        (compare_ref(leaf, f1, w, ddist, F64)[0] * ddist.double()).sum().backward()
        assert float((leaf.grad - want_g).abs().max()) <= 1e-12 * float(want_g.abs().max())
    y_d, y_g = compare_ref(f0, f1, w, ddist, torch.float32)
    # two samples only: the float32 run can land closer than float32 resolves; floor of one ulp of the value, as in tests/test_loss_ops.py
    floor = 2.0 ** -23 * float(want_d.abs().max())
    e = (y_d.double() - want_d).abs()
    yard_d = (max(float(e.max()), floor), max(float((e ** 2).mean().sqrt()), floor))
    yard_g = float((y_g.double() - want_g).abs().max())
    dist = torch.zeros(2, dtype=torch.float32, device="cuda")
    out = loss_ops.lpips_compare_fwd(f0.cuda(), f1.cuda(), w.cuda(), dist)
    assert out is dist
    e = (dist.double().cpu() - want_d).abs()
    mx, rms = float(e.max()), float((e ** 2).mean().sqrt())
    print(f"compare fwd Cc {cc} HW {hw}: max {mx:.2e} = {mx / yard_d[0]:.2f} x yardstick, rms {rms:.2e} = {rms / yard_d[1]:.2f} x yardstick")
    assert mx <= 4 * yard_d[0] and rms <= 2 * yard_d[1]
    once = dist.clone()
    loss_ops.lpips_compare_fwd(f0.cuda(), f1.cuda(), w.cuda(), dist)      # accumulates: the five taps share one dist
    assert torch.equal(dist, once + once)
    got_g = loss_ops.lpips_compare_bwd(f0.cuda(), f1.cuda(), w.cuda(), ddist.cuda())
    assert got_g.dtype == BF16 and got_g.shape == f0.shape
    over = ((got_g.double().cpu() - want_g).abs() - (2.0 ** -8 * want_g.abs() + 4 * yard_g)).max()
    print(f"compare bwd Cc {cc} HW {hw}: float32 yardstick max {yard_g:.2e}, worst excess over the bound {float(over):.2e}")
    assert float(over) <= 0


@pytest.mark.parametrize("cc", [64, 512])
def test_compare_backward_at_an_all_zero_pixel_is_finite_and_the_first_term_only(cc):
    from v2v_amd import loss_ops
    f0, f1, w, ddist = compare_operands(cc, 48, zero_pixel=True)
    want_d, want_g = compare_ref(f0, f1, w, ddist, F64)
    _, y_g = compare_ref(f0, f1, w, ddist, torch.float32)
    leaf = f0.double().requires_grad_(True)
    (compare_ref(leaf, f1, w, ddist, F64)[0] * ddist.double()).sum().backward()
    assert bool(torch.isnan(leaf.grad[1, 0, 1]).all()) and int(torch.isnan(leaf.grad).sum()) == cc      # autograd: NaN there, and only there
    n1 = f1.double()[1, 0, 1] / (f1.double()[1, 0, 1].norm() + 1e-10)
    first = 2 * w.double() * (0 - n1) * (2.0 / 48) / 1e-10
    assert torch.allclose(want_g[1, 0, 1], first, rtol=1e-12, atol=0) and float(first.abs().max()) > 1e6
    got = loss_ops.lpips_compare_bwd(f0.cuda(), f1.cuda(), w.cuda(), ddist.cuda()).double().cpu()
    assert bool(torch.isfinite(got).all())
    keep = torch.ones(got.shape[:3], dtype=torch.bool)
    keep[1, 0, 1] = False
    yard = float((y_g.double() - want_g)[keep].abs().max())
    assert float(((got - want_g).abs() - (2.0 ** -8 * want_g.abs() + 4 * yard))[keep].max()) <= 0
    # the zero pixel: g / eps with eps = 1e-10 rounded to float32 (relative 3e-8) and one bf16 rounding
    assert float(((got - want_g)[1, 0, 1].abs() / first.abs().clamp_min(1e-30)).max()) <= 2.0 ** -8
    dist = loss_ops.lpips_compare_fwd(f0.cuda(), f1.cuda(), w.cuda(), torch.zeros(2, dtype=torch.float32, device="cuda"))
    assert float((dist.double().cpu() - want_d).abs().max()) <= 1e-5 * float(want_d.max())
