"""The backward kernels of LPIPS-AlexNet (v2v_amd/csrc/v2v_alex_train.hpp) pinned one by one through the raw operators of
v2v_amd/lpips_alex.py.

Convolution input gradient and stem backward, bit-exact on integers: dy in [-4, 4] and weights in [-2, 2] keep every partial sum an
integer far below 2^24 (the longest sum is K = 9 * 384 = 3456 terms of at most 8), so every float32 operation is exact and the result
must equal torch's float64 autograd of conv2d (exact for the same reason) bit for bit whatever the order of summation.  Random integer
weights are asymmetric: a missing flip, a transposed pack or a permuted k cannot hide.
Pool backward, bit-exact against max_pool2d's backward on the device: dy holds small integers, because torch's backward adds the up to
four windows of a pixel with atomics in no fixed order -- on integers every order gives the same bits.
Compare backward against the formula in float64 (itself checked against torch's float64 autograd of the forward expression): the kernel
evaluates in float64 and rounds once, so |got - want| <= 2^-24 |want| (half a float32 ulp), plus 2^-45 (|g / n0| + |f0 * second|) for the
float64 evaluation order on the two terms that may cancel, plus the smallest denormal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ints(g, lo, hi, *shape):
    return g.integers(lo, hi + 1, size=shape).astype(np.float32)


def _nhwc(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).permute(0, 2, 3, 1).contiguous()


# ---- convolution input gradient --------------------------------------------------------------------------------------------------------------
# (ks, the forward's Cin, Cout, n, H, W): 256->256 on one pixel; 384->192 on 189 pixels (two GEMM tiles, the second partial); the 5x5 layer
# on a map smaller than its kernel and on 135 pixels; 256->384 for the fourth instance of the network
DGRAD = [(3, 256, 256, 1, 1, 1), (3, 192, 384, 3, 7, 9), (5, 64, 192, 2, 3, 3), (5, 64, 192, 1, 9, 15), (3, 384, 256, 1, 2, 3)]


@pytest.mark.parametrize("case", DGRAD, ids=[f"k{k}_{co}to{ci}_n{n}_{h}x{w}" for k, ci, co, n, h, w in DGRAD])
def test_conv_dgrad_is_exact_on_integers(case):
    from v2v_amd import lpips_alex as LA
    ks, cin, cout, n, h, w = case
    g = np.random.Generator(np.random.PCG64([35, ks, cin, cout, n, h, w]))
    wt, dy = _ints(g, -2, 2, cout, cin, ks, ks), _ints(g, -4, 4, n, cout, h, w)
    dtap = _ints(g, -8, 8, n, cin, h, w)
    mask = np.maximum(g.standard_normal((n, cin, h, w)), 0).astype(np.float32)       # a post-ReLU activation: about half zeros
    mask[:, ::5] *= -1.0                                                               # "not > 0" holds for negative values and -0.0 too
    x = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
    F.conv2d(x, torch.from_numpy(wt).double(), padding=ks // 2).backward(torch.from_numpy(dy).double())
    want = x.grad.numpy()
    assert np.array_equal(want, np.rint(want)) and np.abs(want).max() + 8 < 2 ** 24 and (want != 0).any()
    packed = LA.pack_dgrad_weights(torch.from_numpy(wt).to(DEV))
    dyt, dt, mt = _nhwc(dy), _nhwc(dtap), _nhwc(mask)
    for use_tap in (False, True):
        for use_mask in (False, True):
            ref = (want + dtap if use_tap else want) * ((mask > 0) if use_mask else 1.0)
            got = LA.conv_dgrad(dyt, packed, ks, dtap=dt if use_tap else None, mask=mt if use_mask else None)
            assert got.shape == (n, h, w, cin) and got.dtype == torch.float32
            assert np.array_equal(got.permute(0, 3, 1, 2).cpu().numpy().astype(np.float64), ref + 0.0), f"dtap {use_tap}, mask {use_mask}"
    assert torch.equal(LA.conv_dgrad(dyt, packed, ks, dtap=dt, mask=mt), got)


def test_conv_dgrad_does_not_depend_on_what_shares_the_launch():
    from v2v_amd import lpips_alex as LA
    g = np.random.Generator(np.random.PCG64(351))
    wt = (g.standard_normal((384, 192, 3, 3)) * 0.05).astype(np.float32)
    dy = _nhwc(g.standard_normal((5, 384, 7, 7)).astype(np.float32))
    packed = LA.pack_dgrad_weights(torch.from_numpy(wt).to(DEV))
    all5 = LA.conv_dgrad(dy, packed, 3)
    for i in range(5):
        assert torch.equal(LA.conv_dgrad(dy[i:i + 1].contiguous(), packed, 3)[0], all5[i])


# ---- max-pool backward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(3, 3), (7, 7), (8, 10)])
@pytest.mark.parametrize("c", [64, 192])
@pytest.mark.parametrize("ties", [False, True])
def test_pool_bwd_matches_max_pool2d_backward(ties, c, hw):
    from v2v_amd import lpips_alex as LA
    h, w = hw
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    g = np.random.Generator(np.random.PCG64([35, c, h, w, int(ties)]))
    n = 2
    if ties:
        x = g.integers(0, 4, size=(n, c, h, w)).astype(np.float32)            # tied positive maxima in most windows
    else:
        x = np.maximum(g.standard_normal((n, c, h, w)), 0).astype(np.float32)
        x[1] = g.standard_normal((c, h, w)).astype(np.float32) - 2.0           # all negative: the maximum is not a ReLU survivor
    dy, dtap = _ints(g, -4, 4, n, c, oh, ow), _ints(g, -8, 8, n, c, h, w)
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    F.max_pool2d(xt, 3, 2).backward(torch.from_numpy(dy).to(DEV))
    want = xt.grad.cpu().numpy()
    assert (want != 0).any()
    if hw == (8, 10):
        assert (oh, ow) == (3, 4) and not want[:, :, 7].any() and not want[:, :, :, 9].any(), "floor mode drops the last row and column"
    if ties:
        win = np.lib.stride_tricks.sliding_window_view(x, (3, 3), axis=(2, 3))[:, :, ::2, ::2].reshape(n, c, oh, ow, 9)
        assert ((win == win.max(-1, keepdims=True)).sum(-1) > 1).mean() > 0.5 and (win.max(-1) > 0).mean() > 0.99
    a, d, t = _nhwc(x), _nhwc(dy), _nhwc(dtap)
    for use_tap in (False, True):
        for use_mask in (False, True):
            ref = (want + dtap if use_tap else want) * ((x > 0) if use_mask else 1.0)
            got = LA.pool_bwd(a, d, dtap=t if use_tap else None, relu_mask=use_mask)
            assert got.shape == (n, h, w, c) and got.dtype == torch.float32
            assert np.array_equal(got.permute(0, 3, 1, 2).cpu().numpy(), (ref + 0.0).astype(np.float32)), f"dtap {use_tap}, mask {use_mask}"
    if hw == (8, 10):
        assert torch.equal(got[:, 7], (t * (a > 0))[:, 7]) and torch.equal(got[:, :, 9], (t * (a > 0))[:, :, 9]), "dropped row / column: dtap only"


# ---- stem backward -----------------------------------------------------------------------------------------------------------------------------
def _stem_grad64(dz, wt, cin, h, w):
    """dz [n,64,OH,OW], wt [64,3,11,11] -> float64 [n,cin,h,w]: torch's float64 autograd of the stem's convolution, a one-channel image read
    three times"""
    x = torch.zeros((dz.shape[0], cin, h, w), dtype=torch.float64, requires_grad=True)
    x3 = x.expand(-1, 3, -1, -1) if cin == 1 else x
    F.conv2d(x3, torch.from_numpy(wt).double(), stride=4, padding=2).backward(torch.from_numpy(dz).double())
    return x.grad.numpy()


@pytest.mark.parametrize("hw", [(31, 31), (47, 143)])
@pytest.mark.parametrize("cin", [1, 3])
def test_stem_bwd_is_exact_on_integers(cin, hw):
    from v2v_amd import lpips_alex as LA
    h, w = hw
    (oh, ow) = LA.tap_sizes(h, w)[0]
    g = np.random.Generator(np.random.PCG64([35, cin, h, w]))
    n = 2
    dz, wt = _ints(g, -4, 4, n, 64, oh, ow), _ints(g, -2, 2, 64, 3, 11, 11)
    want = _stem_grad64(dz, wt, cin, h, w)
    assert np.array_equal(want, np.rint(want)) and np.abs(want).max() < 2 ** 22 and (want != 0).any()
    packed, one = LA.pack_stem_weights(torch.from_numpy(wt).to(DEV)), torch.ones(3, device=DEV)
    dzt = _nhwc(dz)
    got = LA.stem_bwd(dzt, packed, one, cin, h, w)
    assert got.shape == (n, cin, h, w) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want + 0.0)
    # * 2 (exact) and / 255: one float32 rounding of an exact integer quotient -- the float64 quotient rounded to float32 is that value
    # (53 >= 2 * 24 + 2 bits: the double rounding is innocuous for a division)
    got = LA.stem_bwd(dzt, packed, one, cin, h, w, divisor=255.0, normalize=True)
    assert np.array_equal(got.cpu().numpy(), (2.0 * want / 255.0).astype(np.float32) + np.float32(0))
    assert np.array_equal(LA.stem_bwd(dzt, packed, one, cin, h, w, divisor=255.0).cpu().numpy(), (want / 255.0).astype(np.float32) + np.float32(0))
    if cin == 3:
        # the scaling layer's own divisors, per channel: integer / scale[c] in float32, once
        scale = np.array([.458, .448, .450], dtype=np.float32)
        got = LA.stem_bwd(dzt, packed, torch.from_numpy(scale).to(DEV), cin, h, w, normalize=True)
        ref = np.float32(2) * (want.astype(np.float32) / scale.reshape(1, 3, 1, 1))
        assert np.array_equal(got.cpu().numpy(), ref + np.float32(0))
    # an image alone gives the bits it has in the batch
    assert torch.equal(LA.stem_bwd(dzt[1:2].contiguous(), packed, one, cin, h, w)[0], LA.stem_bwd(dzt, packed, one, cin, h, w)[1])


# ---- compare backward --------------------------------------------------------------------------------------------------------------------------
def _compare_bwd64(f0, f1, w, ddist):
    """f0, f1 [n,HW,C] -> (df0 float64, the magnitude of the two terms that are subtracted): the issue's formula, the norm's derivative
    taken as 0 at a pixel whose pred features are all zero"""
    f0, f1, w = f0.astype(np.float64), f1.astype(np.float64), w.astype(np.float64)
    hw = f0.shape[1]
    r0 = np.sqrt((f0 ** 2).sum(-1, keepdims=True))
    n0, n1 = r0 + 1e-10, np.sqrt((f1 ** 2).sum(-1, keepdims=True)) + 1e-10
    g = 2 * w * (f0 / n0 - f1 / n1) * (ddist.astype(np.float64).reshape(-1, 1, 1) / hw)
    dot = (g * f0).sum(-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        second = np.where(r0 > 0, dot / (r0 * n0 ** 2), 0.0)
    return g / n0 - f0 * second, np.abs(g / n0) + np.abs(f0 * second)


@pytest.mark.parametrize("hw", [1, 49, 65])
@pytest.mark.parametrize("c", [64, 192, 256, 384])
def test_compare_bwd_matches_the_float64_formula(c, hw):
    from v2v_amd import lpips_alex as LA
    g = np.random.Generator(np.random.PCG64([36, c, hw]))
    n = 3
    f0 = np.maximum(g.standard_normal((n, hw, c)), 0).astype(np.float32)
    f1 = np.maximum(g.standard_normal((n, hw, c)), 0).astype(np.float32)
    f0[1, 0] = 0.0                                   # a pixel whose pred features are all zero
    w = g.random(c).astype(np.float32)
    w[::7] = 0.0                                     # the reference's lin weights hold exact zeros
    ddist = np.array([0.5, -1.25, 2.0], dtype=np.float32)
    want, mag = _compare_bwd64(f0, f1, w, ddist)
    # the formula is torch's float64 autograd of the forward expression wherever the features are not all zero
    t0 = torch.from_numpy(f0).double().requires_grad_(True)
    t1, tw = torch.from_numpy(f1).double(), torch.from_numpy(w).double()
    nrm = lambda f: f / (torch.sqrt((f ** 2).sum(-1, keepdim=True)) + 1e-10)   # noqa: E731
    ((((nrm(t0) - nrm(t1)) ** 2) * tw).sum(-1).mean(-1) * torch.from_numpy(ddist).double()).sum().backward()
    auto = t0.grad.numpy()
    live = np.ones((n, hw), dtype=bool)
    live[1, 0] = False
    assert np.isnan(auto[1, 0]).all(), "the reference's gradient is NaN there"
    assert (np.abs(auto[live] - want[live]) <= 1e-12 * np.abs(want[live]).max()).all()
    # the stated value at the all-zero pixel: g_c / 1e-10 with g_c = -2 w_c f1_c / n1 * ddist / HW -- large and finite
    n1 = np.sqrt((f1[1, 0].astype(np.float64) ** 2).sum()) + 1e-10
    stated = -2.0 * w.astype(np.float64) * f1[1, 0] / n1 * (float(ddist[1]) / hw) / 1e-10
    assert np.allclose(want[1, 0], stated, rtol=1e-12, atol=0) and np.abs(stated).max() < 1e30
    a, b = (torch.from_numpy(f).to(DEV).reshape(n, 1, hw, c) for f in (f0, f1))
    wt, dd = torch.from_numpy(w).to(DEV), torch.from_numpy(ddist).to(DEV)
    bound = 2.0 ** -24 * np.abs(want) + 2.0 ** -45 * mag + 2.0 ** -149
    for relu_mask in (False, True):
        got = LA.compare_bwd(a, b, wt, dd, relu_mask=relu_mask)
        assert got.shape == (n, 1, hw, c) and got.dtype == torch.float32
        got = got.reshape(n, hw, c).cpu().numpy().astype(np.float64)
        ref = want * (f0 > 0) if relu_mask else want
        assert np.isfinite(got).all()
        err = np.abs(got - ref)
        print(f"compare_bwd C {c} HW {hw} mask {relu_mask}: largest error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        if relu_mask:
            assert not got[1, 0].any()
        else:
            assert (np.abs(got[1, 0] - stated) <= 2.0 ** -24 * np.abs(stated) * (1 + 1e-6)).all() and got[1, 0].any()
    assert torch.equal(LA.compare_bwd(a, b, wt, dd.reshape(n, 1, 1, 1), relu_mask=True).reshape(n, hw, c).cpu().double(), torch.from_numpy(got))
    # an image alone gives the bits it has in the batch
    assert torch.equal(LA.compare_bwd(a[2:3].contiguous(), b[2:3].contiguous(), wt, dd[2:3].contiguous())[0], LA.compare_bwd(a, b, wt, dd)[2])
