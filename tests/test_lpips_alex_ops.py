"""The kernels of the LPIPS-AlexNet metric (v2v_amd/csrc/v2v_alex.hpp) pinned one by one through the raw operators of v2v_amd/lpips_alex.py.

Stem and convolution, bit-exact on integers: inputs in [-4, 4] and weights in [-2, 2] keep every partial sum an integer below 2^24 (the
longest sum is K = 3456: 3456 * 8 < 2^15), so every float32 operation is exact and the result must equal the integer evaluation bit for
bit whatever the order of summation.  The integer evaluation is an im2col product in float64, exact for the same reason (checked: it is
integer-valued), converted to int64.  Random integer weights are asymmetric: a row / column swap or a permuted k cannot hide.
Pool: exact for any floats.  Compare: against a float64 NumPy restatement at relative 2^-40 per tap mean -- float64 moments over at most a
few thousand terms, each with a relative rounding of 2^-53, as tests/test_metrics_ops.py reasons."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M_TILE = 128          # pixels per workgroup of alex_conv_kernel (kAlexBM)
CMP_TILE = 64         # pixels per workgroup of alex_compare_kernel (kAlexCmpPix)


def _ints(g, lo, hi, *shape):
    return g.integers(lo, hi + 1, size=shape).astype(np.float32)


def _conv_int(x, w, b, stride, pad, relu):
    """x [n,C,H,W], w [O,C,K,K], b [O] integer-valued float32 -> int64 [n,OH,OW,O] (NHWC)"""
    n, c, h, wd = x.shape
    o, _, k, _ = w.shape
    xp = np.zeros((n, c, h + 2 * pad, wd + 2 * pad), dtype=np.float64)
    xp[:, :, pad:pad + h, pad:pad + wd] = x
    win = np.lib.stride_tricks.sliding_window_view(xp, (k, k), axis=(2, 3))[:, :, ::stride, ::stride]      # [n,C,OH,OW,K,K]
    oh, ow = win.shape[2], win.shape[3]
    cols = win.transpose(0, 2, 3, 1, 4, 5).reshape(n * oh * ow, c * k * k)
    y = cols @ w.astype(np.float64).reshape(o, -1).T + b.astype(np.float64)
    assert np.array_equal(y, np.rint(y)) and np.abs(y).max() < 2 ** 24
    y = y.astype(np.int64).reshape(n, oh, ow, o)
    return np.maximum(y, 0) if relu else y


# ---- stem ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(31, 31), (32, 34), (47, 63)])
@pytest.mark.parametrize("cin", [1, 3])
def test_stem_is_exact_on_integers(cin, hw):
    from v2v_amd import lpips_alex as LA
    h, w = hw
    g = np.random.Generator(np.random.PCG64([34, cin, h, w]))
    n = 3
    x = _ints(g, -4, 4, n, cin, h, w)
    wt, b = _ints(g, -2, 2, 64, 3, 11, 11), _ints(g, -2, 2, 64)
    x3 = np.repeat(x, 3, axis=1) if cin == 1 else x
    want = _conv_int(x3, wt, b, 4, 2, True)
    assert want.shape[1:3] == LA.tap_sizes(h, w)[0] and (want > 0).any() and (want == 0).any()
    dev = torch.device("cuda")
    packed, bias = LA.pack_stem_weights(torch.from_numpy(wt).to(dev)), torch.from_numpy(b).to(dev)
    shift, scale = torch.zeros(3, device=dev), torch.ones(3, device=dev)
    xt = torch.from_numpy(x).to(dev)
    got = LA.stem(xt, xt.stride(0), packed, bias, shift, scale, 1.0, False)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().astype(np.int64), want)
    # frames 37 elements further apart than they are long
    wide = torch.full((n, cin * h * w + 37), 99.0, device=dev)
    wide[:, :cin * h * w] = xt.reshape(n, -1)
    frames = wide[:, :cin * h * w].view(n, cin, h, w)
    assert frames.stride(0) == cin * h * w + 37
    assert torch.equal(LA.stem(frames, frames.stride(0), packed, bias, shift, scale, 1.0, False), got)
    # a frame stride of 0: one frame, n times
    rep = xt[1:2].expand(n, cin, h, w)
    assert rep.stride(0) == 0
    got0 = LA.stem(rep, 0, packed, bias, shift, scale, 1.0, False)
    assert all(torch.equal(got0[i], got[1]) for i in range(n))


def test_stem_prepares_the_image_as_the_reference_does():
    """/ divisor (a true division), 2x - 1, (x - shift) / scale per channel, zero padding AFTER the scaling: against stock float32 torch on
    the CPU with a weight that picks single pixels (one non-zero tap per output channel), so that no sum has more than one term."""
    from v2v_amd import lpips_alex as LA
    g = np.random.Generator(np.random.PCG64(341))
    h, w = 35, 39
    x = (g.random((2, 1, h, w)) * 255).astype(np.float32)
    wt = np.zeros((64, 3, 11, 11), dtype=np.float32)
    for o in range(64):
        wt[o, o % 3, (o * 7) % 11, (o * 5) % 11] = 1.0 if o % 2 else -1.0
    b = np.zeros(64, dtype=np.float32)
    shift, scale = torch.tensor([-.030, -.088, -.188]), torch.tensor([.458, .448, .450])
    xs = torch.from_numpy(x) / torch.tensor(255.0)                       # tensor / tensor: a true division
    xs = ((2 * xs - 1) - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1)
    want = torch.relu(torch.nn.functional.conv2d(xs, torch.from_numpy(wt), stride=4, padding=2)).permute(0, 2, 3, 1)
    dev = torch.device("cuda")
    xt = torch.from_numpy(x).to(dev)
    got = LA.stem(xt, xt.stride(0), LA.pack_stem_weights(torch.from_numpy(wt).to(dev)), torch.from_numpy(b).to(dev), shift.to(dev), scale.to(dev), 255.0, True)
    assert torch.equal(got.cpu(), want)


# ---- convolution ---------------------------------------------------------------------------------------------------------------------------
INSTANCES = [(5, 64, 192), (3, 192, 384), (3, 384, 256), (3, 256, 256)]
MAPS = [(1, 1), (2, 3), (5, 7), (1, M_TILE - 1), (8, M_TILE // 8), (3, (M_TILE + 1) // 3)]


@pytest.mark.parametrize("hw", MAPS, ids=[f"{h}x{w}" for h, w in MAPS])
@pytest.mark.parametrize("inst", INSTANCES, ids=[f"k{k}_{ci}to{co}" for k, ci, co in INSTANCES])
def test_conv_is_exact_on_integers(inst, hw):
    from v2v_amd import lpips_alex as LA
    ks, cin, cout = inst
    h, w = hw
    assert (3 * ((M_TILE + 1) // 3), 8 * (M_TILE // 8)) == (M_TILE + 1, M_TILE)
    g = np.random.Generator(np.random.PCG64([34, ks, cin, cout, h, w]))
    dev = torch.device("cuda")
    wt, b = _ints(g, -2, 2, cout, cin, ks, ks), _ints(g, -2, 2, cout)
    packed, bias = LA.pack_conv_weights(torch.from_numpy(wt).to(dev)), torch.from_numpy(b).to(dev)
    for n in ((1,) if h * w >= M_TILE - 1 else (1, 3)):
        x = _ints(g, -4, 4, n, cin, h, w)
        xt = torch.from_numpy(x).to(dev).permute(0, 2, 3, 1).contiguous()
        for relu in (True, False):
            want = _conv_int(x, wt, b, 1, ks // 2, relu)
            got = LA.conv(xt, packed, bias, ks, relu=relu)
            assert got.shape == (n, h, w, cout) and got.dtype == torch.float32
            assert np.array_equal(got.cpu().numpy().astype(np.int64), want), f"n {n}, relu {relu}"
            assert (want < 0).any() != relu


# ---- max-pool --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(3, 3), (7, 7), (8, 11), (6, 6)])
@pytest.mark.parametrize("c", [64, 192])
def test_pool_is_exact(c, hw):
    from v2v_amd import lpips_alex as LA
    h, w = hw
    g = np.random.Generator(np.random.PCG64([35, c, h, w]))
    x = g.standard_normal((3, c, h, w)).astype(np.float32) - 2.0          # mostly negative: a zero start value would show
    x[1] = g.integers(-3, 1, size=(c, h, w)).astype(np.float32)          # ties
    want = torch.nn.functional.max_pool2d(torch.from_numpy(x), 3, 2).permute(0, 2, 3, 1)
    if hw == (6, 6):
        assert want.shape[1:3] == (2, 2)
    got = LA.pool(torch.from_numpy(x).cuda().permute(0, 2, 3, 1).contiguous())
    assert (want < 0).any(), "negative maxima are there"
    assert got.shape == want.shape and torch.equal(got.cpu(), want)


# ---- compare and sum -----------------------------------------------------------------------------------------------------------------------
def _compare64(f0, f1, w):
    """f0, f1 [n,HW,C], w [C] -> float64 [n]"""
    f0, f1, w = f0.astype(np.float64), f1.astype(np.float64), w.astype(np.float64)
    n0 = f0 / (np.sqrt((f0 ** 2).sum(-1, keepdims=True)) + 1e-10)
    n1 = f1 / (np.sqrt((f1 ** 2).sum(-1, keepdims=True)) + 1e-10)
    return (((n0 - n1) ** 2) * w).sum(-1).mean(-1)


@pytest.mark.parametrize("hw", [1, 6, 35, CMP_TILE - 1, CMP_TILE, CMP_TILE + 1])
@pytest.mark.parametrize("c", [64, 192, 384, 256])
def test_compare_matches_the_float64_restatement(c, hw):
    from v2v_amd import lpips_alex as LA
    g = np.random.Generator(np.random.PCG64([36, c, hw]))
    n = 4
    f0 = np.maximum(g.standard_normal((n, hw, c)), 0).astype(np.float32)
    f1 = np.maximum(g.standard_normal((n, hw, c)), 0).astype(np.float32)
    f0[1, 0] = 0.0                                   # all-zero features in one image
    f0[2, hw - 1] = 0.0                              # ... and in both
    f1[2, hw - 1] = 0.0
    f1[3] = f0[3]                                    # identical taps
    w = g.random(c).astype(np.float32)
    w[::7] = 0.0                                     # the reference's lin weights hold exact zeros
    want = _compare64(f0, f1, w)
    dev = torch.device("cuda")
    taps = torch.full((n, 5), -1.0, dtype=torch.float64, device=dev)
    tap = (c + hw) % 5
    a, b = (torch.from_numpy(f).to(dev).reshape(n, 1, hw, c) for f in (f0, f1))
    LA.compare(a, b, torch.from_numpy(w).to(dev), tap, taps)
    got = taps.cpu().numpy()
    assert np.isfinite(got).all() and (np.delete(got, tap, axis=1) == -1.0).all()
    assert got[3, tap] == 0.0 and want[3] == 0.0
    assert (np.abs(got[:, tap] - want) <= 2.0 ** -40 * want).all(), (got[:, tap], want)
    again = torch.full((n, 5), -1.0, dtype=torch.float64, device=dev)
    LA.compare(a, b, torch.from_numpy(w).to(dev), tap, again)
    assert torch.equal(again, taps)


def test_sum_adds_the_float32_taps_in_order():
    from v2v_amd import lpips_alex as LA
    g = np.random.Generator(np.random.PCG64(37))
    taps = g.random((300, 5)) * np.array([1.0, 1e-3, 10.0, 1e-7, 0.3])
    want = taps[:, 0].astype(np.float32)
    for k in range(1, 5):
        want = want + taps[:, k].astype(np.float32)
    got = LA.tap_sum(torch.from_numpy(taps).cuda())
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
