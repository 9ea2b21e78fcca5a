"""NER-Net's learned voxelisation on the GPU (v2v_amd/nernet.py, v2v_nernet.hpp) against golden G32 and the stock restatement
(tests/nernet_stock.py):

  * normalisation: t_out equals G32's t_n bit for bit in every golden case;
  * integer-exact scatter: on the inputs of tests/nernet_inputs.py every sum is exact in any order, so the grid equals the float64
    restatement bit for bit -- across wave and workgroup borders, every padded-width instance, the polarity-half order, clamp, wrap-once,
    dropped, raw 0/1 polarity and the empty-interval row; the combined layer too;
  * one-hot: one event lands in exactly C cells;
  * real-valued accuracy against G32's float64 truth: max and rms of |device - truth| at most 2x the same norms of the reference's float32
    output (recorded in G32).  Measured on an MI355X (device / reference, max and rms; the test prints them):
        real_c5_f64 0.83 0.90   real_c5_f64_norm 1.04 0.91   real_c9_f32 0.73 0.86   real_c9_f32_norm 0.86 0.81
        real_c5_f32_b3 0.54 0.89   real_c5_f32_b3_norm 0.51 0.93   real_c4_f64_norm 1.56 0.95   real_c4_f64 0.67 0.92
    (the maxima move with the order in which the float32 atomics land -- real_c4_f64_norm 1.19 and 1.56 in two runs -- the rms figures stay);
  * forward_sequence equals forward per interval: bit for bit on the exact inputs, within m 2^-24 sum |terms| per cell on real ones;
  * batch_size= given: no host synchronisation."""
import numpy as np
import pytest
import torch
from torch import nn

import nernet_inputs as NI
import nernet_stock as NS
import seeded_weights as SW

pytestmark = pytest.mark.gpu
H, W = 12, 20


@pytest.fixture(scope="module")
def g32(golden):
    return golden("g32_nernet_voxelization.npz")


def _cases():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g32_nernet_voxelization.npz"))
    return [str(c) for c in z["cases"]]


def _golden_layer(g32, name):
    from v2v_amd import nernet
    Cb, h, w, B, norm, comb, seed = (int(v) for v in g32[f"{name}__cfg"])
    slope = float(g32[f"{name}__slope"][0])
    cls = nernet.QuantizationLayer_trail_combined if comb else nernet.QuantizationLayer_trail
    layer = cls((Cb, h, w), [int(v) for v in g32[f"{name}__mlp"]], nn.ReLU() if slope == 0.0 else nn.LeakyReLU(negative_slope=slope), bool(norm))
    SW.load_seeded(layer.value_layer, seed)
    return layer.cuda(), B


def _run_golden(g32, name, **kw):
    from v2v_amd import nernet
    layer, B = _golden_layer(g32, name)
    w, b = layer._params()
    ev = torch.from_numpy(g32[f"{name}__events"]).cuda()
    with torch.no_grad():
        out, tn = nernet.learned_voxel(ev, w, b, layer.dim, layer.slope, layer.normalize, layer.combined, return_t=True, **kw)
    return out, tn, B


@pytest.mark.parametrize("name", _cases())
def test_normalised_time_is_the_references_bit_for_bit(g32, name):
    out, tn, B = _run_golden(g32, name)
    assert out.shape == g32[f"{name}__out"].shape and out.dtype == torch.float32
    assert np.array_equal(tn.cpu().numpy(), g32[f"{name}__tn"], equal_nan=True)
    # the grid itself: loosely here (the accuracy test below is the sharp one), so that a wrong cell shows in every case
    np.testing.assert_allclose(out.cpu().numpy(), g32[f"{name}__out"], rtol=1e-4, atol=1e-4 * float(np.abs(g32[f"{name}__out"]).max() + 1))


@pytest.mark.parametrize("name", [c for c in _cases() if c.startswith("real_")])
def test_real_valued_accuracy_against_the_float64_truth(g32, name):
    out, _, _ = _run_golden(g32, name)
    err = np.abs(out.cpu().numpy().astype(np.float64) - g32[f"{name}__truth"])
    ref_max, ref_rms = g32[f"{name}__err"]
    got_max, got_rms = err.max(), np.sqrt((err ** 2).mean())
    print(f"{name}: device / reference error  max {got_max / ref_max:.2f}  rms {got_rms / ref_rms:.2f}   (reference max {ref_max:.3g} rms {ref_rms:.3g})")
    assert got_max <= 2 * ref_max and got_rms <= 2 * ref_rms


def _exact(ev, mlp, Cb, B, hw, combined=False, seed=3):
    """(device grid, float64 restatement, float64 sum of magnitudes) on integer-exact inputs"""
    from v2v_amd import nernet
    h, w = hw
    ws, bs = NI.exact_mlp(mlp, seed)
    tn = NS.normalise_t(ev, B, Cb, False).float()
    want = NS.truth64(ev, tn, ws, bs, (Cb, h, w), NI.SLOPE, False, combined, B, drop_below=True)
    mag = NS.truth64(ev, tn, ws, bs, (Cb, h, w), NI.SLOPE, False, combined, B, drop_below=True, reduce="abs")
    assert float(mag.max()) < 2 ** 18 and bool((want * 64 == (want * 64).round()).all()), "the test's own inputs must make every sum exact"
    with torch.no_grad():
        got, tn_dev = nernet.learned_voxel(ev.cuda(), [v.cuda() for v in ws], [v.cuda() for v in bs], (Cb, h, w), NI.SLOPE, combined=combined, batch_size=B,
                                           return_t=True)
    assert torch.equal(tn_dev.cpu(), tn)
    return got.cpu(), want, mag


@pytest.mark.parametrize("hw", [(12, 20), (1, 7)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Cb", [2, 5, 9])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_integer_exact_scatter(n, Cb, B, hw):
    mlps = [[1, 7, 1], [1, 30, 30, 1], [1, 50, 50, 50, 1], [1, 128, 128, 1]]
    mlp = mlps[([1, 63, 64, 65, 257, 4097].index(n) + Cb + B) % 4]
    ev = NI.with_specials(NI.exact_rows(7, n, Cb, B, hw[0], hw[1]), Cb, B, hw[0], hw[1])
    got, want, _ = _exact(ev, mlp, Cb, B, hw)
    assert got.shape == (B, 2 * Cb, hw[0], hw[1]) and float(want.abs().max()) > 0
    assert torch.equal(got.double(), want), f"{int((got.double() != want).sum())} cells differ"


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mlp", [[1, 7, 1], [1, 30, 30, 1], [1, 50, 50, 50, 1], [1, 128, 128, 1], [1, 16, 17, 1], [1, 100, 100, 1], [1, 3, 90, 70, 40, 1]])
def test_integer_exact_scatter_every_width(mlp, dtype):
    ev = NI.with_specials(NI.exact_rows(11, 257, 5, 3, H, W, dtype), 5, 3, H, W)
    got, want, _ = _exact(ev, mlp, 5, 3, (H, W))
    assert torch.equal(got.double(), want), f"{int((got.double() != want).sum())} cells differ"


def test_polarity_halves_raw_polarity_and_the_empty_interval_row():
    mlp = [1, 30, 30, 1]
    pos = NI.exact_rows(5, 100, 5, 1, H, W, pol=(1,))
    got, want, _ = _exact(pos, mlp, 5, 1, (H, W))
    assert torch.equal(got.double(), want) and float(got[:, :5].abs().max()) > 0 and not got[:, 5:].any(), "positive events fill the FIRST half"
    neg = NI.exact_rows(5, 100, 5, 1, H, W, pol=(-1,))
    got, want, _ = _exact(neg, mlp, 5, 1, (H, W))
    assert torch.equal(got.double(), want) and float(got[:, 5:].abs().max()) > 0 and not got[:, :5].any()
    raw = NI.exact_rows(5, 100, 5, 1, H, W, pol=(0, 1))                       # p01 = 0.5: half a polarity block further
    got, want, _ = _exact(raw, mlp, 5, 1, (H, W))
    assert torch.equal(got.double(), want)
    standin = torch.zeros((1, 5), dtype=torch.float64)                        # TestH5EventDataset's stand-in for an interval without events
    got, want, _ = _exact(standin, mlp, 5, 1, (H, W))
    assert not got.any() and not want.any()


@pytest.mark.parametrize("n,mlp", [(65, [1, 7, 1]), (257, [1, 30, 30, 1]), (4097, [1, 50, 50, 50, 1])])
def test_combined_layer_integer_exact(n, mlp):
    ev = NI.exact_rows(13, n, 5, 3, H, W, torch.float32)                   # p = -1 rows: negative MLP inputs and factors
    got, want, _ = _exact(ev, mlp, 5, 3, (H, W), combined=True)
    assert got.shape == (3, 5, H, W) and float(want.abs().max()) > 0 and torch.equal(got.double(), want)


@pytest.mark.parametrize("x,y,p,b", [(0, 0, 1, 0), (W - 1, 0, -1, 0), (0, H - 1, 1, 1), (W - 1, H - 1, -1, 1), (W - 1, H - 1, 1, 1)])
def test_one_event_lands_in_exactly_c_cells(x, y, p, b):
    from v2v_amd import nernet
    Cb, B, t = 5, 2, 3.0
    mlp = [1, 50, 50, 50, 1]
    ws, bs = NI.exact_mlp(mlp, 3)
    ev = torch.tensor([[x, y, t, p, b]], dtype=torch.float64)                 # one row: dt == 0, t stays raw
    with torch.no_grad():
        got = nernet.learned_voxel(ev.cuda(), [v.cuda() for v in ws], [v.cuda() for v in bs], (Cb, H, W), NI.SLOPE, batch_size=B).cpu()
    want = torch.zeros((B, 2 * Cb, H, W))
    net = NS.StockValueLayer(mlp, nn.LeakyReLU(NI.SLOPE))
    for m, wt, bi in zip(net.mlp, ws, bs):
        m.weight.data, m.bias.data = wt, bi
    with torch.no_grad():
        for i_bin in range(Cb):
            want[b, (0 if p > 0 else Cb) + i_bin, y, x] = t * float(net(torch.tensor([t - i_bin])))
    assert int((want != 0).sum()) == Cb
    assert torch.equal(got, want)
    if (x, y, p, b) == (W - 1, H - 1, 1, 1):
        assert got.flatten(1)[1, Cb * H * W - 1] != 0, "the reference's last cell (p = 1, last bin) is the end of the FIRST half"


def test_forward_sequence_equals_forward_per_interval(g32):
    from v2v_amd import nernet
    # integer-exact: bit for bit
    Cb, B = 5, 1
    mlp = [1, 50, 50, 50, 1]
    ws, bs = NI.exact_mlp(mlp, 3)
    net = nernet.Voxelization({}, False, (Cb, H, W), mlp, nn.LeakyReLU(NI.SLOPE)).cuda()
    for m, wt, bi in zip(net.quantization_layer.value_layer.mlp, ws, bs):
        m.weight.data, m.bias.data = wt.cuda(), bi.cuda()
    seq = [NI.exact_rows(1, 300, Cb, B, H, W), torch.zeros((1, 5), dtype=torch.float64), NI.exact_rows(2, 77, Cb, B, H, W)]
    with torch.no_grad():
        got = net.forward_sequence(seq, batch_size=B)
        each = torch.stack([net(e) for e in seq])
    assert got.shape == (3, B, 2 * Cb, H, W) and torch.equal(got, each) and not got[1].any() and float(got[2].abs().max()) > 0
    # real-valued: the worst case of any fp32 summation order per cell, m 2^-24 sum |terms| (tests/test_backward_ops.py's criterion)
    name = "real_c5_f64"
    layer, B = _golden_layer(g32, name)
    net = nernet.Voxelization({}, False, layer.dim, [int(v) for v in g32[f"{name}__mlp"]]).cuda()
    net.quantization_layer.load_state_dict(layer.state_dict())
    ev = torch.from_numpy(g32[f"{name}__events"])
    seq = [ev[:1500], torch.zeros((1, 5), dtype=torch.float64), ev[1500:]]
    with torch.no_grad():
        got = net.forward_sequence(seq, batch_size=B).cpu()
        each = torch.stack([net(e) for e in seq]).cpu()
    wts = [m.weight.detach().cpu() for m in layer.value_layer.mlp]
    bss = [m.bias.detach().cpu() for m in layer.value_layer.mlp]
    for k, e in enumerate(seq):
        tn = NS.normalise_t(e, B, layer.dim[0], False).float()
        mag = NS.truth64(e, tn, wts, bss, layer.dim, layer.slope, batch_size=B, reduce="abs")
        cnt = NS.truth64(e, tn, wts, bss, layer.dim, layer.slope, batch_size=B, reduce="count")
        bound = cnt * 2.0 ** -24 * mag
        assert bool(((got[k] - each[k]).abs().double() <= bound).all()), f"interval {k}"
    assert float(got[0].abs().max()) > 0 and float(got[2].abs().max()) > 0


def test_batch_size_given_means_no_host_synchronisation(g32):
    name = "real_c5_f32_b3"
    layer, B = _golden_layer(g32, name)
    ev = torch.from_numpy(g32[f"{name}__events"]).cuda()
    with torch.no_grad():
        read = layer(ev)                                    # reads B from the last row: one synchronisation
        layer(ev, batch_size=B)                             # warm: the parameter block is packed
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            given = layer(ev, batch_size=B)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert read.shape[0] == B == 3
    # the same launches on the same rows; float32 atomics may land in another order
    np.testing.assert_allclose(given.cpu().numpy(), read.cpu().numpy(), rtol=0, atol=2e-6 * float(read.abs().max()))
    # ... and on exact inputs the two are identical
    ws, bs = NI.exact_mlp([1, 30, 30, 1], 3)
    from v2v_amd import nernet
    rows = NI.exact_rows(3, 500, 5, 3, H, W).cuda()
    args = ([v.cuda() for v in ws], [v.cuda() for v in bs], (5, H, W), NI.SLOPE)
    with torch.no_grad():
        assert torch.equal(nernet.learned_voxel(rows, *args), nernet.learned_voxel(rows, *args, batch_size=3))
