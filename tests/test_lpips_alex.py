"""v2v_amd.lpips_alex.LPIPSAlex end to end on the GPU against golden G34 (tests/golden/g34_lpips_alex.npz: the reference's PNetLin on the
CPU in float64 and in float32).

The bar: per tap mean within 8 x e32_tap and per frame within 8 x e32_dist of the float64 run, both relative, where e32_* is the
reference's OWN float32 error, the maximum over all cases and frames (a single frame's value is luck).  A plain k-ordered float32
accumulation chain emulated on the CPU sits at 2.4-2.8 x that yardstick on these cases; 8 leaves a factor of three and still stays near
7e-6, three orders below what bf16 operands or a dropped k-slice would give.  The achieved errors are printed before they are asserted."""
import numpy as np
import pytest
import torch

import lpips_alex_weights as LW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g34(golden):
    return golden("g34_lpips_alex.npz")


@pytest.fixture(scope="module")
def model(g34):
    from v2v_amd.lpips_alex import LPIPSAlex
    m = LPIPSAlex()
    m.load_state_dict(LW.golden_state(g34), strict=True)
    return m.cuda()


@pytest.fixture(scope="module")
def inputs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = tuple(torch.from_numpy(v).cuda() for v in LW.case_inputs(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(LW.CASES))
def test_sequence_is_within_the_references_own_float32_error_of_the_float64_run(g34, model, inputs, name):
    pred, target = inputs(name)
    dist, taps = model.sequence(pred, target, divisor=1.0, normalize=True, taps=True)
    assert dist.dtype == torch.float32 and dist.shape == (pred.shape[0],) and taps.dtype == torch.float64 and taps.shape == (pred.shape[0], 5)
    taps, dist = taps.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
    t64, d64 = g34[f"{name}__taps64"], g34[f"{name}__dist64"]
    et, ed = np.abs(taps - t64) / t64, np.abs(dist - d64) / d64
    print(f"lpips_alex {name}: tap error {et.max():.3e} ({et.max() / float(g34['e32_tap']):.2f} x e32_tap), dist error {ed.max():.3e} "
          f"({ed.max() / float(g34['e32_dist']):.2f} x e32_dist)")
    assert (et <= 8 * float(g34["e32_tap"])).all(), et
    assert (ed <= 8 * float(g34["e32_dist"])).all(), ed
    # dist is the five float32 tap means added in tap order
    want = taps[:, 0].astype(np.float32)
    for k in range(1, 5):
        want = want + taps[:, k].astype(np.float32)
    assert np.array_equal(dist.astype(np.float32), want)


@pytest.mark.parametrize("name", ["a", "b", "c", "close"])
def test_every_way_in_gives_the_same_bits_per_frame(model, inputs, name):
    pred, target = inputs(name)
    T = pred.shape[0]
    ref, ref_taps = model.sequence(pred, target, divisor=1.0, taps=True)
    for chunk in (1, 2, 40):
        d, t = model.sequence(pred, target, divisor=1.0, chunk=chunk, taps=True)
        assert torch.equal(d, ref) and torch.equal(t, ref_taps), f"chunk {chunk}"
    assert torch.equal(model.sequence(pred[None], target[None], divisor=1.0), ref)
    again, again_taps = model.sequence(pred, target, divisor=1.0, taps=True)
    assert torch.equal(again, ref) and torch.equal(again_taps, ref_taps)
    # forward, frame by frame as the reference's loop calls it ([C,H,W], normalize=True), and as a batch
    for t in range(T):
        one = model(pred[t], target[t], normalize=True)
        assert one.shape == (1, 1, 1, 1) and one.dtype == torch.float32 and torch.equal(one.reshape(()), ref[t])
    assert torch.equal(model(pred, target, normalize=True).reshape(-1), ref)
    # a tail of other frames behind it, and the same frame many times (frame stride 0), change nothing
    more = torch.cat([pred, pred.flip(0), target], 0), torch.cat([target, target, pred], 0)
    assert torch.equal(model.sequence(*more, divisor=1.0, chunk=3)[:T], ref)
    rep = model.sequence(pred[:1].expand(5, -1, -1, -1), target[:1].expand(5, -1, -1, -1), divisor=1.0)
    assert torch.equal(rep, ref[:1].expand(5))
    # the divisor is a true float32 division in front of everything else
    assert torch.equal(model.sequence(pred * 4, target * 4, divisor=4.0), ref)
    # without normalize the image is taken as it is
    assert torch.equal(model.sequence(2 * pred - 1, 2 * target - 1, divisor=1.0, normalize=False), ref)


def test_identical_images_and_dead_pixels(model, inputs):
    pred, target = inputs("b")
    d, t = model.sequence(target, target, divisor=1.0, taps=True)
    assert not d.any() and not t.any()
    # an image whose every stem output is dead cannot be made with seeded weights; a zero backbone gives all-zero features everywhere
    from v2v_amd.lpips_alex import LPIPSAlex
    dead = LPIPSAlex().cuda()
    dead.load_state_dict({k: torch.zeros_like(v) if k.startswith("net.") else v for k, v in model.state_dict().items()})
    d = dead.sequence(pred, target, divisor=1.0)
    assert torch.isfinite(d).all() and not d.any()


def test_errors(model, inputs):
    pred, target = inputs("a")
    with pytest.raises(ValueError, match="31"):
        model.sequence(pred[:, :, :30], target[:, :, :30])
    with pytest.raises(ValueError, match="31"):
        model(pred[:, :, :, :30], target[:, :, :, :30])
    with pytest.raises(ValueError, match="float32"):
        model.sequence(pred.double(), target.double())
    with pytest.raises(ValueError, match="float32"):
        model(pred.bfloat16(), target)
    with pytest.raises(ValueError, match="CUDA"):
        model.sequence(pred.cpu(), target.cpu())
    with pytest.raises(ValueError, match="shape"):
        model.sequence(pred, target[:1])
    with pytest.raises(ValueError):
        model.sequence(pred.expand(-1, 2, -1, -1), target.expand(-1, 2, -1, -1))
    with pytest.raises(ValueError):
        model.sequence(pred, target, chunk=0)
    assert model.sequence(pred[:0], target[:0]).shape == (0,)


def test_compute_metrics_takes_the_batched_pass(model):
    """compute_metrics with an LPIPSAlex against the per-frame path with the same module (handed over behind a plain function, which takes
    today's loop): same keys in the same order, LPIPS equal bit for bit, MSE and SSIM unchanged.

    The per-frame path divides by 255 in torch, and torch's CUDA division by a Python scalar multiplies by the rounded reciprocal, which
    differs from the kernels' true division in the last bit for about half of all values.  The frames here hold the 8-bit levels on which
    the two agree (130 of the 256: checked below on the CPU, where the arithmetic is IEEE either way), so the comparison is about the two
    call paths and not about that bit."""
    from v2v_amd import metrics
    levels = np.arange(256, dtype=np.float32)
    levels = levels[levels * (np.float32(1) / np.float32(255)) == levels / np.float32(255)]
    assert levels.size >= 100
    g = np.random.Generator(np.random.PCG64(342))
    T, H, W = 5, 47, 63
    frame = torch.from_numpy(levels[g.integers(0, levels.size, size=(1, T, 1, H, W))]).cuda()
    pred = torch.from_numpy(levels[g.integers(0, levels.size, size=(1, T, 1, H, W))]).cuda()
    batch = {"frame": frame, "sequence_name": [["seq"]], "data_source_idx": torch.tensor([0])}
    fast = metrics.compute_metrics(pred, batch, lpips_fn=model)
    slow = metrics.compute_metrics(pred, batch, lpips_fn=lambda p, f, normalize: model(p, f, normalize=normalize))
    none = metrics.compute_metrics(pred, batch)
    assert list(fast) == list(slow) and [k.split("/")[-1] for k in fast] == ["MSE", "LPIPS", "SSIM"]
    for k in fast:
        assert type(fast[k]) is list and len(fast[k]) == T and all(type(v) is float for v in fast[k])
        assert fast[k] == slow[k], k
        if not k.endswith("LPIPS"):
            assert fast[k] == none[k]
    lp = fast[[k for k in fast if k.endswith("LPIPS")][0]]
    assert all(0.0 < v < 2.0 for v in lp)
    assert lp == model.sequence(pred, frame).double().cpu().tolist()
