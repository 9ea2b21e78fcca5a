"""LPIPS-VGG end to end on the GPU (v2v_amd/lpips.py, v2v_amd/losses.perceptual_loss) against golden G30's float64 values.

Accuracy rule (the issue's): for every case the relative L2 error of dist and of dpred (the gradient of sum_b (b + 1) dist_b) is at most
2 x the error of the reference's OWN CPU bf16-autocast run of the same quantity (stored in G30) + 1e-3 -- the margin tests/test_train_grad.py
grants every gradient of the package -- and 1 - cos(dpred, dpred64) at most 2 x the yardstick's.  The cos >= 0.99 half of that file's rule
does not apply: stock autocast itself is at 0.984 .. 0.990 here.  Measured ratios (MI355X) are recorded in DESIGN 4.16.
Everything else is bit-exact: chunking, repetition, no_grad, the normalize switch, co-scheduling with matrix-core work."""
import numpy as np
import pytest
import torch

import lpips_weights as LW
from test_convgru_concurrency import _disturbers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g30(golden):
    return golden("g30_lpips_vgg.npz")


@pytest.fixture(scope="module")
def state(g30):
    return LW.golden_state(g30)


@pytest.fixture(scope="module")
def model(state):
    from v2v_amd.lpips import LPIPSVGG
    m = LPIPSVGG()
    m.load_state_dict(state, strict=True)
    return m.cuda()


def run(model, pred, target, normalize=True, **kw):
    """(dist [B], dpred) on the GPU; dpred = the gradient of sum_b (b + 1) dist_b."""
    p = torch.as_tensor(pred).cuda().requires_grad_(True)
    dist = model(p, torch.as_tensor(target).cuda(), normalize=normalize, **kw)
    (dist * torch.arange(1, dist.numel() + 1, device="cuda", dtype=torch.float32)).sum().backward()
    return dist.detach(), p.grad


@pytest.fixture(scope="module")
def results(model, g30):
    return {name: run(model, g30[f"{name}__pred"], g30[f"{name}__target"]) for name in LW.CASES}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def one_minus_cos(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return 1.0 - float(a @ b / np.linalg.norm(a) / np.linalg.norm(b))


@pytest.mark.parametrize("name", sorted(LW.CASES))
def test_dist_and_gradient_within_twice_the_bf16_autocast_yardstick_of_g30(results, g30, name):
    dist, dpred = (t.cpu().numpy() for t in results[name])
    assert dist.dtype == np.float32 and dist.shape == LW.CASES[name][:1] and dpred.dtype == np.float32 and dpred.shape == LW.CASES[name]
    d64, g64, d16, g16 = (g30[f"{name}__{k}"] for k in ("dist64", "dpred64", "dist16", "dpred16"))
    e_d, y_d = rel(dist, d64), rel(d16, d64)
    e_g, y_g = rel(dpred, g64), rel(g16, g64)
    c_g, yc_g = one_minus_cos(dpred, g64), one_minus_cos(g16, g64)
    print(f"lpips {name}: dist rel-L2 {e_d:.2e} = {e_d / y_d:.2f} x autocast ({y_d:.2e}); dpred rel-L2 {e_g:.3f} = {e_g / y_g:.2f} x autocast ({y_g:.3f}); "
          f"1 - cos {c_g:.2e} = {c_g / yc_g:.2f} x autocast ({yc_g:.2e})")
    assert e_d <= 2 * y_d + 1e-3
    assert e_g <= 2 * y_g + 1e-3
    assert c_g <= 2 * yc_g


def test_results_do_not_depend_on_the_chunk_size_bit_for_bit(model, results, g30):
    for name in ("c", "a"):
        dist, dpred = run(model, g30[f"{name}__pred"], g30[f"{name}__target"], chunk=1)
        assert torch.equal(dist, results[name][0]) and torch.equal(dpred, results[name][1]), name
    dist, dpred = run(model, g30["c__pred"], g30["c__target"], chunk=2)           # chunks of 2 + 1
    assert torch.equal(dist, results["c"][0]) and torch.equal(dpred, results["c"][1])


def test_two_identical_calls_give_identical_bits(model, results, g30):
    for name in ("b", "c"):
        dist, dpred = run(model, g30[f"{name}__pred"], g30[f"{name}__target"])
        assert torch.equal(dist, results[name][0]) and torch.equal(dpred, results[name][1]), name


def test_no_grad_forward_equals_the_grad_mode_forward(model, results, g30):
    pred, target = (torch.from_numpy(g30[f"c__{k}"]).cuda() for k in ("pred", "target"))
    with torch.no_grad():
        dist = model(pred, target, normalize=True)
    assert not dist.requires_grad and torch.equal(dist, results["c"][0])
    assert torch.equal(model(pred, target, normalize=True), dist)                  # grad mode, but nothing requires grad
    # symmetric, and bf16 images are taken as they are
    swapped = model(target, pred, normalize=True)
    assert float((swapped - dist).abs().max()) <= 1e-5 * float(dist.max())
    q = torch.from_numpy(g30["c__pred"]).cuda().bfloat16()
    assert torch.equal(model(q, target, normalize=True), model(q.float(), target, normalize=True))


def test_perceptual_loss_drop_in(model, results, state, g30):
    from v2v_amd import losses, loss_ops
    loss = losses.perceptual_loss(weight=0.5, net="vgg", state_dict=state)
    pred, target = (torch.from_numpy(g30[f"c__{k}"]).cuda() for k in ("pred", "target"))
    per = loss(pred, target, reduce_batch=False)
    assert tuple(per.shape) == (3,) and torch.equal(per, 0.5 * results["c"][0])
    scalar = loss(pred, target)
    assert scalar.dim() == 0 and torch.equal(scalar, 0.5 * results["c"][0].mean())
    assert torch.equal(loss_ops.lpips_vgg(model, pred, target), results["c"][0].mean())
    assert torch.equal(loss_ops.lpips_vgg(model, pred, target, reduce_batch=False), results["c"][0])
    p = pred.clone().requires_grad_(True)
    loss(p, target).backward()
    pw = pred.clone().requires_grad_(True)
    (0.5 * model(pw, target, normalize=True).mean()).backward()
    assert p.grad.dtype == torch.float32 and p.grad.shape == pred.shape and torch.equal(p.grad, pw.grad) and float(p.grad.abs().max()) > 0
    # normalize=False on images already in [-1, 1] == normalize=True on the originals, bit for bit, when 2x - 1 is exact
    g = np.random.default_rng(31)
    x, y = (torch.from_numpy((g.integers(0, 257, (2, 1, 32, 32)) / 256).astype(np.float32)) for _ in range(2))
    d1, g1 = run(model, x, y, normalize=True)
    d0, g0 = run(model, 2 * x - 1, 2 * y - 1, normalize=False)
    assert torch.equal(d1, d0) and torch.equal(g1, 2 * g0)


def test_the_loss_does_not_depend_on_what_shares_the_cu(model, results, g30):
    side = torch.cuda.Stream()
    solo = results["a"]
    torch.cuda.synchronize()
    for name, disturb in _disturbers().items():
        for rep in range(3):
            with torch.cuda.stream(side):
                for _ in range(24):
                    disturb()
            outs = [run(model, g30["a__pred"], g30["a__target"]) for _ in range(2)]
            torch.cuda.synchronize()
            for o in outs:
                for k, (a, b) in enumerate(zip(o, solo)):
                    assert torch.equal(a, b), f"lpips output {k} differs from its stand-alone result while {name} runs on another stream ({int((a != b).sum())} elements)"
