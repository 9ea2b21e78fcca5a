"""v2v_amd.lpips_alex.LPIPSAlex as a training loss, end to end on the GPU against golden G35 (tests/golden/g35_lpips_alex_grad.npz: the
gradient of the reference's PNetLin to the prediction, CPU float64 autograd, on  sum_b c_b dist_b  with c_b = 0.5 + 0.75 b).

The bar: per frame  max|g - g64| / max|g64| <= 8 x e32_grad, e32_grad being the reference's OWN float32 error (the maximum over all
cases and frames).  It is the bar tests/test_lpips_alex.py sets for these kernels' forward against the same kind of yardstick: a k-ordered
float32 chain accumulates differently from the CPU's blocked sums.  A comparison within a tolerance needs every ReLU gate and every pool
arg-max to fall as in the float64 run; the generator asserted margins for that, and the first test checks it on this hardware.
Measured multiples are printed before they are asserted and recorded in DESIGN 4.20."""
import numpy as np
import pytest
import torch

import lpips_alex_grad_cases as GC
import lpips_alex_stock as STOCK
import lpips_alex_weights as LW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g34(golden):
    return golden("g34_lpips_alex.npz")


@pytest.fixture(scope="module")
def g35(golden):
    return golden("g35_lpips_alex_grad.npz")


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
            cache[name] = tuple(torch.from_numpy(v).cuda() for v in GC.case_inputs(name))
        return cache[name]
    return get


def _grad(model, pred, target, coef=None):
    """(dist [T], d (sum_b c_b dist_b) / d pred) through the module's autograd path"""
    p = pred.clone().requires_grad_(True)
    dist = model(p, target, normalize=True)
    assert dist.shape == (pred.shape[0], 1, 1, 1) and dist.dtype == torch.float32 and dist.grad_fn is not None
    c = torch.from_numpy(GC.coefficients(pred.shape[0])).float().cuda() if coef is None else coef
    (c * dist.reshape(-1)).sum().backward()
    assert p.grad is not None and p.grad.shape == pred.shape and p.grad.dtype == torch.float32
    return dist.detach(), p.grad


@pytest.fixture(scope="module")
def grads(model, inputs):
    """The gradient of every case, computed once and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _grad(model, *inputs(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(GC.CASES))
def test_the_gates_fall_as_in_the_float64_run(g35, model, inputs, name):
    """The number of active ReLU units of the pred half per tap equals the float64 run's: the case is valid on this hardware."""
    from v2v_amd.lpips_alex import _images
    pred, target = inputs(name)
    p, ps = _images("pred", pred)
    t, ts = _images("target", target)
    _, _, saved = model._run(p, ps, t, ts, 1.0, True, pred.shape[0], save=True)
    assert len(saved) == 1 and len(saved[0]) == 5
    active = [int((f0 > 0).sum()) for f0, _ in saved[0]]
    assert active == g35[f"{name}__active"].tolist()


@pytest.mark.parametrize("name", list(GC.CASES))
def test_gradient_is_within_the_references_own_float32_error_of_the_float64_run(g35, grads, name):
    dist, grad = grads(name)
    g64 = g35[f"{name}__grad64"]
    T = g64.shape[0]
    got = grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - g64).reshape(T, -1).max(1) / np.abs(g64).reshape(T, -1).max(1)
    print(f"lpips_alex grad {name}: error {err.max():.3e} = {err.max() / float(g35['e32_grad']):.2f} x e32_grad")
    assert (err <= 8 * float(g35["e32_grad"])).all(), err
    d64 = g35[f"{name}__dist64"]
    assert (np.abs(dist.reshape(-1).cpu().numpy() - d64) <= 1e-4 * d64).all()


@pytest.mark.parametrize("name", ["a", "b", "c", "close"])
def test_forward_bits_and_backward_bits(model, inputs, grads, name):
    pred, target = inputs(name)
    T = pred.shape[0]
    dist, grad = grads(name)
    # dist is today's forward, bit for bit
    with torch.no_grad():
        plain = model(pred, target, normalize=True)
    assert plain.grad_fn is None and torch.equal(plain, dist)
    assert torch.equal(model.sequence(pred, target, divisor=1.0, normalize=True), dist.reshape(-1))
    # without requires_grad, and under no_grad with it: no graph, the same bits
    out = model(pred, target, normalize=True)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, dist)
    with torch.no_grad():
        out = model(pred.clone().requires_grad_(True), target, normalize=True)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, dist)
    # two backward runs agree bitwise
    again_d, again_g = _grad(model, pred, target)
    assert torch.equal(again_d, dist) and torch.equal(again_g, grad)
    # chunk = 1 and chunk = T (and the default) give the same gradient bitwise
    keep = model.grad_chunk
    try:
        for chunk in (1, T):
            model.grad_chunk = chunk
            d, g = _grad(model, pred, target)
            assert torch.equal(d, dist) and torch.equal(g, grad), f"chunk {chunk}"
    finally:
        model.grad_chunk = keep
    # frame by frame, [C,H,W] as the reference's loops hand images over: the frame's bits, scaled by its own coefficient
    coef = torch.from_numpy(GC.coefficients(T)).float().cuda()
    for t in range(T):
        p = pred[t].clone().requires_grad_(True)
        one = model(p, target[t], normalize=True)
        assert one.shape == (1, 1, 1, 1)
        (coef[t] * one.reshape(())).backward()
        assert torch.equal(p.grad, grad[t])
    # without normalize the image is taken as it is: d/dpred of f(2 pred - 1) is 2 f'
    p = (2 * pred - 1).requires_grad_(True)
    d = model(p, 2 * target - 1, normalize=False)
    (coef * d.reshape(-1)).sum().backward()
    assert torch.equal(d, dist) and torch.equal(2 * p.grad, grad)


def test_errors_and_the_target(model, inputs):
    pred, target = inputs("a")
    with pytest.raises(ValueError, match="target"):
        model(pred.clone().requires_grad_(True), target.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="float32"):
        model(pred.double().requires_grad_(True), target.double())
    with pytest.raises(ValueError, match="31"):
        model(pred[:, :, :30].clone().requires_grad_(True), target[:, :, :30])
    with pytest.raises(ValueError, match="shape"):
        model(pred.clone().requires_grad_(True), target[:1])
    # sequence() stays a metric
    out = model.sequence(pred.clone().requires_grad_(True), target, divisor=1.0)
    assert out.grad_fn is None and not out.requires_grad
    # an empty batch
    p = pred[:0].clone().requires_grad_(True)
    d = model(p, target[:0])
    d.sum().backward()
    assert d.shape == (0, 1, 1, 1) and p.grad.shape == p.shape


def test_zero_gradient_for_identical_images(model, inputs):
    _, target = inputs("b")
    p = target.clone().requires_grad_(True)
    d = model(p, target, normalize=True)
    d.sum().backward()
    assert not d.any() and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) < 1e-6


@pytest.mark.parametrize("reduce_batch", [True, False])
def test_perceptual_loss_alex_matches_the_stock_module(g34, g35, inputs, reduce_batch):
    """loss and gradient of the drop-in class against the stock restatement in float64 on the CPU, the same bar."""
    from v2v_amd import losses
    state = LW.golden_state(g34)
    weight = 0.7
    fn = losses.perceptual_loss_alex(weight=weight, state_dict=state)
    pred, target = inputs("b")
    T = pred.shape[0]
    coef = GC.coefficients(T)
    p = pred.clone().requires_grad_(True)
    loss = fn(p, target, reduce_batch=reduce_batch)
    assert loss.shape == (() if reduce_batch else (T,)) and loss.dtype == torch.float32
    (loss if reduce_batch else (torch.from_numpy(coef).float().cuda() * loss).sum()).backward()
    s64 = {k: v.double() for k, v in state.items()}
    q = pred.cpu().double().requires_grad_(True)
    dist = STOCK.lpips_alex(s64, q, target.cpu().double(), normalize=True).reshape(-1)
    want = weight * dist.mean() if reduce_batch else weight * dist
    (want if reduce_batch else (torch.from_numpy(coef) * want).sum()).backward()
    e32_dist, e32_grad = float(g34["e32_dist"]), float(g35["e32_grad"])
    le = (loss.detach().cpu().double() - want.detach()).abs() / want.detach().abs()
    g64, got = q.grad.numpy(), p.grad.cpu().numpy().astype(np.float64)
    ge = np.abs(got - g64).reshape(T, -1).max(1) / np.abs(g64).reshape(T, -1).max(1)
    print(f"perceptual_loss_alex reduce_batch {reduce_batch}: loss error {float(le.max()) / e32_dist:.2f} x e32_dist, gradient {ge.max() / e32_grad:.2f} x e32_grad")
    assert (le <= 8 * e32_dist).all() and (ge <= 8 * e32_grad).all()
