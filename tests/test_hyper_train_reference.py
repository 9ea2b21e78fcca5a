"""HyperE2VID training, CPU side: the stock training-mode restatement (tests/hyper_train_stock.py) reproduces the reference's own layer
in .train() mode (golden G31: forward, every gradient, the running statistics) in float64, and the trainable package modules keep the
reference's state_dict."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import hyper_train_stock as hts  # noqa: E402


@pytest.fixture(scope="module")
def stock64():
    """The restatement in float64 on G31's weights and inputs: (golden, output, {name: gradient}, parameter dict after the call)."""
    g = hts.g31()
    p = hts.to_params(hts.g31_state(g), torch.float64)
    x, ev, prev, gy = (torch.from_numpy(a).double() for a in hts.g31_inputs(g))
    x.requires_grad_(True)
    y = hts.stock_layer_train(x, ev, prev, p)
    y.backward(gy)
    grads = {"x": x.grad.numpy()}
    grads.update({k: v.grad.numpy() for k, v in p.items() if v.requires_grad})
    return g, y.detach().numpy(), grads, p


# The two convolutions of bases_net sit in front of a BatchNorm on batch statistics, which removes a per-channel constant: their BIAS
# gradient sum_p dz[p, c] is zero in exact arithmetic, and what the reference stores there is float64 cancellation noise (1e-13 beside
# summands of 1e+1).  "1e-9 of the array's largest magnitude" has no meaning for such an array; its bound is 1e-9 of the largest magnitude
# of the same convolution's WEIGHT gradient, which sums the same dz against inputs of order one.
ZERO_BY_BATCHNORM = {"dynamic_atom_generation.bases_net.0.bias": "dynamic_atom_generation.bases_net.0.weight",
                     "dynamic_atom_generation.bases_net.3.bias": "dynamic_atom_generation.bases_net.3.weight"}


def _close(got, want, what, scale=None):
    scale = float(np.abs(want).max()) if scale is None else scale
    worst = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
    print(f"{what}: max |diff| {worst:.3e}, largest magnitude {scale:.3e}")
    assert worst <= 1e-9 * scale, what


def test_the_float64_restatement_reproduces_the_reference_output(stock64):
    g, y, _, _ = stock64
    _close(y, hts.g31_array(g, "y"), "output")


def test_the_float64_restatement_reproduces_every_reference_gradient(stock64):
    g, _, grads, _ = stock64
    names = [str(n) for n in g["grad__names"]]
    assert set(names) == set(grads)                                     # x and every trainable parameter of the layer
    for name in names:
        want, got = hts.g31_grad(g, name, grads[name])
        _close(got, want, name, float(np.abs(grads[ZERO_BY_BATCHNORM[name]]).max()) if name in ZERO_BY_BATCHNORM else None)
        if "grad_norm__" + name in g.files:                              # stored as every n-th row: the full norm covers the rest
            assert abs(np.linalg.norm(grads[name].ravel()) - float(g["grad_norm__" + name])) <= 1e-9 * float(g["grad_norm__" + name])


def test_the_float64_restatement_reproduces_the_running_statistics(stock64):
    g, _, _, p = stock64
    keys = [k for k in g.files if k.startswith("state__")]
    assert len(keys) == 6
    for k in keys:
        got = p[k[len("state__"):]].numpy()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(g[k]) == 1
        else:
            _close(got, g[k].astype(np.float64), k)


def test_the_fixture_is_small_and_records_the_autocast_yardstick():
    import os
    g = hts.g31()
    assert os.path.getsize(os.path.join(hts.HERE, "golden", "g31_hyper_train.npz")) < 600_000
    for name in g["grad__names"]:
        rel, cos = g["bf16_autocast__" + str(name)]
        assert np.isfinite(rel) and -1.0 <= cos <= 1.0


def test_the_trainable_network_keeps_the_state_dict():
    from v2v_amd.hyper import HyperE2VID
    a, b = HyperE2VID(dict(hts.KW), trainable=True).state_dict(), HyperE2VID(dict(hts.KW), trainable=False).state_dict()
    assert list(a) == list(b)
    assert all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
