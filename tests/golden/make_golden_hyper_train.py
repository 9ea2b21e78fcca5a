"""Golden G31 (tests/golden/g31_hyper_train.npz): the reference's DynamicUpsampleLayer (model/hyper_model.py:33-60) in .train() mode --
BatchNorm on the batch's statistics -- forward and backward in float64 on the CPU, on tests/hyper_weights.py's seeded recipe.

    python tests/golden/make_golden_hyper_train.py REFERENCE_DIR        (the reference checkout; or V2V_REFERENCE in the environment)

Inputs (recipes, not stored): x [2,256,6,10], events [2,5,48,80], a non-zero prev_recs and an upstream gradient of bf16 values
(tests/hyper_train_stock.py g31_inputs).  Stored in float64: the output, dx, the gradient of every trainable parameter of the layer
(compositional_coefficients.grad as rows 0::8 and bases_net.3.weight.grad as rows 0::2, each with its full norm: 176,640 values at the
30 bits that 1e-9 takes do not fit 600 KB otherwise), the updated running statistics and num_batches_tracked; and, per
gradient, the reference's OWN (relative error, cosine) under CPU bf16 autocast against that float64 gradient: the yardstick of the GPU
tests.  Arrays of more than 4096 elements are stored as int32 fixed point at 2^-31 of the array's largest magnitude (key + "__q31" with
key + "__scale"; hyper_train_stock.g31_array decodes): the rounding is 2.3e-10 of that magnitude, inside the 1e-9 the CPU test asks for, and
the file stays under 600 KB (plain float64 took 1.16 MB).  Regenerates byte for byte."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("V2V_REFERENCE")
if not REF:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)

from hyper_train_stock import bf16_exact, rel_cos  # noqa: E402
from hyper_weights import load_hyper  # noqa: E402
from seeded_weights import seeded_input  # noqa: E402
import model.hyper_model as hm  # noqa: E402

LAYER_SEED, LAYER_GAIN, LAYER_COEFF_SCALE = 3101, 1.0, 1.0 / 32
X_SEEDS = (31010, 31011, 31012, 31013)
ROWS = {"dynamic_conv.compositional_coefficients": 8, "dynamic_atom_generation.bases_net.3.weight": 2}    # stored as rows 0::n + the full norm
Q31 = float(2 ** 31 - 1)


def put(out, key, a):
    a = np.asarray(a, dtype=np.float64)
    if a.size <= 4096:
        out[key] = a
        return
    scale = float(np.abs(a).max()) or 1.0
    out[key + "__q31"] = np.rint(a / scale * Q31).astype(np.int32)
    out[key + "__scale"] = np.array(scale)


def layer(dtype):
    with contextlib.redirect_stdout(io.StringIO()):
        m = hm.DynamicUpsampleLayer(256, 128, 5, padding=2, in_fuse_channels=6)
    load_hyper(m, LAYER_SEED, gain=LAYER_GAIN, coeff_scale=LAYER_COEFF_SCALE)
    return m.to(dtype).train()


def run(m, dtype, autocast=False):
    x = torch.from_numpy(seeded_input(X_SEEDS[0], 2, 256, 6, 10)).to(dtype).requires_grad_(True)
    ev = torch.from_numpy(seeded_input(X_SEEDS[1], 2, 5, 48, 80)).to(dtype)
    prev = torch.from_numpy(0.5 * seeded_input(X_SEEDS[2], 2, 1, 48, 80)).to(dtype)
    gy = torch.from_numpy(bf16_exact(seeded_input(X_SEEDS[3], 2, 128, 12, 20)))
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        y = m(x, ev, prev)
    y.backward(gy.to(y.dtype))
    grads = {"x": x.grad.double().numpy()}
    grads.update({k: p.grad.double().numpy() for k, p in m.named_parameters()})
    return y.detach().double().numpy(), grads


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    m = layer(torch.float64)
    sd0 = m.state_dict()
    out = dict(layer__seed=np.array(LAYER_SEED), layer__gain=np.array(LAYER_GAIN), layer__coeff_scale=np.array(LAYER_COEFF_SCALE),
               layer__x_seeds=np.array(X_SEEDS), layer__keys=np.array(list(sd0)),
               layer__shapes=np.array([",".join(map(str, v.shape)) for v in sd0.values()]),
               bases=sd0["dynamic_atom_generation.bases"].float().numpy())
    y, grads = run(m, torch.float64)
    y16, grads16 = run(layer(torch.float32), torch.float32, autocast=True)
    put(out, "y", y)
    out["y__bf16_autocast"] = np.array(rel_cos(y16, y))
    names = []
    for k, g in grads.items():
        names.append(k)
        put(out, "grad__" + k, g[0::ROWS.get(k, 1)])
        if k in ROWS:
            out["grad_rows__" + k] = np.array(ROWS[k])
            out["grad_norm__" + k] = np.array(float(np.linalg.norm(g.ravel())))
        out["bf16_autocast__" + k] = np.array(rel_cos(grads16[k], g))
        print(f"g31 {k}: |grad| {np.linalg.norm(g.ravel()):.3e}, reference bf16 autocast rel {out['bf16_autocast__' + k][0]:.3e} cos {out['bf16_autocast__' + k][1]:.6f}")
    out["grad__names"] = np.array(names)
    for k, v in m.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out["state__" + k] = v.numpy()
    path = os.path.join(HERE, "g31_hyper_train.npz")
    np.savez_compressed(path, **out)
    print(f"g31_hyper_train.npz: {os.path.getsize(path) / 1024:.1f} KiB; output |max| {np.abs(y).max():.2f}, bf16 autocast rel {out['y__bf16_autocast'][0]:.3e}")


if __name__ == "__main__":
    main()
