"""Golden G32 (tests/golden/g32_nernet_voxelization.npz): the reference's learned voxelisation, model/nernet/representation_modules.py
(ValueLayer, QuantizationLayer_trail, QuantizationLayer_trail_combined, Voxelization), run on the CPU.

    python tests/golden/make_golden_nernet.py REFERENCE_DIR        (the reference checkout; or V2V_REFERENCE in the environment)

The module imports tqdm for an initialisation routine its forward never calls; it is stubbed in sys.modules when missing.  The MLP's
parameters are the seeded recipe of tests/seeded_weights.py (load_seeded(layer.value_layer, seed)), not stored.  The file holds no code.

State dicts:  `sd__names` lists the recorded configurations ([1,30,30,1] and [1,50,50,50,1], with and without RepresentationCNN, plus the
combined layer); `sd__<name>__keys` / `sd__<name>__shapes` are the reference's state_dict keys and shapes (shapes padded with -1 to 4).

Cases:  `cases` lists them; per case
    <case>__events   the rows [n, 5] (x, y, t, p, b) as handed to the layer (float64 or float32)
    <case>__cfg      int64 [C, H, W, B, normalize, combined, seed]        <case>__mlp  int64 mlp_layers        <case>__slope  float64 [1]
    <case>__out      the reference's float32 output [B, 2C, H, W] (combined: [B, C, H, W])
    <case>__tn       float32 [n]: t as the reference normalised it (read back from the tensor it changes in place)
    <case>__truth    float64: the same layer evaluated in float64 from that float32 t_n and the float32 parameters (tests/nernet_stock.truth64)
    <case>__err      float64 [max, rms] of |out - truth|
Grids are 12 x 20; `real_*` cases have several events per cell (4000 events on the 2400 cells of C = 5).  Regenerates value for value; one CPU thread (the GEMM's blocking, and with it the last bits of `out`, depends on the thread count)."""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("V2V_REFERENCE")
if not REF:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
try:
    import tqdm  # noqa: F401
except ImportError:
    sys.modules["tqdm"] = types.ModuleType("tqdm")

import nernet_stock as NS  # noqa: E402
import seeded_weights as SW  # noqa: E402
from model.nernet import representation_modules as RM  # noqa: E402

H, W = 12, 20
NET_KW = {"RepCNN_kernel_size": 3, "RepCNN_padding": 1, "RepCNN_channel": 16, "RepCNN_num_layers": 4}


def rows(seed, n, B=1, dtype=np.float64, pol=(-1, 1), sort=True, span=0.05, interleave=True):
    g = np.random.Generator(np.random.PCG64(seed))
    ev = np.zeros((n, 5), dtype=np.float64)
    ev[:, 0] = g.integers(0, W, n)
    ev[:, 1] = g.integers(0, H, n)
    t = 10.0 + g.uniform(0, span, n)
    ev[:, 2] = np.sort(t) if sort else t
    ev[:, 3] = g.choice(pol, n)
    b = g.integers(0, B, n) if interleave else np.sort(g.integers(0, B, n))
    b[-1] = B - 1                                                  # the layer reads the batch size from the last row
    ev[:, 4] = b
    return ev.astype(dtype)


def cases():
    c = {}
    big, small = [1, 50, 50, 50, 1], [1, 30, 30, 1]
    # name: (rows, C, B, normalize, combined, mlp, slope, seed)
    c["real_c5_f64"] = (rows(1, 4000), 5, 1, 0, 0, big, 0.1, 11)
    c["real_c5_f64_norm"] = (rows(1, 4000), 5, 1, 1, 0, big, 0.1, 11)
    c["real_c9_f32"] = (rows(2, 900, dtype=np.float32, span=0.5), 9, 1, 0, 0, small, 0.1, 12)
    c["real_c9_f32_norm"] = (rows(2, 900, dtype=np.float32, span=0.5), 9, 1, 1, 0, small, 0.1, 12)
    c["real_c5_f32_b3"] = (rows(10, 900, B=3, dtype=np.float32, span=0.5), 5, 3, 0, 0, small, 0.1, 21)
    c["real_c5_f32_b3_norm"] = (rows(10, 900, B=3, dtype=np.float32, span=0.5), 5, 3, 1, 0, small, 0.1, 21)
    c["real_c4_f64_norm"] = (rows(3, 500), 4, 1, 1, 0, small, 0.1, 13)
    c["real_c4_f64"] = (rows(3, 500), 4, 1, 0, 0, small, 0.2, 13)
    c["unsorted_c5_f64_b3"] = (rows(4, 500, B=3, sort=False), 5, 3, 0, 0, small, 0.1, 14)            # first / last row are not min / max
    c["unsorted_c5_f64_b3_norm"] = (rows(4, 500, B=3, sort=False), 5, 3, 1, 0, small, 0.1, 14)
    dt0 = rows(5, 400, B=3)
    dt0[dt0[:, 4] == 1, 2] = 10.0125                                                                 # batch 1: every t equal
    c["dt0_c5_f64_b3"] = (dt0, 5, 3, 0, 0, small, 0.1, 15)
    c["dt0_c5_f64_b3_norm"] = (dt0.copy(), 5, 3, 1, 0, small, 0.1, 15)
    c["standin_c5_f64"] = (np.zeros((1, 5)), 5, 1, 0, 0, big, 0.1, 16)                               # the dataset's empty-interval row
    c["standin_c5_f64_norm"] = (np.zeros((1, 5)), 5, 1, 1, 0, big, 0.1, 16)
    c["raw01_c5_f64"] = (rows(6, 400, pol=(0, 1)), 5, 1, 0, 0, small, 0.1, 17)                       # p01 = 0.5 and 1
    cl = rows(7, 400, B=2)
    cl[:40, 1] += H                                                                                  # past the sensor ...
    cl[-30:, 1] += 3 * H                                                                             # ... and past the grid's end: clamped
    cl[100:130, 0] -= W + 7                                                                          # negative indices of batch 0: wrapped once
    cl[100:130, 1] = 0
    cl[100:130, 3] = -1
    cl[100:130, 4] = 0
    c["clamp_c5_f64_b2"] = (cl, 5, 2, 0, 0, small, 0.1, 18)
    c["relu_c5_f32"] = (rows(8, 400, dtype=np.float32, span=0.5), 5, 1, 0, 0, [1, 7, 1], 0.0, 19)    # nn.ReLU
    c["combined_c5_f32_b2"] = (rows(9, 600, B=2, dtype=np.float32, span=0.5), 5, 2, 0, 1, small, 0.1, 20)
    c["combined_c5_f32_b2_norm"] = (rows(9, 600, B=2, dtype=np.float32, span=0.5), 5, 2, 1, 1, small, 0.1, 20)
    return c


def main():
    torch.set_num_threads(1)                 # the GEMM's last bits depend on how many threads share it; tests/test_nernet_golden.py pins the same
    out = {}
    sd_cfgs = {"mlp30": (small := [1, 30, 30, 1], False, False), "mlp30_cnn": (small, True, False), "mlp50": (big := [1, 50, 50, 50, 1], False, False),
               "mlp50_cnn": (big, True, False), "mlp30_combined_cnn": (small, True, True)}
    out["sd__names"] = np.array(sorted(sd_cfgs))
    for name, (mlp, cnn, comb) in sd_cfgs.items():
        sd = RM.Voxelization(NET_KW, cnn, voxel_dimension=(5, H, W), mlp_layers=mlp, combine_voxel=comb).state_dict()
        out[f"sd__{name}__keys"] = np.array(list(sd))
        out[f"sd__{name}__shapes"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    cs = cases()
    out["cases"] = np.array(list(cs))
    for name, (ev, C, B, norm, comb, mlp, slope, seed) in cs.items():
        act = nn.ReLU() if slope == 0.0 else nn.LeakyReLU(negative_slope=slope)
        cls = RM.QuantizationLayer_trail_combined if comb else RM.QuantizationLayer_trail
        layer = cls((C, H, W), mlp, act, bool(norm))
        SW.load_seeded(layer.value_layer, seed)
        events = torch.from_numpy(ev)
        work = events.clone()                                       # the reference normalises column 2 of its argument in place
        with torch.no_grad():
            got = layer(work)
        tn = work[:, 2].float()
        wts = [m.weight.detach() for m in layer.value_layer.mlp]
        bss = [m.bias.detach() for m in layer.value_layer.mlp]
        truth = NS.truth64(events, tn, wts, bss, (C, H, W), slope, bool(norm), bool(comb))
        assert got.shape == truth.shape and got.dtype == torch.float32 and int(got.shape[0]) == B, name
        err = (got.double() - truth).abs()
        out[f"{name}__events"] = ev
        out[f"{name}__cfg"] = np.array([C, H, W, B, norm, comb, seed], dtype=np.int64)
        out[f"{name}__mlp"] = np.array(mlp, dtype=np.int64)
        out[f"{name}__slope"] = np.array([slope], dtype=np.float64)
        out[f"{name}__out"] = got.numpy()
        out[f"{name}__tn"] = tn.numpy()
        out[f"{name}__truth"] = truth.numpy()
        out[f"{name}__err"] = np.array([float(err.max()), float(err.pow(2).mean().sqrt())])
        print(f"{name:28s} n {ev.shape[0]:5d} out {tuple(got.shape)} |out| max {float(got.abs().max()):.4g} err max {float(err.max()):.3g} "
              f"rms {float(err.pow(2).mean().sqrt()):.3g}")
    path = os.path.join(HERE, "g32_nernet_voxelization.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
