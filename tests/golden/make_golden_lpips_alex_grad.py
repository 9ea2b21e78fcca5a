"""Golden G35 (tests/golden/g35_lpips_alex_grad.npz): the gradient of the reference's LPIPS network with the alex backbone with respect
to the prediction, as training takes it (model/loss.py:95-119 with net='alex' -> PerceptualLoss.forward(pred, target, normalize=True) ->
PNetLin.forward(2 target - 1, 2 pred - 1)): PerceptualSimilarity/models/networks_basic.py:PNetLin(pnet_type='alex', version='0.1',
spatial=False, eval mode) on the CPU with autograd, one-channel images concatenated to three, the whole case as one batch.

    python tests/golden/make_golden_lpips_alex_grad.py REFERENCE_DIR [--search]     (or V2V_REFERENCE in the environment)

The network is G34's (tests/lpips_alex_weights.py: the seeded backbone; lin / shift / scale from g34_lpips_alex.npz, which the reference's
alex.pth is checked against here), the stubs are make_golden_lpips_alex.py's.  The scalar is sum_b c_b dist_b, c_b = 0.5 + 0.75 b.

Per case (tests/lpips_alex_grad_cases.CASES): <case>__grad64 [T,C,H,W] and __dist64 [T] from the float64 run, __active int64 [5] (the
number of pred-branch units with a pre-activation > 0 per tap, float64 run), __pred / __target float32 for the cases in GC.STORED (t128's
inputs are recipe only, as G34's large cases are: with them the file is 716 KiB and fails condition iv).  e32_grad: the maximum over ALL
cases and frames of  max|g32 - g64| / max|g64|  per frame, g32 the same network's float32 CPU run -- the yardstick of the GPU tests.

Asserted before writing (conditions, not measurements):
  (i)   no tap pixel of either branch has all-zero features
  (ii)  in every layer of the pred branch  min |pre-activation (float64)|  >=  8 x  max |pre-activation float32 - float64|  of that layer
  (iii) in every pool window whose maximum is > 0 the two largest values differ by >= 8 x that error of the layer they come from
  (iv)  the file stays under 640 KiB
  (v)   it regenerates byte for byte (written twice, compared)
(ii) and (iii) keep a float32 rounding from flipping a ReLU gate or an arg-max, which changes the gradient discontinuously.  --search
prints, per case, the smallest draw j that satisfies (i)-(iii); tests/lpips_alex_grad_cases.J records it."""
import io
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_lpips_alex as G34GEN  # noqa: E402  (takes REFERENCE_DIR from the command line and puts tests/ and the reference on sys.path)

import lpips_alex_grad_cases as GC  # noqa: E402
import lpips_alex_weights as LW  # noqa: E402


def run(net, pred, target, dtype):
    """(grad [T,C,H,W], dist [T], pre-activations of the target branch, of the pred branch) of one batched call with autograd."""
    net = net.to(dtype)
    convs = [m for s in range(1, 6) for m in getattr(net.net, f"slice{s}") if isinstance(m, nn.Conv2d)]
    assert len(convs) == 5
    pre = []
    hooks = [c.register_forward_hook(lambda m, i, o: pre.append(o.detach().clone())) for c in convs]   # clone: the ReLU behind is in place
    p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    t = torch.from_numpy(target).to(dtype)
    p3, t3 = (torch.cat([v, v, v], dim=1) if v.shape[1] == 1 else v for v in (p, t))
    dist = net(2 * t3 - 1, 2 * p3 - 1)
    for h in hooks:
        h.remove()
    assert dist.shape == (pred.shape[0], 1, 1, 1) and len(pre) == 10
    (torch.from_numpy(GC.coefficients(pred.shape[0])).to(dtype) * dist.reshape(-1)).sum().backward()
    return p.grad.numpy(), dist.detach().reshape(-1).numpy(), pre[:5], pre[5:]


def case(net, name, j=None):
    """One case: its arrays and its margins {floor, layer, pool, e32}."""
    pred, target = GC.case_inputs(name, j)
    g64, d64, pre_t, pre_p = run(net, pred, target, torch.float64)
    g32, _, _, pre_p32 = run(net, pred, target, torch.float32)
    net.float()
    floor = min(float((F.relu(z).double() ** 2).sum(1).min()) for z in pre_t + pre_p)
    layer, pool = np.inf, np.inf
    for k, (z, z32) in enumerate(zip(pre_p, pre_p32)):
        err = float((z32.double() - z).abs().max())
        layer = min(layer, float(z.abs().min()) / err)
        if k < 2:                                                        # relu1 and relu2 feed the two pools
            win = F.unfold(F.relu(z), 3, stride=2).reshape(z.shape[0], z.shape[1], 9, -1)
            top = win.topk(2, dim=2).values
            gap = (top[:, :, 0] - top[:, :, 1])[top[:, :, 0] > 0]
            pool = min(pool, float(gap.min()) / err)
    scale = np.abs(g64).reshape(g64.shape[0], -1).max(1)
    e32 = float((np.abs(g32.astype(np.float64) - g64).reshape(g64.shape[0], -1).max(1) / scale).max())
    arrays = {"grad64": g64, "dist64": d64, "active": np.array([int((z > 0).sum()) for z in pre_p], dtype=np.int64), "pred": pred, "target": target}
    return arrays, {"floor": floor, "layer": layer, "pool": pool, "e32": e32}


def holds(m):
    return m["floor"] > 0 and m["layer"] >= GC.MARGIN and m["pool"] >= GC.MARGIN


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    G34GEN.install_stubs()
    from PerceptualSimilarity.models.networks_basic import PNetLin
    net = PNetLin(pnet_type="alex", pnet_rand=True, use_dropout=True, version="0.1").eval()
    g34 = np.load(os.path.join(HERE, "g34_lpips_alex.npz"))
    lin = torch.load(os.path.join(G34GEN.REF, "PerceptualSimilarity", "models", "weights", "v0.1", "alex.pth"), map_location="cpu")
    assert all(np.array_equal(lin[k].numpy().astype(np.float32), g34[k]) for k in LW.LIN_KEYS), "alex.pth is not what G34 stores"
    state = LW.golden_state(g34)
    assert list(net.state_dict()) == LW.reference_keys()
    net.load_state_dict(state, strict=True)
    if "--search" in sys.argv:
        for name in GC.CASES:
            for j in range(200):
                _, m = case(net, name, j)
                if holds(m):
                    print(f"g35 {name}: smallest passing j = {j} ({m})")
                    break
        return
    out, e32 = {}, 0.0
    for name in GC.CASES:
        arrays, m = case(net, name)
        print(f"g35 {name} (j = {GC.J[name]}): dist {arrays['dist64']}, active {arrays['active']}, smallest squared feature norm {m['floor']:.3g}, "
              f"layer ratio {m['layer']:.1f}, pool ratio {m['pool']:.1f}, e32_grad {m['e32']:.2e}")
        assert m["floor"] > 0, f"{name}: (i) a tap pixel with all-zero features"
        assert m["layer"] >= GC.MARGIN, f"{name}: (ii) a pre-activation within {GC.MARGIN} x the float32 error of zero"
        assert m["pool"] >= GC.MARGIN, f"{name}: (iii) a pool window whose two largest values are within {GC.MARGIN} x the float32 error"
        assert np.isfinite(arrays["grad64"]).all() and np.abs(arrays["grad64"]).max() > 0
        out.update({f"{name}__{k}": v for k, v in arrays.items() if name in GC.STORED or k not in ("pred", "target")})
        e32 = max(e32, m["e32"])
    out["e32_grad"] = np.float64(e32)
    print(f"g35: e32_grad {e32:.3e}")
    blobs = []
    for _ in range(2):
        buf = io.BytesIO()
        np.savez_compressed(buf, **out)
        blobs.append(buf.getvalue())
    assert blobs[0] == blobs[1], "(v) two writes differ"
    assert len(blobs[0]) < 640 * 1024, f"(iv) {len(blobs[0]) / 1024:.1f} KiB"
    path = os.path.join(HERE, "g35_lpips_alex_grad.npz")
    with open(path, "wb") as f:
        f.write(blobs[0])
    print(f"g35_lpips_alex_grad.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
