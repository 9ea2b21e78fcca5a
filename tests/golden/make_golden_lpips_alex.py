"""Golden G34 (tests/golden/g34_lpips_alex.npz): the reference's LPIPS network PerceptualSimilarity/models/networks_basic.py:PNetLin
(pnet_type='alex', version='0.1', spatial=False, eval mode) called the way ModelInterface.compute_metrics (model/train_utils.py:236) calls
it through PerceptualLoss.forward: frame by frame, a [C,H,W] image (one channel broadcasts to three in the scaling layer), normalize=True:
2x - 1, forward(target, pred), on the CPU.

    python tests/golden/make_golden_lpips_alex.py REFERENCE_DIR        (the reference checkout; or V2V_REFERENCE in the environment)

networks_basic.py imports four modules its forward never touches; they are stubbed in sys.modules here as in make_golden_lpips.py
(torchvision.models.alexnet -> an object whose .features is the standard 13-module nn.Sequential, skimage, IPython.embed, tqdm).  The five
linear layers come from the reference's models/weights/v0.1/alex.pth (1,152 floats, some exactly 0) and are stored with the scaling
layer's shift and scale; the backbone is the seeded recipe of tests/lpips_alex_weights.py, not stored.

Per case (tests/lpips_alex_weights.CASES): <case>__taps64 [T,5] / __dist64 [T] from the float64 run, __taps32 / __dist32 from the float32
run; <case>__pred / __target for a, b, c and `close` only (r180 and r260 are recipe only).  e32_tap / e32_dist: the maximum over ALL cases
and frames of the float32 run's relative error against the float64 run -- the yardstick of the GPU tests.  Asserted before writing: every
tap term > 0, no tap pixel whose features are all zero.  Regenerates byte for byte."""
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

import lpips_alex_weights as LW  # noqa: E402


def _alexnet(pretrained=False, **_):
    features = nn.Sequential(
        nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2))
    assert len(features) == 13
    return types.SimpleNamespace(features=features)


def install_stubs():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    tv_models = module("torchvision.models", alexnet=_alexnet)
    module("torchvision", models=tv_models)
    sk = module("skimage")
    sk.__path__ = []
    for sub in ("color", "transform", "measure"):
        setattr(sk, sub, module(f"skimage.{sub}"))
    sk.metrics = module("skimage.metrics", structural_similarity=None)
    module("IPython", embed=None)
    module("tqdm", tqdm=None)


def run(net, pred, target, dtype):
    """(taps [T,5], dist [T], the smallest squared feature norm of any tap pixel) of PNetLin, frame by frame as compute_metrics drives it."""
    net = net.to(dtype)
    taps, dist, floor = [], [], np.inf
    feats = []
    res = []
    hooks = [getattr(net.net, f"slice{s}").register_forward_hook(lambda m, i, o: feats.append(o.detach())) for s in range(1, 6)]
    # the tap means from the lin layers' outputs, averaged as spatial_average does: forward's own list shares its first entry with the sum
    # (`val = res[0]; val += res[l]` adds in place)
    hooks += [lin.model.register_forward_hook(lambda m, i, o: res.append(o.detach().mean([2, 3], keepdim=True))) for lin in net.lins]
    with torch.no_grad():
        for t in range(pred.shape[0]):
            p, g = torch.from_numpy(pred[t]).to(dtype), torch.from_numpy(target[t]).to(dtype)
            del res[:]
            val = net(2 * g - 1, 2 * p - 1)
            assert val.shape == (1, 1, 1, 1) and len(res) == 5
            taps.append([float(r) for r in res] if dtype == torch.float64 else [np.float32(r.item()) for r in res])
            dist.append(val.item())
    for h in hooks:
        h.remove()
    for f in feats:
        floor = min(floor, float((f.double() ** 2).sum(1).min()))
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    return np.array(taps, dtype=np_dtype), np.array(dist, dtype=np_dtype), floor


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    install_stubs()
    from PerceptualSimilarity.models.networks_basic import PNetLin
    net = PNetLin(pnet_type="alex", pnet_rand=True, use_dropout=True, version="0.1").eval()
    assert list(net.state_dict()) == LW.reference_keys(), "PNetLin's state dict is not the 17 keys tests/lpips_alex_weights.py lists"
    lin = torch.load(os.path.join(REF, "PerceptualSimilarity", "models", "weights", "v0.1", "alex.pth"), map_location="cpu")
    assert sorted(lin) == sorted(LW.LIN_KEYS) and all(float(v.min()) >= 0 for v in lin.values()) and sum(v.numel() for v in lin.values()) == 1152
    state = {k: torch.from_numpy(v) for k, v in LW.backbone_state().items()}
    state.update(lin)
    missing = net.load_state_dict(state, strict=False)
    assert sorted(missing.missing_keys) == ["scaling_layer.scale", "scaling_layer.shift"] and not missing.unexpected_keys
    out = {k: lin[k].numpy().astype(np.float32) for k in LW.LIN_KEYS}
    out["shift"] = net.scaling_layer.shift.numpy().astype(np.float32)
    out["scale"] = net.scaling_layer.scale.numpy().astype(np.float32)
    e_tap = e_dist = 0.0
    for name in LW.CASES:
        pred, target = LW.case_inputs(name)
        if name in LW.STORED:
            out[f"{name}__pred"], out[f"{name}__target"] = pred, target
        t64, d64, floor = run(net, pred, target, torch.float64)
        t32, d32, _ = run(net, pred, target, torch.float32)
        net.float()
        assert floor > 0, f"{name}: a pixel with all-zero features at a tap"
        assert (t64 > 0).all() and np.isfinite(t32).all(), f"{name}: a tap term that is not > 0"
        out[f"{name}__taps64"], out[f"{name}__dist64"], out[f"{name}__taps32"], out[f"{name}__dist32"] = t64, d64, t32, d32
        rt = float((np.abs(t32.astype(np.float64) - t64) / t64).max())
        rd = float((np.abs(d32.astype(np.float64) - d64) / d64).max())
        e_tap, e_dist = max(e_tap, rt), max(e_dist, rd)
        print(f"g34 {name}: dist {d64}, smallest squared feature norm {floor:.3g}, float32 relative error tap {rt:.2e}, dist {rd:.2e}")
    out["e32_tap"], out["e32_dist"] = np.float64(e_tap), np.float64(e_dist)
    print(f"g34: e32_tap {e_tap:.3e}, e32_dist {e_dist:.3e}")
    path = os.path.join(HERE, "g34_lpips_alex.npz")
    np.savez_compressed(path, **out)
    print(f"g34_lpips_alex.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
