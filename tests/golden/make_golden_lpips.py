"""Golden G30 (tests/golden/g30_lpips_vgg.npz): the reference's LPIPS network PerceptualSimilarity/models/networks_basic.py:PNetLin
(pnet_type='vgg', version='0.1', spatial=False, eval mode) called the way model/loss.py:95-119 calls it (one channel repeated three times,
normalize=True: 2x - 1, forward(target, pred)), on the CPU.

    python tests/golden/make_golden_lpips.py REFERENCE_DIR        (the reference checkout; or V2V_REFERENCE in the environment)

networks_basic.py imports four modules its forward never touches; they are stubbed in sys.modules here (torchvision.models.vgg16 -> an object
whose .features is the standard 13-convolution / 5-pool nn.Sequential, skimage with color / transform / metrics / measure, IPython.embed,
tqdm).  The five linear layers come from the reference's models/weights/v0.1/vgg.pth and are stored (with the scaling layer's shift and
scale: 1,479 floats); the backbone is the seeded recipe of tests/lpips_weights.py, not stored.

Per case (tests/lpips_weights.CASES: a, b, c and `close`): pred, target, and -- from the float64 run, the float32 run and the CPU
bf16-autocast run (the yardstick of the GPU tests) -- dist [B] and dpred = the gradient of sum_b (b + 1) dist_b:
<case>__dist64 / __dpred64 / __dist32 / __dpred32 / __dist16 / __dpred16.  Nothing tap-sized.  Asserted before writing: no pixel whose
features are all zero at any tap (the reference's gradient is NaN there), finite gradients.  Regenerates byte for byte."""
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

import lpips_weights as LW  # noqa: E402


def _vgg16(pretrained=False, **_):
    cfg = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
    layers, cin = [], 3
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return types.SimpleNamespace(features=nn.Sequential(*layers))


def install_stubs():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    tv_models = module("torchvision.models", vgg16=_vgg16)
    module("torchvision", models=tv_models)
    sk = module("skimage")
    sk.__path__ = []
    for sub in ("color", "transform", "measure"):
        setattr(sk, sub, module(f"skimage.{sub}"))
    sk.metrics = module("skimage.metrics", structural_similarity=None)
    module("IPython", embed=None)
    module("tqdm", tqdm=None)


def run(net, pred, target, dtype, autocast=False):
    """(dist [B], dpred, taps) of PNetLin the way perceptual_loss.__call__ drives it."""
    net = net.to(dtype)
    p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    t = torch.from_numpy(target).to(dtype)
    p3 = torch.cat([p, p, p], dim=1) if p.shape[1] == 1 else p
    t3 = torch.cat([t, t, t], dim=1) if t.shape[1] == 1 else t
    taps = []
    hooks = [getattr(net.net, f"slice{s}").register_forward_hook(lambda m, i, o: taps.append(o.detach().clone())) for s in range(1, 6)]
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            dist = net(2 * t3 - 1, 2 * p3 - 1)
    else:
        dist = net(2 * t3 - 1, 2 * p3 - 1)
    for h in hooks:
        h.remove()
    dist = dist.reshape(-1).to(dtype)
    (dist * torch.arange(1, dist.numel() + 1, dtype=dtype)).sum().backward()
    return dist.detach().numpy(), p.grad.numpy(), taps


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    install_stubs()
    from PerceptualSimilarity.models.networks_basic import PNetLin
    net = PNetLin(pnet_type="vgg", pnet_rand=True, use_dropout=True, version="0.1").eval()
    assert list(net.state_dict()) == LW.reference_keys(), "PNetLin's state dict is not the 33 keys tests/lpips_weights.py lists"
    lin = torch.load(os.path.join(REF, "PerceptualSimilarity", "models", "weights", "v0.1", "vgg.pth"), map_location="cpu")
    assert sorted(lin) == sorted(LW.LIN_KEYS) and all(float(v.min()) > 0 for v in lin.values())
    state = {k: torch.from_numpy(v) for k, v in LW.backbone_state().items()}
    state.update(lin)
    missing = net.load_state_dict(state, strict=False)
    assert sorted(missing.missing_keys) == ["scaling_layer.scale", "scaling_layer.shift"] and not missing.unexpected_keys
    out = {k: lin[k].numpy().astype(np.float32) for k in LW.LIN_KEYS}
    out["shift"] = net.scaling_layer.shift.numpy().astype(np.float32)
    out["scale"] = net.scaling_layer.scale.numpy().astype(np.float32)
    for name in LW.CASES:
        pred, target = LW.case_inputs(name)
        out[f"{name}__pred"], out[f"{name}__target"] = pred, target
        for tag, dtype, autocast in (("32", torch.float32, False), ("16", torch.float32, True), ("64", torch.float64, False)):
            dist, dpred, taps = run(net, pred, target, dtype, autocast)
            assert np.isfinite(dist).all() and np.isfinite(dpred).all(), (name, tag)
            if tag == "64":
                assert len(taps) == 10
                for tp in taps:
                    assert float((tp ** 2).sum(1).min()) > 0, f"{name}: a pixel with all-zero features at a tap"
                peak = max(float(tp.max()) for tp in taps)
            out[f"{name}__dist{tag}"], out[f"{name}__dpred{tag}"] = dist, dpred
        net.float()

        def rel(a, b):
            return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))
        g16, g64 = out[f"{name}__dpred16"].astype(np.float64).ravel(), out[f"{name}__dpred64"].ravel()
        print(f"g30 {name}: dist {out[f'{name}__dist64']}, tap peak {peak:.1f}, bf16-autocast rel-L2 error dist {rel(out[f'{name}__dist16'], out[f'{name}__dist64']):.2e}, "
              f"dpred {rel(out[f'{name}__dpred16'], out[f'{name}__dpred64']):.3f}, cos {float(g16 @ g64 / np.linalg.norm(g16) / np.linalg.norm(g64)):.4f}")
    path = os.path.join(HERE, "g30_lpips_vgg.npz")
    np.savez_compressed(path, **out)
    print(f"g30_lpips_vgg.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
