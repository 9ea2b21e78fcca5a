"""Golden G33 (tests/golden/g33_metrics.npz): the evaluation metrics of the reference's test loop on the seeded inputs of
tests/metrics_reference.py.

    python tests/golden/make_golden_metrics.py REFERENCE_DIR        (the reference checkout; or V2V_REFERENCE in the environment)

Flow part -- the reference's OWN FlowModelInterface.compute_metrics (model/train_flow_utils.py:229-294), called on a stand-in `self` that has
only `.device`.  The module is imported from REFERENCE_DIR by file path; empty stand-in modules take the place of what it imports at
module level and the call does not need, third-party packages included (torchmetrics, skimage, torchvision, PerceptualSimilarity, utils.util,
model.loss, model.train_utils; utils.data only gives `data_sources`, taken from v2v_amd.datasets).  No line-by-line restatement was needed.
Per case `<name>` of FLOW_CASES: `__ratios` float32 [T,6] (dense_EPE, dense_1PE, dense_3PE, sparse_EPE, sparse_1PE, sparse_3PE: the
reference's values, float32 on the CPU), `__counts` int64 [T,6] and `__ee_sums` float64 [T,2] (the float64 sum of the float32 EE with
the square root correctly rounded, as sqrtf is on the device; torch's vectorised CPU sqrt, which the reference's CPU run above goes
through, is an ulp off on a few values in a hundred, far inside the float32 summation error that the ratios are compared with; both from
tests/metrics_reference.flow_terms -- the maker asserts that the reference's N-PE values are exactly these counts' float32 quotients and
its EPE values these sums' quotients to float32 summation error, exactly in the integer-exact case), `__sha` the SHA-256 of the
regenerated inputs.  The maker asserts that no EE of a valid pixel lies within 1e-4 of 1 or 3, so an ulp in EE moves no count.

Image part -- the maker does not depend on skimage or torchmetrics: the SSIM truth is skimage.metrics.structural_similarity's published
algorithm (defaults: 7x7 uniform window, use_sample_covariance, K1 0.01, K2 0.03; crop 3) restated on scipy.ndimage.uniform_filter
(tests/metrics_reference.ssim_skimage), on frames divided by 255 in float32 as the reference does.  Per case of IMAGE_CASES and per
data_range `r` in (2, 1): `__ssim64_r<r>` float64 [T] the truth, `__ssim32_r<r>` float64 [T] the same algorithm computed in float32 (what
current skimage does for float32 frames); `__mse32` / `__mse64` [T]: F.mse_loss in float32 (the reference's number) and in float64 on the
float32 frames; `__sha`.  The four small cases also store `__S_r<r>` float64 [T,H-6,W-6], the truth's S of every window.  Inputs are not
stored: they are regenerated from their seeds and checked against `__sha`.

Only arrays go into the file.  Regenerates byte for byte."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("V2V_REFERENCE")
if not REF:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import metrics_reference as MR  # noqa: E402
from v2v_amd.datasets import data_sources  # noqa: E402

GAP = 1e-4


def stand_in(name, **attrs):
    mod = types.ModuleType(name)
    mod.__path__ = []
    mod.__getattr__ = lambda attr: None          # every `from <stand-in> import x` gives None
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    return mod


def load_reference_flow_module():
    for name in ("torchmetrics", "torchmetrics.image", "torchmetrics.image.lpip", "skimage", "skimage.metrics", "PerceptualSimilarity",
                 "PerceptualSimilarity.models", "torchvision", "torchvision.models", "torchvision.models.optical_flow", "utils", "utils.util",
                 "model", "model.loss", "model.train_utils"):
        stand_in(name)
    stand_in("utils.data", data_sources=data_sources)
    spec = importlib.util.spec_from_file_location("reference_train_flow_utils", os.path.join(REF, "model", "train_flow_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def flow_part(out):
    RF = load_reference_flow_module()
    me = types.SimpleNamespace(device=torch.device("cpu"))
    for name, (T, C, H, W, _, exact) in MR.FLOW_CASES.items():
        pred, gt, events = (torch.from_numpy(v) for v in MR.flow_case(name))
        batch = {"sequence_name": [["seq"]], "data_source_idx": torch.tensor([2]), "frame": torch.zeros((1, T + 1, 1, H, W)), "flow": gt[None],
                 "events": events[None]}
        got = RF.FlowModelInterface.compute_metrics(me, pred[None], batch)
        assert list(got) == [f"MVSEC/seq/{k}" for k in MR.FLOW_NAMES], list(got)
        ratios = np.array([got[f"MVSEC/seq/{k}"] for k in MR.FLOW_NAMES], dtype=np.float64).T
        assert np.array_equal(ratios.astype(np.float32).astype(np.float64), ratios)
        counts, sums = [], []
        for t in range(T):
            c, s, EE = MR.flow_terms(pred[t], gt[t], events[t])
            valid = torch.logical_not(torch.isnan(gt[t, 0]) | torch.isnan(gt[t, 1]) | ((gt[t, 0] == 0) & (gt[t, 1] == 0)))
            if not exact and c[0]:
                gap = float(torch.minimum((EE[valid] - 1).abs(), (EE[valid] - 3).abs()).min())
                assert gap > GAP, f"{name} frame {t}: an EE sits {gap:.2e} from a threshold"
            for m in range(2):                   # the reference's N-PE values are these counts' float32 quotients, its EPE their sums' (to float32 summation error)
                for k in range(2):
                    want = np.float32(c[2 + 2 * m + k]) / np.float32(c[m]) if c[m] else np.float32(0)
                    assert np.float32(ratios[t, 3 * m + 1 + k]) == want, (name, t, m, k)
                if c[m]:
                    assert abs(ratios[t, 3 * m] - s[m] / c[m]) <= H * W * 2.0 ** -24 * abs(s[m] / c[m]), (name, t, m)
                    assert not exact or np.float32(ratios[t, 3 * m]) == np.float32(s[m] / c[m])
                else:
                    assert ratios[t, 3 * m] == 0
            counts.append(c)
            sums.append(s)
        counts = np.stack(counts)
        assert T < 4 or (counts[1] == 0).all() and counts[2, 0] == counts[2, 1] > 0 and counts[3, 0] > 0 and counts[3, 1] == 0
        out[f"{name}__ratios"] = ratios.astype(np.float32)
        out[f"{name}__counts"] = counts
        out[f"{name}__ee_sums"] = np.stack(sums)
        out[f"{name}__sha"] = np.array(MR.sha(*MR.flow_case(name)))
        print(f"g33 {name}: counts of frame 0 {counts[0].tolist()}, ratios {ratios[0].tolist()}")


def image_part(out):
    for name, (T, H, W, _) in MR.IMAGE_CASES.items():
        pred, image = MR.image_case(name)
        x, y = MR.scaled(pred, 255.0), MR.scaled(image, 255.0)
        tx, ty = torch.from_numpy(x), torch.from_numpy(y)
        out[f"{name}__mse32"] = np.array([float(F.mse_loss(tx[t], ty[t])) for t in range(T)])
        out[f"{name}__mse64"] = np.array([float(F.mse_loss(tx[t].double(), ty[t].double())) for t in range(T)])
        for r in MR.DATA_RANGES:
            tag = f"r{int(r)}"
            truth = [MR.ssim_skimage(x[t], y[t], r, np.float64) for t in range(T)]
            f32 = [MR.ssim_skimage(x[t], y[t], r, np.float32) for t in range(T)]
            out[f"{name}__ssim64_{tag}"] = np.array([m for m, _ in truth])
            out[f"{name}__ssim32_{tag}"] = np.array([m for m, _ in f32])
            if name in MR.SMALL_IMAGE_CASES:
                out[f"{name}__S_{tag}"] = np.stack([S for _, S in truth])
        out[f"{name}__sha"] = np.array(MR.sha(pred, image))
        print(f"g33 {name}: mse {out[f'{name}__mse64'].tolist()}, ssim (data_range 2) {out[f'{name}__ssim64_r2'].tolist()}, float32 restatement off by "
              f"{np.abs(out[f'{name}__ssim32_r2'] - out[f'{name}__ssim64_r2']).max():.2e}")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    out = {}
    flow_part(out)
    image_part(out)
    path = os.path.join(HERE, "g33_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"g33_metrics.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
