"""Golden G29 (tests/golden/g29_tc_loss.npz): the reference's temporal_consistency_loss (utils/loss.py:6-69) run in float64 on the CPU on
the seeded inputs of tests/loss_inputs.py, with torch.autograd for the gradients.

    python tests/golden/make_golden_tc_loss.py REFERENCE_DIR        (the reference checkout; or V2V_REFERENCE in the environment)

utils/loss.py is loaded by file path (it needs numpy and torch only).  Stored per pair case (`a` [2,1,20,28], `b` [1,3,13,19]): the
per-sample losses, the four maps, dprocessed0 and dprocessed1 of sum(per-sample losses); for the sequence case `seq` ([2,4,1,24,40],
L0 = 2: the step loop of model/train_utils.py:402-424 with l1, l2 and temporal consistency at weight 1, the flow negated as the classes of
model/loss.py do): the three [B,T] loss tables and dpred of their plain sum.  As the yardstick of the GPU tests, for each of those outputs
the (max, rms) error of the reference's OWN float32 run against its float64 run (`<name>__f32_err`).  The maker asserts in float64 that
no pixel sits on a kink (|processed1 - w|, |processed0|, |processed1| all above 1e-5), so the tests exclude nothing.  Only arrays go
into the file.  Regenerates byte for byte."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("V2V_REFERENCE")
if not REF:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.dirname(HERE))

import loss_inputs as LI  # noqa: E402

spec = importlib.util.spec_from_file_location("reference_utils_loss", os.path.join(REF, "utils", "loss.py"))
RL = importlib.util.module_from_spec(spec)
spec.loader.exec_module(RL)

KINK = 1e-5


def err(a, b):
    d = (a.double() - b.double()).abs()
    return np.array([float(d.max()), float((d ** 2).mean().sqrt())])


def run_pair(inp, dtype):
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    t["processed0"].requires_grad_(True)
    t["processed1"].requires_grad_(True)
    loss, maps = RL.temporal_consistency_loss(*(t[k] for k in LI.KEYS), output_images=True, reduce_batch=False)
    d0, d1 = torch.autograd.grad(loss.sum(), (t["processed0"], t["processed1"]))
    out = {k: maps[k].detach() for k in ("image0_warped_to1", "processed0_warped_to1", "visibility_mask", "error_map")}
    out.update(loss=loss.detach(), dprocessed0=d0, dprocessed1=d1)
    return out, t


def run_seq(inp, dtype):
    pred = torch.from_numpy(inp["pred"]).to(dtype).requires_grad_(True)
    frame, flow = torch.from_numpy(inp["frame"]).to(dtype), torch.from_numpy(inp["flow"]).to(dtype)
    b, t = pred.shape[:2]
    rows = {k: [] for k in ("tc", "l1", "l2")}
    gaps = []
    for s in range(t):
        p, f = pred[:, s], frame[:, s]
        rows["l1"].append((p - f).abs().mean(dim=(1, 2, 3)))
        rows["l2"].append(((p - f) ** 2).mean(dim=(1, 2, 3)))
        if s >= LI.SEQ_L0:
            tc, maps = RL.temporal_consistency_loss(frame[:, s - 1], f, pred[:, s - 1], p, -flow[:, s], output_images=True, reduce_batch=False)
            gaps.append((p - maps["processed0_warped_to1"]).abs().min().item())
        else:
            tc = torch.zeros(b, dtype=dtype)
        rows["tc"].append(tc)
    out = {k: torch.stack(v, 1) for k, v in rows.items()}
    (dpred,) = torch.autograd.grad(sum(v.sum() for v in out.values()), pred)
    return dict({k: v.detach() for k, v in out.items()}, dpred=dpred), min(gaps)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    out = dict(seed=np.array(LI.SEED))
    for name in sorted(LI.PAIR_SHAPES):
        inp = LI.pair_inputs(name)
        r64, t = run_pair(inp, torch.float64)
        r32, _ = run_pair(inp, torch.float32)
        gap = min((t["processed1"] - r64["processed0_warped_to1"]).abs().min().item(), t["processed0"].abs().min().item(), t["processed1"].abs().min().item())
        assert gap > KINK, f"{name}: a pixel sits {gap:.2e} from a kink"
        for k, v in r64.items():
            e = err(r32[k], v)
            assert (e > 0).all(), (name, k)
            out[f"{name}__{k}"] = v.numpy()
            out[f"{name}__{k}__f32_err"] = e
        print(f"g29 {name}: loss {r64['loss'].tolist()}, nearest kink {gap:.2e}, float32 errors " + ", ".join(f"{k} {out[f'{name}__{k}__f32_err'].tolist()}" for k in r64))
    inp = LI.seq_inputs()
    r64, gap = run_seq(inp, torch.float64)
    r32, _ = run_seq(inp, torch.float32)
    gap = min(gap, float(np.abs(inp["pred"]).min()))
    assert gap > KINK, f"seq: a pixel sits {gap:.2e} from a kink"
    for k, v in r64.items():
        e = err(r32[k], v)
        assert (e > 0).all(), ("seq", k)
        out[f"seq__{k}"] = v.numpy()
        out[f"seq__{k}__f32_err"] = e
    print(f"g29 seq: nearest kink {gap:.2e}, float32 errors " + ", ".join(f"{k} {out[f'seq__{k}__f32_err'].tolist()}" for k in r64))
    path = os.path.join(HERE, "g29_tc_loss.npz")
    np.savez_compressed(path, **out)
    print(f"g29_tc_loss.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
