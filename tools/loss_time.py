"""Image-loss timing at the training shape (config/train_v2v_e2vid_10k.yaml: pred / frame [12,40,1,128,128], temporal_consistency_L0 20, l1 +
temporal consistency at weight 1), forward + backward to pred:

    fused    v2v_amd.loss_ops.sequence_losses: one autograd Function, a fixed number of launches for all 40 steps
    stock    the same losses by the reference's formula (utils/loss.py:6-69, model/loss.py) in stock PyTorch operators, step by step as
             ModelInterface.calc_loss does (model/train_utils.py:402-424), float32, under torch.autograd

Protocol (tools/convgru_time.py's `alternate`): HIP events, the two variants alternating inside the timed loop, median and minimum of --reps
rounds after warm-up, both orders (fused first, stock first).  Launch counts come from one torch.profiler pass per variant, run after the
timing ("not measured" when the profiler gives no device events).  The two variants' loss tables are compared first; the gradients' difference is reported.

Run on the GPU box:  python tools/loss_time.py [--reps 30] [--out profiles/loss/loss_time.jsonl]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from convgru_time import alternate, emit  # noqa: E402

SHAPE, L0 = (12, 40, 1, 128, 128), 20


def stock_warp(img, flow):
    import torch
    import torch.nn.functional as F
    h, w = img.shape[2:]
    xx, yy = torch.meshgrid(torch.arange(w, device=img.device), torch.arange(h, device=img.device), indexing="xy")
    gx = (2 * (xx.float() + flow[:, 0]) / (w - 1)) - 1
    gy = (2 * (yy.float() + flow[:, 1]) / (h - 1)) - 1
    return F.grid_sample(img, torch.stack([gx, gy], dim=3), align_corners=True)


def stock_losses(pred, frame, flow, l0, alpha=50.0):
    import torch
    b, t = pred.shape[:2]
    l1, tc = torch.zeros((b, t), device=pred.device), torch.zeros((b, t), device=pred.device)
    for s in range(t):
        image, p1 = frame[:, s], pred[:, s]
        l1[:, s] = torch.mean(torch.abs(p1 - image).reshape((b, -1)), dim=1)
        if s >= l0:
            vis = torch.exp(-alpha * (image - stock_warp(frame[:, s - 1], -flow[:, s])) ** 2)
            w = stock_warp(torch.clamp(pred[:, s - 1], 0, 255), -flow[:, s])
            tc[:, s] = (vis * torch.abs(p1 - w) / (torch.abs(p1) + torch.abs(w) + 1e-5)).mean(dim=(1, 2, 3))
    return l1, tc


def launches(fn):
    """Device kernel and memset / memcpy events of one call, or None when the profiler reports none."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as e:                                                     # the measurement goes on without the count
        print(f"launch count not measured: {e!r}", flush=True)
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from v2v_amd import loss_ops
    assert torch.cuda.is_available(), "loss_time.py needs the GPU"
    b, t, c, h, w = SHAPE
    g = torch.Generator().manual_seed(1)
    frame = (0.3 + 0.4 * torch.rand(SHAPE, generator=g)).cuda()
    flow = (6 * torch.rand((b, t, 2, h, w), generator=g) - 3).cuda()
    pred = (1.4 * torch.rand(SHAPE, generator=g) - 0.2).cuda().requires_grad_(True)

    def fused():
        pred.grad = None
        out = loss_ops.sequence_losses(pred, frame, flow, 1.0, None, 1.0, L0)
        (out["l1_loss"].sum() + out["temporal_consistency_loss"].sum()).backward()
        return out["l1_loss"], out["temporal_consistency_loss"], pred.grad

    def stock():
        pred.grad = None
        l1, tc = stock_losses(pred, frame, flow, L0)
        (l1.sum() + tc.sum()).backward()
        return l1, tc, pred.grad

    f, s = [v.detach().clone() for v in fused()], [v.detach().clone() for v in stock()]
    names = ("l1", "tc", "dpred")
    diff = {k: float((x.double() - y.double()).abs().max()) for k, x, y in zip(names, f, s)}
    rel = {k: float((x.double() - y.double()).norm() / y.double().norm()) for k, x, y in zip(names, f, s)}
    emit(a, {"what": "agreement", "max_abs_diff": diff, "rel_l2_diff": rel, "max_abs_stock": {k: float(y.abs().max()) for k, y in zip(names, s)}})
    # the loss tables must agree; the gradient is reported only: pixels with processed1 and the warp both near 0 have gradients thousands
    # of times the typical one, set by the last bits of the warp, and dominate any norm (tests/test_loss_ops.py pins the gradient)
    assert rel["l1"] <= 1e-5 and rel["tc"] <= 1e-5, "fused and stock disagree"
    res = {}
    for order in (("fused", "stock"), ("stock", "fused")):
        fns = {k: {"fused": fused, "stock": stock}[k] for k in order}
        for k, (med, mn) in alternate(fns, a.reps).items():
            res.setdefault(k, []).append((med, mn))
            emit(a, {"what": "fwd+bwd", "variant": k, "order": "-".join(order), "shape": list(SHAPE), "L0": L0, "ms_median": round(med, 4), "ms_min": round(mn, 4),
                     "reps": a.reps})
    count = {"fused": launches(fused), "stock": launches(stock)}
    med = {k: sum(m for m, _ in v) / len(v) for k, v in res.items()}
    emit(a, {"what": "summary", "fused_ms": round(med["fused"], 4), "stock_ms": round(med["stock"], 4), "stock_over_fused": round(med["stock"] / med["fused"], 2),
             "device_events_fused": count["fused"], "device_events_stock": count["stock"]})


if __name__ == "__main__":
    main()
