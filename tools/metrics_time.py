"""Evaluation-metric timing for one test sequence of T = 40 frames, at 180x240 and at 260x346:

    image   v2v_amd.metrics.compute_metrics (two launches, one device-to-host copy) against the reference's loop restated
            (model/train_utils.py:212-248 without LPIPS): per frame `/ 255`, F.mse_loss(...).item(), both frames copied to the host, and
            skimage's structural_similarity there -- its algorithm restated on scipy.ndimage.uniform_filter
            (tests/metrics_reference.ssim_skimage, float32 as current skimage computes float32 frames)
    flow    v2v_amd.metrics.compute_flow_metrics against the reference's operators (model/train_flow_utils.py:229-294 restated: about
            fifteen small torch operators and eight .item() calls per frame), events with 5 channels

Protocol (tools/loss_time.py's): the two variants alternate inside the timed loop, median and minimum of --reps rounds after warm-up, both
orders.  Every variant ends with its results on the host, so the clock is the host's (perf_counter around the call, the device idle before).
The two variants' values are compared first.

Run on the GPU box:  python tools/metrics_time.py [--reps 20] [--out profiles/metrics/metrics_time.jsonl]
For a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/metrics_time.py --calls 20): only N calls of the two raw operators, T = 40
at 260x346."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from convgru_time import emit  # noqa: E402

T, SIZES, EVENT_CHANNELS = 40, ((180, 240), (260, 346)), 5
NAMES = ("dense_EPE", "dense_1PE", "dense_3PE", "sparse_EPE", "sparse_1PE", "sparse_3PE")


def alternate_wall(fns, reps, warmup=3):
    """{name: callable that leaves its results on the host} -> {name: (median ms, min ms)}"""
    import numpy as np
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), float(min(v))) for k, v in times.items()}


def stock_image(pred, frame):
    import torch.nn.functional as F
    import metrics_reference as MR
    import numpy as np
    mse, ssim = [], []
    for t in range(frame.shape[1]):
        p, f = pred[0, t] / 255, frame[0, t] / 255
        mse.append(F.mse_loss(p, f).item())
        p, f = p.detach().cpu().numpy().squeeze(), f.detach().cpu().numpy().squeeze()
        ssim.append(MR.ssim_skimage(p, f, 2, np.float32)[0])
    return mse, ssim


def stock_flow(pred, batch):
    import metrics_reference as MR
    rows = [MR.flow_ratios(pred[0, t], batch["flow"][0, t], batch["events"][0, t]) for t in range(batch["frame"].shape[1] - 1)]
    return [list(c) for c in zip(*rows)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--calls", type=int, default=0, help="only run this many calls of image_metrics and flow_metrics at 260x346 (for a kernel trace)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from v2v_amd import metrics
    assert torch.cuda.is_available(), "metrics_time.py needs the GPU"
    if a.calls:
        h, w = SIZES[-1]
        g = torch.Generator().manual_seed(1)
        frame = (255 * torch.rand((T, 1, h, w), generator=g)).cuda()
        pred = (frame + 20 * torch.randn((T, 1, h, w), generator=g).cuda()).clamp(0, 255)
        flow = (2 * torch.randn((T, 2, h, w), generator=g)).cuda()
        fpred = flow + 1.5 * torch.randn((T, 2, h, w), generator=g).cuda()
        events = torch.randint(-3, 4, (T, EVENT_CHANNELS, h, w), generator=g).float().cuda()
        for _ in range(a.calls):
            metrics.image_metrics(pred, frame)
            metrics.flow_metrics(fpred, flow, events)
        torch.cuda.synchronize()
        return
    for h, w in SIZES:
        g = torch.Generator().manual_seed(h)
        frame = (255 * torch.rand((1, T + 1, 1, h, w), generator=g)).cuda()
        pred = (frame[:, :T] + 20 * torch.randn((1, T, 1, h, w), generator=g).cuda()).clamp(0, 255)
        flow = (2 * torch.randn((1, T, 2, h, w), generator=g)).cuda()
        flow[:, :, :, : h // 4] = 0
        events = (torch.randint(-3, 4, (1, T, EVENT_CHANNELS, h, w), generator=g) * (torch.rand((1, T, 1, h, w), generator=g) < 0.4)).float().cuda()
        fpred = flow + 1.5 * torch.randn((1, T, 2, h, w), generator=g).cuda()
        ibatch = {"frame": frame[:, :T], "sequence_name": [["seq"]], "data_source_idx": torch.tensor([1])}
        fbatch = {"frame": frame, "flow": flow, "events": events, "sequence_name": [["seq"]], "data_source_idx": torch.tensor([2])}
        jobs = {"image": {"fused": lambda: metrics.compute_metrics(pred, ibatch), "stock": lambda: stock_image(pred, ibatch["frame"])},
                "flow": {"fused": lambda: metrics.compute_flow_metrics(fpred, fbatch), "stock": lambda: stock_flow(fpred, fbatch)}}
        got, (mse, ssim) = jobs["image"]["fused"](), jobs["image"]["stock"]()
        d_mse = float(np.max(np.abs(np.array(got["IJRR/seq/MSE"]) - mse) / np.array(mse)))
        d_ssim = float(np.max(np.abs(np.array(got["IJRR/seq/SSIM"]) - ssim)))
        fgot, fstock = jobs["flow"]["fused"](), jobs["flow"]["stock"]()
        d_flow = float(max(np.max(np.abs(np.array(fgot[f"MVSEC/seq/{k}"]) - np.array(v))) for k, v in zip(NAMES, fstock)))
        emit(a, {"what": "agreement", "size": [h, w], "mse_max_rel_diff": d_mse, "ssim_max_abs_diff": d_ssim, "flow_max_abs_diff": d_flow})
        assert d_mse <= 1e-5 and d_ssim <= 1e-5 and d_flow <= 1e-4, "fused and stock disagree"
        for job, pair in jobs.items():
            res = {}
            for order in (("fused", "stock"), ("stock", "fused")):
                for k, (med, mn) in alternate_wall({k: pair[k] for k in order}, a.reps).items():
                    res.setdefault(k, []).append(med)
                    emit(a, {"what": job, "variant": k, "order": "-".join(order), "size": [h, w], "T": T, "ms_median": round(med, 4), "ms_min": round(mn, 4),
                             "reps": a.reps})
            med = {k: sum(v) / len(v) for k, v in res.items()}
            emit(a, {"what": f"{job} summary", "size": [h, w], "T": T, "fused_ms": round(med["fused"], 4), "stock_ms": round(med["stock"], 4),
                     "stock_over_fused": round(med["stock"] / med["fused"], 2)})


if __name__ == "__main__":
    main()
