"""The evaluation metrics of the reference's test loop on the device kernels of v2v_amd/csrc/v2v_metrics.hpp (include/v2v_metrics.h).

    image_metrics(pred, image, ...)       MSE and SSIM (skimage's defaults: 7x7 uniform window, sample covariance) of T frame pairs:
                                          float64 [T, 2] on the device, two launches, no host synchronisation
    flow_metrics(pred, gt, events)        the counts int64 [T, 6] and end-point-error sums float64 [T, 2] of T flow frames, likewise
    compute_metrics(pred, batch)          ModelInterface.compute_metrics (model/train_utils.py:212-248): same keys, lists of floats,
                                          one device-to-host copy per call
    compute_flow_metrics(pred, batch)     FlowModelInterface.compute_metrics (model/train_flow_utils.py:229-294), likewise

The reference divides both frames by 255 in float32, takes F.mse_loss on the device, copies both frames to the host and runs
skimage.metrics.structural_similarity(data_range=2) there, frame by frame; the kernels do the same arithmetic with every moment in float64.
Single channel only.  The LPIPS-alex network is v2v_amd.lpips_alex.LPIPSAlex: handed to compute_metrics as `lpips_fn` it takes all T frames
in one batched pass; any other callable (the reference's own module) is called frame by frame.  No CPU path.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np
import torch

from . import _lib
from ._lib import launch, ptr
from .datasets import data_sources

COUNTS = ("n_dense", "n_sparse", "dense_gt1", "dense_gt3", "sparse_gt1", "sparse_gt3")
FLOW_METRICS = ("dense_EPE", "dense_1PE", "dense_3PE", "sparse_EPE", "sparse_1PE", "sparse_3PE")
WIN = 7


def _frames(name, t, channels=None):
    """t as [T, C, H, W]: float32, CUDA, every frame contiguous; frames may be any distance apart.  -> (tensor, frame stride)"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 (got {t.dtype})")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA tensor (v2v_amd has no CPU fallback)")
    if t.dim() == 5:
        if t.shape[0] != 1:
            raise ValueError(f"{name}: the batch size must be 1 for testing (got {t.shape[0]})")
        t = t[0]
    if t.dim() != 4:
        raise ValueError(f"{name} must be [T,C,H,W] or [1,T,C,H,W] (got {tuple(t.shape)})")
    if channels is not None and t.shape[1] != channels:
        raise ValueError(f"{name} must have {channels} channel(s) (got {t.shape[1]})")
    t = t.detach()
    _, c, h, w = t.shape
    if t.stride()[1:] != (h * w, w, 1) or t.stride(0) < 0:
        t = t.contiguous()
    return t, t.stride(0)


def _with_channel(t):
    return t.unsqueeze(1) if isinstance(t, torch.Tensor) and t.dim() == 3 else t


def image_metrics(pred: torch.Tensor, image: torch.Tensor, divisor: float = 255.0, data_range: float = 2.0, ssim_map: bool = False):
    """pred, image [T,H,W], [T,1,H,W] or [1,T,1,H,W] float32 CUDA -> float64 [T, 2] = (mse, ssim) of `pred / divisor` against
    `image / divisor`; with ssim_map also S of every window, float64 [T, H-6, W-6].  Nothing is copied to the host."""
    _lib.require_gpu()
    pred, ps = _frames("pred", _with_channel(pred), 1)
    image, is_ = _frames("image", _with_channel(image), 1)
    if pred.shape != image.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and image {tuple(image.shape)} differ in shape")
    if pred.device != image.device:
        raise ValueError("pred and image are on different devices")
    T, _, H, W = pred.shape
    if H < WIN or W < WIN:
        raise ValueError(f"the 7x7 window needs H >= 7 and W >= 7 (got {H} x {W})")
    L = _lib.lib()
    dev = pred.device
    out = torch.empty((T, 2), dtype=torch.float64, device=dev)
    smap = torch.empty((T, H - WIN + 1, W - WIN + 1), dtype=torch.float64, device=dev) if ssim_map else None
    if T:
        n = L.v2v_image_metrics_workspace_bytes(T, H, W)
        _lib.check(min(n, 0))
        ws = torch.empty((n // 8,), dtype=torch.float64, device=dev)
        launch("v2v_image_metrics_hip", dev, ptr(pred), ps, ptr(image), is_, T, H, W, float(divisor), float(data_range), ptr(ws), ptr(out), ptr(smap))
    return (out, smap) if ssim_map else out


def flow_metrics(pred: torch.Tensor, gt: torch.Tensor, events: torch.Tensor):
    """pred, gt [T,2,H,W], events [T,C,H,W] (or with a leading batch of 1) float32 CUDA -> counts int64 [T, 6] (COUNTS) and ee_sums
    float64 [T, 2]: the sum of the float32 end-point error over the valid and over the sparse pixels.  Nothing is copied to the host."""
    _lib.require_gpu()
    pred, ps = _frames("pred", pred, 2)
    gt, gs = _frames("gt", gt, 2)
    events, es = _frames("events", events)
    if pred.shape != gt.shape or events.shape[0] != pred.shape[0] or events.shape[2:] != pred.shape[2:]:
        raise ValueError(f"pred {tuple(pred.shape)}, gt {tuple(gt.shape)} and events {tuple(events.shape)} do not match")
    if not (pred.device == gt.device == events.device):
        raise ValueError("pred, gt and events are on different devices")
    T, _, H, W = pred.shape
    Cn = events.shape[1]
    if Cn < 1 or H < 1 or W < 1 or H * W >= 1 << 24:
        raise ValueError(f"need at least one event channel and 1 <= H * W < 2^24 (got C {Cn}, {H} x {W})")
    L = _lib.lib()
    dev = pred.device
    counts = torch.empty((T, 6), dtype=torch.int64, device=dev)
    sums = torch.empty((T, 2), dtype=torch.float64, device=dev)
    if T:
        n = L.v2v_flow_metrics_workspace_bytes(T, H, W)
        _lib.check(min(n, 0))
        ws = torch.empty((n // 8,), dtype=torch.int64, device=dev)
        launch("v2v_flow_metrics_hip", dev, ptr(pred), ps, ptr(gt), gs, ptr(events), es, T, Cn, H, W, ptr(ws), ptr(counts), ptr(sums))
    return counts, sums


def _log_prefix(batch):
    data_source = data_sources[batch["data_source_idx"][0]]
    return f"{data_source.upper()}/{batch['sequence_name'][0][0]}"


def compute_metrics(pred, batch, lpips_fn=None):
    """ModelInterface.compute_metrics: pred and batch["frame"] [1,T,1,H,W] -> {"SOURCE/sequence/MSE": [T floats], ".../SSIM": [...]} and
    ".../LPIPS" when lpips_fn is given: a v2v_amd.lpips_alex.LPIPSAlex runs all T frames in one batched pass (its `sequence`); any other
    callable is called as the reference calls its own, lpips_fn(pred / 255, frame / 255, normalize=True) per frame.  One device-to-host copy."""
    _lib.require_gpu()
    frame = batch["frame"]
    if frame.dim() != 5 or frame.shape[0] != 1:
        raise ValueError("Batch size must be 1 for testing.")
    prefix = _log_prefix(batch)
    cols = [image_metrics(pred, frame)]
    from .lpips_alex import LPIPSAlex   # here, not at the top: this module's names stay what they are
    if isinstance(lpips_fn, LPIPSAlex):
        cols.append(lpips_fn.sequence(pred, frame).double().reshape(-1, 1))
    elif lpips_fn is not None:
        lp = [lpips_fn(pred[0, t] / 255, frame[0, t] / 255, normalize=True).reshape(()) for t in range(frame.shape[1])]
        cols.append(torch.stack(lp).double().reshape(-1, 1) if lp else torch.empty((0, 1), dtype=torch.float64, device=frame.device))
    host = torch.cat(cols, dim=1).cpu().numpy()
    metrics = defaultdict(list)
    metrics[f"{prefix}/MSE"] = host[:, 0].tolist()
    if lpips_fn is not None:
        metrics[f"{prefix}/LPIPS"] = host[:, 2].tolist()
    metrics[f"{prefix}/SSIM"] = host[:, 1].tolist()
    return metrics


def flow_ratios(counts: np.ndarray, ee_sums: np.ndarray) -> np.ndarray:
    """host side of compute_flow_metrics: counts [T,6], ee_sums [T,2] -> float32 [T,6] in FLOW_METRICS order.  N-PE is the float32 count over
    the float32 count, EPE the float64 sum over the count rounded to float32, 0 where the count is 0."""
    counts, ee_sums = np.asarray(counts, dtype=np.int64), np.asarray(ee_sums, dtype=np.float64)
    out = np.zeros((counts.shape[0], 6), dtype=np.float32)
    for m in range(2):
        n = counts[:, m]
        ok = n > 0
        div = np.where(ok, n, 1)
        out[:, 3 * m] = np.where(ok, (ee_sums[:, m] / div).astype(np.float32), np.float32(0))
        for k in range(2):
            out[:, 3 * m + 1 + k] = np.where(ok, counts[:, 2 + 2 * m + k].astype(np.float32) / div.astype(np.float32), np.float32(0))
    return out


def compute_flow_metrics(pred, batch):
    """FlowModelInterface.compute_metrics: pred [1,T,2,H,W], batch["frame"] [1,T+1,...], batch["flow"], batch["events"] ->
    {"SOURCE/sequence/dense_EPE": [T floats], ...} for the six metrics.  One device-to-host copy."""
    _lib.require_gpu()
    frame = batch["frame"]
    if frame.dim() != 5 or frame.shape[0] != 1:
        raise ValueError("Batch size must be 1 for testing.")
    T = frame.shape[1] - 1
    prefix = _log_prefix(batch)
    counts, sums = flow_metrics(pred[:, :T], batch["flow"][:, :T], batch["events"][:, :T])
    host = torch.cat([counts, sums.view(torch.int64)], dim=1).cpu().numpy()
    ratios = flow_ratios(host[:, :6], np.ascontiguousarray(host[:, 6:]).view(np.float64))
    metrics = defaultdict(list)
    for k, name in enumerate(FLOW_METRICS):
        metrics[f"{prefix}/{name}"] = ratios[:, k].astype(np.float64).tolist()
    return metrics
