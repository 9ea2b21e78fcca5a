"""Restatements of the reference's evaluation metrics for the tests of v2v_amd/metrics.py, and the seeded inputs they share with golden G33
(tests/golden/make_golden_metrics.py).

    ssim_direct64 / mse64       what the kernels compute, operation for operation: direct 49-tap window sums (row-major) and the formula of
                                DESIGN 4.18 in float64; the float32 difference squared and added in float64
    ssim_skimage                skimage.metrics.structural_similarity's published algorithm (defaults, one channel) on
                                scipy.ndimage.uniform_filter, in the dtype it is given: float64 is G33's truth, float32 is what current
                                skimage computes for float32 frames
    flow_terms / flow_ratios    FlowModelInterface.compute_metrics (model/train_flow_utils.py:229-294) restated: masks, EE, counts, the float64
                                sums of the float32 EE; the six float32 ratios as the reference forms them
    image_case / flow_case      the seeded inputs
"""
import hashlib

import numpy as np
import torch

WIN = 7
K1, K2 = 0.01, 0.03
FLOW_NAMES = ("dense_EPE", "dense_1PE", "dense_3PE", "sparse_EPE", "sparse_1PE", "sparse_3PE")

# name: (T, H, W, seed); the first four are stored in G33 with their S maps, the last two only as scalars
IMAGE_CASES = {"i7x7": (3, 7, 7, 11), "i8x9": (3, 8, 9, 12), "i23x70": (3, 23, 70, 13), "i45x31": (3, 45, 31, 14),
               "i180x240": (2, 180, 240, 15), "i260x346": (1, 260, 346, 16)}
SMALL_IMAGE_CASES = ("i7x7", "i8x9", "i23x70", "i45x31")
DATA_RANGES = (2.0, 1.0)

# name: (T, C, H, W, seed, integer-exact)
FLOW_CASES = {"f13x17": (5, 5, 13, 17, 21, False), "f50x47": (5, 3, 50, 47, 22, False), "fexact41x53": (5, 2, 41, 53, 23, True),
              "f180x240": (2, 5, 180, 240, 24, False)}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def image_case(name):
    """-> pred, image float32 [T,H,W] in 0..255 (the reference divides by 255 first)"""
    T, H, W, seed = IMAGE_CASES[name]
    rng = np.random.default_rng(seed)
    image = (rng.random((T, H, W), dtype=np.float32) * np.float32(255.0)).astype(np.float32)
    noise = rng.standard_normal((T, H, W), dtype=np.float32) * np.float32(25.0)
    pred = np.clip(image + noise, np.float32(0.0), np.float32(255.0)).astype(np.float32)
    return pred, image


def flow_case(name):
    """-> pred [T,2,H,W], gt [T,2,H,W], events [T,C,H,W] float32.  Frame 0 is general (NaN, +0 and -0 in gt, sparse events), frame 1 has no
    valid pixel, frame 2 events everywhere, frame 3 events nowhere, later frames are general again.  The integer-exact case has
    Pythagorean differences, so every EE is an integer and every sum exact."""
    T, C, H, W, seed, exact = FLOW_CASES[name]
    rng = np.random.default_rng(seed)
    if exact:
        gt = rng.integers(-6, 7, (T, 2, H, W)).astype(np.float32)
    else:
        gt = (rng.standard_normal((T, 2, H, W), dtype=np.float32) * np.float32(2.0)).astype(np.float32)
    u = rng.random((T, H, W))
    gt[:, 0][u < 0.05] = np.nan
    gt[:, 1][(u >= 0.05) & (u < 0.10)] = np.nan
    both = (u >= 0.10) & (u < 0.25)
    gt[:, 0][both] = 0.0
    gt[:, 1][both] = 0.0
    gt[:, 0][(u >= 0.10) & (u < 0.15)] = -0.0
    gt[:, 1][(u >= 0.12) & (u < 0.20)] = -0.0
    gt[:, 0][(u >= 0.25) & (u < 0.30)] = 0.0                                                # one zero component alone stays valid
    if T > 1:
        v = rng.random((H, W))
        gt[1, 0] = np.where(v < 0.3, np.nan, np.where(v < 0.6, -0.0, 0.0))
        gt[1, 1] = np.where(v < 0.3, 1.0, np.where(v < 0.8, 0.0, -0.0))
    base = np.nan_to_num(gt, nan=0.5)
    if exact:
        legs = np.array([[0, 0], [0, 1], [3, 4], [4, 3], [0, 2], [6, 8], [5, 12], [0, 3], [1, 0], [8, 15]], dtype=np.float32)
        pick = legs[rng.integers(0, len(legs), (T, H, W))]                                  # [T,H,W,2]
        sign = rng.integers(0, 2, (T, H, W, 2)).astype(np.float32) * 2 - 1
        pred = base + np.moveaxis(pick * sign, -1, 1)
    else:
        pred = (base + rng.standard_normal((T, 2, H, W), dtype=np.float32) * np.float32(1.5)).astype(np.float32)
        ee = np.sqrt(((pred.astype(np.float64) - base) ** 2).sum(axis=1))                  # keep every EE away from the thresholds 1 and 3
        near = (np.abs(ee - 1.0) < 1e-2) | (np.abs(ee - 3.0) < 1e-2)
        pred[:, 0][near] += np.float32(0.25) * np.sign(pred[:, 0] - base[:, 0])[near] + np.float32(0.125)
    events = rng.integers(-3, 4, (T, C, H, W)).astype(np.float32) * (rng.random((T, 1, H, W)) < 0.4)
    events = events.astype(np.float32)
    if T > 2:
        events[2] = np.float32(1.0)
        events[2, 0, ::2] = np.float32(-2.0)
    if T > 3:
        events[3] = np.float32(0.0)
        events[3, C - 1, 1::2] = np.float32(-0.0)
    return pred.astype(np.float32), gt.astype(np.float32), events


# ---- images -------------------------------------------------------------------------------------------------------------------------------
def scaled(x, divisor):
    """float32 true division, as the reference's `/ 255`"""
    x = np.asarray(x, dtype=np.float32)
    return x if divisor == 1.0 else (x / np.float32(divisor)).astype(np.float32)


def ssim_direct64(x, y, data_range):
    """x, y float32 [H,W] (already divided) -> S float64 [H-6, W-6], every operation in the kernels' order"""
    x, y = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(y, dtype=np.float32).astype(np.float64)
    H, W = x.shape
    h, w = H - (WIN - 1), W - (WIN - 1)
    s_x, s_y, s_xx, s_yy, s_xy = (np.zeros((h, w)) for _ in range(5))
    for dy in range(WIN):
        for dx in range(WIN):
            a, b = x[dy:dy + h, dx:dx + w], y[dy:dy + h, dx:dx + w]
            s_x = s_x + a
            s_y = s_y + b
            s_xx = s_xx + a * a
            s_yy = s_yy + b * b
            s_xy = s_xy + a * b
    NP = float(WIN * WIN)
    ux, uy, uxx, uyy, uxy = s_x / NP, s_y / NP, s_xx / NP, s_yy / NP, s_xy / NP
    cov = NP / (NP - 1.0)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    C1, C2 = (K1 * data_range) * (K1 * data_range), (K2 * data_range) * (K2 * data_range)
    A1, A2 = 2.0 * ux * uy + C1, 2.0 * vxy + C2
    B1, B2 = ux * ux + uy * uy + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def mse64(x, y):
    """the float32 difference, squared and added in float64"""
    d = (np.asarray(x, dtype=np.float32) - np.asarray(y, dtype=np.float32)).astype(np.float64)
    return float((d * d).sum() / d.size)


def ssim_skimage(x, y, data_range, dtype=np.float64):
    """-> (mean, S cropped by 3): skimage's algorithm for a single channel with its defaults, computed in `dtype`"""
    from scipy.ndimage import uniform_filter
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    NP = WIN * WIN
    cov_norm = NP / (NP - 1)
    ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
    uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    pad = (WIN - 1) // 2
    S = S[pad:S.shape[0] - pad, pad:S.shape[1] - pad]
    return float(S.mean(dtype=np.float64)), S


# ---- flow ---------------------------------------------------------------------------------------------------------------------------------
def flow_terms(pred, gt, events):
    """one frame: pred, gt [2,H,W], events [C,H,W] float32 tensors -> counts int64 [6] (n_dense, n_sparse, dense >1, dense >3, sparse >1,
    sparse >3), sums float64 [2] of the correctly rounded float32 EE under each mask, and EE"""
    valid = torch.logical_not(torch.isnan(gt[0]) | torch.isnan(gt[1]) | torch.logical_and(gt[0] == 0, gt[1] == 0))
    sparse = valid & (torch.abs(events).sum(axis=0) > 0)
    # the correctly rounded float32 root (the float64 root of a float32 number, rounded once more, is that): what sqrtf gives on the device.
    # torch's vectorised CPU sqrt is off by an ulp on a few values in a hundred, so `** 0.5` on the CPU is not used for the sums.
    EE = torch.from_numpy(np.sqrt(((pred - gt) ** 2).sum(axis=0).numpy().astype(np.float64)).astype(np.float32))
    counts, sums = [int(valid.sum()), int(sparse.sum())], []
    for m in (valid, sparse):
        e = torch.where(m, EE, torch.zeros_like(EE))
        counts += [int((e > 1).sum()), int((e > 3).sum())]
        sums.append(float(e.double().sum()))
    return np.array(counts, dtype=np.int64), np.array(sums), EE


def flow_ratios(pred, gt, events):
    """one frame -> the six values of the reference, formed as it forms them in float32 (0 where the count is 0)"""
    valid = torch.logical_not(torch.isnan(gt[0]) | torch.isnan(gt[1]) | torch.logical_and(gt[0] == 0, gt[1] == 0))
    sparse = valid & (torch.abs(events).sum(axis=0) > 0)
    EE = ((pred - gt) ** 2).sum(axis=0) ** 0.5
    out = []
    for m in (valid, sparse):
        n = torch.sum(m).item()
        e = torch.where(m, EE, torch.zeros_like(EE))
        if n > 0:
            out += [(torch.sum(e) / n).item(), (torch.sum((e > 1).float()) / n).item(), (torch.sum((e > 3).float()) / n).item()]
        else:
            out += [0, 0, 0]
    return out
