"""The cases and inputs of golden G35 (tests/golden/g35_lpips_alex_grad.npz), shared by its generator
(tests/golden/make_golden_lpips_alex_grad.py, which runs the REFERENCE's PNetLin with autograd) and by the tests.  The network is G34's:
the backbone recipe of tests/lpips_alex_weights.py and the lin / shift / scale values stored in g34_lpips_alex.npz.

The scalar that is differentiated is  sum_b c_b * dist_b  with c_b = 0.5 + 0.75 b, so a gradient that reads the wrong d dist shows.

J: the draw of every case.  A gradient can only be compared within a tolerance where no float32 rounding flips a ReLU gate or a pool's
arg-max; the generator asserts margins for both (its conditions ii and iii) and J holds, per case, the smallest draw that has them."""
import numpy as np

# (T, C, H, W)
CASES = {"a": (2, 1, 31, 31),        # the smallest: taps 7x7, 3x3, 1x1
         "b": (3, 1, 47, 63),        # odd sizes; both pools drop a row or a column
         "c": (1, 3, 40, 55),        # three channels
         "wide": (2, 1, 47, 143),    # stem output 11 x 35 crosses the forward's tiles in x and y; 170 pixels at the 5x5 layer cross a GEMM tile
         "t128": (1, 1, 128, 128),   # the training frame
         "close": (1, 1, 31, 47)}    # pred = clip(target + 0.05 N(0,1), 0, 1): small differences
CLOSE = ("close",)
STORED = ("a", "b", "c", "wide", "close")   # inputs in the npz; t128's are recipe only (with them the file would pass its 640 KiB bound)
J = {"a": 0, "b": 1, "c": 0, "wide": 20, "t128": 0, "close": 1}
MARGIN = 8                            # conditions (ii) and (iii): margins of 8 x the float32 run's error


def coefficients(T):
    """c_b = 0.5 + 0.75 b, float64 [T]"""
    return 0.5 + 0.75 * np.arange(T, dtype=np.float64)


def case_inputs(name, j=None):
    """(pred, target) float32 in [0, 1]: uniform from PCG64(35 + sum(shape) + 1000 j), pred drawn first, then target; the `close` case:
    pred = clip(target + 0.05 N(0,1), 0, 1), as in G34."""
    shape = CASES[name]
    j = J[name] if j is None else j
    g = np.random.Generator(np.random.PCG64(35 + sum(shape) + 1000 * j))
    pred = g.random(shape).astype(np.float32)
    target = g.random(shape).astype(np.float32)
    if name in CLOSE:
        pred = np.clip(target + np.float32(0.05) * g.standard_normal(shape).astype(np.float32), 0.0, 1.0).astype(np.float32)
    return pred, target
