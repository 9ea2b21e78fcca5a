"""Seeded inputs of the image-loss tests, shared by tests/golden/make_golden_tc_loss.py and the tests (float32 numpy arrays).

    pair_inputs(name)      G29's pair cases: frames in [0.3, 0.7], processed images in [-0.2, 1.2] (the clamp at 0 acts), flows within +-3 px
                           (samples leave the frame)
    seq_inputs()           G29's sequence case [2,4,1,24,40], L0 = 2
    integer_cases(shape)   inputs on which the warp and its adjoint are exact in float32 (H-1, W-1 powers of two, flows multiples of 1/4 px,
                           small integer images): name -> (img, flow)
"""
import numpy as np

SEED = 7
PAIR_SHAPES = {"a": (2, 1, 20, 28), "b": (1, 3, 13, 19)}      # b: 247 pixels, no multiple of 4 or 64
SEQ_SHAPE, SEQ_L0 = (2, 4, 1, 24, 40), 2
KEYS = ("image0", "image1", "processed0", "processed1", "flow01")


def _fields(g, shape):
    n, c, h, w = shape
    u = lambda lo, hi, s: g.uniform(lo, hi, s).astype(np.float32)   # noqa: E731
    return dict(image0=u(0.3, 0.7, shape), image1=u(0.3, 0.7, shape), processed0=u(-0.2, 1.2, shape), processed1=u(-0.2, 1.2, shape),
                flow01=u(-3.0, 3.0, (n, 2, h, w)))


def pair_inputs(name):
    return _fields(np.random.default_rng(SEED + sorted(PAIR_SHAPES).index(name)), PAIR_SHAPES[name])


def seq_inputs():
    b, t, c, h, w = SEQ_SHAPE
    g = np.random.default_rng(SEED + 10)
    u = lambda lo, hi, s: g.uniform(lo, hi, s).astype(np.float32)   # noqa: E731
    return dict(pred=u(-0.2, 1.2, SEQ_SHAPE), frame=u(0.3, 0.7, SEQ_SHAPE), flow=u(-3.0, 3.0, (b, t, 2, h, w)))


def integer_cases(shape, seed=11):
    n, c, h, w = shape
    assert (h - 1) & (h - 2) == 0 and (w - 1) & (w - 2) == 0, "H-1 and W-1 must be powers of two"
    g = np.random.default_rng(seed)
    img = g.integers(-7, 8, shape).astype(np.float32)
    quarter = lambda lo, hi: (g.integers(4 * lo, 4 * hi + 1, (n, 2, h, w)) / 4.0).astype(np.float32)   # noqa: E731
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    one = np.zeros((n, 2, h, w), np.float32)                        # every pixel samples source pixel ((W-1)/2, 1): one accumulator takes it all
    one[:, 0], one[:, 1] = (w - 1) // 2 - xs, 1 - ys
    cases = {"zero": np.zeros((n, 2, h, w), np.float32), "beyond": np.full((n, 2, h, w), float(2 * max(h, w)), np.float32),
             "quarters": quarter(-3, 3), "all_to_one": one}
    for k, (axis, sign) in enumerate(((0, -1), (0, 1), (1, -1), (1, 1))):   # out through the left, right, top, bottom border
        f = quarter(-1, 1)
        f[:, axis] = sign * np.abs(quarter(0, 3)[:, axis]) + sign * 0.25
        cases[("left", "right", "top", "bottom")[k]] = f
    return img, cases
