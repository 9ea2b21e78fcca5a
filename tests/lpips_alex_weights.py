"""The weights and inputs of golden G34 (tests/golden/g34_lpips_alex.npz), shared by its generator (tests/golden/make_golden_lpips_alex.py,
which loads them into the REFERENCE's PNetLin) and by the tests (which load them into v2v_amd.lpips_alex.LPIPSAlex and into
tests/lpips_alex_stock.py).

The AlexNet backbone (2.5 M parameters) is a recipe, not data: tests/seeded_weights.seeded_state over the ten `net.*` keys in state-dict
order, seed 34, gain sqrt(6) (He-uniform: activations keep their scale through five ReLU layers, so no tap dies).  The five linear layers
and the scaling layer's constants are data and live in the npz (1,158 floats)."""
import numpy as np

from seeded_weights import seeded_state

SEED, GAIN = 34, 6 ** 0.5
# (slice, index in torchvision's alexnet().features, Cin, Cout, kernel): PerceptualSimilarity/models/pretrained_networks.py:57-95
CONVS = ((1, 0, 3, 64, 11), (2, 3, 64, 192, 5), (3, 6, 192, 384, 3), (4, 8, 384, 256, 3), (5, 10, 256, 256, 3))
CHANNELS = (64, 192, 384, 256, 256)
LIN_KEYS = tuple(f"lin{k}.model.1.weight" for k in range(5))
# (T, C, H, W)
CASES = {"a": (2, 1, 31, 31), "b": (3, 1, 47, 63), "c": (1, 3, 64, 95), "close": (2, 1, 47, 63), "r180": (1, 1, 180, 240), "r260": (1, 1, 260, 346)}
CLOSE = ("close", "r180", "r260")          # pred = clip(target + 0.05 N(0,1), 0, 1)
STORED = ("a", "b", "c", "close")          # inputs in the npz; r180 and r260 are recipe only


def backbone_shapes():
    """Ordered {key: shape} of the ten backbone tensors, in PNetLin's state-dict order."""
    shapes = {}
    for s, idx, cin, cout, ks in CONVS:
        shapes[f"net.slice{s}.{idx}.weight"] = (cout, cin, ks, ks)
        shapes[f"net.slice{s}.{idx}.bias"] = (cout,)
    return shapes


def backbone_state():
    """{key: float32 ndarray} of the seeded backbone."""
    return seeded_state(backbone_shapes(), SEED, gain=GAIN)


def reference_keys():
    """The 17 keys of PNetLin(pnet_type='alex', version='0.1'), in state-dict order."""
    return ["scaling_layer.shift", "scaling_layer.scale"] + list(backbone_shapes()) + list(LIN_KEYS)


def golden_state(g34):
    """The full 17-key state dict (torch tensors, float32) of the network G34 was made with."""
    import torch
    state = {"scaling_layer.shift": g34["shift"], "scaling_layer.scale": g34["scale"]}
    state.update(backbone_state())
    state.update({k: g34[k] for k in LIN_KEYS})
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()}


def case_inputs(name):
    """(pred, target) float32 in [0, 1]: uniform from PCG64(sum(shape)), pred drawn first; the `close`-style cases:
    pred = clip(target + 0.05 N(0,1), 0, 1)."""
    shape = CASES[name]
    g = np.random.Generator(np.random.PCG64(sum(shape)))
    pred = g.random(shape).astype(np.float32)
    target = g.random(shape).astype(np.float32)
    if name in CLOSE:
        pred = np.clip(target + np.float32(0.05) * g.standard_normal(shape).astype(np.float32), 0.0, 1.0).astype(np.float32)
    return pred, target


def tap_sizes(h, w):
    """The five (H, W) of the taps: 11x11 / 4 / pad 2, then a 3x3 / 2 pool before the second and the third convolution."""
    s1 = ((h - 7) // 4 + 1, (w - 7) // 4 + 1)
    s2 = ((s1[0] - 3) // 2 + 1, (s1[1] - 3) // 2 + 1)
    s3 = ((s2[0] - 3) // 2 + 1, (s2[1] - 3) // 2 + 1)
    return (s1, s2, s3, s3, s3)
