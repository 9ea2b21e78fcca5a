"""The weights and inputs of golden G30 (tests/golden/g30_lpips_vgg.npz), shared by its generator (tests/golden/make_golden_lpips.py, which
loads them into the REFERENCE's PNetLin) and by the tests (which load them into v2v_amd.lpips.LPIPSVGG and into tests/lpips_stock.py).

The VGG16 backbone (14.7 M parameters) is a recipe, not data: tests/seeded_weights.seeded_state over the 26 `net.*` keys in state-dict order,
seed 30, gain sqrt(6) (He-uniform: activations keep their scale through thirteen ReLU layers, so no tap dies).  The five linear layers and
the scaling layer's constants are data and live in the npz (1,479 floats)."""
import numpy as np

from seeded_weights import seeded_state

SEED, GAIN = 30, 6 ** 0.5
# (slice, index in torchvision's vgg16().features, Cin, Cout): PerceptualSimilarity/models/pretrained_networks.py:97-135
CONVS = ((1, 0, 3, 64), (1, 2, 64, 64), (2, 5, 64, 128), (2, 7, 128, 128), (3, 10, 128, 256), (3, 12, 256, 256), (3, 14, 256, 256),
         (4, 17, 256, 512), (4, 19, 512, 512), (4, 21, 512, 512), (5, 24, 512, 512), (5, 26, 512, 512), (5, 28, 512, 512))
CHANNELS = (64, 128, 256, 512, 512)
LIN_KEYS = tuple(f"lin{k}.model.1.weight" for k in range(5))
CASES = {"a": (2, 1, 32, 32), "b": (1, 3, 16, 64), "c": (3, 1, 48, 64), "close": (2, 1, 32, 32)}


def backbone_shapes():
    """Ordered {key: shape} of the 26 backbone tensors, in PNetLin's state-dict order."""
    shapes = {}
    for s, idx, cin, cout in CONVS:
        shapes[f"net.slice{s}.{idx}.weight"] = (cout, cin, 3, 3)
        shapes[f"net.slice{s}.{idx}.bias"] = (cout,)
    return shapes


def backbone_state():
    """{key: float32 ndarray} of the seeded backbone."""
    return seeded_state(backbone_shapes(), SEED, gain=GAIN)


def reference_keys():
    """The 33 keys of PNetLin(pnet_type='vgg', version='0.1'), in state-dict order."""
    return ["scaling_layer.shift", "scaling_layer.scale"] + list(backbone_shapes()) + list(LIN_KEYS)


def golden_state(g30):
    """The full 33-key state dict (torch tensors, float32) of the network G30 was made with."""
    import torch
    state = {"scaling_layer.shift": g30["shift"], "scaling_layer.scale": g30["scale"]}
    state.update(backbone_state())
    state.update({k: g30[k] for k in LIN_KEYS})
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()}


def case_inputs(name):
    """(pred, target) float32 in [0, 1): uniform from PCG64(sum(shape)), pred drawn first; `close`: pred = clip(target + 0.05 N(0,1), 0, 1)."""
    shape = CASES[name]
    g = np.random.Generator(np.random.PCG64(sum(shape)))
    pred = g.random(shape).astype(np.float32)
    target = g.random(shape).astype(np.float32)
    if name == "close":
        pred = np.clip(target + np.float32(0.05) * g.standard_normal(shape).astype(np.float32), 0.0, 1.0).astype(np.float32)
    return pred, target
