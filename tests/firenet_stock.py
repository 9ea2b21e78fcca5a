"""FireNet (model/model.py:264-311) restated in stock PyTorch -- plain torch.nn.functional on a dict of tensors keyed like the reference's
state_dict: head ConvLayer(num_bins -> 16, 3x3, relu), G1 = ConvGRU, R1 = ResidualBlock, G2, R2, pred 1x1, all at full resolution.  The
float32 yardstick of the FireNet GPU tests where golden G28 does not reach, pinned to the reference's own outputs (G28) on the CPU by
tests/test_firenet.py::test_stock_restatement_equals_the_reference_on_cpu.  Also the seeded inputs / weights those tests share."""
import os

import numpy as np

from convgru_stock import _conv, err, sparse_voxels, stock_gru  # noqa: F401
from seeded_weights import seeded_state

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = ("a", "b")                       # G28's two inputs: 4 steps of [2, 5, 32, 48]; 2 steps of the odd-sized [1, 5, 19, 37]
SHAPES = {"a": (4, 2, 5, 32, 48), "b": (2, 1, 5, 19, 37)}


def g28():
    return np.load(os.path.join(HERE, "golden", "g28_firenet.npz"))


def g28_state(g):
    """{reference key: float32 ndarray} of the network from G28's recipe."""
    shapes = {str(k): tuple(int(x) for x in str(s).split(",")) for k, s in zip(g["net__keys"], g["net__shapes"])}
    return seeded_state(shapes, int(g["net__seed"]), float(g["net__gain"]))


def g28_vox(g, name):
    return sparse_voxels(int(g["net__vox_seed"]) + INPUTS.index(name), *SHAPES[name])


def stock_resblock(x, p, name):
    import torch.nn.functional as F
    return F.relu(_conv(F.relu(_conv(x, p, name + ".conv1")), p, name + ".conv2") + x)


class StockFireNet:
    """Call it per time step; `states` = [G1's, G2's] as the reference keeps them."""

    def __init__(self, p):
        self.p = p
        self.states = [None, None]

    def reset_states(self):
        self.states = [None, None]

    def __call__(self, x):
        import torch.nn.functional as F
        p = self.p
        x = F.relu(_conv(x, p, "head.conv2d"))
        x = self.states[0] = stock_gru(x, self.states[0], p, "G1")
        x = stock_resblock(x, p, "R1")
        x = self.states[1] = stock_gru(x, self.states[1], p, "G2")
        x = stock_resblock(x, p, "R2")
        return {"image": _conv(x, p, "pred.conv2d")}
