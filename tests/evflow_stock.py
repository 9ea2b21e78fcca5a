"""The flow network EVFlowNet restated in stock PyTorch (plain torch.nn.functional on a dict of tensors keyed like the reference's
state_dict): the float32 yardstick of the EVFlowNet GPU tests, pinned to the reference's own outputs (golden G25) on the CPU by
tests/test_evflow.py::test_stock_restatement_equals_the_reference_on_cpu.  Also the seeded inputs / weights those tests share."""
import os

import numpy as np

from seeded_weights import seeded_state

HERE = os.path.dirname(os.path.abspath(__file__))
KW = dict(num_bins=5, base_num_channels=32, num_encoders=4, num_residual_blocks=2, num_output_channels=2, skip_type="concat", norm=None,
          use_upsample_conv=True, kernel_size=3, channel_multiplier=2)


def g25():
    return np.load(os.path.join(HERE, "golden", "g25_evflow.npz"))


def g25_state(g):
    """{reference key (with the `unet.` prefix): float32 ndarray} from G25's recipe."""
    shapes = {str(k): tuple(int(x) for x in str(s).split(",")) for k, s in zip(g["evflow__keys"], g["evflow__shapes"])}
    return seeded_state(shapes, int(g["evflow__seed"]), float(g["evflow__gain"]))


def sparse_voxels(seed, *shape):
    """G18 / G25's input recipe: integers in -3..3, 60 % zeroed."""
    g = np.random.Generator(np.random.PCG64(int(seed)))
    vox = g.integers(-3, 4, size=shape).astype(np.float32)
    vox[g.random(vox.shape) < 0.6] = 0.0
    return vox


def _conv(x, p, name, stride=1):
    import torch.nn.functional as F
    w = p[name + ".weight"]
    return F.conv2d(x, w, p[name + ".bias"], stride=stride, padding=w.shape[-1] // 2)


def stock_flow(x, p):
    """Four stride-2 3x3 encoders with ReLU (the first reads the voxel bins), two residual blocks relu(conv2(relu(conv1(x))) + x) at 512
    channels, four decoders relu(conv3x3(bilinear_x2(cat(x, encoder output of the same level)))), a 1x1 prediction without activation."""
    import torch
    import torch.nn.functional as F
    kept = []
    for i in range(4):
        x = F.relu(_conv(x, p, f"unet.encoders.{i}.conv2d", stride=2))
        kept.append(x)
    for i in range(2):
        x = F.relu(_conv(F.relu(_conv(x, p, f"unet.resblocks.{i}.conv1")), p, f"unet.resblocks.{i}.conv2") + x)
    for i in range(4):
        x = F.interpolate(torch.cat([x, kept[3 - i]], dim=1), scale_factor=2, mode="bilinear", align_corners=False)
        x = F.relu(_conv(x, p, f"unet.decoders.{i}.conv2d"))
    return _conv(x, p, "unet.pred.conv2d")


def err(got, want):
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    return float(d.max()), float(np.sqrt((d ** 2).mean()))
