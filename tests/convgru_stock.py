"""ConvGRU and the recurrent flow network UNetFlow / FlowNet (model/submodules.py:238-278, model/unet.py:133-194, model/model.py:111-139)
restated in stock PyTorch -- plain torch.nn.functional on a dict of tensors keyed like the reference's state_dict: the float32 yardstick of
the ConvGRU / FlowNet GPU tests where golden G27 does not reach, pinned to the reference's own outputs (G27) on the CPU by
tests/test_flownet.py::test_stock_restatement_equals_the_reference_on_cpu.  Also the seeded inputs / weights those tests share."""
import os

import numpy as np

from seeded_weights import seeded_state

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCKS = ("convlstm", "convgru")


def kwargs(block, **more):
    """unet_kwargs of config/test_e2vid++_original.yaml:24-33 with the recurrent block type chosen."""
    kw = dict(num_bins=5, skip_type="sum", recurrent_block_type=block, num_encoders=3, base_num_channels=32, num_residual_blocks=2,
              use_upsample_conv=True, norm="none", num_output_channels=3)
    kw.update(more)
    return kw


def g27():
    return np.load(os.path.join(HERE, "golden", "g27_flownet_convgru.npz"))


def g27_state(g, block):
    """{reference key (with the `unetflow.` prefix): float32 ndarray} of the `block` network from G27's recipe."""
    shapes = {str(k): tuple(int(x) for x in str(s).split(",")) for k, s in zip(g[f"{block}__keys"], g[f"{block}__shapes"])}
    return seeded_state(shapes, int(g["net__seed"]), float(g["net__gain"]))


def sparse_voxels(seed, *shape):
    """G18 / G25 / G27's input recipe: integers in -3..3, 60 % zeroed."""
    g = np.random.Generator(np.random.PCG64(int(seed)))
    vox = g.integers(-3, 4, size=shape).astype(np.float32)
    vox[g.random(vox.shape) < 0.6] = 0.0
    return vox


def _conv(x, p, name, stride=1):
    import torch.nn.functional as F
    w = p[name + ".weight"]
    return F.conv2d(x, w, p[name + ".bias"], stride=stride, padding=w.shape[-1] // 2)


def stock_gru(x, h, p, name):
    """One ConvGRU step: update / reset gates from cat(x, h), the candidate from cat(x, h * reset), h' = h (1 - u) + o u; h None = zeros."""
    import torch
    if h is None:
        h = torch.zeros_like(x)
    xh = torch.cat([x, h], dim=1)
    u = torch.sigmoid(_conv(xh, p, name + ".update_gate"))
    r = torch.sigmoid(_conv(xh, p, name + ".reset_gate"))
    o = torch.tanh(_conv(torch.cat([x, h * r], dim=1), p, name + ".out_gate"))
    return h * (1 - u) + o * u


def stock_lstm(x, state, p, name):
    """One ConvLSTM step: (hidden, cell) from the four gates in / remember / out / cell of one convolution over cat(x, hidden)."""
    import torch
    h, c = state if state is not None else (torch.zeros_like(x), torch.zeros_like(x))
    i, r, o, g = _conv(torch.cat([x, h], dim=1), p, name + ".Gates").chunk(4, 1)
    c = torch.sigmoid(r) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


class StockRecurrentUNet:
    """The recurrent UNet with sum skips on parameters `p` under `prefix` ('unetflow.' / 'unetrecurrent.'): a 5x5 head, stride-2 5x5
    encoders each followed by its recurrent block, residual blocks, decoders relu(conv5x5(bilinear_x2(x + encoder output of that level))),
    a 1x1 prediction of (x + head) without activation.  Call it per time step; `states` as the reference keeps them."""

    def __init__(self, p, prefix, block, num_encoders=3, num_residual_blocks=2):
        self.p, self.prefix, self.block, self.ne, self.nr = p, prefix, block, num_encoders, num_residual_blocks
        self.states = [None] * num_encoders

    def reset_states(self):
        self.states = [None] * self.ne

    def __call__(self, x):
        import torch.nn.functional as F
        p, pre = self.p, self.prefix
        x = head = F.relu(_conv(x, p, pre + "head.conv2d"))
        kept = []
        for i in range(self.ne):
            x = F.relu(_conv(x, p, f"{pre}encoders.{i}.conv.conv2d", stride=2))
            if self.block == "convlstm":
                self.states[i] = stock_lstm(x, self.states[i], p, f"{pre}encoders.{i}.recurrent_block")
                x = self.states[i][0]
            else:
                x = self.states[i] = stock_gru(x, self.states[i], p, f"{pre}encoders.{i}.recurrent_block")
            kept.append(x)
        for i in range(self.nr):
            x = F.relu(_conv(F.relu(_conv(x, p, f"{pre}resblocks.{i}.conv1")), p, f"{pre}resblocks.{i}.conv2") + x)
        for i in range(self.ne):
            x = F.interpolate(x + kept[self.ne - 1 - i], scale_factor=2, mode="bilinear", align_corners=False)
            x = F.relu(_conv(x, p, f"{pre}decoders.{i}.conv2d"))
        return _conv(x + head, p, pre + "pred.conv2d")


class StockFlowNet(StockRecurrentUNet):
    """FlowNet: the network above at prediction width 3 under `unetflow.`, returning {'image': [:, 0:1], 'flow': [:, 1:3]}."""

    def __init__(self, p, block):
        super().__init__(p, "unetflow.", block)

    def __call__(self, x):
        y = super().__call__(x)
        return {"image": y[:, 0:1], "flow": y[:, 1:3]}


def err(got, want):
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    return float(d.max()), float(np.sqrt((d ** 2).mean()))
