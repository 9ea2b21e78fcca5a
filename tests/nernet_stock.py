"""Stock-torch restatement of NER-Net's learned voxelisation (the reference's model/nernet/representation_modules.py: ValueLayer :12-54,
QuantizationLayer_trail :175-261, QuantizationLayer_trail_combined :91-172) for machines without the reference: the same torch operations
in the same order, so on the CPU it reproduces golden G32 bit for bit (tests/test_nernet_golden.py holds it there).  It is the yardstick of
the GPU tests and the baseline of tools/nernet_voxel_time.py -- never the code under test.

One difference, on purpose: the reference normalises t in place through views of its argument; this works on a copy and can hand the
normalised t back.  A batch id without rows is skipped (the reference raises IndexError there).

`truth64` evaluates the same layer in float64 from the float32 t_n and the float32 parameters -- the "truth" of G32 (the reference casts to
float32 itself, so .double() on it would prove nothing)."""
import numpy as np
import torch
from torch import nn


class StockValueLayer(nn.Module):
    def __init__(self, mlp_layers, activation):
        super().__init__()
        self.mlp = nn.ModuleList(nn.Linear(i, o) for i, o in zip(mlp_layers[:-1], mlp_layers[1:]))
        self.activation = activation

    def forward(self, x):
        x = x[None, ..., None]
        for lin in self.mlp[:-1]:
            x = self.activation(lin(x))
        return self.mlp[-1](x).squeeze()


def normalise_t(events, B, C, normalize):
    """The per-batch time normalisation, in the rows' dtype; returns a new [n] tensor."""
    t = events[:, 2].clone()
    b = events[:, 4]
    for bi in range(B):
        m = b == bi
        if not bool(m.any()):
            continue
        if normalize:
            t[m] = t[m] - t[m][0]
            if t[m].max() == 0:
                continue
            t[m] /= t[m].max()
        else:
            dt = t[m][-1] - t[m][0]
            if dt == 0:
                continue
            t[m] = (t[m] - t[m][0]) / dt * (C - 1)
    return t


def base_index(events, dim, combined):
    C, H, W = dim
    x, y, p, b = events[:, 0], events[:, 1], events[:, 3], events[:, 4]
    if combined:
        return x + W * y + 0 + W * H * C * b
    p = (p + 1) / 2
    return x + W * y + 0 + W * H * C * p + W * H * C * 2 * b


def bin_shift(i_bin, C, normalize):
    return i_bin / (C - 1) if normalize else i_bin


def stock_voxel(events, value_layer, dim, normalize=False, combined=False, batch_size=None, return_t=False):
    """events [n, 5] -> float32 [B, 2C, H, W] (combined: [B, C, H, W], in the rows' dtype)."""
    C, H, W = dim
    B = int((1 + events[-1, -1]).item()) if batch_size is None else int(batch_size)
    numel = int((1 if combined else 2) * np.prod(dim) * B)
    t = normalise_t(events, B, C, normalize)
    t_n = t.float()
    if combined:
        vox = events.new_zeros(numel)
        fac = events[:, 3] * t
    else:
        vox = events.new_zeros(numel, dtype=torch.float)
        fac = t_n
    idx0 = base_index(events, dim, combined)
    for i_bin in range(C):
        values = fac * value_layer(fac - bin_shift(i_bin, C, normalize))
        idx = torch.clamp((idx0 + W * H * i_bin).long(), max=numel - 1)
        vox.put_(idx, values, accumulate=True)
    if combined:
        vox = vox.view(-1, C, H, W)
    else:
        vox = vox.view(-1, 2, C, H, W)
        vox = torch.cat([vox[:, 1], vox[:, 0]], 1)
    return (vox, t_n) if return_t else vox


class StockQuantization(nn.Module):
    """Constructor of the reference's quantisation layers plus `combined`; state_dict keys `value_layer.mlp.{i}.{weight,bias}`."""

    def __init__(self, dim, mlp_layers=(1, 100, 100, 1), activation=None, normalize=False, combined=False):
        super().__init__()
        self.value_layer = StockValueLayer(list(mlp_layers), activation if activation is not None else nn.LeakyReLU(negative_slope=0.1))
        self.dim, self.normalize, self.combined = tuple(dim), normalize, combined

    def forward(self, events, batch_size=None, return_t=False):
        return stock_voxel(events, self.value_layer, self.dim, self.normalize, self.combined, batch_size, return_t)


def truth64(events, t_n, weights, biases, dim, slope, normalize=False, combined=False, batch_size=None, drop_below=False, reduce="sum"):
    """float64 evaluation from the float32 t_n and float32 parameters: exact products and sums to ~1e-16, indices as the layer forms them.
    Returns float64 [B, 2C, H, W] (combined: [B, C, H, W]).  drop_below: drop the terms whose index lies below -numel (where put_ raises).
    reduce: "sum" the terms, or per cell the sum of their magnitudes ("abs") / their number ("count") -- what a summation bound needs."""
    C, H, W = dim
    B = int((1 + events[-1, -1]).item()) if batch_size is None else int(batch_size)
    numel = int((1 if combined else 2) * np.prod(dim) * B)
    tn = t_n.double()
    fac = events[:, 3].float().double() * tn if combined else tn
    vox = torch.zeros(numel, dtype=torch.float64)
    idx0 = base_index(events, dim, combined)
    for i_bin in range(C):
        shift = torch.tensor(bin_shift(i_bin, C, normalize), dtype=torch.float32).double()      # the scalar as float32 arithmetic sees it
        h = (fac - shift)[:, None]
        for i, (w, b) in enumerate(zip(weights, biases)):
            h = h @ w.double().t() + b.double()
            if i < len(weights) - 1:
                h = torch.where(h > 0, h, h * float(np.float32(slope)))
        values = fac * h[:, 0]
        if reduce != "sum":
            values = values.abs() if reduce == "abs" else torch.ones_like(values)
        idx = torch.clamp((idx0 + W * H * i_bin).long(), max=numel - 1)
        if drop_below:
            keep = idx >= -numel
            idx, values = idx[keep], values[keep]
        vox.put_(idx, values, accumulate=True)
    if combined:
        return vox.view(-1, C, H, W)
    vox = vox.view(-1, 2, C, H, W)
    return torch.cat([vox[:, 1], vox[:, 0]], 1)
