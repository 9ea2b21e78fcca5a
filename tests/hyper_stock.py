"""HyperE2VID restated in stock PyTorch (plain torch.nn.functional on a dict of tensors keyed like the reference's state_dict): the dynamic
decoder layer and the recurrent network.  Pinned to the reference's own outputs (golden G26) on the CPU by
tests/test_hyper.py::test_stock_restatement_equals_the_reference_on_cpu; on the GPU it is the float32 yardstick at sizes the fixture does
not cover and the speed baseline of tools/hyper_time.py.  Also the seeded inputs / weights those tests share."""
import os

import numpy as np

from hyper_weights import hyper_state

HERE = os.path.dirname(os.path.abspath(__file__))
KW = dict(num_bins=5, skip_type="sum", recurrent_block_type="convlstm", kernel_size=5, channel_multiplier=2, num_encoders=3,
          base_num_channels=32, num_residual_blocks=2, use_upsample_conv=True, norm="none", num_output_channels=1, use_dynamic_decoder=True)
LAYER = "unetrecurrent.decoders.0."


def g26():
    return np.load(os.path.join(HERE, "golden", "g26_hyper.npz"))


def _shapes(g, name):
    return {str(k): tuple(int(x) for x in str(s).split(",") if x) for k, s in zip(g[name + "__keys"], g[name + "__shapes"])}


def g26_state(g):
    """{reference key (`unetrecurrent.` prefix): ndarray} from G26's recipe."""
    return hyper_state(_shapes(g, "net"), int(g["net__seed"]), float(g["net__gain"]), g["bases"])


def g26_layer_state(g):
    """{key of one DynamicUpsampleLayer: ndarray} from G26's recipe."""
    return hyper_state(_shapes(g, "layer"), int(g["layer__seed"]), float(g["layer__gain"]), g["bases"], float(g["layer__coeff_scale"]))


def sparse_voxels(seed, *shape):
    """G18 / G25 / G26's input recipe: integers in -3..3, 60 % zeroed."""
    g = np.random.Generator(np.random.PCG64(int(seed)))
    vox = g.integers(-3, 4, size=shape).astype(np.float32)
    vox[g.random(vox.shape) < 0.6] = 0.0
    return vox


def _conv(x, p, name, stride=1):
    import torch.nn.functional as F
    w = p[name + ".weight"]
    return F.conv2d(x, w, p[name + ".bias"], stride=stride, padding=w.shape[-1] // 2)


def _bn(x, p, name):
    import torch.nn.functional as F
    return F.batch_norm(x, p[name + ".running_mean"], p[name + ".running_var"], p[name + ".weight"], p[name + ".bias"], False, 0.1, 1e-5)


def stock_context(ev, prev, p, pre=""):
    import torch
    import torch.nn.functional as F
    ctx = F.interpolate(torch.cat([ev, prev], 1), scale_factor=0.25, mode="bilinear", align_corners=False)
    return _conv(ctx, p, pre + "context_fusion.conv")


def stock_atoms(ctx, p, pre=""):
    """[B,6,25,h,w]: tanh(bn(conv(tanh(bn(conv(ctx)))))) as [B,6,12,h,w] coefficients times the [12,25] bases."""
    import torch
    net = pre + "dynamic_atom_generation.bases_net."
    c = torch.tanh(_bn(_conv(ctx, p, net + "0"), p, net + "1"))
    c = torch.tanh(_bn(_conv(c, p, net + "3"), p, net + "4"))
    n, _, h, w = c.shape
    return torch.einsum("bmkhw,kl->bmlhw", c.reshape(n, 6, 12, h, w), p[pre + "dynamic_atom_generation.bases"])


def stock_dynconv(x, atoms, p, pre="", unfold=False):
    """x [B,C,H,W], atoms [B,6,25,H,W] -> [B,128,H,W].  Default: one window tap at a time (float32 sums in tap order, no 25 x tensor).
    unfold=True: the stock formulation itself -- F.unfold, einsum, 1x1 convolution (model/hyper/hyper_dynamic.py:87-91) -- which is what
    tools/hyper_time.py times as the stock baseline."""
    import torch
    import torch.nn.functional as F
    n, c, h, w = x.shape
    if unfold:
        cols = F.unfold(x, kernel_size=5, padding=2).view(n, c, 25, h, w)
        feat = torch.einsum("bmlhw,bclhw->bcmhw", atoms.to(cols.dtype), cols).reshape(n, c * 6, h, w)
        return F.conv2d(feat, p[pre + "dynamic_conv.compositional_coefficients"], p[pre + "dynamic_conv.bias"])
    xp = F.pad(x, (2, 2, 2, 2))
    feat = x.new_zeros((n, c, 6, h, w))
    for l in range(25):
        dy, dx = divmod(l, 5)
        feat += xp[:, :, None, dy:dy + h, dx:dx + w] * atoms[:, None, :, l]
    return F.conv2d(feat.reshape(n, c * 6, h, w), p[pre + "dynamic_conv.compositional_coefficients"], p[pre + "dynamic_conv.bias"])


def stock_layer(x, ev, prev, p, pre="", unfold=False):
    """DynamicUpsampleLayer.forward (model/hyper_model.py:53-60) -> (context, atoms, output)."""
    import torch
    import torch.nn.functional as F
    ctx = stock_context(ev, prev, p, pre)
    atoms = stock_atoms(ctx, p, pre)
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    return ctx, atoms, torch.relu(stock_dynconv(up, atoms, p, pre, unfold))


def stock_step(ev, prev, states, p, unfold=False):
    """One HyperE2VID step: (image, new states).  states: list of (hidden, cell) or None per encoder."""
    import torch
    import torch.nn.functional as F
    u = "unetrecurrent."
    head = x = F.relu(_conv(ev, p, u + "head.conv2d"))
    kept, new_states = [], []
    for i in range(3):
        x = F.relu(_conv(x, p, u + f"encoders.{i}.conv.conv2d", stride=2))
        hp, cp = states[i] if states[i] is not None else (torch.zeros_like(x), torch.zeros_like(x))
        gi, gr, go, gc = _conv(torch.cat([x, hp], 1), p, u + f"encoders.{i}.recurrent_block.Gates").chunk(4, 1)
        cell = torch.sigmoid(gr) * cp + torch.sigmoid(gi) * torch.tanh(gc)
        x = torch.sigmoid(go) * torch.tanh(cell)
        kept.append(x)
        new_states.append((x, cell))
    for i in range(2):
        x = F.relu(_conv(F.relu(_conv(x, p, u + f"resblocks.{i}.conv1")), p, u + f"resblocks.{i}.conv2") + x)
    x = stock_layer(x + kept[2], ev, prev, p, LAYER, unfold)[2]
    for i in (1, 2):
        x = F.interpolate(x + kept[2 - i], scale_factor=2, mode="bilinear", align_corners=False)
        x = F.relu(_conv(x, p, u + f"decoders.{i}.conv2d"))
    return _conv(x + head, p, u + "pred.conv2d"), new_states


def stock_sequence(events, p, prev=None):
    """events [N,T,5,H,W] -> images [N,T,1,H,W]; prev_recs starts as zeros (or `prev`) and is each step's image."""
    import torch
    n, t = events.shape[:2]
    states = [None] * 3
    prev = torch.zeros((n, 1) + tuple(events.shape[-2:]), dtype=events.dtype, device=events.device) if prev is None else prev
    out = []
    for k in range(t):
        prev, states = stock_step(events[:, k], prev.to(events.dtype), states, p)
        out.append(prev)
    return torch.stack(out, 1)


def err(got, want):
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    return float(d.max()), float(np.sqrt((d ** 2).mean()))
