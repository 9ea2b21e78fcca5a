"""HyperE2VID's TRAINING mode restated in stock PyTorch: tests/hyper_stock.py with BatchNorm on the batch's statistics
(F.batch_norm(..., training=True), which also updates the running statistics held in the parameter dict) -- differentiable, any dtype.
Pinned to the reference's own training-mode layer (golden G31) in float64 on the CPU by tests/test_hyper_train_reference.py; on the GPU it
is the float32 yardstick, the bf16-autocast yardstick (the `unfold=True` formulation) and the speed baseline of tools/hyper_train_time.py."""
import os

import numpy as np

from hyper_stock import KW, LAYER, _conv, _shapes, stock_context, stock_dynconv  # noqa: F401
from hyper_weights import hyper_state

HERE = os.path.dirname(os.path.abspath(__file__))
BN_KEYS = ("running_mean", "running_var", "num_batches_tracked")


def g31():
    return np.load(os.path.join(HERE, "golden", "g31_hyper_train.npz"))


def g31_array(g, key):
    """One stored array as float64: as it is, or decoded from its int32 fixed point (key__q31 / (2^31 - 1) * key__scale)."""
    if key in g.files:
        return np.asarray(g[key], dtype=np.float64)
    return g[key + "__q31"].astype(np.float64) * (float(g[key + "__scale"]) / float(2 ** 31 - 1))


def g31_grad(g, name, full):
    """(stored gradient, the part of `full` it corresponds to): G31 keeps the two largest gradients as rows 0::n (+ their full norm)."""
    rows = int(g["grad_rows__" + name]) if "grad_rows__" + name in g.files else 1
    return g31_array(g, "grad__" + name), np.asarray(full)[0::rows]


def g31_state(g):
    """{key of one DynamicUpsampleLayer: ndarray} from G31's recipe."""
    return hyper_state(_shapes(g, "layer"), int(g["layer__seed"]), float(g["layer__gain"]), g["bases"], float(g["layer__coeff_scale"]))


def g31_inputs(g):
    """(x [2,256,6,10], events [2,5,48,80], prev_recs [2,1,48,80], upstream gradient [2,128,12,20] of bf16 values) as float32 arrays."""
    from seeded_weights import seeded_input
    sx, sev, sprev, sg = (int(v) for v in g["layer__x_seeds"])
    return (seeded_input(sx, 2, 256, 6, 10), seeded_input(sev, 2, 5, 48, 80), 0.5 * seeded_input(sprev, 2, 1, 48, 80), bf16_exact(seeded_input(sg, 2, 128, 12, 20)))


def bf16_exact(a):
    """float32 values rounded to bfloat16 (nearest even), as float32."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


def is_float_param(k):
    return not k.endswith(BN_KEYS) and not k.endswith("bases")


def to_params(state, dtype, device="cpu", requires_grad=True):
    """{key: tensor}: parameters as `dtype` leaves that require grad, BatchNorm's running statistics as `dtype` buffers, the counter int64."""
    import torch
    p = {}
    for k, v in state.items():
        t = torch.from_numpy(np.asarray(v)).to(device)
        if k.endswith("num_batches_tracked"):
            p[k] = t.clone()
        else:
            p[k] = t.to(dtype).clone()
            if requires_grad and is_float_param(k):
                p[k].requires_grad_(True)
    return p


def _bn_train(x, p, name):
    import torch.nn.functional as F
    p[name + ".num_batches_tracked"] += 1
    return F.batch_norm(x, p[name + ".running_mean"], p[name + ".running_var"], p[name + ".weight"], p[name + ".bias"], True, 0.1, 1e-5)


def stock_atoms_train(ctx, p, pre=""):
    import torch
    net = pre + "dynamic_atom_generation.bases_net."
    c = torch.tanh(_bn_train(_conv(ctx, p, net + "0"), p, net + "1"))
    c = torch.tanh(_bn_train(_conv(c, p, net + "3"), p, net + "4"))
    n, _, h, w = c.shape
    return torch.einsum("bmkhw,kl->bmlhw", c.reshape(n, 6, 12, h, w), p[pre + "dynamic_atom_generation.bases"].to(c.dtype))


def stock_layer_train(x, ev, prev, p, pre="", unfold=False):
    """DynamicUpsampleLayer.forward in .train() mode -> output [B,128,2h,2w]."""
    import torch
    import torch.nn.functional as F
    atoms = stock_atoms_train(stock_context(ev, prev, p, pre), p, pre)
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    return torch.relu(stock_dynconv(up, atoms, p, pre, unfold))


def stock_step_train(ev, prev, states, p, unfold=False):
    """hyper_stock.stock_step with the training-mode dynamic layer: (image, new states)."""
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
    x = stock_layer_train(x + kept[2], ev, prev, p, LAYER, unfold)
    for i in (1, 2):
        x = F.interpolate(x + kept[2 - i], scale_factor=2, mode="bilinear", align_corners=False)
        x = F.relu(_conv(x, p, u + f"decoders.{i}.conv2d"))
    return _conv(x + head, p, u + "pred.conv2d"), new_states


def stock_train_sequence(events, gt, beta, p, unfold=False):
    """HyperE2VID.forward in .train() mode over events [N,T,5,H,W] with gt [N,T,1,H,W]: prev_recs starts as zeros, is each step's DETACHED
    image and is mixed with gt_image (prev (1 - beta) + gt beta) when beta > 0 -> images [N,T,1,H,W]."""
    import torch
    n, t = events.shape[:2]
    states, out = [None] * 3, []
    prev = torch.zeros((n, 1) + tuple(events.shape[-2:]), dtype=events.dtype, device=events.device)
    for k in range(t):
        mixed = prev * (1 - beta) + gt[:, k].detach() * beta if beta > 0 else prev
        img, states = stock_step_train(events[:, k], mixed.to(events.dtype), states, p, unfold)
        prev = img.detach()
        out.append(img)
    return torch.stack(out, 1)


def rel_cos(got, want):
    """(|got - want|_2 / |want|_2, cosine) in float64; a zero `want` gives (|got|_2, 1 if got is zero too else 0)."""
    a, b = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    nb, na = float(np.linalg.norm(b)), float(np.linalg.norm(a))
    if nb == 0.0:
        return na, 1.0 if na == 0.0 else 0.0
    return float(np.linalg.norm(a - b)) / nb, (float(a @ b) / (na * nb) if na > 0.0 else 0.0)


def within(rel, cos, rel16, cos16):
    """The gradient criterion of the training tests: rel <= 2 rel_bf16 + 1e-3 and 1 - cos <= max(1e-2, 2 (1 - cos_bf16))."""
    return np.isfinite(rel) and rel <= 2.0 * rel16 + 1e-3 and (1.0 - cos) <= max(1e-2, 2.0 * (1.0 - cos16))
