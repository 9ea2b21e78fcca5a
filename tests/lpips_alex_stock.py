"""LPIPS-AlexNet in plain torch.nn.functional: the stock restatement of PNetLin(pnet_type='alex', version='0.1', spatial=False) in eval mode
behind ModelInterface.compute_metrics (model/train_utils.py:236), on a 17-key state dict.  Any dtype / device the state and the inputs
share.  It is what the test loop runs today, so it is the CPU cross-check of golden G34 and the baseline of tools/lpips_alex_time.py."""
import torch
import torch.nn.functional as F

# (slice, index, stride, padding, a 3x3 / stride-2 max-pool opens the slice)
CONVS = ((1, 0, 4, 2, False), (2, 3, 1, 2, True), (3, 6, 1, 1, True), (4, 8, 1, 1, False), (5, 10, 1, 1, False))


def features(state, x):
    """x [B,3,H,W] (already through the scaling layer) -> the five taps relu1 .. relu5."""
    taps = []
    for s, idx, stride, pad, pooled in CONVS:
        if pooled:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, state[f"net.slice{s}.{idx}.weight"], state[f"net.slice{s}.{idx}.bias"], stride=stride, padding=pad))
        taps.append(x)
    return taps


def normalize_tensor(f, eps=1e-10):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + eps)


def lpips_alex(state, pred, target, normalize=True, per_layer=False):
    """pred, target [B,1|3,H,W] or [1|3,H,W] -> dist [B,1,1,1] in the inputs' dtype (and the five tap means [B,5]).  A one-channel image
    broadcasts to three channels in the scaling layer, as it does in the reference."""
    if pred.dim() == 3:
        pred, target = pred[None], target[None]
    if normalize:
        target, pred = 2 * target - 1, 2 * pred - 1
    shift, scale = state["scaling_layer.shift"], state["scaling_layer.scale"]
    taps0, taps1 = features(state, (target - shift) / scale), features(state, (pred - shift) / scale)
    val, res = None, []
    for k, (f0, f1) in enumerate(zip(taps0, taps1)):
        diff = (normalize_tensor(f0) - normalize_tensor(f1)) ** 2
        res.append(F.conv2d(diff, state[f"lin{k}.model.1.weight"]).mean([2, 3], keepdim=True))
        val = res[0].clone() if val is None else val + res[k]
    return (val, torch.cat(res, dim=1).reshape(-1, 5)) if per_layer else val


class StockLPIPSAlex(torch.nn.Module):
    """The restatement as a module with the reference's call: fn(pred, target, normalize=...) -> [B,1,1,1]."""

    def __init__(self, state):
        super().__init__()
        self.state = state

    def forward(self, pred, target, normalize=False):
        return lpips_alex(self.state, pred, target, normalize)
