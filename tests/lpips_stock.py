"""LPIPS-VGG in plain torch.nn.functional: the stock restatement of PNetLin(pnet_type='vgg', version='0.1', spatial=False) in eval mode behind
model/loss.py:95-119, on a 33-key state dict.  Any dtype / device the state and the inputs share; autograd gives the gradient.  It is what
training runs today, so it is the CPU cross-check of golden G30 and the baseline of tools/lpips_time.py."""
import torch
import torch.nn.functional as F

SLICES = ((1, (0, 2)), (2, (5, 7)), (3, (10, 12, 14)), (4, (17, 19, 21)), (5, (24, 26, 28)))


def features(state, x):
    """x [B,3,H,W] (already through the scaling layer) -> the five taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3."""
    taps = []
    for s, convs in SLICES:
        if s > 1:
            x = F.max_pool2d(x, 2, 2)
        for idx in convs:
            x = F.relu(F.conv2d(x, state[f"net.slice{s}.{idx}.weight"], state[f"net.slice{s}.{idx}.bias"], padding=1))
        taps.append(x)
    return taps


def normalize_tensor(f, eps=1e-10):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + eps)


def lpips_vgg(state, pred, target, normalize=True):
    """-> dist [B] in the inputs' dtype."""
    if pred.shape[1] == 1:
        pred = torch.cat([pred, pred, pred], dim=1)
    if target.shape[1] == 1:
        target = torch.cat([target, target, target], dim=1)
    if normalize:
        target, pred = 2 * target - 1, 2 * pred - 1
    shift, scale = state["scaling_layer.shift"], state["scaling_layer.scale"]
    taps0, taps1 = features(state, (target - shift) / scale), features(state, (pred - shift) / scale)
    val = None
    for k, (f0, f1) in enumerate(zip(taps0, taps1)):
        diff = (normalize_tensor(f0) - normalize_tensor(f1)) ** 2
        res = F.conv2d(diff, state[f"lin{k}.model.1.weight"]).mean([2, 3], keepdim=True)
        val = res if val is None else val + res
    return val.reshape(-1)


def dist_and_grad(state, pred, target, normalize=True, dtype=torch.float32, autocast=False):
    """(dist [B], dpred) with dpred = the gradient of sum_b (b + 1) dist_b; state / inputs converted to `dtype`; autocast: under CPU or CUDA
    bf16 autocast (float32 weights and inputs)."""
    state = {k: v.to(dtype) for k, v in state.items()}
    pred = pred.detach().to(dtype).requires_grad_(True)
    target = target.detach().to(dtype)
    if autocast:
        with torch.autocast(pred.device.type, dtype=torch.bfloat16):
            dist = lpips_vgg(state, pred, target, normalize)
    else:
        dist = lpips_vgg(state, pred, target, normalize)
    dist = dist.to(dtype)
    w = torch.arange(1, dist.numel() + 1, dtype=dtype, device=dist.device)
    (dist * w).sum().backward()
    return dist.detach(), pred.grad
