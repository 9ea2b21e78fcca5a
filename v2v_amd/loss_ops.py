"""The image losses of training on the device kernels of v2v_amd/csrc/v2v_loss.hpp: raw operators (one per C entry point), the autograd
Functions on them, and the functional drop-in for utils/loss.py's temporal_consistency_loss.

    warp_bilinear(img, flow)                        img sampled at (x + flow_x, y + flow_y): F.grid_sample(img, grid(flow), align_corners=True)
    warp_bilinear_adjoint(dout, flow, hw)           its adjoint (the gradient to img), bitwise reproducible: 64-bit fixed point, integer atomics
    tc_loss_fwd / tc_loss_bwd                       temporal consistency + l1 + l2 of N image pairs: weighted per-sample means [3, N], gradients
    seq_loss_fwd / seq_loss_bwd                     the same for all T steps of [B,T,C,H,W] tensors in a fixed number of launches
    temporal_consistency_loss(...)                  utils/loss.py:6-69, same signature and return values
    sequence_losses(...)                            {class name: [B,T]} of v2v_amd/losses.py's classes called step by step, in one Function
    lpips_stem / lpips_pool / lpips_compare_fwd     the LPIPS-VGG kernels around the backbone's convolutions (v2v_lpips.hpp), each with its
    (+ _bwd), lpips_vgg(model, pred, target)        backward; lpips_vgg = the distance of a v2v_amd.lpips.LPIPSVGG, mean or per sample

Everything but LPIPS' bf16 activations is float32 (other dtypes are widened), on the GPU; gradients go to the processed images only, frames and flow are data.  Rows of a
[3, N] loss tensor are temporal consistency, l1, l2; a zero weight skips that loss.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import DTYPE_CODES, launch, need, ptr
from .nhwc_ops import _DTYPES

TC, L1, L2 = 0, 1, 2
MAPS = ("image0_warped_to1", "processed0_warped_to1", "visibility_mask", "error_map")


def _f32(name, t, shape=None):
    """t as a contiguous float32 CUDA tensor (other dtypes are widened); no CPU fallback."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA tensor (v2v_amd has no CPU fallback)")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def _workspace(n_img, c, h, w, backward, device):
    n = _lib.lib().v2v_tc_loss_workspace_bytes(n_img, c, h, w, int(backward))
    _lib.check(min(n, 0))
    return torch.empty((max(n, 16),), dtype=torch.uint8, device=device)


def _weights(weights):
    w = tuple(float(0.0 if v is None else v) for v in weights)
    if len(w) != 3:
        raise ValueError("weights = (temporal consistency, l1, l2)")
    return w


# ---- the warp alone -------------------------------------------------------------------------------------------------------------------
def warp_bilinear(img: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """img [N,C,H,W], flow [N,2,H,W] (x, y displacement in pixels) -> img sampled bilinearly at (x + flow_x, y + flow_y), zero outside."""
    _lib.require_gpu()
    if img.dim() != 4:
        raise ValueError("img must be [N,C,H,W]")
    n, c, h, w = img.shape
    img, flow = _f32("img", img), _f32("flow", flow, (n, 2, h, w))
    out = torch.empty_like(img)
    launch("v2v_warp_bilinear_hip", img.device, ptr(img), ptr(flow), n, c, h, w, ptr(out))
    return out


def warp_bilinear_adjoint(dout: torch.Tensor, flow: torch.Tensor, hw=None) -> torch.Tensor:
    """The gradient of sum(dout * warp_bilinear(img, flow)) to img [N,C,*hw]; the warp keeps the size, so hw must be dout's."""
    _lib.require_gpu()
    if dout.dim() != 4:
        raise ValueError("dout must be [N,C,H,W]")
    n, c, h, w = dout.shape
    if hw is not None and tuple(hw) != (h, w):
        raise ValueError(f"the warp keeps the image size: hw {tuple(hw)} != {(h, w)}")
    dout, flow = _f32("dout", dout), _f32("flow", flow, (n, 2, h, w))
    din = torch.empty_like(dout)
    ws = _workspace(n, c, h, w, True, dout.device)
    launch("v2v_warp_bilinear_adjoint_hip", dout.device, ptr(dout), ptr(flow), n, c, h, w, ptr(din), ptr(ws))
    return din


# ---- N image pairs --------------------------------------------------------------------------------------------------------------------
def _pair_inputs(image0, image1, processed0, processed1, flow, weights):
    if processed1.dim() != 4:
        raise ValueError("processed1 must be [N,C,H,W]")
    n, c, h, w = processed1.shape
    image1, processed1 = _f32("image1", image1, (n, c, h, w)), _f32("processed1", processed1)
    if weights[TC] != 0.0:
        image0, processed0 = _f32("image0", image0, (n, c, h, w)), _f32("processed0", processed0, (n, c, h, w))
        flow = _f32("flow", flow, (n, 2, h, w))
    else:
        image0 = processed0 = flow = None
    return image0, image1, processed0, processed1, flow, (n, c, h, w)


def tc_loss_fwd(image0, image1, processed0, processed1, flow, alpha=50.0, weights=(1.0, 0.0, 0.0), flow_sign=1.0, output_images=False):
    """-> losses float32 [3, N] = weight * per-sample mean (rows temporal consistency, l1, l2); with output_images also the four maps
    (image0_warped_to1, processed0_warped_to1, visibility_mask, error_map), each [N,C,H,W].  With a zero temporal weight image0, processed0
    and flow are not read (None is fine)."""
    _lib.require_gpu()
    weights = _weights(weights)
    image0, image1, processed0, processed1, flow, (n, c, h, w) = _pair_inputs(image0, image1, processed0, processed1, flow, weights)
    dev = processed1.device
    losses = torch.empty((3, n), dtype=torch.float32, device=dev)
    maps = tuple(torch.empty((n, c, h, w), dtype=torch.float32, device=dev) for _ in MAPS) if output_images else (None,) * 4
    ws = _workspace(n, c, h, w, False, dev)
    launch("v2v_tc_loss_fwd_hip", dev, ptr(image0), ptr(image1), ptr(processed0), ptr(processed1), ptr(flow), n, 1, c * h * w, 0, 2 * h * w, 0,
           0, c, h, w, alpha, flow_sign, *weights, ptr(losses), *(ptr(m) for m in maps), ptr(ws))
    return (losses, maps) if output_images else losses


def tc_loss_bwd(image0, image1, processed0, processed1, flow, gout, alpha=50.0, weights=(1.0, 0.0, 0.0), flow_sign=1.0):
    """Gradient of sum(gout * losses), gout [3, N] -> (dprocessed0 or None without a temporal term, dprocessed1)."""
    _lib.require_gpu()
    weights = _weights(weights)
    image0, image1, processed0, processed1, flow, (n, c, h, w) = _pair_inputs(image0, image1, processed0, processed1, flow, weights)
    gout = _f32("gout", gout, (3, n))
    d1 = torch.empty_like(processed1)
    d0 = torch.empty_like(processed1) if weights[TC] != 0.0 else None
    ws = _workspace(n, c, h, w, True, d1.device)
    launch("v2v_tc_loss_bwd_hip", d1.device, ptr(image0), ptr(image1), ptr(processed0), ptr(processed1), ptr(flow), n, 1, c * h * w, 0, 2 * h * w, 0,
           0, c, h, w, alpha, flow_sign, *weights, ptr(gout), 0, ptr(d1), ptr(d0), ptr(ws))
    return d0, d1


# ---- T steps of a sequence ------------------------------------------------------------------------------------------------------------
def _seq_inputs(pred, frame, flow, L0, weights):
    if pred.dim() != 5:
        raise ValueError("pred must be [B,T,C,H,W]")
    b, t, c, h, w = pred.shape
    L0 = int(L0)
    if L0 < 1:
        raise ValueError("L0 must be at least 1 (the reference asserts L0 > 0)")
    pred, frame = _f32("pred", pred), _f32("frame", frame, (b, t, c, h, w))
    tc = weights[TC] != 0.0 and L0 < t
    flow = _f32("flow", flow, (b, t, 2, h, w)) if tc else None
    chw = c * h * w
    # image0 / processed0 / flow start at the first step that has a temporal term: frame and pred one step earlier, the flow of step L0
    ptrs = (ptr(frame, (L0 - 1) * chw) if tc else None, ptr(frame), ptr(pred, (L0 - 1) * chw) if tc else None, ptr(pred),
            ptr(flow, L0 * 2 * h * w) if tc else None)
    layout = (b, t, t * chw, chw, t * 2 * h * w, 2 * h * w, L0, c, h, w)
    return pred, frame, flow, ptrs, layout


def seq_loss_fwd(pred, frame, flow, L0, alpha=50.0, weights=(1.0, 1.0, 0.0)):
    """pred / frame [B,T,C,H,W], flow [B,T,2,H,W] -> float32 [3, B, T]: what temporal_consistency_loss(weight, L0), l1_loss, l2_loss of
    v2v_amd/losses.py return step by step with reduce_batch=False (temporal consistency: 0 for t < L0, the flow negated), in two launches."""
    _lib.require_gpu()
    weights = _weights(weights)
    pred, frame, flow, ptrs, layout = _seq_inputs(pred, frame, flow, L0, weights)
    b, t, c, h, w = pred.shape
    losses = torch.empty((3, b, t), dtype=torch.float32, device=pred.device)
    ws = _workspace(b * t, c, h, w, False, pred.device)
    launch("v2v_tc_loss_fwd_hip", pred.device, *ptrs, *layout, alpha, -1.0, *weights, ptr(losses), None, None, None, None, ptr(ws))
    return losses


def seq_loss_bwd(pred, frame, flow, L0, gout, alpha=50.0, weights=(1.0, 1.0, 0.0)):
    """Gradient of sum(gout * seq_loss_fwd(...)), gout [3, B, T], to pred: bit for bit what autograd accumulates into pred when the step
    loop calls l1_loss, l2_loss, temporal_consistency_loss in that order on pred[:, t]."""
    _lib.require_gpu()
    weights = _weights(weights)
    pred, frame, flow, ptrs, layout = _seq_inputs(pred, frame, flow, L0, weights)
    b, t, c, h, w = pred.shape
    gout = _f32("gout", gout, (3, b, t))
    dpred = torch.empty_like(pred)
    ws = _workspace(b * t, c, h, w, True, pred.device)
    launch("v2v_tc_loss_bwd_hip", pred.device, *ptrs, *layout, alpha, -1.0, *weights, ptr(gout), 1, ptr(dpred), None, ptr(ws))
    return dpred


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
class PairLossFn(torch.autograd.Function):
    """losses [3, N] (and the four maps, not differentiable) of N image pairs; gradients to processed0 and processed1 only."""

    @staticmethod
    def forward(ctx, processed0, processed1, image0, image1, flow, alpha, weights, flow_sign, output_images):
        ctx.save_for_backward(*(t for t in (processed0, processed1, image0, image1, flow) if t is not None))
        ctx.have = [t is not None for t in (processed0, processed1, image0, image1, flow)]
        ctx.cfg = (alpha, weights, flow_sign)
        out = tc_loss_fwd(image0, image1, processed0, processed1, flow, alpha, weights, flow_sign, output_images)
        if not output_images:
            return out
        ctx.mark_non_differentiable(*out[1])
        return (out[0],) + out[1]

    @staticmethod
    def backward(ctx, gout, *_):
        saved = iter(ctx.saved_tensors)
        processed0, processed1, image0, image1, flow = (next(saved) if h else None for h in ctx.have)
        alpha, weights, flow_sign = ctx.cfg
        d0, d1 = tc_loss_bwd(image0, image1, processed0, processed1, flow, gout, alpha, weights, flow_sign)
        if d0 is not None:
            d0 = d0.to(processed0.dtype)
        return d0, d1.to(processed1.dtype), None, None, None, None, None, None, None


class SeqLossFn(torch.autograd.Function):
    """losses [3, B, T] of a whole sequence; gradient to pred only."""

    @staticmethod
    def forward(ctx, pred, frame, flow, L0, alpha, weights):
        ctx.save_for_backward(pred, frame, flow)
        ctx.cfg = (L0, alpha, weights)
        return seq_loss_fwd(pred, frame, flow, L0, alpha, weights)

    @staticmethod
    def backward(ctx, gout):
        pred, frame, flow = ctx.saved_tensors
        L0, alpha, weights = ctx.cfg
        return seq_loss_bwd(pred, frame, flow, L0, gout, alpha, weights).to(pred.dtype), None, None, None, None, None


def temporal_consistency_loss(image0, image1, processed0, processed1, flow01, alpha=50.0, output_images=False, reduce_batch=True):
    """utils/loss.py:6-69 on the device kernels: the warping error between processed1 and processed0 warped by flow01, weighted by the
    visibility mask of the frames.  Same signature and return values: a scalar (reduce_batch) or [N], and with output_images also the
    dict of image0, image1, image0_warped_to1, processed0_warped_to1, visibility_mask, error_map."""
    out = PairLossFn.apply(processed0, processed1, image0, image1, flow01, float(alpha), (1.0, 0.0, 0.0), 1.0, bool(output_images))
    per_sample = (out[0] if output_images else out)[TC]
    loss = per_sample.mean() if reduce_batch else per_sample
    if not output_images:
        return loss
    return loss, dict(image0=image0, image1=image1, **dict(zip(MAPS, out[1:])))


def sequence_losses(pred, frame, flow, l1_weight, l2_weight, temporal_consistency_weight, L0, alpha=50.0):
    """All T steps of ModelInterface.calc_loss's image losses (model/train_utils.py:402-424) at once: pred / frame [B,T,C,H,W], flow
    [B,T,2,H,W] -> {"l1_loss" / "l2_loss" / "temporal_consistency_loss": [B,T]} for every weight that is not None, bit-identical -- values
    and the gradient to pred -- to calling the classes of v2v_amd/losses.py step by step with reduce_batch=False."""
    weights = (temporal_consistency_weight, l1_weight, l2_weight)
    out = SeqLossFn.apply(pred, frame, flow, int(L0), float(alpha), _weights(weights))
    names = ("temporal_consistency_loss", "l1_loss", "l2_loss")
    return {names[k]: out[k] for k in (L1, L2, TC) if weights[k] is not None}


# ---- LPIPS-VGG: the raw operators around the backbone's convolutions (v2v_amd/csrc/v2v_lpips.hpp; the network is v2v_amd/lpips.py) -----------
def _lp_vec(name, t, n, device):
    """t as a contiguous float32 vector of n elements on `device` (a [1,3,1,1] buffer or a [1,C,1,1] weight is fine)."""
    if not isinstance(t, torch.Tensor) or t.numel() != n or t.device != device:
        raise ValueError(f"{name} must hold {n} values on {device}")
    return t.detach().to(torch.float32).reshape(-1).contiguous()


def lpips_stem(x, weight, bias, shift, scale, normalize=False, out=None):
    """x float32 / bfloat16 [B,1|3,H,W] -> bfloat16 [B,H,W,64] = relu(conv3x3(((2x - 1 if normalize else x) - shift_c) / scale_c) + bias), zero
    padding AFTER the scaling; weight float32 [64,3,3,3] (a one-channel x stands for three equal channels).  out: write into this tensor."""
    _lib.require_gpu()
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in _DTYPES or x.dim() != 4 or x.shape[1] not in (1, 3):
        raise ValueError("x must be a float32 or bfloat16 CUDA tensor [B,1|3,H,W]")
    x = x.detach().contiguous()
    b, cin, h, w = x.shape
    if weight.dtype != torch.float32 or tuple(weight.shape) != (64, 3, 3, 3) or weight.device != x.device:
        raise ValueError("weight must be float32 [64,3,3,3] on x's device")
    out = torch.empty((b, h, w, 64), dtype=torch.bfloat16, device=x.device) if out is None else need("out", out, shape=(b, h, w, 64))
    launch("v2v_lpips_stem_hip", x.device, ptr(x), DTYPE_CODES[x.dtype], b, cin, h, w, ptr(weight.detach().contiguous()), ptr(_lp_vec("bias", bias, 64, x.device)),
           ptr(_lp_vec("shift", shift, 3, x.device)), ptr(_lp_vec("scale", scale, 3, x.device)), int(bool(normalize)), ptr(out))
    return out


def lpips_stem_bwd(dz, weight, scale, cin, normalize=False):
    """dz bfloat16 [B,H,W,64] (ReLU-masked) -> float32 [B,cin,H,W]: the gradient of lpips_stem's x (the three channels summed for cin = 1)."""
    _lib.require_gpu()
    need("dz", dz)
    b, h, w, c = dz.shape
    if c != 64 or cin not in (1, 3) or weight.dtype != torch.float32 or tuple(weight.shape) != (64, 3, 3, 3) or weight.device != dz.device:
        raise ValueError("dz must be [B,H,W,64], cin 1 or 3, weight float32 [64,3,3,3] on dz's device")
    dpred = torch.empty((b, cin, h, w), dtype=torch.float32, device=dz.device)
    launch("v2v_lpips_stem_bwd_hip", dz.device, ptr(dz), b, cin, h, w, ptr(weight.detach().contiguous()), ptr(_lp_vec("scale", scale, 3, dz.device)),
           int(bool(normalize)), ptr(dpred))
    return dpred


def _lp_pool_shape(x):
    b, h, w, c = x.shape
    if h % 2 or w % 2 or c % 8:
        raise ValueError(f"the 2x2 max-pool needs even H and W and C % 8 == 0 (got {tuple(x.shape)})")
    return b, h, w, c


def lpips_pool(x):
    """2x2 max-pool on NHWC bfloat16: [B,H,W,C] -> [B,H/2,W/2,C]."""
    _lib.require_gpu()
    b, h, w, c = _lp_pool_shape(need("x", x))
    out = torch.empty((b, h // 2, w // 2, c), dtype=torch.bfloat16, device=x.device)
    launch("v2v_lpips_pool_hip", x.device, ptr(x), b, h, w, c, ptr(out))
    return out


def lpips_pool_bwd(dy, x, dtap=None, relu_mask=False):
    """Backward of lpips_pool: dy [B,H/2,W/2,C] goes to the first maximum (row-major) of each window of x [B,H,W,C]; + dtap [B,H,W,C] in
    float32 with ONE rounding to bfloat16; relu_mask: zero where x <= 0 (x is the post-ReLU tensor that was pooled)."""
    _lib.require_gpu()
    b, h, w, c = _lp_pool_shape(need("x", x))
    need("dy", dy, shape=(b, h // 2, w // 2, c))
    if dtap is not None:
        need("dtap", dtap, shape=x.shape)
    dx = torch.empty_like(x)
    launch("v2v_lpips_pool_bwd_hip", x.device, ptr(dy), ptr(x), ptr(dtap), int(bool(relu_mask)), b, h, w, c, ptr(dx))
    return dx


def _lp_compare_args(f0, f1, w):
    need("f0", f0)
    need("f1", f1, shape=f0.shape)
    n, cc = f0.shape[0], f0.shape[3]
    if cc not in (64, 128, 256, 512) or f1.device != f0.device:
        raise ValueError("f0 / f1 must have 64, 128, 256 or 512 channels and share a device")
    return n, f0.shape[1] * f0.shape[2], cc, _lp_vec("w", w, cc, f0.device)


def lpips_compare_fwd(f0, f1, w, dist):
    """dist[b] += mean_pixels sum_c w_c (n0_c - n1_c)^2, n = f / (|f| + 1e-10) per pixel; f0 / f1 bfloat16 [B,H,W,Cc] (the two halves of one
    tap), w [Cc] (any shape), dist float32 [B], accumulated in place (zeros before the first tap) and returned."""
    _lib.require_gpu()
    n, hw, cc, w = _lp_compare_args(f0, f1, w)
    if not isinstance(dist, torch.Tensor) or dist.dtype != torch.float32 or tuple(dist.shape) != (n,) or not dist.is_contiguous() or dist.device != f0.device:
        raise ValueError(f"dist must be a contiguous float32 [{n}] tensor on f0's device")
    ws = torch.empty((_lib.lib().v2v_lpips_compare_workspace_bytes(n, hw),), dtype=torch.uint8, device=f0.device)
    launch("v2v_lpips_compare_fwd_hip", f0.device, ptr(f0), ptr(f1), ptr(w), n, hw, cc, ptr(dist), ptr(ws))
    return dist


def lpips_compare_bwd(f0, f1, w, ddist):
    """df0 bfloat16 [B,H,W,Cc]: the gradient of sum_b ddist[b] * (lpips_compare_fwd's term of sample b) to f0.  At a pixel with f0 == 0
    everywhere the norm's own derivative (NaN in autograd) is taken as 0: df0 = g / eps there."""
    _lib.require_gpu()
    n, hw, cc, w = _lp_compare_args(f0, f1, w)
    ddist = _f32("ddist", ddist, (n,))
    df0 = torch.empty_like(f0)
    launch("v2v_lpips_compare_bwd_hip", f0.device, ptr(f0), ptr(f1), ptr(w), ptr(ddist), n, hw, cc, ptr(df0))
    return df0


def lpips_vgg(model, pred, target, normalize=True, reduce_batch=True):
    """The LPIPS-VGG distance of model (a v2v_amd.lpips.LPIPSVGG) between pred and target [B,1|3,H,W]: the mean over the batch, or float32 [B]
    with reduce_batch=False; the gradient goes to pred only.  Time has no state in this loss: a sequence [N,T,...] is evaluated as the
    batch [N*T,...] (reshape before the call), there is no step loop to fold."""
    dist = model(pred, target, normalize=normalize)
    return dist.mean() if reduce_batch else dist
