"""Float64 references of the image-loss operators of v2v_amd/loss_ops.py, on the CPU: what "right" means for every kernel of
v2v_amd/csrc/v2v_loss.hpp.

Every function takes and returns NCHW float64 tensors and is written as an explicit formula -- a gather or a scatter over the four corners,
no grid_sample and no autograd here.  tests/test_loss_reference.py checks each of them against the reference's formula under
torch.autograd in float64 (to 1e-12) and against golden G29; tests/test_loss_ops.py compares the device kernels with them.

Conventions (utils/loss.py:6-69): flow [N,2,H,W] = (x, y) displacement in pixels; the sampling position goes through the reference's
normalisation to [-1, 1] and grid_sample's un-normalisation with align_corners=True; samples outside the frame are zero.
"""
import torch

F64 = torch.float64
EPS = 1e-5


def corners(flow):
    """The four corners of every pixel's sampling position: a list of (flat index [N, H*W] int64, weight [N, H*W]) in grid_sample's order
    nw, ne, sw, se; a corner outside the frame has weight 0 (its index is clamped into the frame)."""
    n, _, h, w = flow.shape
    flow = flow.to(F64)
    xs = torch.arange(w, dtype=F64).view(1, 1, w)
    ys = torch.arange(h, dtype=F64).view(1, h, 1)
    gx = 2 * (xs + flow[:, 0]) / (w - 1) - 1
    gy = 2 * (ys + flow[:, 1]) / (h - 1) - 1
    ix = (gx + 1) / 2 * (w - 1)
    iy = (gy + 1) / 2 * (h - 1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    out = []
    for cy, cx, wgt in ((y0, x0, (x0 + 1 - ix) * (y0 + 1 - iy)), (y0, x0 + 1, (ix - x0) * (y0 + 1 - iy)),
                        (y0 + 1, x0, (x0 + 1 - ix) * (iy - y0)), (y0 + 1, x0 + 1, (ix - x0) * (iy - y0))):
        inside = (cx >= 0) & (cx <= w - 1) & (cy >= 0) & (cy <= h - 1)
        idx = (cy.clamp(0, h - 1) * w + cx.clamp(0, w - 1)).long()
        out.append((idx.reshape(n, h * w), torch.where(inside, wgt, torch.zeros_like(wgt)).reshape(n, h * w)))
    return out


def ref_warp(img, flow):
    """out[n, c, y, x] = sum over the corners of weight * img[n, c, corner]."""
    n, c, h, w = img.shape
    flat = img.to(F64).reshape(n, c, h * w)
    out = torch.zeros((n, c, h * w), dtype=F64)
    for idx, wgt in corners(flow):
        out += flat.gather(2, idx[:, None].expand(n, c, h * w)) * wgt[:, None]
    return out.reshape(n, c, h, w)


def ref_warp_adjoint(dout, flow):
    """din[n, c, corner] += weight * dout[n, c, y, x]: the gradient of sum(dout * ref_warp(img, flow)) to img."""
    n, c, h, w = dout.shape
    flat = dout.to(F64).reshape(n, c, h * w)
    din = torch.zeros((n, c, h * w), dtype=F64)
    for idx, wgt in corners(flow):
        din.scatter_add_(2, idx[:, None].expand(n, c, h * w), flat * wgt[:, None])
    return din.reshape(n, c, h, w)


def ref_tc_maps(image0, image1, processed0, processed1, flow01, alpha=50.0):
    """-> dict(image0_warped_to1, processed0_warped_to1, visibility_mask, error_map, loss [N] = mean over (C,H,W) of error_map)."""
    image0, image1, processed0, processed1 = (t.to(F64) for t in (image0, image1, processed0, processed1))
    i0w = ref_warp(image0, flow01)
    vis = torch.exp(-alpha * (image1 - i0w) ** 2)
    p0w = ref_warp(processed0.clamp(0, 255), flow01)
    err = vis * (processed1 - p0w).abs() / (processed1.abs() + p0w.abs() + EPS)
    return dict(image0_warped_to1=i0w, processed0_warped_to1=p0w, visibility_mask=vis, error_map=err, loss=err.mean(dim=(1, 2, 3)))


def ref_tc_grads(image0, image1, processed0, processed1, flow01, gout, alpha=50.0):
    """Gradient of sum_n gout[n] * loss[n] -> (dprocessed0, dprocessed1).  With d = processed1 - w, D = |processed1| + |w| + 1e-5,
    k = gout / (C*H*W):   d/dprocessed1 = k m (sgn(d) D - |d| sgn(processed1)) / D^2,   d/dw = k m (-sgn(d) D - |d| sgn(w)) / D^2,
    dprocessed0 = [0 <= processed0 <= 255] * adjoint(d/dw)."""
    processed0, processed1 = processed0.to(F64), processed1.to(F64)
    m = ref_tc_maps(image0, image1, processed0, processed1, flow01, alpha)
    vis, w = m["visibility_mask"], m["processed0_warped_to1"]
    n, c, h, wd = processed1.shape
    k = gout.to(F64).view(n, 1, 1, 1) / (c * h * wd)
    d = processed1 - w
    div = processed1.abs() + w.abs() + EPS
    d1 = k * vis * (torch.sign(d) * div - d.abs() * torch.sign(processed1)) / div ** 2
    dw = k * vis * (-torch.sign(d) * div - d.abs() * torch.sign(w)) / div ** 2
    inside = ((processed0 >= 0) & (processed0 <= 255)).to(F64)
    return ref_warp_adjoint(dw, flow01) * inside, d1


def ref_l1(pred, target):
    return (pred.to(F64) - target.to(F64)).abs().mean(dim=(1, 2, 3))


def ref_l2(pred, target):
    return ((pred.to(F64) - target.to(F64)) ** 2).mean(dim=(1, 2, 3))


def ref_l1_grad(pred, target, gout):
    n, c, h, w = pred.shape
    return gout.to(F64).view(n, 1, 1, 1) / (c * h * w) * torch.sign(pred.to(F64) - target.to(F64))


def ref_l2_grad(pred, target, gout):
    n, c, h, w = pred.shape
    return gout.to(F64).view(n, 1, 1, 1) / (c * h * w) * 2 * (pred.to(F64) - target.to(F64))


def ref_sequence(pred, frame, flow, L0, weights=(1.0, 1.0, 1.0), alpha=50.0):
    """The step loop of ModelInterface.calc_loss (model/train_utils.py:402-424) over pred / frame [B,T,C,H,W], flow [B,T,2,H,W] with
    weights = (temporal consistency, l1, l2): -> (losses [3, B, T], dpred = the gradient of their plain sum)."""
    b, t = pred.shape[:2]
    pred, frame, flow = pred.to(F64), frame.to(F64), flow.to(F64)
    losses = torch.zeros((3, b, t), dtype=F64)
    dpred = torch.zeros_like(pred)
    ones = torch.ones(b, dtype=F64)
    for s in range(t):
        losses[1, :, s] = weights[1] * ref_l1(pred[:, s], frame[:, s])
        losses[2, :, s] = weights[2] * ref_l2(pred[:, s], frame[:, s])
        dpred[:, s] += ref_l1_grad(pred[:, s], frame[:, s], weights[1] * ones) + ref_l2_grad(pred[:, s], frame[:, s], weights[2] * ones)
        if s >= L0:
            args = (frame[:, s - 1], frame[:, s], pred[:, s - 1], pred[:, s], -flow[:, s])
            losses[0, :, s] = weights[0] * ref_tc_maps(*args, alpha)["loss"]
            d0, d1 = ref_tc_grads(*args, weights[0] * ones, alpha)
            dpred[:, s - 1] += d0
            dpred[:, s] += d1
    return losses, dpred
