"""Float64 references of the backward operators of v2v_amd/nhwc_ops.py, on the CPU: what "right" means for every kernel of
v2v_amd/csrc/v2v_train_tu.hip and for the EPI == 2 epilogue of v2v_convlstm.hpp.

Every function takes and returns NCHW float64 tensors and is written as an explicit formula or a loop over the taps -- no autograd here.
tests/test_backward_reference.py checks each of them against torch.autograd.grad in float64 (to 1e-12), tests/test_backward_ops.py
compares the device kernels with them.

Conventions: a convolution is F.conv2d(x, w, stride=stride, padding=ks // 2), w [Cout, Cin, ks, ks]; output size (Hin - 1) // stride + 1.
The x2 upsampling is F.interpolate(scale_factor=2, mode="bilinear", align_corners=False).
"""
import torch

F64 = torch.float64


def bf16_round(t):
    """t -> the float64 values of rne_bf16(rne_f32(t)): what a kernel that forms t in float32 and stores bfloat16 keeps."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def _out_size(n, stride):
    return (n - 1) // stride + 1


def ref_relu_bwd(dy, y):
    """dy where y > 0, else 0 (y = the saved post-ReLU output)."""
    return torch.where(y > 0, dy, torch.zeros_like(dy))


def ref_conv_fwd(x, w, bias=None, stride=1):
    """The convolution itself, tap by tap: out[b, o, oy, ox] = bias[o] + sum_{i, ky, kx} w[o, i, ky, kx] x[b, i, oy s + ky - pad, ox s + kx - pad]."""
    b, cin, hin, win = x.shape
    cout, ks = w.shape[0], w.shape[2]
    pad, ho, wo = ks // 2, _out_size(hin, stride), _out_size(win, stride)
    xp = torch.zeros((b, cin, hin + 2 * pad, win + 2 * pad), dtype=F64)
    xp[:, :, pad:pad + hin, pad:pad + win] = x
    out = torch.zeros((b, cout, ho, wo), dtype=F64)
    for ky in range(ks):
        for kx in range(ks):
            out += torch.einsum("oi,bihw->bohw", w[:, :, ky, kx], xp[:, :, ky:ky + stride * ho:stride, kx:kx + stride * wo:stride])
    return out if bias is None else out + bias.view(1, -1, 1, 1)


def ref_conv_dgrad(dy, w, stride, hin, win, residual=None):
    """dx [B, Cin, hin, win]: dx[b, i, oy s + ky - pad, ox s + kx - pad] += w[o, i, ky, kx] dy[b, o, oy, ox] (+ residual, the identity branch)."""
    b, cout, ho, wo = dy.shape
    cin, ks = w.shape[1], w.shape[2]
    pad = ks // 2
    assert (ho, wo) == (_out_size(hin, stride), _out_size(win, stride)) and w.shape[0] == cout
    dxp = torch.zeros((b, cin, hin + 2 * pad, win + 2 * pad), dtype=F64)
    for ky in range(ks):
        for kx in range(ks):
            dxp[:, :, ky:ky + stride * ho:stride, kx:kx + stride * wo:stride] += torch.einsum("oi,bohw->bihw", w[:, :, ky, kx], dy)
    dx = dxp[:, :, pad:pad + hin, pad:pad + win].clone()
    return dx if residual is None else dx + residual


def ref_conv_wgrad(dy, x, ks, stride):
    """(dW [Cout, Cin, ks, ks], db [Cout]): dW[o, i, ky, kx] = sum_{b, oy, ox} dy[b, o, oy, ox] x[b, i, oy s + ky - pad, ox s + kx - pad]."""
    b, cout, ho, wo = dy.shape
    cin, hin, win = x.shape[1], x.shape[2], x.shape[3]
    pad = ks // 2
    assert (ho, wo) == (_out_size(hin, stride), _out_size(win, stride))
    xp = torch.zeros((b, cin, hin + 2 * pad, win + 2 * pad), dtype=F64)
    xp[:, :, pad:pad + hin, pad:pad + win] = x
    dw = torch.zeros((cout, cin, ks, ks), dtype=F64)
    for ky in range(ks):
        for kx in range(ks):
            dw[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", dy, xp[:, :, ky:ky + stride * ho:stride, kx:kx + stride * wo:stride])
    return dw, dy.sum((0, 2, 3))


def upsample2x_matrix(n):
    """U [2n, n] of the x2 bilinear upsampling along one axis: row 2m reads (max(m - 1, 0), m) with (0.25, 0.75), row 2m + 1 reads
    (m, min(m + 1, n - 1)) with (0.75, 0.25); clamped neighbours add up."""
    u = torch.zeros((2 * n, n), dtype=F64)
    for m in range(n):
        u[2 * m, max(m - 1, 0)] += 0.25
        u[2 * m, m] += 0.75
        u[2 * m + 1, m] += 0.75
        u[2 * m + 1, min(m + 1, n - 1)] += 0.25
    return u


def ref_upsample2x_bwd(dout):
    """Adjoint of the x2 bilinear upsampling: [B, C, 2H, 2W] -> [B, C, H, W] = U_H^T dout U_W."""
    h2, w2 = dout.shape[2], dout.shape[3]
    assert h2 % 2 == 0 and w2 % 2 == 0
    return torch.einsum("jk,bcjl,lm->bckm", upsample2x_matrix(h2 // 2), dout, upsample2x_matrix(w2 // 2))


def ref_conv1x1_bwd(dy, x, skip, w):
    """The prediction layer out = w . bf16(x + skip) + b with the kernel's contract: the weights are rounded to bf16, x + skip is rounded
    to bf16 before the product.  dy [B, Cout, H, W], x / skip [B, C, H, W], w [Cout, C(, 1, 1)] ->
    (dx = sum_o dy_o bf16(w_o) [B, C, H, W], dW [Cout, C], db [Cout])."""
    wb = bf16_round(w.reshape(w.shape[0], -1))
    xs = x if skip is None else bf16_round(x + skip)
    dx = torch.einsum("bohw,oc->bchw", dy, wb)
    return dx, torch.einsum("bohw,bchw->oc", dy, xs), dy.sum((0, 2, 3))


def _sigmoid(v):
    return 1.0 / (1.0 + torch.exp(-v))


def ref_convlstm_step_bwd(x, h_prev, c_prev, w, bias, dh, dc):
    """Backward of one ConvLSTM step (gates = conv3x3(cat(x, h_prev)) + bias, chunks i, r, o, g; c = sig(r) c_prev + sig(i) tanh(g);
    h = sig(o) tanh(c)) for the upstream gradients dh, dc (None: zero), h_prev / c_prev None: the zero state.
        tc = tanh(c);  dc_tot = dc + dh o (1 - tc^2);  d_o = dh tc;  d_i = dc_tot g;  d_g = dc_tot i;  d_r = dc_tot c_prev
        dgates = (d_i i(1-i), d_r r(1-r), d_o o(1-o), d_g (1-g^2));  dc_prev = dc_tot r
    -> (dgates [B, 4C, H, W] = the gradient of the pre-activation gates, in gate order i, r, o, g; dc_prev [B, C, H, W])."""
    h_prev = torch.zeros_like(x) if h_prev is None else h_prev
    c_prev = torch.zeros_like(x) if c_prev is None else c_prev
    dc = torch.zeros_like(x) if dc is None else dc
    pre = ref_conv_fwd(torch.cat([x, h_prev], 1), w, bias)
    c = x.shape[1]
    i, r, o = (_sigmoid(pre[:, k * c:(k + 1) * c]) for k in range(3))
    g = torch.tanh(pre[:, 3 * c:])
    tc = torch.tanh(r * c_prev + i * g)
    dct = dc + dh * o * (1.0 - tc * tc)
    d_i, d_r, d_o, d_g = dct * g, dct * c_prev, dh * tc, dct * i
    dgates = torch.cat([d_i * i * (1.0 - i), d_r * r * (1.0 - r), d_o * o * (1.0 - o), d_g * (1.0 - g * g)], 1)
    return dgates, dct * r
