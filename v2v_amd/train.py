"""Backward passes of the recurrent UNet's layers: host side of the training kernels (v2v_amd/csrc/v2v_train_tu.hip and the ConvLSTM
step's EPI = 2 epilogue) and the torch.autograd.Functions that the layers of v2v_amd.convlstm / v2v_amd.unet record when they are built
with trainable=True and run with grad enabled.

Every Function's forward calls the SAME forward kernels on the SAME operands as the inference path (its values are bit-identical to
it) and saves what its backward needs: the layer's input and its post-ReLU output (the ReLU backward masks with y > 0).  The backward
runs only HIP kernels: the data gradient of a convolution is the stride-1 convolution of the output gradient (spread onto the input
grid for stride 2) with the flipped, transposed weights on the forward convolution kernel; the weight / bias gradient is an MFMA GEMM
over the pixels (slabs + a fixed-order sum); the ConvLSTM step recomputes its gate GEMM and runs the cell backward on the accumulators.
Activation gradients are bf16 NHWC, the cell-state gradient fp32, parameter gradients fp32.  No float atomics: bitwise reproducible.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .convlstm import conv1x1_nhwc, conv_head_nhwc, conv_nhwc, convlstm_step, upsample2x_nhwc


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _workspace(nbytes: int, device) -> torch.Tensor:
    if nbytes < 0:
        raise ValueError("shape not taken by the backward kernels")
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)


def _nhwc_bf16(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    return t.contiguous()


# ---- raw operators ----------------------------------------------------------------------------------------------------------------
def relu_bwd_nhwc(dy, y):
    """y > 0 ? dy : 0 on NHWC bfloat16 (y = the saved post-ReLU output)."""
    dy = _nhwc_bf16(dy)
    out = torch.empty_like(dy)
    with torch.cuda.device(dy.device):
        _lib.check(_lib.lib().v2v_relu_bwd_nhwc_hip(_ptr(dy), _ptr(y), dy.numel() // dy.shape[-1], dy.shape[-1], _ptr(out), _lib.stream_ptr()))
    return out


def pack_dgrad_weights(weight: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d weight float32 [Cout, Cin, ks, ks] -> the packed stream of the transposed convolution (Cout -> Cin, flipped taps)."""
    cout, cin, ks = weight.shape[0], weight.shape[1], weight.shape[2]
    n = _lib.lib().v2v_conv_dgrad_packed_elems(cin, cout, ks)
    if n < 0:
        raise ValueError(f"no data-gradient kernel for {cin} -> {cout} channels, {ks}x{ks}")
    packed = torch.empty((n,), dtype=torch.bfloat16, device=weight.device)
    scratch = torch.empty((weight.numel(),), dtype=torch.float32, device=weight.device)
    with torch.cuda.device(weight.device):
        _lib.check(_lib.lib().v2v_conv_dgrad_pack_weights_hip(_ptr(weight.detach().float().contiguous()), cin, cout, ks, _ptr(scratch), _ptr(packed),
                                                              _lib.stream_ptr()))
    return packed


def conv_dgrad_nhwc(dy, packed, cin: int, ks: int, stride: int, hin: int, win: int, residual=None):
    """dx [B,Hin,Win,Cin] bf16 of a ks x ks convolution (pad ks//2) from its output gradient dy [B,Hout,Wout,Cout] (ReLU already applied)."""
    dy = _nhwc_bf16(dy)
    b, cout = dy.shape[0], dy.shape[3]
    ws = _workspace(_lib.lib().v2v_conv_dgrad_workspace_bytes(b, hin, win, cin, cout, stride), dy.device)
    dx = torch.empty((b, hin, win, cin), dtype=torch.bfloat16, device=dy.device)
    with torch.cuda.device(dy.device):
        _lib.check(_lib.lib().v2v_conv_dgrad_nhwc_hip(_ptr(dy), _ptr(packed), _ptr(residual), b, hin, win, cin, cout, ks, stride, _ptr(ws), _ptr(dx),
                                                      _lib.stream_ptr()))
    return dx


def conv_wgrad_nhwc(dy, x1, x2=None, c2: int = 0, cin_out: int | None = None, ks: int = 3, stride: int = 1):
    """(dW float32 [Cout, Cin_out, ks, ks], db float32 [Cout]) of a convolution with input x1 [B,Hin,Win,C1] | x2 [.., C2] (x2 None = zeros)."""
    dy = _nhwc_bf16(dy)
    b, ho, wo, cout = dy.shape
    hin, win, c1 = x1.shape[1], x1.shape[2], x1.shape[3]
    cin_out = c1 + c2 if cin_out is None else cin_out
    ws = _workspace(_lib.lib().v2v_conv_wgrad_workspace_bytes(b, ho, wo, c1 + c2, cout, ks), dy.device)
    dw = torch.empty((cout, cin_out, ks, ks), dtype=torch.float32, device=dy.device)
    db = torch.empty((cout,), dtype=torch.float32, device=dy.device)
    with torch.cuda.device(dy.device):
        _lib.check(_lib.lib().v2v_conv_wgrad_nhwc_hip(_ptr(dy), _ptr(x1), c1, _ptr(x2), c2, cin_out, b, hin, win, cout, ks, stride, _ptr(ws), _ptr(dw),
                                                      _ptr(db), _lib.stream_ptr()))
    return dw, db


def upsample2x_bwd_nhwc(dout):
    """Adjoint of upsample2x_nhwc: [B,2H,2W,C] -> [B,H,W,C] bf16 (the gradient of x and of the skip)."""
    dout = _nhwc_bf16(dout)
    b, h2, w2, c = dout.shape
    dx = torch.empty((b, h2 // 2, w2 // 2, c), dtype=torch.bfloat16, device=dout.device)
    with torch.cuda.device(dout.device):
        _lib.check(_lib.lib().v2v_upsample2x_bwd_nhwc_hip(_ptr(dout), b, h2 // 2, w2 // 2, c, _ptr(dx), _lib.stream_ptr()))
    return dx


def conv1x1_bwd_nhwc(dy, x, skip, weight):
    """Prediction layer (C -> 1 on bf16(x + skip)): dy [B,H,W,1] (read as float32) -> (dx [B,H,W,C] bf16 = the gradient of x and skip,
    dW [1,C,1,1], db [1])."""
    dy = dy.float().contiguous()
    b, h, w, c = x.shape
    m = b * h * w
    ws = _workspace(_lib.lib().v2v_conv1x1_bwd_workspace_bytes(m, c), x.device)
    dx = torch.empty_like(x)
    dw = torch.empty((c,), dtype=torch.float32, device=x.device)
    db = torch.empty((1,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().v2v_conv1x1_bwd_nhwc_hip(_ptr(dy), _ptr(x), _ptr(skip), _ptr(weight.detach().float().reshape(-1).contiguous()), m, c,
                                                       _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws), _lib.stream_ptr()))
    return dx, dw.reshape(weight.shape), db


def convlstm_step_bwd(x, h_prev, c_prev, packed, bias, dh, dc):
    """Backward of convlstm_step from the saved x / h_prev / c_prev: (dgates bf16 [B,H,W,4C], dc_prev float32 [B,H,W,C])."""
    b, h, w, c = x.shape
    dh = dh.float().contiguous()
    dc = dc.float().contiguous() if dc is not None else None
    dgates = torch.empty((b, h, w, 4 * c), dtype=torch.bfloat16, device=x.device)
    dc_prev = torch.empty((b, h, w, c), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().v2v_convlstm_step_bwd_hip(_ptr(x), _ptr(h_prev), _ptr(c_prev), _ptr(packed), _ptr(bias), _ptr(dh), _ptr(dc), b, h, w, c,
                                                        _ptr(dgates), _ptr(dc_prev), _lib.stream_ptr()))
    return dgates, dc_prev


def dgrad_weights(layer, conv) -> torch.Tensor:
    """The transposed convolution's packed weights of `conv` (an nn.Conv2d of `layer`), repacked when the weight changes (_version)."""
    w = conv.weight
    key = (w.data_ptr(), w._version, w.device)
    cache = layer.__dict__.setdefault("_dgrad_packed", {})
    hit = cache.get(id(conv))
    if hit is None or hit[0] != key:
        hit = cache[id(conv)] = (key, pack_dgrad_weights(w.detach()))
    return hit[1]


# ---- autograd Functions -------------------------------------------------------------------------------------------------------------
class ConvFn(torch.autograd.Function):
    """[relu](conv_ks(x, stride) + bias) on NHWC bf16 (ConvLayer: the encoders' 5x5 stride-2 convolutions)."""

    @staticmethod
    def forward(ctx, x, weight, bias, layer):
        conv = layer.conv2d
        out = conv_nhwc(x, layer._weights(), bias.detach().float(), conv.kernel_size[0], conv.stride[0], relu=layer.relu)
        ctx.layer = layer
        ctx.save_for_backward(x, out, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out, _ = ctx.saved_tensors
        layer = ctx.layer
        conv = layer.conv2d
        ks, stride = conv.kernel_size[0], conv.stride[0]
        dz = relu_bwd_nhwc(dout, out if layer.relu else None)
        dx = conv_dgrad_nhwc(dz, dgrad_weights(layer, conv), x.shape[3], ks, stride, x.shape[1], x.shape[2]) if ctx.needs_input_grad[0] else None
        dw, db = conv_wgrad_nhwc(dz, x, ks=ks, stride=stride)
        return dx, dw, db, None


class UpConvFn(torch.autograd.Function):
    """[relu](conv_ks(up2(x [+ skip])) + bias) (UpsampleConvLayer with the decoder's sum skip folded into the upsampling)."""

    @staticmethod
    def forward(ctx, x, skip, weight, bias, layer):
        conv = layer.conv2d
        u = upsample2x_nhwc(x, skip)
        out = conv_nhwc(u, layer._weights(), bias.detach().float(), conv.kernel_size[0], 1, relu=layer.relu)
        ctx.layer, ctx.has_skip = layer, skip is not None
        ctx.save_for_backward(u, out, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        u, out, _ = ctx.saved_tensors
        layer = ctx.layer
        conv = layer.conv2d
        ks = conv.kernel_size[0]
        dz = relu_bwd_nhwc(dout, out if layer.relu else None)
        dsum = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            du = conv_dgrad_nhwc(dz, dgrad_weights(layer, conv), u.shape[3], ks, 1, u.shape[1], u.shape[2])
            dsum = upsample2x_bwd_nhwc(du)
        dw, db = conv_wgrad_nhwc(dz, u, ks=ks, stride=1)
        return dsum, dsum if ctx.has_skip else None, dw, db, None


class HeadFn(torch.autograd.Function):
    """The head (voxel bins -> 32 channels): x8 = the input as bf16 NHWC padded to 8 channels; no input gradient (the voxel grid is data)."""

    @staticmethod
    def forward(ctx, x8, weight, bias, layer):
        conv = layer.conv2d
        out = conv_head_nhwc(x8, layer._weights(), bias, conv.kernel_size[0], relu=layer.relu)
        ctx.layer = layer
        ctx.save_for_backward(x8, out, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x8, out, weight = ctx.saved_tensors
        layer = ctx.layer
        dz = relu_bwd_nhwc(dout, out if layer.relu else None)
        dw, db = conv_wgrad_nhwc(dz, x8, cin_out=weight.shape[1], ks=layer.conv2d.kernel_size[0], stride=1)
        return None, dw, db, None


class PredFn(torch.autograd.Function):
    """The 1x1 prediction layer pred(x + skip), one output channel: [B,H,W,C] bf16 (+ skip) -> [B,H,W,1] float32 holding the values of
    the kernel's output in out_dtype (bf16: widened exactly), so that the loss gradient reaches the backward kernel unrounded (an
    L1 gradient sign / N is not a bf16 value for N = 12 x 128^2: rounding it would scale every gradient of the network by ~1 + 2e-3)."""

    @staticmethod
    def forward(ctx, x, skip, weight, bias, out_dtype):
        out = conv1x1_nhwc(x, weight, bias, skip, out_dtype=out_dtype).float()
        ctx.has_skip = skip is not None
        ctx.save_for_backward(x, skip, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, skip, weight = ctx.saved_tensors
        dx, dw, db = conv1x1_bwd_nhwc(dout, x, skip, weight)
        return dx, dx if ctx.has_skip else None, dw, db, None


class ResidualBlockFn(torch.autograd.Function):
    """relu(conv2(relu(conv1(x) + b1)) + b2 + x) on NHWC bf16 (ResidualBlock)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, block):
        mid = conv_nhwc(x, block._weights(block.conv1, "conv1"), b1.detach().float(), 3, relu=True)
        out = conv_nhwc(mid, block._weights(block.conv2, "conv2"), b2.detach().float(), 3, residual=x, relu=True)
        ctx.block = block
        ctx.save_for_backward(x, mid, out, w1, w2)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, mid, out, _, _ = ctx.saved_tensors
        block = ctx.block
        c = x.shape[3]
        h, w = x.shape[1], x.shape[2]
        dz2 = relu_bwd_nhwc(dout, out)
        dmid = conv_dgrad_nhwc(dz2, dgrad_weights(block, block.conv2), c, 3, 1, h, w)
        dw2, db2 = conv_wgrad_nhwc(dz2, mid, ks=3)
        dz1 = relu_bwd_nhwc(dmid, mid)
        dx = conv_dgrad_nhwc(dz1, dgrad_weights(block, block.conv1), c, 3, 1, h, w, residual=dz2)   # + the identity branch, one rounding
        dw1, db1 = conv_wgrad_nhwc(dz1, x, ks=3)
        return dx, dw1, db1, dw2, db2, None


class ConvLSTMFn(torch.autograd.Function):
    """One ConvLSTM step on NHWC state: (x bf16, h_prev bf16 | None, c_prev fp32 | None) -> (h bf16, c fp32, n_twins copies of h
    [, h as NCHW in nchw_dtype]).  input_relu: x is the PRE-activation input; the step reads relu(x) (the ReLU folded into the step's
    input) and dx is masked.  Every use of h (the layer downstream, the next step, a skip connection) reads its own output, so their
    gradients -- each rounded to bf16 once, by the kernel that made it -- are summed in fp32 here, never by autograd in bf16."""

    @staticmethod
    def forward(ctx, x, h_prev, c_prev, weight, bias, module, nchw_dtype, input_relu, n_twins=0):
        xr = torch.relu(x) if input_relu else x
        packed = module._weights()
        b32 = bias.detach().float().contiguous()
        h_state, c_state, h_nchw = convlstm_step(xr, h_prev, c_prev, packed, b32, nchw_dtype=nchw_dtype)
        ctx.module, ctx.input_relu = module, input_relu
        ctx.has_h, ctx.has_c = h_prev is not None, c_prev is not None
        ctx.save_for_backward(xr, h_prev, c_prev, weight, b32)
        ctx.n_twins = n_twins
        outs = (h_state, c_state) + tuple(h_state.clone() for _ in range(n_twins))
        return outs if h_nchw is None else outs + (h_nchw,)

    @staticmethod
    def backward(ctx, dh, dc, *dh_more):
        xr, h_prev, c_prev, _, b32 = ctx.saved_tensors
        module = ctx.module
        c = xr.shape[3]
        dh32 = dh.float()                                                # the uses of h summed in fp32 (one rounding: the kernel's)
        for k, g in enumerate(dh_more):
            dh32 = dh32 + (g.float() if k < ctx.n_twins else g.float().permute(0, 2, 3, 1))
        dgates, dc_prev = convlstm_step_bwd(xr, h_prev, c_prev, module._weights(), b32, dh32, dc)
        dxh = conv_dgrad_nhwc(dgates, dgrad_weights(module, module.Gates), 2 * c, 3, 1, xr.shape[1], xr.shape[2])
        dx = dxh[..., :c]
        if ctx.input_relu:
            dx = relu_bwd_nhwc(dx, xr)
        dh_prev = dxh[..., c:] if ctx.has_h else None
        dw, db = conv_wgrad_nhwc(dgates, xr, h_prev, c, ks=3)             # h_prev None: its half of K reads zeros
        return dx, dh_prev, dc_prev if ctx.has_c else None, dw, db, None, None, None, None
