"""The recurrent UNet's layers as torch.autograd.Functions: what the layers of v2v_amd.convlstm / v2v_amd.unet record when they are built
with trainable=True and run with grad enabled.  The raw forward and backward operators are those of v2v_amd/nhwc_ops.py (backward kernels:
v2v_amd/csrc/v2v_train_tu.hip and the ConvLSTM step's EPI = 2 epilogue).

Every Function states its layer's forward kernel sequence ONCE, in its static `kernels(...)`: the layer module calls that directly when it
does not train, and Function.forward calls it and saves what backward needs (the layer's input and its post-ReLU output: the ReLU backward
masks with y > 0).  Training forward and inference are therefore the same kernels on the same operands, bit for bit.  The backward runs
only HIP kernels; no float atomics: bitwise reproducible.

`kernels` reads the parameters from the layer it is given.  The weight / bias arguments of every `forward` are there for autograd alone (it
routes their gradients): they must be that layer's own parameters, as the layers of v2v_amd.convlstm pass them.

    ConvFn / UpConvFn (sum or concat skip) / VoxelConvFn (head, stem, 16-channel head)     ConvLayer's roles; one backward: conv_backward
    PredFn / ResidualBlockFn / ConvLSTMFn                                                 the prediction layer, ResidualBlock, ConvLSTM
    DynamicUpsampleFn                                                                     HyperE2VID's dynamic decoder in training mode (BatchNorm on batch statistics)
"""
from __future__ import annotations

import torch

from .nhwc_ops import (context_conv_nhwc, conv1x1_bwd_cout_nhwc, conv1x1_nhwc, conv_dgrad_nhwc, conv_head16_nhwc, conv_head_nhwc, conv_nhwc,
                       conv_stem_nhwc, conv_wgrad_nhwc, convlstm_step, convlstm_step_bwd, dynconv_datoms_nhwc, dynconv_df_nhwc, dynconv_dx_nhwc,
                       dynconv_nhwc, dynconv_wgrad_nhwc, hyper_atoms, hyper_atoms_bwd, hyper_bn_apply, hyper_bn_bwd, hyper_bn_stats,
                       hyper_context_nhwc8, pack_dgrad_weights, packed_weights, relu_bwd_nhwc, upsample2x_bwd_nhwc, upsample2x_cat_bwd_nhwc,
                       upsample2x_cat_nhwc, upsample2x_nhwc)


def dgrad_weights(layer, name: str) -> torch.Tensor:
    """The transposed convolution's packed weights of getattr(layer, name) (an nn.Conv2d), through the layer's packed-weight cache."""
    return packed_weights(layer._packed, name + ".dgrad", getattr(layer, name).weight, pack_dgrad_weights)


def conv_backward(layer, dout, out, x, need_dx: bool, cin_out=None, adjoint=None):
    """The backward every convolution layer shares, from the layer's input x and its post-ReLU output `out`: ReLU mask -> data gradient
    (when need_dx; handed through `adjoint`, the backward of what stood in front of the convolution, before the next launch) -> weight /
    bias gradient.  -> (dx | None, dw, db).  cin_out: the weight's input channels when x carries more (the voxel layers' 8-channel pad)."""
    conv = layer.conv2d
    ks, stride = conv.kernel_size[0], conv.stride[0]
    dz = relu_bwd_nhwc(dout, out if layer.relu else None)
    dx = None
    if need_dx:
        dx = conv_dgrad_nhwc(dz, dgrad_weights(layer, "conv2d"), x.shape[3], ks, stride, x.shape[1], x.shape[2])
        if adjoint is not None:
            dx = adjoint(dx)
    dw, db = conv_wgrad_nhwc(dz, x, cin_out=cin_out, ks=ks, stride=stride)
    return dx, dw, db


class ConvFn(torch.autograd.Function):
    """[relu](conv_ks(x, stride) + bias) on NHWC bf16 (ConvLayer: the encoders' 5x5 stride-2 convolutions)."""

    @staticmethod
    def kernels(x, layer):
        conv = layer.conv2d
        return conv_nhwc(x, layer._weights(), conv.bias.detach().float(), conv.kernel_size[0], conv.stride[0], relu=layer.relu)

    @staticmethod
    def forward(ctx, x, weight, bias, layer):
        out = ConvFn.kernels(x, layer)
        ctx.layer = layer
        ctx.save_for_backward(x, out, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out, _ = ctx.saved_tensors
        return conv_backward(ctx.layer, dout, out, x, ctx.needs_input_grad[0]) + (None,)


class UpConvFn(torch.autograd.Function):
    """[relu](conv_ks(up2(x [+ skip])) + bias), or with cat=True [relu](conv_ks(up2(cat(x, skip))) + bias): UpsampleConvLayer with the
    decoder's sum skip folded into the upsampling, or behind the plain UNet's concat skip (model/unet.py:350).  The two differ in the
    upsampling call and in its adjoint."""

    @staticmethod
    def kernels(x, skip, layer, cat=False):
        """-> (out, u = the upsampled sum / concat buffer the convolution read)."""
        conv = layer.conv2d
        u = upsample2x_cat_nhwc(x, skip) if cat else upsample2x_nhwc(x, skip)
        return conv_nhwc(u, layer._weights(), conv.bias.detach().float(), conv.kernel_size[0], conv.stride[0], relu=layer.relu), u

    @staticmethod
    def forward(ctx, x, skip, weight, bias, layer, cat=False):
        out, u = UpConvFn.kernels(x, skip, layer, cat)
        ctx.layer, ctx.cat, ctx.has_skip, ctx.c1 = layer, cat, skip is not None, x.shape[3]
        ctx.save_for_backward(u, out, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        u, out, _ = ctx.saved_tensors
        need_x, need_skip = ctx.needs_input_grad[:2]

        def adjoint(du):
            if not ctx.cat:
                dsum = upsample2x_bwd_nhwc(du)
                return dsum, dsum if ctx.has_skip else None
            return (upsample2x_cat_bwd_nhwc(du, 0, ctx.c1) if need_x else None,
                    upsample2x_cat_bwd_nhwc(du, ctx.c1, u.shape[3] - ctx.c1) if need_skip else None)
        dxs, dw, db = conv_backward(ctx.layer, dout, out, u, need_x or need_skip, adjoint=adjoint)
        return (dxs or (None, None)) + (dw, db, None, None)


class VoxelConvFn(torch.autograd.Function):
    """The layers that read the voxel grid, by the layer's role: the head (voxel bins -> 32 channels, stride 1), the plain UNet's stem
    (-> 64 channels, 3x3, stride 2) and FireNet's 16-channel head (inference only: ConvLayer refuses trainable=True).  x8 = the input as
    bf16 NHWC padded to 8 channels; no input gradient (the voxel grid is data)."""

    @staticmethod
    def kernels(x8, layer):
        conv = layer.conv2d
        if layer.role == "stem":
            return conv_stem_nhwc(x8, layer._weights(), conv.bias, relu=layer.relu)
        if layer.role == "head16":
            return conv_head16_nhwc(x8, layer._weights(), conv.bias, relu=layer.relu)
        return conv_head_nhwc(x8, layer._weights(), conv.bias, conv.kernel_size[0], relu=layer.relu)

    @staticmethod
    def forward(ctx, x8, weight, bias, layer):
        out = VoxelConvFn.kernels(x8, layer)
        ctx.layer = layer
        ctx.save_for_backward(x8, out, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x8, out, weight = ctx.saved_tensors
        return conv_backward(ctx.layer, dout, out, x8, False, cin_out=weight.shape[1]) + (None,)


class PredFn(torch.autograd.Function):
    """The 1x1 prediction layer pred(x + skip), 1..3 output channels (more than one: the backward kernel for Cout outputs): [B,H,W,C] bf16
    (+ skip) -> [B,H,W,Cout] float32 holding the values of
    the kernel's output in out_dtype (bf16: widened exactly), so that the loss gradient reaches the backward kernel unrounded (an
    L1 gradient sign / N is not a bf16 value for N = 12 x 128^2: rounding it would scale every gradient of the network by ~1 + 2e-3)."""

    @staticmethod
    def kernels(x, skip, layer, out_dtype):
        return conv1x1_nhwc(x, layer.conv2d.weight, layer.conv2d.bias, skip, out_dtype=out_dtype)

    @staticmethod
    def forward(ctx, x, skip, weight, bias, layer, out_dtype):
        out = PredFn.kernels(x, skip, layer, out_dtype).float()
        ctx.has_skip = skip is not None
        ctx.save_for_backward(x, skip, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, skip, weight = ctx.saved_tensors
        dx, dw, db = conv1x1_bwd_cout_nhwc(dout, x, skip, weight)
        return dx, dx if ctx.has_skip else None, dw, db, None, None


class ResidualBlockFn(torch.autograd.Function):
    """relu(conv2(relu(conv1(x) + b1)) + b2 + x) on NHWC bf16 (ResidualBlock)."""

    @staticmethod
    def kernels(x, block):
        """-> (out, mid = relu(conv1(x) + b1))."""
        p1, p2 = block._weights()
        mid = conv_nhwc(x, p1, block.conv1.bias.detach().float(), 3, relu=True)
        return conv_nhwc(mid, p2, block.conv2.bias.detach().float(), 3, residual=x, relu=True), mid

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, block):
        out, mid = ResidualBlockFn.kernels(x, block)
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
        dmid = conv_dgrad_nhwc(dz2, dgrad_weights(block, "conv2"), c, 3, 1, h, w)
        dw2, db2 = conv_wgrad_nhwc(dz2, mid, ks=3)
        dz1 = relu_bwd_nhwc(dmid, mid)
        dx = conv_dgrad_nhwc(dz1, dgrad_weights(block, "conv1"), c, 3, 1, h, w, residual=dz2)   # + the identity branch, one rounding
        dw1, db1 = conv_wgrad_nhwc(dz1, x, ks=3)
        return dx, dw1, db1, dw2, db2, None


class ConvLSTMFn(torch.autograd.Function):
    """One ConvLSTM step on NHWC state: (x bf16, h_prev bf16 | None, c_prev fp32 | None) -> (h bf16, c fp32, n_twins copies of h
    [, h as NCHW in nchw_dtype]).  input_relu: x is the PRE-activation input; the step reads relu(x) (the ReLU folded into the step's
    input) and dx is masked.  Every use of h (the layer downstream, the next step, a skip connection) reads its own output, so their
    gradients -- each rounded to bf16 once, by the kernel that made it -- are summed in fp32 here, never by autograd in bf16."""

    @staticmethod
    def kernels(xr, h_prev, c_prev, module, b32, nchw_dtype):
        """xr = the POST-ReLU input (inference applies an input ReLU on the way in, ConvLSTM.forward / _nhwc_in; training in `forward`
        below, which saves xr), b32 = Gates.bias as float32 -> (h_state, c_state, h_nchw | None)."""
        return convlstm_step(xr, h_prev, c_prev, module._weights(), b32, nchw_dtype=nchw_dtype)

    @staticmethod
    def forward(ctx, x, h_prev, c_prev, weight, bias, module, nchw_dtype, input_relu, n_twins=0):
        xr = torch.relu(x) if input_relu else x
        b32 = bias.detach().float().contiguous()
        h_state, c_state, h_nchw = ConvLSTMFn.kernels(xr, h_prev, c_prev, module, b32, nchw_dtype)
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
        dxh = conv_dgrad_nhwc(dgates, dgrad_weights(module, "Gates"), 2 * c, 3, 1, xr.shape[1], xr.shape[2])
        dx = dxh[..., :c]
        if ctx.input_relu:
            dx = relu_bwd_nhwc(dx, xr)
        dh_prev = dxh[..., c:] if ctx.has_h else None
        dw, db = conv_wgrad_nhwc(dgates, xr, h_prev, c, ks=3)             # h_prev None: its half of K reads zeros
        return dx, dh_prev, dc_prev if ctx.has_c else None, dw, db, None, None, None, None


def _update_running_stats(bn, mean, var, m: int) -> None:
    """nn.BatchNorm2d's bookkeeping of one training-mode call: running = (1 - momentum) running + momentum batch, the variance unbiased
    (m / (m - 1)), num_batches_tracked += 1; momentum None = the cumulative average."""
    if not bn.track_running_stats or bn.running_mean is None:
        return
    with torch.no_grad():
        bn.num_batches_tracked += 1
        mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
        c = bn.num_features
        bn.running_mean.mul_(1.0 - mom).add_(mean[:c].to(bn.running_mean.dtype), alpha=mom)
        bn.running_var.mul_(1.0 - mom).add_(var[:c].to(bn.running_var.dtype) * (m / (m - 1.0)), alpha=mom)


class DynamicUpsampleFn(torch.autograd.Function):
    """HyperE2VID's DynamicUpsampleLayer (v2v_amd.hyper) in TRAINING mode on NHWC bf16: relu(DynamicConv(up2(x [+ skip]), atoms)), the atoms
    from context_fusion.conv -> bases_net (convolution with its own weights and bias, BatchNorm on the batch's statistics, tanh; twice) ->
    the Fourier-Bessel bases.  Saved per call: the upsampled input u, the atoms, the post-ReLU output, the two BatchNorm inputs z1 / z2 with
    their mean / rstd, the context staging x8 and the context; the BatchNorm outputs are recomputed from z (bit for bit), the dynamic
    convolution's features F inside the weight-gradient kernel.  events and prev_recs get no gradient (the reference detaches prev_recs)."""

    @staticmethod
    def kernels(x, skip, ev, prev, layer):
        """The training-mode forward (also what .train() under no_grad runs); updates the running statistics.
        -> (out, (u, atoms, z1, mean1, rstd1, z2, mean2, rstd2, x8, ctx))."""
        fus, gen, dyn = layer.context_fusion, layer.dynamic_atom_generation, layer.dynamic_conv
        bn1, bn2 = gen.bases_net[1], gen.bases_net[4]
        x8 = fus.stage(ev, prev)
        ctx = context_conv_nhwc(x8, fus.conv.weight.detach().float(), fus.conv.bias)
        m = ctx.shape[0] * ctx.shape[1] * ctx.shape[2]
        if m <= 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {[ctx.shape[0], 64, ctx.shape[1], ctx.shape[2]]}")
        (p1, b1), (p2, b2) = gen._train_weights()
        z1 = conv_nhwc(ctx, p1, b1, 3)
        mean1, var1, rstd1 = hyper_bn_stats(z1, bn1.eps)
        hid = hyper_bn_apply(z1, mean1, rstd1, bn1.weight, bn1.bias, tanh=True)
        z2 = conv_nhwc(hid, p2, b2, 3)                                   # 72 outputs in 128 columns (zero weights and bias behind them)
        mean2, var2, rstd2 = hyper_bn_stats(z2, bn2.eps)
        pre = hyper_bn_apply(z2, mean2, rstd2, bn2.weight, bn2.bias, tanh=False)
        atoms = hyper_atoms(pre, gen.bases.float().contiguous())
        _update_running_stats(bn1, mean1, var1, m)
        _update_running_stats(bn2, mean2, var2, m)
        u = upsample2x_nhwc(x, skip)
        out = dynconv_nhwc(u, atoms, dyn._weights(), dyn.bias.detach().float(), relu=layer.relu)
        return out, (u, atoms, z1, mean1, rstd1, z2, mean2, rstd2, x8, ctx)

    @staticmethod
    def forward(ctx_, x, skip, ev, prev, wc, bc, w1, b1, g1, be1, w2, b2, g2, be2, wd, bd, layer):
        out, saved = DynamicUpsampleFn.kernels(x, skip, ev, prev, layer)
        ctx_.layer, ctx_.has_skip = layer, skip is not None
        ctx_.save_for_backward(out, *saved, wc, w1, g1, be1, w2, g2, be2, wd)
        return out

    @staticmethod
    def backward(ctx_, dout):
        out, u, atoms, z1, mean1, rstd1, z2, mean2, rstd2, x8, ctx, wc, w1, g1, be1, w2, g2, be2, wd = ctx_.saved_tensors
        layer = ctx_.layer
        gen, dyn = layer.dynamic_atom_generation, layer.dynamic_conv
        h, w = ctx.shape[1], ctx.shape[2]
        # the dynamic convolution
        dz = relu_bwd_nhwc(dout, out if layer.relu else None)
        df = dynconv_df_nhwc(dz, dyn._weights_t())
        datoms = dynconv_datoms_nhwc(u, df)
        dx = dskip = None
        if ctx_.needs_input_grad[0] or ctx_.needs_input_grad[1]:
            dsum = upsample2x_bwd_nhwc(dynconv_dx_nhwc(atoms, df))
            dx, dskip = dsum, dsum if ctx_.has_skip else None
        del df
        dwd, dbd = dynconv_wgrad_nhwc(dz, u, atoms)
        # atoms -> bases_net.4 (BatchNorm) -> bases_net.3 -> tanh, bases_net.1 (BatchNorm) -> bases_net.0 -> context_fusion.conv
        pre = hyper_bn_apply(z2, mean2, rstd2, g2, be2, tanh=False)
        dpre = hyper_atoms_bwd(datoms, pre, gen.bases.float().contiguous())
        dz2, dg2, dbe2, db2 = hyper_bn_bwd(dpre, z2, mean2, rstd2, g2, be2, tanh=False)
        hid = hyper_bn_apply(z1, mean1, rstd1, g1, be1, tanh=True)
        dhid = conv_dgrad_nhwc(dz2, gen._dgrad_weights(3), 64, 3, 1, h, w)
        dw2 = conv_wgrad_nhwc(dz2, hid, ks=3)[0][:w2.shape[0]]
        dz1, dg1, dbe1, db1 = hyper_bn_bwd(dhid, z1, mean1, rstd1, g1, be1, tanh=True)
        dctx = conv_dgrad_nhwc(dz1, gen._dgrad_weights(0), 32, 3, 1, h, w)
        dw1 = conv_wgrad_nhwc(dz1, ctx, ks=3)[0]
        dwc, dbc = conv_wgrad_nhwc(dctx, x8, cin_out=wc.shape[1], ks=3)
        return (dx, dskip, None, None, dwc, dbc, dw1, db1.clone(), dg1.clone(), dbe1.clone(), dw2.contiguous(), db2.clone(), dg2.clone(), dbe2.clone(),
                dwd, dbd, None)
