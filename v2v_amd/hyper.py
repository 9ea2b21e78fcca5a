"""HyperE2VID (model/hyper_model.py) on the device kernels: the recurrent E2VID network of v2v_amd/unet.py with decoders[0] replaced by the
per-pixel DYNAMIC decoder (model/hyper_model.py:33-60, model/hyper/hyper_dynamic.py), under the reference's own module tree so that a
reference checkpoint loads with strict=True:

    HyperE2VID(unet_kwargs)                 model/hyper_model.py:198-237    keys  unetrecurrent.*
    UNetRecurrent(unet_kwargs)              model/hyper_model.py:138-196    as v2v_amd.unet.UNetRecurrent, plus
                                                                            decoders.0.context_fusion.conv.*,
                                                                            decoders.0.dynamic_atom_generation.bases / .bases_net.{0,1,3,4}.*,
                                                                            decoders.0.dynamic_conv.compositional_coefficients / .bias
    DynamicUpsampleLayer / ConvolutionalContextFusion / DynamicAtomGeneration / DynamicConv   the reference's constructors and members

Configuration covered = config/train_v2v_hyper_10k.yaml / config/test_hypere2vid_original.yaml: skip 'sum', 'convlstm', kernel_size 5, base 32,
multiplier 2, norm none, use_upsample_conv, 3 encoders, one output channel; anything else raises ValueError (no stock fallback).  Inference
by default: eval mode (BatchNorm runs on its running statistics, folded into the convolutions' packed weights) under torch.no_grad().
trainable=True (HyperE2VID / UNetRecurrent / DynamicUpsampleLayer) adds training: in .train() mode the dynamic layer runs BatchNorm on the
batch's statistics (and updates the running ones), and under grad it records v2v_amd.train.DynamicUpsampleFn like every other layer
records its Function; .eval() stays the inference path.

What runs per time step for the dynamic layer (raw operators in v2v_amd/nhwc_ops.py, kernels in v2v_amd/csrc/v2v_hyper.hpp):
    hyper_context_nhwc8 -> context_conv_nhwc (context_fusion.conv) -> conv_nhwc (bases_net.0 + folded BatchNorm) -> tanh_bf16_ ->
    conv_nhwc (bases_net.3 + folded BatchNorm, 72 outputs zero-padded to 128) -> hyper_atoms (tanh + the Fourier-Bessel einsum, float32) ->
    upsample2x_nhwc (sum skip folded in) -> dynconv_nhwc (features in registers -> matrix cores, bias, ReLU).

The layers follow v2v_amd/convlstm.py's protocol: `_packed` + `_weights()` on nhwc_ops.packed_weights (the BatchNorm fold is keyed on all six
tensors it reads), convlstm._fold_sum_skip for the sum skip.  HyperE2VID keeps its own states / reset_states (it also clears prev_recs and
has no graphed sequence: sharing unet._Stateful would need as many lines as it saves).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import unet as _unet
from .convlstm import _fold_sum_skip, _nchw_out, _nhwc_in, _out_dtype
from .nhwc_ops import (context_conv_nhwc, conv_nhwc, dynconv_nhwc, hyper_atoms, hyper_context_nhwc8, pack_conv_weights, pack_dgrad_weights,
                       pack_dynconv_weights, pack_dynconv_weights_t, packed_weights, tanh_bf16_, upsample2x_nhwc)
from .train import DynamicUpsampleFn


def fourier_bessel_bases(kernel_size: int, num_bases: int) -> torch.Tensor:
    """The multiscale Fourier-Bessel bases DynamicAtomGeneration keeps in its `bases` buffer: float32 [(kernel_size // 2) * num_bases,
    kernel_size ** 2] ([12, 25] for (5, 6)), computed here from scipy's Bessel functions (no table file).

    Scale s = 1 .. kernel_size // 2 is the (2 s + 1)^2 window of radius R = s + 0.5.  Its basis functions are psi_kq(r, t) =
    J_k(z_kq r) / |J_{k+1}(z_kq)| for r < 1 (zero outside), times sqrt(2) cos(k t) and sqrt(2) sin(k t) for k > 0, where z_kq is the q-th
    positive zero of J_k; the pairs (k <= 15, q) kept are those whose NEXT zero z_k,q+1 is at most pi R f (f = 2 for s = 1, else 1.5),
    ordered by z_kq; the first (2 s + 1)^2 - 1 functions, sampled on the window, are divided by the root of their mean energy; the first
    `num_bases` of them, zero-padded to kernel_size x kernel_size, are the scale's rows."""
    import numpy as np
    from scipy import special                                      # here, not at module level: `import v2v_amd` does not need scipy

    rows = []
    for s in range(1, kernel_size // 2 + 1):
        radius, side = s + 0.5, 2 * s + 1
        bound = np.pi * radius * (2.0 if s < 2 else 1.5)
        n_zeros = int(bound / np.pi) + 3                           # consecutive zeros are > pi apart beyond the first: more than enough
        kept = []
        for k in range(16):
            z = special.jn_zeros(k, n_zeros + 1)
            kept += [(z[q], k) for q in range(n_zeros) if z[q + 1] <= bound]
        kept.sort()
        coords = np.arange(-s, s + 1) / radius
        gx, gy = np.meshgrid(coords, coords)                       # gx varies along a window row
        r, t = np.sqrt(gx ** 2 + gy ** 2).ravel(), np.arctan2(gx, gy).ravel()
        funcs = []
        for z, k in kept:
            phi = special.jv(k, r * z) / abs(special.jv(k + 1, z))
            phi[r >= 1] = 0.0
            if k == 0:
                funcs.append(phi)
            else:
                funcs.append(phi * np.cos(k * t) * np.sqrt(2.0))
                funcs.append(phi * np.sin(k * t) * np.sqrt(2.0))
        psi = np.array(funcs[:side * side - 1])
        psi = psi / np.sqrt((psi ** 2).sum(axis=1).mean())
        pad = kernel_size // 2 - s
        block = torch.from_numpy(psi[:num_bases].astype(np.float32)).reshape(-1, side, side)
        rows.append(nn.functional.pad(block, (pad, pad, pad, pad)).reshape(block.shape[0], kernel_size * kernel_size))
    return torch.cat(rows, 0)


def fold_batchnorm(conv: nn.Conv2d, bn: nn.BatchNorm2d):
    """(w', b') with conv'(x) == bn(conv(x)) in eval mode: w' = w * g / sqrt(var + eps), b' = (b - mean) * g / sqrt(var + eps) + beta."""
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    b = conv.bias.detach().float() if conv.bias is not None else torch.zeros_like(scale)
    return conv.weight.detach().float() * scale[:, None, None, None], (b - bn.running_mean.detach().float()) * scale + bn.bias.detach().float()


class ConvolutionalContextFusion(nn.Module):
    """model/hyper/hyper_dynamic.py:7-23: cat(events, previous reconstruction) -> bilinear x1/4 -> 3x3 convolution.  forward() returns the
    context as bfloat16 NHWC [B,H/4,W/4,32] (the next kernel's layout)."""

    def __init__(self, in_channels, out_channels, downsample_factor=4, kernel_size=3, padding="same"):
        super().__init__()
        if in_channels > 8 or out_channels != 32 or downsample_factor != 4 or kernel_size != 3 or padding not in ("same", 1):
            raise ValueError("the context kernels cover <= 8 fused channels -> 32, downsample_factor 4, kernel_size 3, padding 'same'")
        self.scale = 1.0 / downsample_factor
        self.conv = nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, padding=padding)

    def _weights(self):
        return None                                                  # context_conv_nhwc reads the float32 weight itself

    def stage(self, ev_tensor, prev_recs):
        """cat(events, prev_recs) at 1/4 scale as bfloat16 NHWC8: the convolution's input (what its weight gradient reads in training)."""
        if ev_tensor.shape[1] + 1 != self.conv.in_channels:
            raise ValueError(f"context fusion was built for {self.conv.in_channels - 1} event bins + 1 image, got {ev_tensor.shape[1]} bins")
        return hyper_context_nhwc8(ev_tensor.detach().float(), prev_recs.detach().float().contiguous())

    def forward(self, ev_tensor, prev_recs):
        return context_conv_nhwc(self.stage(ev_tensor, prev_recs), self.conv.weight.detach().float(), self.conv.bias)


class DynamicAtomGeneration(nn.Module):
    """model/hyper/hyper_dynamic.py:26-57: context -> bases_net (conv + BatchNorm + tanh, twice) -> per-pixel atoms = coefficients x bases.
    forward(context bf16 NHWC [B,h,w,32]) -> atoms float32 [B,h,w,25,6] (tap-major; the reference's [B,6,25,h,w] is permute(0,4,3,1,2))."""

    def __init__(self, kernel_size=3, num_atoms=6, num_bases=6, in_context_channels=32, hid_channels=64, stride=1):
        super().__init__()
        if kernel_size != 5 or num_atoms != 6 or num_bases != 6 or in_context_channels != 32 or hid_channels != 64 or stride != 1:
            raise ValueError("the atom kernels cover kernel_size 5, 6 atoms, 6 bases per scale, 32 context channels, 64 hidden channels, stride 1")
        self.stride = stride
        self.num_atoms = num_atoms
        bases = fourier_bessel_bases(kernel_size, num_bases)
        self.register_buffer("bases", bases)
        self.num_multiscale_bases = bases.shape[0]
        num_basis_coeff = num_atoms * self.num_multiscale_bases
        self.bases_net = nn.Sequential(
            nn.Conv2d(in_context_channels, hid_channels, kernel_size=3, padding="same", stride=stride),
            nn.BatchNorm2d(hid_channels),
            nn.Tanh(),
            nn.Conv2d(hid_channels, num_basis_coeff, kernel_size=3, padding="same"),
            nn.BatchNorm2d(num_basis_coeff),
            nn.Tanh())
        self._packed = {}

    def _fold(self, i: int, pad_to: int):
        conv, bn = self.bases_net[i], self.bases_net[i + 1]
        w, b = fold_batchnorm(conv, bn)
        if pad_to > w.shape[0]:                                    # 72 -> 128 output columns (what the convolution kernel takes): zero rows
            w = torch.cat([w, w.new_zeros((pad_to - w.shape[0],) + tuple(w.shape[1:]))])
            b = torch.cat([b, b.new_zeros(pad_to - b.shape[0])])
        return pack_conv_weights(w.contiguous()), b.contiguous()

    def _weights(self):
        """((packed, bias) of bases_net.0 + .1, (packed, bias) of bases_net.3 + .4), BatchNorm folded in at pack time."""
        out = []
        for i, pad_to in ((0, 64), (3, 128)):
            conv, bn = self.bases_net[i], self.bases_net[i + 1]
            out.append(packed_weights(self._packed, f"bases_net.{i}", (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var),
                                      lambda *_, i=i, pad_to=pad_to: self._fold(i, pad_to)))   # _fold reads the same six tensors from the modules
        return out

    @staticmethod
    def _pad_rows(t, pad_to: int):
        return t if pad_to <= t.shape[0] else torch.cat([t, t.new_zeros((pad_to - t.shape[0],) + tuple(t.shape[1:]))])

    def _train_weights(self):
        """Training mode: ((packed, bias) of bases_net.0, (packed, bias) of bases_net.3) WITHOUT the BatchNorm fold (the statistics are
        the batch's), each pack keyed on its convolution weight alone, beside the folded entries; 72 outputs still padded to 128."""
        out = []
        for i, pad_to in ((0, 64), (3, 128)):
            conv = self.bases_net[i]
            packed = packed_weights(self._packed, f"bases_net.{i}.train", conv.weight,
                                    lambda w, pad_to=pad_to: pack_conv_weights(self._pad_rows(w.float(), pad_to).contiguous()))
            bias = conv.bias.detach().float() if conv.bias is not None else conv.weight.new_zeros(conv.out_channels, dtype=torch.float32)
            out.append((packed, self._pad_rows(bias, pad_to).contiguous()))
        return out

    def _dgrad_weights(self, i: int):
        """The transposed convolution's packed weights of bases_net.i (i = 0 or 3; the 72 outputs padded to 128 as the forward pads them)."""
        pad_to = 64 if i == 0 else 128
        return packed_weights(self._packed, f"bases_net.{i}.dgrad", self.bases_net[i].weight,
                              lambda w: pack_dgrad_weights(self._pad_rows(w.float(), pad_to).contiguous()))

    def forward(self, context):
        (p0, b0), (p1, b1) = self._weights()
        hid = tanh_bf16_(conv_nhwc(context, p0, b0, 3))
        return hyper_atoms(conv_nhwc(hid, p1, b1, 3), self.bases.float().contiguous())


def _pack_coefficients(w):
    return pack_dynconv_weights(w.float().contiguous())


class DynamicConv(nn.Module):
    """model/hyper/hyper_dynamic.py:60-92 on the fused kernel: forward(x bf16 NHWC [B,H,W,256], atoms float32 [B,H,W,25,6], relu) ->
    bf16 NHWC [B,H,W,128]."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, num_atoms=6):
        super().__init__()
        if (in_channels, out_channels, kernel_size, stride, padding, num_atoms) != (256, 128, 5, 1, 2, 6):
            raise ValueError("the dynamic-convolution kernel covers 256 -> 128 channels, kernel_size 5, stride 1, padding 2, 6 atoms")
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding, self.num_atoms = stride, padding, num_atoms
        self.compositional_coefficients = nn.Parameter(torch.empty(out_channels, in_channels * num_atoms, 1, 1))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()
        self._packed = {}

    def reset_parameters(self):
        nn.init.kaiming_normal_(self.compositional_coefficients, mode="fan_out", nonlinearity="relu")
        nn.init.zeros_(self.bias)

    def _weights(self):
        return packed_weights(self._packed, "compositional_coefficients", self.compositional_coefficients, _pack_coefficients)

    def _weights_t(self):
        """The transposed stream the backward's dF kernel reads."""
        return packed_weights(self._packed, "compositional_coefficients.t", self.compositional_coefficients,
                              lambda w: pack_dynconv_weights_t(w.float().contiguous()))

    def forward(self, x, atoms, relu=False):
        return dynconv_nhwc(x, atoms, self._weights(), self.bias.detach().float(), relu=relu)


class DynamicUpsampleLayer(nn.Module):
    """model/hyper_model.py:33-60: bilinear x2 upsampling, then the dynamic convolution whose per-pixel kernels come from the events and the
    previous reconstruction, then ReLU.  forward(x, ev_tensor, prev_recs, skip=None): skip = the decoder's sum skip, folded into the
    upsampling kernel (layer(x, ev, prev, skip) == layer(x + skip, ev, prev)).  x [B,256,h,w]: channels-last bfloat16 is consumed and produced
    in place, anything else goes through the layout kernel and comes back NCHW in x's dtype.  ev_tensor [B,bins,8h,8w] float of any layout,
    prev_recs [B,1,8h,8w].  trainable=False: eval mode and no grad, else RuntimeError.  trainable=True: .train() runs BatchNorm on the
    batch's statistics and updates the running ones (under grad it records v2v_amd.train.DynamicUpsampleFn; events and prev_recs get no
    gradient); .eval() is the inference path, without a backward."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, activation="relu", in_fuse_channels=6, out_fuse_channels=32,
                 num_atoms=6, trainable: bool = False):
        super().__init__()
        if activation not in ("relu", None):
            raise ValueError("the dynamic layer's epilogue covers activation 'relu' or None")
        self.context_fusion = ConvolutionalContextFusion(in_fuse_channels, out_fuse_channels)
        self.dynamic_atom_generation = DynamicAtomGeneration(kernel_size=kernel_size, num_atoms=num_atoms, num_bases=6,
                                                             in_context_channels=out_fuse_channels, hid_channels=64, stride=stride)
        self.dynamic_conv = DynamicConv(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding, num_atoms=num_atoms)
        self.relu = activation == "relu"
        self.trainable = bool(trainable)

    def _weights(self):
        """Everything forward needs packed, now (on the current stream)."""
        return self.context_fusion._weights(), self.dynamic_atom_generation._weights(), self.dynamic_conv._weights()

    def _check_mode(self, x):
        if self.trainable:
            if not self.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
                raise RuntimeError("v2v_amd.hyper.DynamicUpsampleLayer has no backward in eval mode (BatchNorm folded into the convolutions): "
                                   "call .train() to train it, or run it under torch.no_grad()")
            return
        if self.training:
            raise RuntimeError("v2v_amd.hyper.DynamicUpsampleLayer runs BatchNorm on its running statistics only: call .eval() first "
                               "(batch-statistics BatchNorm is not implemented, and using running statistics in training mode would differ "
                               "from the reference)")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError("v2v_amd.hyper.DynamicUpsampleLayer is inference-only (no autograd through the fused kernels): call it under "
                               "torch.no_grad()")

    def context(self, ev_tensor, prev_recs):
        return self.context_fusion(ev_tensor, prev_recs)

    def atoms(self, ev_tensor, prev_recs):
        return self.dynamic_atom_generation(self.context(ev_tensor, prev_recs))

    def forward(self, x, ev_tensor, prev_recs, skip=None):
        self._check_mode(x)
        if tuple(ev_tensor.shape[-2:]) != (8 * x.shape[-2], 8 * x.shape[-1]) or tuple(prev_recs.shape[-2:]) != tuple(ev_tensor.shape[-2:]):
            raise ValueError(f"the 1/4-scale context must meet the x2-upsampled input: events / prev_recs must be 8x the size of x "
                             f"(x {tuple(x.shape[-2:])}, events {tuple(ev_tensor.shape[-2:])}, prev_recs {tuple(prev_recs.shape[-2:])})")
        x, skip, nhwc_io = _fold_sum_skip(x, skip)
        if self.training:                                                # trainable (else _check_mode raised): BatchNorm on batch statistics
            train = torch.is_grad_enabled()
            xn, sn = _nhwc_in(x, nhwc_io, train), None if skip is None else skip.permute(0, 2, 3, 1)
            if train:
                fus, gen, dyn = self.context_fusion, self.dynamic_atom_generation, self.dynamic_conv
                net = gen.bases_net
                out = DynamicUpsampleFn.apply(xn, sn, ev_tensor, prev_recs, fus.conv.weight, fus.conv.bias, net[0].weight, net[0].bias, net[1].weight,
                                              net[1].bias, net[3].weight, net[3].bias, net[4].weight, net[4].bias, dyn.compositional_coefficients,
                                              dyn.bias, self)
            else:
                out = DynamicUpsampleFn.kernels(xn, sn, ev_tensor, prev_recs, self)[0]
            return _nchw_out(out, x, nhwc_io)
        xn, sn = _nhwc_in(x, nhwc_io, False), None if skip is None else skip.permute(0, 2, 3, 1)
        atoms = self.atoms(ev_tensor, prev_recs)
        out = self.dynamic_conv(upsample2x_nhwc(xn, sn), atoms, relu=self.relu)
        return _nchw_out(out, x, nhwc_io)


class UNetRecurrent(_unet.UNetRecurrent):
    """model/hyper_model.py:138-196: v2v_amd.unet.UNetRecurrent whose decoders[0] is the DynamicUpsampleLayer when use_dynamic_decoder is
    true.  forward(x, prev_recs=None) -> {'image'}; prev_recs None = zeros.  trainable: as the base class, and for the dynamic decoder."""

    def __init__(self, unet_kwargs, trainable: bool = False):
        kw = dict(unet_kwargs)
        self_dynamic = bool(kw.pop("use_dynamic_decoder", False))
        if kw.get("num_output_channels", 1) != 1:
            raise ValueError("the device kernels cover num_output_channels 1 (no flow head)")
        if kw.get("kernel_size", 5) != 5 or kw.get("base_num_channels") != 32 or kw.get("channel_multiplier", 2) != 2:
            raise ValueError("the device kernels cover kernel_size 5, base_num_channels 32, channel_multiplier 2 (config/train_v2v_hyper_10k.yaml)")
        if self_dynamic and kw.get("num_encoders") != 3:
            raise ValueError("the dynamic decoder needs num_encoders 3: its 1/4-scale context meets decoders[0]'s output only at three levels")
        super().__init__(kw, trainable=trainable)
        self.use_dynamic_decoder = self_dynamic
        if self_dynamic:
            k = self.kernel_size
            self.decoders[0] = DynamicUpsampleLayer(self.encoder_output_sizes[-1], self.encoder_input_sizes[-1], kernel_size=k, padding=k // 2,
                                                    in_fuse_channels=1 + self.num_bins, trainable=trainable)

    def _decode(self, head, blocks, ev_tensor=None, prev_recs=None):
        x = blocks[-1]
        for resblock in self.resblocks:
            x = resblock(x)
        for i, decoder in enumerate(self.decoders):
            skip = blocks[self.num_encoders - i - 1]
            if isinstance(decoder, DynamicUpsampleLayer):
                x = decoder(x, ev_tensor, prev_recs, skip=skip)            # model/hyper_model.py:184-185
            else:
                x = decoder(x, skip)
        img = self.pred(x, head)
        if self.final_activation is not None:
            img = self.final_activation(img)
        return img

    def check_input(self, x):
        if self.training and not self.trainable:
            raise RuntimeError("v2v_amd.hyper.UNetRecurrent is inference-only and runs BatchNorm on its running statistics: call .eval() first")
        if x.dim() != 4 or x.shape[-2] % 16 != 0 or x.shape[-1] % 16 != 0 or x.shape[-2] < 16 or x.shape[-1] < 16:
            raise ValueError(f"H and W must be multiples of 16 (got {tuple(x.shape)}): pad the events first")

    def forward(self, x, prev_recs=None):
        self.check_input(x)
        out_dtype = _out_dtype(x)
        if prev_recs is None:
            prev_recs = torch.zeros((x.shape[0], 1) + tuple(x.shape[-2:]), dtype=torch.float32, device=x.device)
        head, blocks = self._encode(x, None)
        return {"image": self._decode(head, blocks, x, prev_recs).to(out_dtype)}

    def forward_sequence(self, *args, **kwargs):
        raise ValueError("step t + 1's decoder reads step t's image: use HyperE2VID.forward_sequence (the plain step loop)")


class HyperE2VID(nn.Module):
    """model/hyper_model.py:198-237: `unetrecurrent` + states / reset_states + the previous reconstruction fed back into the dynamic
    decoder.  YAML target v2v_amd.hyper.HyperE2VID (params: {unet_kwargs: .., trainable: true} to train it, as for E2VIDRecurrent).
    trainable=False: call .eval() and run under torch.no_grad().  trainable=True: .train() under grad records every layer's backward;
    prev_recs is detached and mixed with gt_image in plain torch, so nothing flows back through the context's inputs."""

    def __init__(self, unet_kwargs, trainable: bool = False):
        super().__init__()
        self.trainable = bool(trainable)
        self.num_bins = unet_kwargs["num_bins"]
        self.num_encoders = unet_kwargs["num_encoders"]
        self.unetrecurrent = UNetRecurrent(unet_kwargs, trainable=trainable)
        self.prev_recs = None

    @property
    def states(self):
        return _unet.copy_states(self.unetrecurrent.states)

    @states.setter
    def states(self, states):
        self.unetrecurrent.states = states

    def reset_states(self):
        self.unetrecurrent.states = [None] * self.unetrecurrent.num_encoders
        self.prev_recs = None

    def forward(self, event_tensor, gt_image=None, beta=0):
        """event_tensor [N, num_bins, H, W] (H, W multiples of 16) -> {'image': [N,1,H,W]}; the image (detached) is the next call's
        prev_recs, mixed with gt_image when beta > 0 (model/hyper_model.py:229-236)."""
        self.unetrecurrent.check_input(event_tensor)
        if self.prev_recs is None:
            self.prev_recs = torch.zeros((event_tensor.shape[0], 1) + tuple(event_tensor.shape[-2:]), device=event_tensor.device)
        if gt_image is not None and beta > 0:
            prev_recs = self.prev_recs * (1 - beta) + gt_image.detach() * beta
        else:
            prev_recs = self.prev_recs
        output_dict = self.unetrecurrent.forward(event_tensor, prev_recs)
        self.prev_recs = output_dict["image"].detach()
        return output_dict

    def forward_sequence(self, events, out=None):
        """events [N,T,num_bins,H,W] -> images [N,T,1,H,W]: the plain step loop on the caller's stream (step t + 1's decoder needs step t's
        image, so the decoder halves cannot run beside one another as E2VIDRecurrent's do); bit-identical to T calls of forward()."""
        n, t_steps = _unet._sequence_shape(events)
        self.unetrecurrent.check_input(events[:, 0])
        if out is None:
            out = torch.empty((n, t_steps, 1) + tuple(events.shape[-2:]), dtype=_out_dtype(events), device=events.device)
        for t in range(t_steps):
            out[:, t] = self.forward(events[:, t])["image"]
        return out
