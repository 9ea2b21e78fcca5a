"""The recurrent UNet's layers on the matrix cores: host side of v2v_convlstm_step_hip, v2v_conv_nhwc_hip and
v2v_upsample2x_nhwc_hip.

    ConvLSTM(input_size, hidden_size, kernel_size)        model/submodules.py:179-235 -- same constructor, same `Gates`
                                                          parameter names (state_dicts load unchanged), same
                                                          forward(input_, prev_state=None) -> (hidden, cell)
    ResidualBlock(in_channels, out_channels)              model/submodules.py:143-177 (norm=None): `conv1` / `conv2`
    ConvLayer(in, out, kernel_size, stride, padding, activation, norm=None, upsample=False)
                                                          model/submodules.py:6-33, and :68-96 (UpsampleConvLayer) with
                                                          upsample=True; `conv2d`; forward(x, skip=None) folds the sum skip
    ConvGRU(input_size, hidden_size, kernel_size)         model/submodules.py:238-278 -- same constructor, same `reset_gate` / `update_gate` /
                                                          `out_gate` parameters, forward(input_, prev_state) -> new_state; inference only
    convlstm_step / conv_nhwc / conv3x3_nhwc / upsample2x_nhwc     the raw NHWC bfloat16 operators (v2v_amd/nhwc_ops.py, re-exported here)
    convgru_step / pack_gru_weights                        the ConvGRU step (two launches: gates, candidate) and its packing
    conv1x1_nhwc                                           the 1x1 prediction layer on skip_sum(x, head) (ConvLayer with kernel_size 1)
    conv_head_nhwc / to_nhwc8_bf16 / pack_head_weights     the head (voxel bins -> 32 channels; ConvLayer with <= 8 input channels)
    convgru16_step / resblock16_nhwc / conv_head16_nhwc    the 16-channel layers (FireNet): ConvGRU(16, 16, 3), ResidualBlock(16, 16) and
                                                           ConvLayer(<= 8, 16, 3, padding=1), one launch each, any H and W
    conv_stem_nhwc / pack_stem_weights / upsample2x_cat_nhwc   the plain UNet (EVFlowNet): its stem (voxel bins -> 64, 3x3, stride 2) and concat skips
    pack_gate_weights / pack_conv_weights                  one-off weight packing
    nchw_to_nhwc_bf16(x, relu=False)                      layout change in front of them (not needed for channels-last bf16 input)

The 3x3 gate convolution runs as an implicit GEMM on the bf16 matrix cores with fp32 accumulation and the gate / cell / hidden
update fused on the accumulators (v2v_amd/csrc/v2v_convlstm.hpp).  Inference only by default (a call that would need a gradient
raises); trainable=True on a layer records its backward kernels under grad (v2v_amd/train.py).  No fallback: shapes the kernel does not take (hidden_size % 64, H*W % 4, kernel_size
!= 3, input_size != hidden_size) raise ValueError.

How the layers are put together: every layer has `_packed` (the cache of nhwc_ops.packed_weights, the one place that decides when a packed
copy is stale) and `_weights()` (everything its forward needs packed, made or found current on the current stream; a network calls it on
every submodule that has one before it forks streams).  ConvLayer is six layers -- `role`: pred, head, head16, stem, conv, upconv -- told
apart once, in its constructor; ConvLayer._ROLES gives each role its weight packing, its autograd Function and the method forward hands
over to after the argument checks.  _fold_sum_skip (the sum skip in front of a kernel that can add it) and _out_dtype (the dtype a network
hands its prediction out in) are shared with v2v_amd/unet.py and v2v_amd/hyper.py.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .nhwc_ops import (_to_nhwc_bf16, conv1x1_nhwc, conv3x3_nhwc, conv_head16_nhwc, conv_head_nhwc, conv_nhwc, conv_stem_nhwc, convgru16_step, convgru_step,  # noqa: F401
                       convlstm_step, nchw_to_nhwc_bf16, pack_conv3x3_weights, pack_conv_weights, pack_gate_weights, pack_gru16_weights, pack_gru_weights,
                       pack_head16_weights, pack_head_weights, pack_resblock16_weights, pack_stem_weights, packed_weights, resblock16_nhwc,
                       to_nhwc8_bf16, upsample2x_cat_nhwc, upsample2x_nhwc)
from .train import ConvFn, ConvLSTMFn, PredFn, ResidualBlockFn, UpConvFn, VoxelConvFn


def _training(layer, x) -> bool:
    """Decided once at the top of every layer's forward: True = record the layer's autograd Function (trainable=True under grad), False =
    run its kernels plainly.  A call that would need a gradient through a layer that is not trainable raises."""
    if not torch.is_grad_enabled():
        return False
    if not layer.trainable and (x.requires_grad or any(p.requires_grad for p in layer.parameters())):
        raise RuntimeError(f"v2v_amd.convlstm.{type(layer).__name__} is inference-only (no autograd through the fused kernel): "
                           "call it under torch.no_grad() / in eval mode, or build it with trainable=True")
    return layer.trainable


def _is_channels_last(v) -> bool:
    """The head's test on its input and weight, of any dtype."""
    return v.is_contiguous(memory_format=torch.channels_last) and not v.is_contiguous()


def _is_nhwc_bf16(v) -> bool:
    """A channels-last bfloat16 tensor (a network run in torch.channels_last under autocast): its memory IS the kernels' NHWC layout, so it
    is consumed as a view (no layout-change kernel) and the result goes out as a channels-last view of the kernel's own NHWC buffer."""
    return v.dtype == torch.bfloat16 and v.dim() == 4 and v.is_contiguous(memory_format=torch.channels_last) and not v.is_contiguous()


def _nhwc_in(x: torch.Tensor, nhwc: bool, train: bool, relu: bool = False) -> torch.Tensor:
    """[B,C,H,W] -> a contiguous bfloat16 [B,H,W,C] tensor (optionally through ReLU).  nhwc = _is_nhwc_bf16(x), which every caller needs
    for the way back too: such a tensor goes in as the view of its memory; anything else through the layout kernel (_to_nhwc_bf16) when
    not training, and under training through differentiable torch ops that round to bfloat16 the same values the layout kernel writes."""
    if nhwc:
        x = x.permute(0, 2, 3, 1)
    elif not train:
        return _to_nhwc_bf16(x, relu=relu)
    else:
        x = x.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()
    return torch.relu(x) if relu else x


def _fold_sum_skip(x, skip):
    """The sum skip in front of a layer whose kernel can add it while it reads: -> (x, skip, nhwc).  Both operands NHWC bfloat16: they go
    in as they are.  Anything else: added here first, skip = None.  nhwc = _is_nhwc_bf16 of the x that comes back."""
    nhwc = _is_nhwc_bf16(x)
    if skip is not None and not (nhwc and _is_nhwc_bf16(skip)):
        x, skip = x + skip, None
        nhwc = _is_nhwc_bf16(x)
    return x, skip, nhwc


def _out_dtype(x: torch.Tensor) -> torch.dtype:
    """What a network hands its prediction out in: the input's dtype, bfloat16 under autocast."""
    return torch.bfloat16 if (x.dtype == torch.bfloat16 or torch.is_autocast_enabled()) else x.dtype


def _nchw_out(out: torch.Tensor, like: torch.Tensor, nhwc_io: bool) -> torch.Tensor:
    """The way back: the kernel's [B,H,W,C] buffer as a channels-last [B,C,H,W] view when the input was NHWC (nhwc_io), else as a
    contiguous NCHW tensor in the input's (`like`'s) dtype."""
    out = out.permute(0, 3, 1, 2)
    return out if nhwc_io else out.contiguous().to(like.dtype)


class ConvLSTM(nn.Module):
    """Drop-in for model/submodules.py:ConvLSTM (:179-235) on the fused kernel.

    forward(input_, prev_state=None) -> (hidden, cell), both logically [B,C,H,W] as in the reference: `hidden` is a
    contiguous NCHW tensor in the input's dtype (float32, or bfloat16 under autocast -- the reference's state takes the
    input's dtype too, :202-203); `cell` is the kernel's float32 NHWC cell buffer seen through permute(0,3,1,2) (a
    channels-last tensor; float32 even under autocast: the cell state is never rounded to bf16).  A bfloat16 input that is
    channels-last (torch.channels_last networks under autocast) is consumed and produced in place: `hidden` is then a
    channels-last view of the kernel's NHWC buffer and no layout-change kernel runs.  The bf16 NHWC copy of `hidden` that the next step's matrix-core GEMM reads is
    kept beside it and reused when the (hidden, cell) pair comes back untouched (UNetRecurrent.forward, model/unet.py:293-296);
    any other prev_state (cloned, loaded, edited) is converted from its float32 values, which gives the same bits."""

    def __init__(self, input_size, hidden_size, kernel_size, trainable: bool = False):
        super().__init__()
        if kernel_size != 3 or input_size != hidden_size:
            raise ValueError("the fused ConvLSTM covers the configuration the reference instantiates "
                             "(model/submodules.py:112: input_size == hidden_size, kernel_size=3)")
        self.input_size, self.hidden_size = input_size, hidden_size
        self.Gates = nn.Conv2d(input_size + hidden_size, 4 * hidden_size, kernel_size, padding=kernel_size // 2)
        self._packed = {}                                              # nhwc_ops.packed_weights' cache
        self._h_cache = None                                           # (hidden tensor, its version, bf16 NHWC twin)
        self.trainable = trainable                                     # True: under grad, forward records v2v_amd.train.ConvLSTMFn
        # trainable, under grad: the hidden state's consumers each get their OWN output of ConvLSTMFn (same values), so that their
        # gradients meet in fp32 inside its backward instead of in a bf16 sum made by autograd: the layer downstream (`hidden`),
        # the next step (the cached twin) and -- when a network asks for it (UNetRecurrent: the decoder's sum skip) -- skip_twin(hidden)
        self.wants_skip_twin = False
        self._skip_twin = None                                         # (hidden tensor, its twin for the skip connection)

    def _weights(self):
        """Everything forward needs packed, now (on the current stream): the gate weights' packed stream."""
        return packed_weights(self._packed, "Gates", self.Gates.weight, pack_gate_weights)

    def forward(self, input_, prev_state=None, input_relu: bool = False):
        """input_relu=True takes the PRE-activation output of the convolution in front (RecurrentConvLayer.conv,
        model/submodules.py:110-116) and applies its ReLU on the way in: inside the layout-change kernel / on the NHWC view, or under
        training inside ConvLSTMFn (which masks dx with it)."""
        train = _training(self, input_)
        nhwc_io = _is_nhwc_bf16(input_)
        x = _nhwc_in(input_, nhwc_io, train, relu=input_relu and not train)
        h_prev = c_prev = None
        if prev_state is not None:
            hidden, cell = prev_state
            cache = self._h_cache
            if cache is not None and cache[0] is hidden and cache[1] == hidden._version:
                h_prev = cache[2]
            else:
                h_prev = _nhwc_in(hidden, _is_nhwc_bf16(hidden), train)
            c_prev = cell.permute(0, 2, 3, 1)
            if c_prev.dtype != torch.float32 or not c_prev.is_contiguous():
                c_prev = c_prev.float().contiguous()
        nchw_dtype = None if nhwc_io else input_.dtype
        if train:
            n_twins = 2 if (nhwc_io and self.wants_skip_twin) else 1
            outs = ConvLSTMFn.apply(x, h_prev, c_prev, self.Gates.weight, self.Gates.bias, self, nchw_dtype, bool(input_relu), n_twins)
            h_state, c_state, twins, h_nchw = outs[0], outs[1], outs[2:2 + n_twins], None if nhwc_io else outs[2 + n_twins]
        else:
            h_state, c_state, h_nchw = ConvLSTMFn.kernels(x, h_prev, c_prev, self, self.Gates.bias.detach().float(), nchw_dtype)
            twins = (h_state,)
        hidden_out = h_state.permute(0, 3, 1, 2) if nhwc_io else h_nchw
        self._h_cache = (hidden_out, hidden_out._version, twins[0])    # the next step's h_prev (training: its own output of the Function)
        if train:
            self._skip_twin = (hidden_out, twins[1].permute(0, 3, 1, 2)) if n_twins == 2 else None
        return hidden_out, c_state.permute(0, 3, 1, 2)

    def skip_twin(self, hidden):
        """The tensor a skip connection should read for `hidden` (the last forward's output): its own twin output under training (see
        wants_skip_twin), `hidden` itself otherwise.  Same values either way."""
        tw = self._skip_twin
        return tw[1] if tw is not None and tw[0] is hidden else hidden


def clone_state(t: torch.Tensor) -> torch.Tensor:
    """detach().clone() of one state tensor that keeps what a ConvGRU state carries beside its values: the float32 master (and its bfloat16
    NHWC twin), cloned too, so that a state read through a network's `states` property and assigned back continues bit for bit."""
    out = t.detach().clone()
    tag = getattr(t, "_v2v_gru", None)
    if tag is not None and tag[2] == t._version:
        out._v2v_gru = (tag[0].clone(), tag[1].clone(), out._version)
    return out


class ConvGRU(nn.Module):
    """Drop-in for model/submodules.py:ConvGRU (:238-278) on the two-launch matrix-core step (v2v_amd/csrc/v2v_convgru.hpp).

    forward(input_, prev_state) -> new_state, logically [B,C,H,W] as in the reference, handed out as ConvLSTM hands out its hidden output:
    a contiguous NCHW tensor in the input's dtype (float32, or bfloat16 under autocast), or -- for a channels-last bfloat16 input -- a
    channels-last view of the kernel's own NHWC buffer.  The hidden state is carried in float32 (a precision choice of this kernel, as the
    LSTM's float32 cell state is): the returned tensor carries that master and its bfloat16 NHWC twin as an attribute, and a state that
    comes back untouched continues from them.  Any other prev_state (cloned, loaded, edited in place) is taken at its own values: widened
    to float32, which for a float32 state gives the same bits (v2v_amd.convlstm.clone_state / v2v_amd.unet.copy_states keep the master).
    Inference only: the step has no backward kernel yet (trainable=True raises)."""

    def __init__(self, input_size, hidden_size, kernel_size, trainable: bool = False):
        super().__init__()
        if kernel_size != 3 or input_size != hidden_size:
            raise ValueError("the fused ConvGRU covers the configuration the reference instantiates "
                             "(model/submodules.py:112: input_size == hidden_size, kernel_size=3)")
        if trainable:
            raise ValueError("ConvGRU is inference-only: the ConvGRU step has no backward kernel (train with recurrent_block_type 'convlstm')")
        self.input_size, self.hidden_size = input_size, hidden_size
        pad = kernel_size // 2
        self.reset_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=pad)
        self.update_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=pad)
        self.out_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=pad)
        for conv in (self.reset_gate, self.update_gate, self.out_gate):          # the reference's initialisation (:253-258)
            nn.init.orthogonal_(conv.weight)
            nn.init.constant_(conv.bias, 0.0)
        self._packed = {}
        self.trainable = False
        self.wants_skip_twin = False                                           # ConvLSTM's training-only switch: nothing to do here
        self.narrow = hidden_size == 16                                        # FireNet's width: the one-launch step (convgru16_step)

    def _weights(self):
        """Everything forward needs packed, now (on the current stream): ((gates stream, candidate stream), gates bias [2C], out bias [C]),
        repacked when any of the six parameters changed (another tensor, an in-place update, another device)."""
        u, r, o = self.update_gate, self.reset_gate, self.out_gate
        return packed_weights(self._packed, "gru", (u.weight, r.weight, o.weight, u.bias, r.bias, o.bias), self._pack)

    def _pack(self, w_u, w_r, w_o, b_u, b_r, b_o):
        pack = pack_gru16_weights if self.narrow else pack_gru_weights
        return pack(w_u, w_r, w_o), torch.cat([b_u, b_r]).float().contiguous(), b_o.float().contiguous()

    def forward(self, input_, prev_state=None, input_relu: bool = False):
        """input_relu=True takes the PRE-activation output of the convolution in front and applies its ReLU on the way in (as ConvLSTM)."""
        _training(self, input_)                                                # raises under grad: inference only
        nhwc_io = _is_nhwc_bf16(input_)
        x = _nhwc_in(input_, nhwc_io, False, relu=input_relu)
        h_prev = h_prev32 = None
        if prev_state is not None:
            tag = getattr(prev_state, "_v2v_gru", None)
            if tag is not None and tag[2] == prev_state._version and tag[0].device == x.device and tuple(tag[0].shape) == tuple(x.shape):
                h_prev32, h_prev = tag[0], tag[1]
            else:
                h_prev32 = prev_state.detach().permute(0, 2, 3, 1).float().contiguous()
                h_prev = h_prev32.to(torch.bfloat16)
        packed, b_gates, b_out = self._weights()
        nchw_dtype = None if nhwc_io else input_.dtype
        if self.narrow:
            outs = convgru16_step(x.contiguous(), h_prev, h_prev32, packed, b_gates, b_out, nchw_dtype=nchw_dtype)
        else:
            outs = convgru_step(x, h_prev, h_prev32, packed, b_gates, b_out, nchw_dtype=nchw_dtype)
        state = outs[0].permute(0, 3, 1, 2) if nhwc_io else outs[-1]             # (h bf16, h float32, .., h as NCHW when nchw_dtype is given)
        state._v2v_gru = (outs[1], outs[0], state._version)
        return state

    def skip_twin(self, hidden):
        return hidden


class ResidualBlock(nn.Module):
    """Drop-in for model/submodules.py:ResidualBlock (:143-177) as E2VID instantiates it (model/unet.py:48: in == out channels,
    stride 1, no downsample, norm=None): relu(conv2(relu(conv1(x))) + x), both convolutions on the matrix-core kernel with the
    bias / residual / ReLU in its epilogue.  Same parameter names (conv1, conv2).  Inference by default, trainable=True records its backward under grad; bfloat16 operands with fp32
    accumulation; a channels-last bfloat16 input is consumed and produced in place, anything else goes through the
    layout-change kernel and comes back NCHW in the input's dtype."""

    def __init__(self, in_channels, out_channels, stride=1, downsample=None, norm=None, BN_momentum=0.1, trainable: bool = False):
        super().__init__()
        if stride != 1 or downsample is not None or norm is not None or in_channels != out_channels:
            raise ValueError("the fused ResidualBlock covers the configuration E2VID instantiates "
                             "(model/unet.py:48: in_channels == out_channels, stride 1, no downsample, norm=None)")
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=True)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=True)
        self._packed = {}
        self.narrow = in_channels == 16                                # FireNet's width: both convolutions in one launch (resblock16_nhwc)
        if self.narrow and trainable:
            raise ValueError("ResidualBlock(16, 16) is inference-only: the one-launch 16-channel block has no backward kernel")
        self.trainable = trainable                                     # True: under grad, forward records v2v_amd.train.ResidualBlockFn

    def _weights(self):
        """Everything forward needs packed, now (on the current stream): (conv1's, conv2's) packed streams (16 channels: one stream of both)."""
        if self.narrow:
            return packed_weights(self._packed, "both", (self.conv1.weight, self.conv2.weight), pack_resblock16_weights)
        return (packed_weights(self._packed, "conv1", self.conv1.weight, pack_conv_weights),
                packed_weights(self._packed, "conv2", self.conv2.weight, pack_conv_weights))

    def forward(self, x):
        train = _training(self, x)
        nhwc_io = _is_nhwc_bf16(x)
        xn = _nhwc_in(x, nhwc_io, train)
        if self.narrow:
            out = resblock16_nhwc(xn.contiguous(), self._weights(), self.conv1.bias, self.conv2.bias)
        elif train:
            out = ResidualBlockFn.apply(xn, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias, self)
        else:
            out = ResidualBlockFn.kernels(xn, self)[0]
        return _nchw_out(out, x, nhwc_io)


class ConvLayer(nn.Module):
    """Drop-in for model/submodules.py:ConvLayer (:6-33) as the recurrent UNet builds its encoder / decoder convolutions
    (model/unet.py: kernel_size 5, padding 2, stride 2 or 1, activation 'relu' or None, norm=None): same constructor, same
    `conv2d` parameter, convolution + bias + ReLU in one matrix-core kernel.  upsample=True puts the bilinear x2 upsampling
    (f.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False), its own bfloat16 NHWC kernel) in front, i.e.
    UpsampleConvLayer (:68-96).  Inference by default, trainable=True records its backward under grad; bfloat16 operands, fp32 accumulation; channels-last bfloat16
    inputs are consumed and produced in place, anything else goes through the layout-change kernel and comes back NCHW in the
    input's dtype.  in_channels % 64 == 0 and out_channels in {32, 64, 128, 256k}; in_channels 32 with 64 / 128 outputs (the first
    encoder); <= 8 input channels with 32 outputs, stride 1 = the head (with 16 outputs, kernel_size 3 = FireNet's head, any H and W), with 64 outputs, kernel_size 3, stride 2 = the plain UNet's stem;
    kernel_size 1 = the prediction layer; else ValueError (no fallback)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, activation="relu", norm=None, BN_momentum=0.1,
                 upsample=False, trainable: bool = False):
        super().__init__()
        if norm is not None or activation not in ("relu", None) or kernel_size not in (1, 3, 5) or padding != kernel_size // 2 or stride not in (1, 2) \
                or (kernel_size == 1 and (stride != 1 or activation is not None or upsample or out_channels > 3)):
            raise ValueError("the fused ConvLayer covers norm=None, activation 'relu' or None, kernel_size 3 or 5 with padding "
                             "kernel_size // 2, stride 1 or 2, and the 1x1 prediction layer (stride 1, no activation, <= 3 outputs)")
        self.conv2d = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=True)
        self.relu, self.upsample = activation == "relu", upsample
        # the plain UNet's stem (model/unet.py:320-326): voxel bins -> 64 channels, 3x3, stride 2
        self.stem = in_channels <= 8 and kernel_size == 3 and stride == 2 and out_channels == 64 and not upsample
        self.head = in_channels <= 8 and kernel_size in (3, 5) and not self.stem   # the recurrent UNet's head: voxel bins -> 32 channels
        self.head16 = self.head and kernel_size == 3 and out_channels == 16 and stride == 1 and not upsample   # FireNet's head: voxel bins -> 16
        if self.head and not self.head16 and (out_channels != 32 or stride != 1 or upsample):
            raise ValueError("with <= 8 input channels the fused ConvLayer is the recurrent UNet's head (32 output channels, stride 1) or the "
                             "plain UNet's stem (64 output channels, kernel_size 3, stride 2)")
        if self.head16 and trainable:
            raise ValueError("ConvLayer(<= 8, 16, 3) is inference-only: the 16-channel head has no backward kernel")
        # which of the six layers this is, decided here once: _ROLES (below the methods) gives its weight packing, its Function and its method
        self.role = ("pred" if kernel_size == 1 else "stem" if self.stem else "head16" if self.head16 else "head" if self.head
                     else "upconv" if upsample else "conv")
        self.force_channels_last = False          # head / stem only: hand out the kernel's NHWC buffer as a channels-last view whatever came in
        self._packed = {}                         # nhwc_ops.packed_weights' cache
        self.trainable = trainable                # True: under grad, forward records the role's v2v_amd.train Function

    def _weights(self):
        """Everything forward needs packed, now (on the current stream): the convolution's packed stream (None for the 1x1 prediction
        layer: its kernel reads the float32 weight)."""
        pack = self._ROLES[self.role][0]
        return packed_weights(self._packed, "conv2d", self.conv2d.weight, pack) if pack is not None else None

    def forward(self, x, skip=None, scales=None, skip_type="sum"):
        """skip (upsample=True only): the sum skip connection model/unet.py:304 adds in front of the decoder, folded into the
        upsampling kernel -- layer(x, skip) == layer(x + skip).  Under training the fusions are differentiated as fused (the skip into
        the upsampling, pred(x + head)).  skip_type "concat" (upsample=True only): layer(x, skip) == layer(cat(x, skip)), the plain UNet's
        concat skip (model/unet.py:350) -- each source is upsampled into its channel slice, the low-resolution cat is never written.
        Every argument check stands here; the role's own method below it only runs kernels."""
        train = _training(self, x)
        role, cat = self.role, skip_type == "concat"
        if skip_type not in ("sum", "concat") or (cat and (not self.upsample or skip is None)):
            raise ValueError("skip_type is 'sum' or 'concat'; 'concat' is the decoder's (upsample=True) skip and needs one")
        if scales is not None and not (self.head or self.stem):
            # only the head kernel (<= 8 input channels, 3x3 / 5x5) divides by normalize_batch_voxel's scales while it reads; anything else
            # would silently run on raw, un-normalised events (RingLoader(normalize='scales') hands out raw voxels)
            raise ValueError("`scales` is applied by the head kernel only (in_channels <= 8, kernel 3 or 5): normalise the events first "
                             "(v2v_amd.postops.apply_scales / RingLoader(normalize=True)) for this layer")
        if skip is not None and not self.upsample and role != "pred":
            raise ValueError("skip is the decoder's (upsample=True) sum skip connection")
        if train and x.requires_grad and (self.head or self.stem):
            raise ValueError("the trainable head / stem computes no gradient for its input (the voxel grid)")
        if cat and self.conv2d.in_channels != x.shape[1] + skip.shape[1]:
            raise ValueError(f"concat skip: conv2d.in_channels {self.conv2d.in_channels} != {x.shape[1]} + {skip.shape[1]}")
        _, fn, run = self._ROLES[role]
        return run(self, fn, x, skip, scales, train, cat)

    def _run_pred(self, fn, x, skip, scales, train, cat):
        """pred(skip_sum(x, head)), model/unet.py:307.  Training: float32 out (the bf16 kernel values widened exactly; with a float32 input
        the inference path's dtype too): the loss gradient then reaches the backward kernel unrounded -- UNetRecurrent.forward's
        .to(out_dtype) gives the inference bits."""
        conv, x_in = self.conv2d, x
        x, skip, nhwc = _fold_sum_skip(x, skip)
        nhwc = nhwc and x is x_in                                   # a sum made here goes through the layout kernel, whatever its layout
        xn, sn = _nhwc_in(x, nhwc, train), None if skip is None else skip.permute(0, 2, 3, 1)
        out_dtype = torch.bfloat16 if nhwc else x.dtype
        out = fn.apply(xn, sn, conv.weight, conv.bias, self, out_dtype) if train else fn.kernels(xn, sn, self, out_dtype)
        return _nchw_out(out, x, nhwc)

    def _run_voxel(self, fn, x, skip, scales, train, cat):
        """head / head16 / stem (model/unet.py:77-78 / :320-326): any float layout in, bf16 out; channels-last out when the input or (as
        torch's own convolution decides) the weight is channels-last."""
        conv = self.conv2d
        low = x.dtype == torch.bfloat16 or (x.is_cuda and torch.is_autocast_enabled())
        cl = self.force_channels_last or _is_channels_last(x) or _is_channels_last(conv.weight)
        x8 = to_nhwc8_bf16(x.detach().float(), scales)
        out = (fn.apply(x8, conv.weight, conv.bias, self) if train else fn.kernels(x8, self)).permute(0, 3, 1, 2)
        out = out if cl else out.contiguous()
        return out if low else out.to(x.dtype)

    def _run_conv(self, fn, x, skip, scales, train, cat):
        nhwc_io = _is_nhwc_bf16(x)
        xn = _nhwc_in(x, nhwc_io, train)
        out = fn.apply(xn, self.conv2d.weight, self.conv2d.bias, self) if train else fn.kernels(xn, self)
        return _nchw_out(out, x, nhwc_io)

    def _run_upconv(self, fn, x, skip, scales, train, cat):
        conv = self.conv2d
        if cat:
            nhwc_x, nhwc_skip = _is_nhwc_bf16(x), _is_nhwc_bf16(skip)
            nhwc_io = nhwc_x and nhwc_skip
            xn, sn = _nhwc_in(x, nhwc_x, train), _nhwc_in(skip, nhwc_skip, train)
        else:
            x, skip, nhwc_io = _fold_sum_skip(x, skip)
            xn, sn = _nhwc_in(x, nhwc_io, train), None if skip is None else skip.permute(0, 2, 3, 1)
        out = fn.apply(xn, sn, conv.weight, conv.bias, self, cat) if train else fn.kernels(xn, sn, self, cat)[0]
        return _nchw_out(out, x, nhwc_io)

    # role -> (weight packing | None, autograd Function whose `kernels` is the forward, the method that runs it)
    _ROLES = {"pred": (None, PredFn, _run_pred),
              "head": (pack_head_weights, VoxelConvFn, _run_voxel),
              "head16": (pack_head16_weights, VoxelConvFn, _run_voxel),
              "stem": (pack_stem_weights, VoxelConvFn, _run_voxel),
              "conv": (pack_conv_weights, ConvFn, _run_conv),
              "upconv": (pack_conv_weights, UpConvFn, _run_upconv)}
