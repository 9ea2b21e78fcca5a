"""The raw NHWC bfloat16 operators of the recurrent UNet, forward and backward: one Python function per C entry point of the layer kernels
(v2v_amd/csrc/v2v_convlstm.hpp, v2v_train_tu.hip), plus the packed-weight cache every layer shares (packed_weights: one tensor or a
tuple of tensors as the key, the only implementation).  No nn.Module and no autograd here: v2v_amd/train.py builds the
torch.autograd.Functions on these, v2v_amd/convlstm.py the layers.  Every operator validates with _lib.need and calls its entry point
through _lib.launch (the operand's device, torch's current stream there, status checked) with _lib.ptr arguments: the package's one
calling convention, nothing of it is defined here.

    convlstm_step / conv_nhwc / conv3x3_nhwc / upsample2x_nhwc     the forward operators
    convgru_step / pack_gru_weights                        the ConvGRU step (gates launch + candidate launch) and its packing
    convgru16_step / resblock16_nhwc / conv_head16_nhwc    the 16-channel layers (FireNet), one launch each; pack_gru16_weights /
                                                           pack_resblock16_weights / pack_head16_weights
    conv1x1_nhwc                                           the 1x1 prediction layer on skip_sum(x, head)
    conv_head_nhwc / to_nhwc8_bf16 / pack_head_weights     the head (voxel bins -> 32 channels)
    conv_stem_nhwc / pack_stem_weights / upsample2x_cat_nhwc       the plain UNet (EVFlowNet): stride-2 stem (voxel bins -> 64), concat-skip upsampling
    nam_step / pack_nam_weights                            NER-Net's NAM cell (three launches on the ConvLSTM / ConvGRU tile geometries) and its packing
    conv_head16in_nhwc / to_nhwc16_bf16 / pack_head16in_weights    the head for 9 to 16 input channels (NER-Net: 2 * num_bins = 10 -> 32, 5x5)
    gcb_nhwc / pack_gcb_weights / valid_extent_nhwc        NER-Net's global context block (1x1 convolution + attention pooling + residual, float32
                                                           arithmetic) and the clear / edge-replicate helper of a canvas larger than its valid extent
    pack_gate_weights / pack_conv_weights / pack_dgrad_weights     one-off weight packing; packed_weights = the cache in front of them
    nchw_to_nhwc_bf16(x, relu=False)                      layout change in front of them (not needed for channels-last bf16 input)
    relu_bwd_nhwc / conv_dgrad_nhwc / conv_wgrad_nhwc / upsample2x_bwd_nhwc / upsample2x_cat_bwd_nhwc / conv1x1_bwd_nhwc / convlstm_step_bwd     the backward operators
                                                          (each pinned against a float64 reference of its own operation: tests/test_backward_ops.py)

Activations are bf16 NHWC with fp32 accumulation; activation gradients bf16 NHWC, the cell-state gradient fp32, parameter gradients fp32.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools

import torch

from . import _lib
from ._lib import DTYPE_CODES, launch, need, ptr


_DTYPES = (torch.float32, torch.bfloat16)            # what the layer kernels read and write (codes: _lib.DTYPE_CODES)


def packed_weights(cache: dict, slot: str, tensors, make):
    """The one packed-weight cache: make(*detached tensors), kept in cache[slot] (a layer's `_packed` dict) and made again when ANY source
    tensor changed -- another tensor (load_state_dict into a new parameter), an in-place update (_version: an optimizer step, copy_) or
    another device.  tensors: one tensor, or a tuple of everything the cached value was computed from (a key that leaves one out serves
    stale weights silently)."""
    if type(tensors) is tuple:
        key = tuple([(t.data_ptr(), t._version, t.device) for t in tensors])
    else:
        key = (tensors.data_ptr(), tensors._version, tensors.device)
    hit = cache.get(slot)
    if hit is None or hit[0] != key:
        hit = cache[slot] = (key, make(*[t.detach() for t in tensors]) if type(tensors) is tuple else make(tensors.detach()))
    return hit[1]


@functools.lru_cache(maxsize=None)
def _conv_packed_elems(cin: int, cout: int, ks: int) -> int:
    """v2v_conv_packed_elems (a pure function of three integers), asked once per shape instead of once per launch."""
    return _lib.lib().v2v_conv_packed_elems(cin, cout, ks)


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc_bf16(x: torch.Tensor, relu: bool = False) -> torch.Tensor:
    """float32 or bfloat16 [B,C,H,W] -> bfloat16 [B,H,W,C] (optionally through ReLU) in one HIP kernel."""
    _lib.require_gpu()
    if not x.is_cuda or x.dtype not in _DTYPES or x.dim() != 4:
        raise ValueError("x must be a float32 or bfloat16 CUDA tensor [B,C,H,W]")
    x = x.contiguous()
    b, c, h, w = x.shape
    out = torch.empty((b, h, w, c), dtype=torch.bfloat16, device=x.device)
    launch("v2v_nchw_to_nhwc_bf16_hip", x.device, ptr(x), DTYPE_CODES[x.dtype], b, c, h, w, int(bool(relu)), ptr(out))
    return out


def _to_nhwc_bf16(x: torch.Tensor, relu: bool = False) -> torch.Tensor:
    """[B,C,H,W] float32 / bfloat16 -> a contiguous bfloat16 [B,H,W,C] tensor: the layout kernel where it applies (64-channel x
    64-pixel tiles: C % 64 == 0 and H*W % 64 == 0), one torch copy otherwise -- the same guard for every layer, so an odd
    spatial size does not surface as an opaque V2V_ERR_SHAPE from the kernel."""
    if x.shape[1] % 64 == 0 and (x.shape[2] * x.shape[3]) % 64 == 0:
        return nchw_to_nhwc_bf16(x, relu=relu)
    if relu:
        x = torch.relu(x)
    return x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)


def to_nhwc8_bf16(x, scales=None):
    """float32 [B, C <= 8, H, W] of any strides -> bfloat16 [B, H, W, 8] with the channels zero-padded to 8: the head's input layout.
    scales: optional float32 [B,2] = (neg_max, pos_max) per sample (v2v_amd.postops.scales_from_stats): normalize_batch_voxel's
    where(x > 0, x / pos_max, x / neg_max) (model/train_utils.py:162-166) applied while the voxels are read."""
    _lib.require_gpu()
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] > 8:
        raise ValueError("x must be a float32 CUDA tensor [B, C <= 8, H, W]")
    b, c, h, w = x.shape
    if scales is not None and (scales.dtype != torch.float32 or tuple(scales.shape) != (b, 2) or not scales.is_contiguous() or scales.device != x.device):
        raise ValueError(f"scales must be a contiguous float32 [{b},2] tensor on x's device")
    out = torch.empty((b, h, w, 8), dtype=torch.bfloat16, device=x.device)
    launch("v2v_to_nhwc8_bf16_scaled_hip", x.device, ptr(x), *x.stride(), b, c, h, w, ptr(scales), ptr(out))
    return out


# ---- the ConvLSTM step ------------------------------------------------------------------------------------------------------------------
def pack_gate_weights(weight: torch.Tensor) -> torch.Tensor:
    """Gates.weight float32 [4C, 2C, 3, 3] -> the packed bfloat16 stream the kernel reads (flat tensor)."""
    _lib.require_gpu()
    if not weight.is_cuda or weight.dtype != torch.float32 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) \
            or weight.shape[0] != 2 * weight.shape[1]:
        raise ValueError("weight must be a float32 CUDA tensor [4C, 2C, 3, 3]")
    c = weight.shape[0] // 4
    n = C.c_uint64(0)
    _lib.check(_lib.lib().v2v_convlstm_packed_bytes(c, C.byref(n)))
    packed = torch.empty((n.value // 2,), dtype=torch.bfloat16, device=weight.device)
    launch("v2v_convlstm_pack_weights_hip", weight.device, ptr(weight.detach().contiguous()), c, ptr(packed))
    return packed


def convlstm_step(x, h_prev, c_prev, packed, bias, nchw_dtype=torch.float32, tile_rows: int = 0, c_out=None):
    """One step on NHWC state.  x, h_prev: bfloat16 [B,H,W,C]; c_prev: float32 [B,H,W,C]; h_prev / c_prev None = zero state.
    Returns (h_state bf16 NHWC, c_state fp32 NHWC, h as [B,C,H,W] in nchw_dtype -- float32 / bfloat16 -- or None when
    nchw_dtype is None).  c_out may be c_prev (updated in place)."""
    _lib.require_gpu()
    need("x", x)
    b, h, w, c = x.shape
    for name, t, dt in (("h_prev", h_prev, torch.bfloat16), ("c_prev", c_prev, torch.float32)):
        if t is not None:
            need(name, t, dt, shape=x.shape, device=x.device)
    if bias.dtype != torch.float32 or bias.numel() != 4 * c or packed.dtype != torch.bfloat16 or packed.numel() != 4 * c * 2 * c * 9:
        raise ValueError("bias must be float32 [4C] and packed the output of pack_gate_weights for the same C")
    h_state = torch.empty_like(x)
    c_state = c_out if c_out is not None else torch.empty((b, h, w, c), dtype=torch.float32, device=x.device)
    if nchw_dtype is not None and nchw_dtype not in _DTYPES:
        raise ValueError("nchw_dtype must be torch.float32, torch.bfloat16 or None")
    h_nchw = torch.empty((b, c, h, w), dtype=nchw_dtype, device=x.device) if nchw_dtype is not None else None
    launch("v2v_convlstm_step_hip", x.device, ptr(x), ptr(h_prev), ptr(c_prev), ptr(packed), ptr(bias.detach().contiguous()), b, h, w, c, ptr(h_state),
           ptr(c_state), ptr(h_nchw), DTYPE_CODES.get(nchw_dtype, _lib.F32), tile_rows)
    return h_state, c_state, h_nchw


# ---- the ConvGRU step (model/submodules.py:260-278): two launches behind one call ---------------------------------------------------------
def pack_gru_weights(update_weight, reset_weight, out_weight):
    """update_gate.weight, reset_gate.weight, out_gate.weight (float32 [C, 2C, 3, 3] each) -> (packed gates stream, packed candidate
    stream), flat bfloat16 tensors (layout: v2v_amd/csrc/v2v_convgru.hpp)."""
    _lib.require_gpu()
    ws = (update_weight, reset_weight, out_weight)
    c = update_weight.shape[0] if update_weight.dim() == 4 else 0
    for w in ws:
        if not w.is_cuda or w.dtype != torch.float32 or tuple(w.shape) != (c, 2 * c, 3, 3) or w.device != update_weight.device:
            raise ValueError("the three gate weights must be float32 CUDA tensors [C, 2C, 3, 3] on one device")
    ng, nc = C.c_uint64(0), C.c_uint64(0)
    _lib.check(_lib.lib().v2v_convgru_packed_bytes(c, C.byref(ng), C.byref(nc)))
    pg = torch.empty((ng.value // 2,), dtype=torch.bfloat16, device=update_weight.device)
    pc = torch.empty((nc.value // 2,), dtype=torch.bfloat16, device=update_weight.device)
    launch("v2v_convgru_pack_weights_hip", update_weight.device, *(ptr(w.detach().contiguous()) for w in ws), c, ptr(pg), ptr(pc))
    return pg, pc


def convgru_step(x, h_prev, h_prev_f32, packed, gates_bias, out_bias, nchw_dtype=None, tile_gates: int = 0, tile_cand: int = 0, h_f32_out=None):
    """One ConvGRU step on NHWC state.  x, h_prev: bfloat16 [B,H,W,C]; h_prev_f32: the float32 master of h_prev; both None = zero state.
    packed = pack_gru_weights(...), gates_bias float32 [2C] = update | reset, out_bias float32 [C].
    Returns (h_bf16, h_f32, u, hr[, h as [B,C,H,W] in nchw_dtype when that is not None]): the new state in bfloat16 (what the next step's
    convolutions and the layers downstream read) and float32 (the master the next step's blend reads), the update gate (float32) and
    rne_bf16(h_prev_f32 * reset) -- the two workspaces between the launches.  h_f32_out may be h_prev_f32 (updated in place).
    tile_gates / tile_cand: kernel instance codes 1..5 (include/v2v_hip.h), 0 = by shape."""
    _lib.require_gpu()
    need("x", x)
    b, h, w, c = x.shape
    if (h_prev is None) != (h_prev_f32 is None):
        raise ValueError("h_prev and h_prev_f32 come together (both None: the zero state)")
    for name, t, dt in (("h_prev", h_prev, torch.bfloat16), ("h_prev_f32", h_prev_f32, torch.float32)):
        if t is not None:
            need(name, t, dt, shape=x.shape, device=x.device)
    pg, pc = packed
    if gates_bias.dtype != torch.float32 or gates_bias.numel() != 2 * c or out_bias.dtype != torch.float32 or out_bias.numel() != c \
            or pg.dtype != torch.bfloat16 or pg.numel() != 2 * c * 2 * c * 9 or pc.dtype != torch.bfloat16 or pc.numel() != c * 2 * c * 9:
        raise ValueError("gates_bias must be float32 [2C], out_bias float32 [C] and packed the output of pack_gru_weights for the same C")
    if nchw_dtype is not None and nchw_dtype not in _DTYPES:
        raise ValueError("nchw_dtype must be torch.float32, torch.bfloat16 or None")
    h_bf16, hr = torch.empty_like(x), torch.empty_like(x)
    u = torch.empty((b, h, w, c), dtype=torch.float32, device=x.device)
    h_f32 = h_f32_out if h_f32_out is not None else torch.empty((b, h, w, c), dtype=torch.float32, device=x.device)
    h_nchw = torch.empty((b, c, h, w), dtype=nchw_dtype, device=x.device) if nchw_dtype is not None else None
    launch("v2v_convgru_step_hip", x.device, ptr(x), ptr(h_prev), ptr(h_prev_f32), ptr(pg), ptr(pc), ptr(gates_bias.detach().contiguous()),
           ptr(out_bias.detach().contiguous()), b, h, w, c, ptr(u), ptr(hr), ptr(h_bf16), ptr(h_f32), ptr(h_nchw), DTYPE_CODES.get(nchw_dtype, _lib.F32),
           tile_gates, tile_cand)
    return (h_bf16, h_f32, u, hr) if nchw_dtype is None else (h_bf16, h_f32, u, hr, h_nchw)


# ---- the 16-channel layer family (FireNet, model/model.py:264-311; v2v_amd/csrc/v2v_narrow.hpp): one launch per layer, any B, H, W ---------
def _is_f32_weight(w, shape):
    return w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == shape


def pack_gru16_weights(update_weight, reset_weight, out_weight):
    """update_gate.weight, reset_gate.weight, out_gate.weight (float32 [16, 32, 3, 3] each) -> the packed bfloat16 stream of convgru16_step."""
    _lib.require_gpu()
    ws = (update_weight, reset_weight, out_weight)
    if any(not _is_f32_weight(w, (16, 32, 3, 3)) or w.device != update_weight.device for w in ws):
        raise ValueError("the three gate weights must be float32 CUDA tensors [16, 32, 3, 3] on one device")
    packed = torch.empty((_lib.lib().v2v_convgru16_packed_elems(),), dtype=torch.bfloat16, device=update_weight.device)
    launch("v2v_convgru16_pack_weights_hip", packed.device, *(ptr(w.detach().contiguous()) for w in ws), ptr(packed))
    return packed


def convgru16_step(x, h_prev, h_prev_f32, packed, gates_bias, out_bias, nchw_dtype=None):
    """One ConvGRU(16, 16, 3) step in ONE launch (gates and candidate through LDS; no u / hr workspaces).  x, h_prev: bfloat16 [B,H,W,16];
    h_prev_f32: the float32 master of h_prev; both None = zero state.  gates_bias float32 [32] = update | reset, out_bias float32 [16].
    Returns (h_bf16, h_f32[, h as [B,16,H,W] in nchw_dtype when that is not None]): convgru_step's precision contract."""
    _lib.require_gpu()
    need("x", x, dims="[B,H,W,16]", last=16)
    b, h, w, c = x.shape
    if (h_prev is None) != (h_prev_f32 is None):
        raise ValueError("h_prev and h_prev_f32 come together (both None: the zero state)")
    for name, t, dt in (("h_prev", h_prev, torch.bfloat16), ("h_prev_f32", h_prev_f32, torch.float32)):
        if t is not None:
            need(name, t, dt, shape=x.shape, device=x.device)
    if gates_bias.dtype != torch.float32 or gates_bias.numel() != 32 or out_bias.dtype != torch.float32 or out_bias.numel() != 16 \
            or packed.dtype != torch.bfloat16 or packed.numel() != _lib.lib().v2v_convgru16_packed_elems():
        raise ValueError("gates_bias must be float32 [32], out_bias float32 [16] and packed the output of pack_gru16_weights")
    if nchw_dtype is not None and nchw_dtype not in _DTYPES:
        raise ValueError("nchw_dtype must be torch.float32, torch.bfloat16 or None")
    h_bf16 = torch.empty_like(x)
    h_f32 = torch.empty((b, h, w, c), dtype=torch.float32, device=x.device)
    h_nchw = torch.empty((b, c, h, w), dtype=nchw_dtype, device=x.device) if nchw_dtype is not None else None
    launch("v2v_convgru16_step_hip", x.device, ptr(x), ptr(h_prev), ptr(h_prev_f32), ptr(packed), ptr(gates_bias.detach().contiguous()),
           ptr(out_bias.detach().contiguous()), b, h, w, ptr(h_bf16), ptr(h_f32), ptr(h_nchw), DTYPE_CODES.get(nchw_dtype, _lib.F32))
    return (h_bf16, h_f32) if nchw_dtype is None else (h_bf16, h_f32, h_nchw)


def pack_resblock16_weights(w1, w2):
    """conv1.weight, conv2.weight (float32 [16, 16, 3, 3] each) -> the packed bfloat16 stream of resblock16_nhwc."""
    _lib.require_gpu()
    if not _is_f32_weight(w1, (16, 16, 3, 3)) or not _is_f32_weight(w2, (16, 16, 3, 3)) or w1.device != w2.device:
        raise ValueError("w1 and w2 must be float32 CUDA tensors [16, 16, 3, 3] on one device")
    packed = torch.empty((_lib.lib().v2v_resblock16_packed_elems(),), dtype=torch.bfloat16, device=w1.device)
    launch("v2v_resblock16_pack_weights_hip", w1.device, ptr(w1.detach().contiguous()), ptr(w2.detach().contiguous()), ptr(packed))
    return packed


def resblock16_nhwc(x, packed, b1, b2):
    """out = relu(conv2(relu(conv1(x) + b1)) + b2 + x) on NHWC bfloat16 [B,H,W,16] in ONE launch (ResidualBlock(16, 16), norm=None)."""
    _lib.require_gpu()
    need("x", x, dims="[B,H,W,16]", last=16)
    if b1.numel() != 16 or b2.numel() != 16 or packed.dtype != torch.bfloat16 or packed.numel() != _lib.lib().v2v_resblock16_packed_elems():
        raise ValueError("b1 and b2 must be [16] and packed the output of pack_resblock16_weights")
    b, h, w, _ = x.shape
    out = torch.empty_like(x)
    launch("v2v_resblock16_nhwc_hip", x.device, ptr(x), ptr(packed), ptr(b1.detach().float().contiguous()), ptr(b2.detach().float().contiguous()), b, h, w,
           ptr(out))
    return out


def pack_head16_weights(weight):
    """nn.Conv2d(Cin <= 8, 16, 3, padding=1).weight float32 -> the packed bfloat16 stream of conv_head16_nhwc."""
    _lib.require_gpu()
    if not weight.is_cuda or weight.dtype != torch.float32 or weight.dim() != 4 or weight.shape[0] != 16 or weight.shape[1] > 8 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("weight must be a float32 CUDA tensor [16, Cin <= 8, 3, 3]")
    packed = torch.empty((_lib.lib().v2v_conv_head16_packed_elems(),), dtype=torch.bfloat16, device=weight.device)
    launch("v2v_conv_head16_pack_weights_hip", weight.device, ptr(weight.detach().contiguous()), weight.shape[1], ptr(packed))
    return packed


def conv_head16_nhwc(x8, packed, bias, relu=True):
    """out = [relu](conv3x3(x, pad 1) + bias): x8 [B,H,W,8] bfloat16 (to_nhwc8_bf16) -> [B,H,W,16] bfloat16, any H and W; FireNet's head
    ConvLayer(num_bins, 16, 3, padding=1) (model/model.py:278)."""
    _lib.require_gpu()
    need("x8", x8, dims="[B,H,W,8]", last=8)
    if bias.numel() != 16 or packed.dtype != torch.bfloat16 or packed.numel() != _lib.lib().v2v_conv_head16_packed_elems():
        raise ValueError("bias must be [16] and packed the output of pack_head16_weights")
    b, h, w, _ = x8.shape
    out = torch.empty((b, h, w, 16), dtype=torch.bfloat16, device=x8.device)
    launch("v2v_conv_head16_nhwc_hip", x8.device, ptr(x8), ptr(packed), ptr(bias.detach().float().contiguous()), int(bool(relu)), b, h, w, ptr(out))
    return out


# ---- the convolutions (ConvLayer / UpsampleConvLayer / ResidualBlock, model/submodules.py:6-96, :143-177) on the same matrix-core kernel ---
def pack_conv_weights(weight: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d(Cin, Cout, ks, padding=ks//2).weight float32 [Cout, Cin, ks, ks] (ks 3 or 5) -> the packed bfloat16 stream."""
    _lib.require_gpu()
    if not weight.is_cuda or weight.dtype != torch.float32 or weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError("weight must be a float32 CUDA tensor [Cout, Cin, ks, ks]")
    cout, cin, ks = weight.shape[0], weight.shape[1], weight.shape[2]
    n = _conv_packed_elems(cin, cout, ks)
    if n < 0:
        raise ValueError(f"the convolution kernel does not take {cin} -> {cout} channels, {ks}x{ks}")
    packed = torch.empty((n,), dtype=torch.bfloat16, device=weight.device)
    launch("v2v_conv_pack_weights_hip", weight.device, ptr(weight.detach().contiguous()), cin, cout, ks, ptr(packed))
    return packed


_tile_like_batch = 0            # > 0 inside tile_like_batch(n): conv_nhwc's automatic tile is the one a batch of n images gets


@contextlib.contextmanager
def tile_like_batch(n: int):
    """Inside, every conv_nhwc with the automatic tile runs the kernel instance a batch of `n` images would get (v2v_conv_nhwc_like_hip):
    a batch that folds T time steps of n images then gives every image the bits of its per-step launch (the instances differ in how they
    split K, so in their fp32 summation order)."""
    global _tile_like_batch
    prev, _tile_like_batch = _tile_like_batch, int(n)
    try:
        yield
    finally:
        _tile_like_batch = prev


def conv_nhwc(x, packed, bias, ks: int, stride: int = 1, residual=None, relu=False, tile_rows: int = 0):
    """out = [relu](conv_ks(x, stride, pad ks//2) + bias [+ residual]) on NHWC bfloat16: x [B,Hin,Win,Cin] -> [B,Hout,Wout,Cout]."""
    _lib.require_gpu()
    need("x", x, dims="[B,H,W,Cin]")
    b, hin, win, cin = x.shape
    cout = bias.numel()
    if bias.dtype != torch.float32 or packed.dtype != torch.bfloat16 or packed.numel() != _conv_packed_elems(cin, cout, ks):
        raise ValueError("bias must be float32 [Cout] and packed the output of pack_conv_weights for the same Cin, Cout, ks")
    h, w = (hin - 1) // stride + 1, (win - 1) // stride + 1
    if residual is not None:
        need("residual", residual, shape=(b, h, w, cout), device=x.device)
    out = torch.empty((b, h, w, cout), dtype=torch.bfloat16, device=x.device)
    like = tile_rows == 0 and _tile_like_batch > 0 and _tile_like_batch != b
    launch("v2v_conv_nhwc_like_hip" if like else "v2v_conv_nhwc_hip", x.device, ptr(x), ptr(packed), ptr(bias.detach().contiguous()), ptr(residual),
           int(bool(relu)), b, hin, win, cin, cout, ks, stride, ptr(out), _tile_like_batch if like else tile_rows)
    return out


def pack_conv3x3_weights(weight: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d(Cin, Cout, 3, padding=1).weight float32 [Cout, Cin, 3, 3] -> its packed bfloat16 stream: pack_conv_weights at ks = 3."""
    if weight.dim() == 4 and tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("weight must be a float32 CUDA tensor [Cout, Cin, 3, 3]")
    return pack_conv_weights(weight)


def conv3x3_nhwc(x, packed, bias, residual=None, relu=False, tile_rows: int = 0):
    """out = [relu](conv3x3(x) + bias [+ residual]) on NHWC bfloat16: x [B,H,W,Cin], residual / out [B,H,W,Cout]: conv_nhwc at ks = 3."""
    return conv_nhwc(x, packed, bias, 3, residual=residual, relu=relu, tile_rows=tile_rows)


def upsample2x_nhwc(x, skip=None):
    """out = bilinear_x2(x [+ skip]) on NHWC bfloat16 ([B,H,W,C] -> [B,2H,2W,C]): f.interpolate(scale_factor=2, mode='bilinear',
    align_corners=False) of UpsampleConvLayer.forward (model/submodules.py:86-87) behind the sum skip (model/unet.py:304)."""
    _lib.require_gpu()
    need("x", x)
    if skip is not None:
        need("skip", skip, shape=x.shape, device=x.device)
    b, h, w, c = x.shape
    out = torch.empty((b, 2 * h, 2 * w, c), dtype=torch.bfloat16, device=x.device)
    launch("v2v_upsample2x_nhwc_hip", x.device, ptr(x), ptr(skip), b, h, w, c, ptr(out))
    return out


def conv1x1_nhwc(x, weight, bias, skip=None, out_dtype=torch.bfloat16):
    """out[..., o] = bias[o] + sum_c weight[o, c] * (x[..., c] + skip[..., c]) on NHWC bfloat16 ([B,H,W,C] -> [B,H,W,Cout], Cout <= 3):
    the prediction layer ConvLayer(base, out, 1, activation=None) on skip_sum(x, head) (model/unet.py:58-64, :307)."""
    _lib.require_gpu()
    need("x", x)
    if skip is not None:
        need("skip", skip, shape=x.shape, device=x.device)
    b, h, w, c = x.shape
    weight = weight.detach().reshape(weight.shape[0], -1).float().contiguous()
    if weight.shape[1] != c or bias.numel() != weight.shape[0] or out_dtype not in _DTYPES:
        raise ValueError("weight must be [Cout, C(,1,1)], bias [Cout], out_dtype float32 or bfloat16")
    out = torch.empty((b, h, w, weight.shape[0]), dtype=out_dtype, device=x.device)
    launch("v2v_conv1x1_nhwc_hip", x.device, ptr(x), ptr(skip), ptr(weight), ptr(bias.detach().float().contiguous()), b * h * w, c, weight.shape[0],
           ptr(out), DTYPE_CODES[out_dtype])
    return out


def pack_head_weights(weight):
    """nn.Conv2d(Cin <= 8, 32, ks, padding=ks//2).weight float32 -> the head kernel's packed bfloat16 stream (taps along K)."""
    _lib.require_gpu()
    if not weight.is_cuda or weight.dtype != torch.float32 or weight.dim() != 4 or weight.shape[0] != 32 or weight.shape[1] > 8 \
            or weight.shape[2] != weight.shape[3] or weight.shape[2] not in (3, 5):
        raise ValueError("weight must be a float32 CUDA tensor [32, Cin <= 8, ks, ks], ks 3 or 5")
    ks = weight.shape[2]
    packed = torch.empty((_lib.lib().v2v_conv_head_packed_elems(ks),), dtype=torch.bfloat16, device=weight.device)
    launch("v2v_conv_head_pack_weights_hip", weight.device, ptr(weight.detach().contiguous()), weight.shape[1], ks, ptr(packed))
    return packed


def conv_head_nhwc(x8, packed, bias, ks: int, relu=True):
    """out = [relu](conv_ks(x, stride 1, pad ks//2) + bias): x8 [B,H,W,8] bfloat16 (to_nhwc8_bf16) -> [B,H,W,32] bfloat16; the UNet's
    head ConvLayer(num_bins, 32, 5, stride 1, padding 2) (model/unet.py:77-78).  H and W multiples of 16."""
    _lib.require_gpu()
    need("x8", x8, dims="[B,H,W,8]", last=8)
    if bias.numel() != 32 or packed.dtype != torch.bfloat16 or packed.numel() != _lib.lib().v2v_conv_head_packed_elems(ks):
        raise ValueError("bias must be [32] and packed the output of pack_head_weights for the same ks")
    b, h, w, _ = x8.shape
    out = torch.empty((b, h, w, 32), dtype=torch.bfloat16, device=x8.device)
    launch("v2v_conv_head_nhwc_hip", x8.device, ptr(x8), ptr(packed), ptr(bias.detach().float().contiguous()), int(bool(relu)), b, h, w, ks, ptr(out))
    return out


def pack_stem_weights(weight):
    """nn.Conv2d(Cin <= 8, 64, 3, stride=2, padding=1).weight float32 -> the stem kernel's packed bfloat16 stream (taps along K)."""
    _lib.require_gpu()
    if not weight.is_cuda or weight.dtype != torch.float32 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[0] != 64 \
            or weight.shape[1] > 8:
        raise ValueError("weight must be a float32 CUDA tensor [64, Cin <= 8, 3, 3]")
    packed = torch.empty((_lib.lib().v2v_conv_stem_packed_elems(),), dtype=torch.bfloat16, device=weight.device)
    launch("v2v_conv_stem_pack_weights_hip", weight.device, ptr(weight.detach().contiguous()), weight.shape[1], ptr(packed))
    return packed


def conv_stem_nhwc(x8, packed, bias, relu=True):
    """out = [relu](conv3x3(x, stride 2, pad 1) + bias): x8 [B,H,W,8] bfloat16 (to_nhwc8_bf16) -> [B,H/2,W/2,64] bfloat16; the plain UNet's
    first encoder ConvLayer(num_bins, 64, 3, stride 2, padding 1) (model/unet.py:320-326).  H and W multiples of 16."""
    _lib.require_gpu()
    need("x8", x8, dims="[B,H,W,8]", last=8)
    if bias.numel() != 64 or packed.dtype != torch.bfloat16 or packed.numel() != _lib.lib().v2v_conv_stem_packed_elems():
        raise ValueError("bias must be [64] and packed the output of pack_stem_weights")
    b, h, w, _ = x8.shape
    out = torch.empty((b, h // 2, w // 2, 64), dtype=torch.bfloat16, device=x8.device)
    launch("v2v_conv_stem_nhwc_hip", x8.device, ptr(x8), ptr(packed), ptr(bias.detach().float().contiguous()), int(bool(relu)), b, h, w, ptr(out))
    return out


def upsample2x_cat_nhwc(x, skip=None):
    """out = cat(bilinear_x2(x), bilinear_x2(skip)) along the channels on NHWC bfloat16 ([B,H,W,C1], [B,H,W,C2] -> [B,2H,2W,C1+C2]):
    f.interpolate(skip_concat(x, skip), scale_factor=2, mode='bilinear', align_corners=False) (model/model_util.py:10, model/unet.py:350,
    model/submodules.py:86-87) without the low-resolution cat tensor."""
    _lib.require_gpu()
    need("x", x)
    if skip is not None:
        need("skip", skip, device=x.device)
        if skip.shape[:3] != x.shape[:3]:
            raise ValueError("skip must have x's batch and spatial size")
    b, h, w, c1 = x.shape
    c2 = 0 if skip is None else skip.shape[3]
    out = torch.empty((b, 2 * h, 2 * w, c1 + c2), dtype=torch.bfloat16, device=x.device)
    launch("v2v_upsample2x_cat_nhwc_hip", x.device, ptr(x), c1, ptr(skip), c2, b, h, w, ptr(out))
    return out


# ---- NER-Net's NAM cell (include/v2v_nam.h, v2v_amd/csrc/v2v_nam.hpp): three launches behind one call --------------------------------------
NAM_KEYS = ("conv_x.0.weight", "conv_h.0.weight", "conv_m.0.weight", "conv_o.0.weight", "conv_last.weight", "LAG_conv.weight")   # under one NAM_withoutGCB


def pack_nam_weights(conv_x, conv_h, conv_m, conv_o, conv_last, lag_conv):
    """The six float32 tensors of NAM_KEYS ([7C,C,3,3], [4C,C,3,3], [3C,C,3,3], [C,2C,3,3], [C,2C,1,1], [C,C,1,1]) -> the packed bfloat16
    streams of the three launches, one flat tensor (layout: v2v_amd/csrc/v2v_nam.hpp)."""
    _lib.require_gpu()
    ws = (conv_x, conv_h, conv_m, conv_o, conv_last, lag_conv)
    c = lag_conv.shape[0] if lag_conv.dim() >= 2 else 0
    shapes = ((7 * c, c, 3, 3), (4 * c, c, 3, 3), (3 * c, c, 3, 3), (c, 2 * c, 3, 3), (c, 2 * c), (c, c))
    for key, w, shape in zip(NAM_KEYS, ws, shapes):
        if not w.is_cuda or w.dtype != torch.float32 or w.device != conv_x.device or tuple(w.shape) not in (shape, shape + (1, 1)):
            raise ValueError(f"{key} must be a float32 CUDA tensor {list(shape)} on one device, C = {c}")
    n = _lib.lib().v2v_nam_packed_elems(c)
    if n < 0:
        _lib.check(int(n))
    packed = torch.empty((n,), dtype=torch.bfloat16, device=conv_x.device)
    launch("v2v_nam_pack_weights_hip", conv_x.device, *(ptr(w.detach().contiguous()) for w in ws), c, ptr(packed))
    return packed


def nam_step(x, m_t, h_prev, c_prev, packed, nchw_dtype=None, tile: int = 0, c_out=None, return_workspaces: bool = False, valid=None):
    """One NAM_withoutGCB step on NHWC state.  x, m_t, h_prev: bfloat16 [B,H,W,C]; c_prev: float32; h_prev and c_prev both None = the zero
    state.  packed = pack_nam_weights(...).  Returns a dict: h, c_bf16, m (bfloat16: what the next convolutions read), h_f32, c (float32;
    c is the carried state, c_out may be c_prev: updated in place), m_f32 (float32), h_nchw ([B,C,H,W] in nchw_dtype, when that is not
    None) and, with return_workspaces, alpha and o_pre (float32).  tile: 0 by shape, 1 / 2 = the 64- / 128-pixel instances.  valid = (Hv, Wv):
    the operands are zero outside that extent of the canvas and the bfloat16 outputs come back zero there (None: the whole canvas)."""
    _lib.require_gpu()
    need("x", x)
    b, h, w, c = x.shape
    need("m_t", m_t, shape=x.shape, device=x.device)
    if (h_prev is None) != (c_prev is None):
        raise ValueError("h_prev and c_prev come together (both None: the zero state)")
    for name, t, dt in (("h_prev", h_prev, torch.bfloat16), ("c_prev", c_prev, torch.float32)):
        if t is not None:
            need(name, t, dt, shape=x.shape, device=x.device)
    if packed.dtype != torch.bfloat16 or packed.numel() != 180 * c * c or packed.device != x.device:
        raise ValueError("packed must be the output of pack_nam_weights for the same C, on x's device")
    if nchw_dtype is not None and nchw_dtype not in _DTYPES:
        raise ValueError("nchw_dtype must be torch.float32, torch.bfloat16 or None")
    f32 = lambda: torch.empty((b, h, w, c), dtype=torch.float32, device=x.device)   # noqa: E731
    out = {"h": torch.empty_like(x), "c_bf16": torch.empty_like(x), "m": torch.empty_like(x), "h_f32": f32(), "m_f32": f32(),
           "c": c_out if c_out is not None else f32(), "alpha": f32(), "o_pre": f32()}
    if nchw_dtype is not None:
        out["h_nchw"] = torch.empty((b, c, h, w), dtype=nchw_dtype, device=x.device)
    launch("v2v_nam_step_hip", x.device, ptr(x), ptr(m_t), ptr(h_prev), ptr(c_prev), ptr(packed), b, h, w, c, ptr(out["alpha"]), ptr(out["o_pre"]), ptr(out["m"]),
           ptr(out["m_f32"]), ptr(out["c"]), ptr(out["c_bf16"]), ptr(out["h"]), ptr(out["h_f32"]), ptr(out.get("h_nchw")),
           DTYPE_CODES.get(nchw_dtype, _lib.F32), tile, *((h, w) if valid is None else (int(valid[0]), int(valid[1]))))
    if not return_workspaces:
        del out["alpha"], out["o_pre"]
    return out


# ---- NER-Net's recurrent network (include/v2v_nam.h, v2v_amd/csrc/v2v_gcb.hpp): the global context block, the valid-extent helper ---------
GCB_KEYS = ("conv_1x1.weight", "conv_1x1.bias", "GCB.conv_mask.weight", "GCB.conv_mask.bias", "GCB.channel_add_conv.0.weight", "GCB.channel_add_conv.0.bias",
            "GCB.channel_add_conv.1.weight", "GCB.channel_add_conv.1.bias", "GCB.channel_add_conv.2.weight", "GCB.channel_add_conv.3.weight",
            "GCB.channel_add_conv.3.bias")        # the reference's state_dict keys under one RecurrentConvLayer_NAM_GCB, in the order pack_gcb_weights takes them


def pack_gcb_weights(*tensors):
    """The eleven float32 tensors of GCB_KEYS (any trailing 1x1 dimensions) -> the tuple gcb_nhwc takes: each flat and contiguous, conv_1x1's
    weight transposed to [Cin][Cout].  No arithmetic; goes through packed_weights like every other packing."""
    if len(tensors) != len(GCB_KEYS):
        raise ValueError(f"pack_gcb_weights takes the {len(GCB_KEYS)} tensors of GCB_KEYS")
    c = tensors[0].shape[0]
    shapes = ((c, c), (c,), (1, c), (1,), (c // 4, c), (c // 4,), (c // 4,), (c // 4,), (1,), (c, c // 4), (c,))
    flat = []
    for key, t, shape in zip(GCB_KEYS, tensors, shapes):
        if not t.is_cuda or t.dtype != torch.float32 or t.device != tensors[0].device or t.numel() != shape[0] * (shape[1] if len(shape) > 1 else 1) \
                or tuple(t.shape[:len(shape)]) != shape:
            raise ValueError(f"{key} must be a float32 CUDA tensor {list(shape)} (+ 1x1 dimensions) on one device, C = {c}")
        flat.append(t.detach().reshape(shape))
    flat[0] = flat[0].t()
    return tuple(t.contiguous().reshape(-1) for t in flat)


def gcb_nhwc(x, packed, valid=None, eps: float = 1e-5, return_context: bool = False):
    """out = x + g + add(ctx(g)), g = conv_1x1(x): RecurrentConvLayer_NAM_GCB's 1x1 convolution, ContextBlock2d (attention pooling,
    channel_add) and the residual (model/nernet/submodules.py:365-442, :768-770) on NHWC bfloat16 [B,H,W,C], C in {32, 64, 128}, float32
    arithmetic, three launches.  packed = pack_gcb_weights(...).  valid = (Hv, Wv): the pooling runs over rows < Hv and columns < Wv only
    and out is zero elsewhere (None: the whole canvas).  return_context: also the float32 [B,2,C] tensor of ctx | add."""
    _lib.require_gpu()
    need("x", x)
    b, h, w, c = x.shape
    hv, wv = (h, w) if valid is None else (int(valid[0]), int(valid[1]))
    if len(packed) != len(GCB_KEYS) or any(t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() for t in packed) \
            or [t.numel() for t in packed] != [c * c, c, c, 1, c * c // 4, c // 4, c // 4, c // 4, 1, c * c // 4, c]:
        raise ValueError("packed must be the output of pack_gcb_weights for x's channel count, on x's device")
    nbytes = _lib.lib().v2v_gcb_workspace_bytes(b, h, w, c)
    if nbytes < 0:
        _lib.check(int(nbytes))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    ctx_add = torch.empty((b, 2, c), dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    launch("v2v_gcb_nhwc_hip", x.device, ptr(x), *(ptr(t) for t in packed), float(eps), b, h, w, c, hv, wv, ptr(ws), nbytes, ptr(ctx_add), ptr(out))
    return (out, ctx_add) if return_context else out


def to_nhwc16_bf16(x):
    """float32 [B, 9 <= C <= 16, H, W] of any strides -> bfloat16 [B, H, W, 16] with the channels zero-padded to 16: conv_head16in_nhwc's
    input layout (to_nhwc8_bf16 is the one for up to 8 channels)."""
    _lib.require_gpu()
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or not 9 <= x.shape[1] <= 16 or min(x.stride()) < 0:
        raise ValueError("x must be a float32 CUDA tensor [B, 9 <= C <= 16, H, W]")
    b, c, h, w = x.shape
    out = torch.empty((b, h, w, 16), dtype=torch.bfloat16, device=x.device)
    launch("v2v_to_nhwc16_bf16_hip", x.device, ptr(x), *x.stride(), b, c, h, w, ptr(out))
    return out


def pack_head16in_weights(weight):
    """nn.Conv2d(9 <= Cin <= 16, 32, 5, padding=2).weight float32 -> the packed bfloat16 stream of conv_head16in_nhwc."""
    _lib.require_gpu()
    if not weight.is_cuda or weight.dtype != torch.float32 or weight.dim() != 4 or weight.shape[0] != 32 or not 9 <= weight.shape[1] <= 16 \
            or tuple(weight.shape[2:]) != (5, 5):
        raise ValueError("weight must be a float32 CUDA tensor [32, 9 <= Cin <= 16, 5, 5]")
    packed = torch.empty((_lib.lib().v2v_conv_head16in_packed_elems(),), dtype=torch.bfloat16, device=weight.device)
    launch("v2v_conv_head16in_pack_weights_hip", weight.device, ptr(weight.detach().contiguous()), weight.shape[1], ptr(packed))
    return packed


def conv_head16in_nhwc(x16, packed, bias, relu=True):
    """out = [relu](conv5x5(x, pad 2) + bias): x16 [B,H,W,16] bfloat16 (to_nhwc16_bf16) -> [B,H,W,32] bfloat16, any H and W; the head
    ConvLayer(2 * num_bins, 32, 5, padding=2) of NER-Net's UNetNIAM_STcell_GCB (model/nernet/unet.py)."""
    _lib.require_gpu()
    need("x16", x16, dims="[B,H,W,16]", last=16)
    if bias.numel() != 32 or packed.dtype != torch.bfloat16 or packed.numel() != _lib.lib().v2v_conv_head16in_packed_elems() or packed.device != x16.device:
        raise ValueError("bias must be [32] and packed the output of pack_head16in_weights, on x16's device")
    b, h, w, _ = x16.shape
    out = torch.empty((b, h, w, 32), dtype=torch.bfloat16, device=x16.device)
    launch("v2v_conv_head16in_nhwc_hip", x16.device, ptr(x16), ptr(packed), ptr(bias.detach().float().contiguous()), int(bool(relu)), b, h, w, ptr(out))
    return out


def valid_extent_nhwc(x, valid, replicate: bool = False):
    """In place on an NHWC canvas [B,H,W,C], bfloat16 or float32: pixels outside the valid extent valid = (Hv, Wv) are cleared; with
    replicate, row Hv and column Wv take the nearest valid pixel instead (what upsample2x_nhwc must find there to compute, inside twice
    the extent, the upsampling of the cropped tensor).  -> x"""
    _lib.require_gpu()
    if not isinstance(x, torch.Tensor) or x.dtype not in _DTYPES:
        raise ValueError("x must be a contiguous float32 or bfloat16 CUDA tensor [B,H,W,C]")
    need("x", x, x.dtype)
    b, h, w, c = x.shape
    launch("v2v_valid_extent_nhwc_hip", x.device, ptr(x), DTYPE_CODES[x.dtype], b, h, w, c, int(valid[0]), int(valid[1]), int(bool(replicate)))
    return x


# ---- backward: the data gradient of a convolution is the stride-1 convolution of the output gradient (spread onto the input grid for
# stride 2) with the flipped, transposed weights on the forward convolution kernel; the weight / bias gradient is an MFMA GEMM over the
# pixels (slabs + a fixed-order sum); the ConvLSTM step recomputes its gate GEMM and runs the cell backward on the accumulators -------------
def _workspace(nbytes: int, device) -> torch.Tensor:
    if nbytes < 0:
        raise ValueError("shape not taken by the backward kernels")
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)


def _nhwc_bf16(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    return t.contiguous()


def relu_bwd_nhwc(dy, y):
    """y > 0 ? dy : 0 on NHWC bfloat16 (y = the saved post-ReLU output)."""
    dy = _nhwc_bf16(dy)
    out = torch.empty_like(dy)
    launch("v2v_relu_bwd_nhwc_hip", dy.device, ptr(dy), ptr(y), dy.numel() // dy.shape[-1], dy.shape[-1], ptr(out))
    return out


def pack_dgrad_weights(weight: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d weight float32 [Cout, Cin, ks, ks] -> the packed stream of the transposed convolution (Cout -> Cin, flipped taps)."""
    cout, cin, ks = weight.shape[0], weight.shape[1], weight.shape[2]
    n = _lib.lib().v2v_conv_dgrad_packed_elems(cin, cout, ks)
    if n < 0:
        raise ValueError(f"no data-gradient kernel for {cin} -> {cout} channels, {ks}x{ks}")
    packed = torch.empty((n,), dtype=torch.bfloat16, device=weight.device)
    scratch = torch.empty((weight.numel(),), dtype=torch.float32, device=weight.device)
    launch("v2v_conv_dgrad_pack_weights_hip", weight.device, ptr(weight.detach().float().contiguous()), cin, cout, ks, ptr(scratch), ptr(packed))
    return packed


def conv_dgrad_nhwc(dy, packed, cin: int, ks: int, stride: int, hin: int, win: int, residual=None):
    """dx [B,Hin,Win,Cin] bf16 of a ks x ks convolution (pad ks//2) from its output gradient dy [B,Hout,Wout,Cout] (ReLU already applied)."""
    dy = _nhwc_bf16(dy)
    b, cout = dy.shape[0], dy.shape[3]
    ws = _workspace(_lib.lib().v2v_conv_dgrad_workspace_bytes(b, hin, win, cin, cout, stride), dy.device)
    dx = torch.empty((b, hin, win, cin), dtype=torch.bfloat16, device=dy.device)
    launch("v2v_conv_dgrad_nhwc_hip", dy.device, ptr(dy), ptr(packed), ptr(residual), b, hin, win, cin, cout, ks, stride, ptr(ws), ptr(dx))
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
    launch("v2v_conv_wgrad_nhwc_hip", dy.device, ptr(dy), ptr(x1), c1, ptr(x2), c2, cin_out, b, hin, win, cout, ks, stride, ptr(ws), ptr(dw), ptr(db))
    return dw, db


def upsample2x_bwd_nhwc(dout):
    """Adjoint of upsample2x_nhwc: [B,2H,2W,C] -> [B,H,W,C] bf16 (the gradient of x and of the skip)."""
    dout = _nhwc_bf16(dout)
    b, h2, w2, c = dout.shape
    dx = torch.empty((b, h2 // 2, w2 // 2, c), dtype=torch.bfloat16, device=dout.device)
    launch("v2v_upsample2x_bwd_nhwc_hip", dout.device, ptr(dout), b, h2 // 2, w2 // 2, c, ptr(dx))
    return dx


def upsample2x_cat_bwd_nhwc(dout, c0: int, c: int):
    """Adjoint of upsample2x_cat_nhwc for the channel slice [c0, c0 + c): [B,2H,2W,Ctot] -> [B,H,W,c] bf16."""
    dout = _nhwc_bf16(dout)
    b, h2, w2, ctot = dout.shape
    dx = torch.empty((b, h2 // 2, w2 // 2, c), dtype=torch.bfloat16, device=dout.device)
    launch("v2v_upsample2x_cat_bwd_nhwc_hip", dout.device, ptr(dout), b, h2 // 2, w2 // 2, ctot, c0, c, ptr(dx))
    return dx


def conv1x1_bwd_cout_nhwc(dy, x, skip, weight):
    """Prediction layer with Cout = 1..3 outputs: dy [B,H,W,Cout] (read as float32) -> (dx [B,H,W,C] bf16, dW [Cout,C,1,1], db [Cout])."""
    dy = dy.float().contiguous()
    b, h, w, c = x.shape
    m, cout = b * h * w, weight.shape[0]
    if dy.numel() != m * cout:
        raise ValueError("dy must be [B,H,W,Cout]")
    ws = _workspace(_lib.lib().v2v_conv1x1_bwd_cout_workspace_bytes(m, c, cout), x.device)
    dx = torch.empty_like(x)
    dw = torch.empty((cout, c), dtype=torch.float32, device=x.device)
    db = torch.empty((cout,), dtype=torch.float32, device=x.device)
    launch("v2v_conv1x1_bwd_cout_nhwc_hip", x.device, ptr(dy), ptr(x), ptr(skip), ptr(weight.detach().float().reshape(cout, c).contiguous()), m, c, cout,
           ptr(dx), ptr(dw), ptr(db), ptr(ws))
    return dx, dw.reshape(weight.shape), db


def conv1x1_bwd_nhwc(dy, x, skip, weight):
    """Prediction layer (C -> 1 on bf16(x + skip)): dy [B,H,W,1] (read as float32) -> (dx [B,H,W,C] bf16 = the gradient of x and skip,
    dW [1,C,1,1], db [1]).  The one-output entry point; it runs conv1x1_bwd_cout_nhwc's kernel at Cout = 1."""
    dy = dy.float().contiguous()
    b, h, w, c = x.shape
    m = b * h * w
    ws = _workspace(_lib.lib().v2v_conv1x1_bwd_workspace_bytes(m, c), x.device)
    dx = torch.empty_like(x)
    dw = torch.empty((c,), dtype=torch.float32, device=x.device)
    db = torch.empty((1,), dtype=torch.float32, device=x.device)
    launch("v2v_conv1x1_bwd_nhwc_hip", x.device, ptr(dy), ptr(x), ptr(skip), ptr(weight.detach().float().reshape(-1).contiguous()), m, c, ptr(dx),
           ptr(dw), ptr(db), ptr(ws))
    return dx, dw.reshape(weight.shape), db


def convlstm_step_bwd(x, h_prev, c_prev, packed, bias, dh, dc):
    """Backward of convlstm_step from the saved x / h_prev / c_prev: (dgates bf16 [B,H,W,4C], dc_prev float32 [B,H,W,C])."""
    b, h, w, c = x.shape
    dh = dh.float().contiguous()
    dc = dc.float().contiguous() if dc is not None else None
    dgates = torch.empty((b, h, w, 4 * c), dtype=torch.bfloat16, device=x.device)
    dc_prev = torch.empty((b, h, w, c), dtype=torch.float32, device=x.device)
    launch("v2v_convlstm_step_bwd_hip", x.device, ptr(x), ptr(h_prev), ptr(c_prev), ptr(packed), ptr(bias), ptr(dh), ptr(dc), b, h, w, c, ptr(dgates),
           ptr(dc_prev))
    return dgates, dc_prev


# ---- HyperE2VID's dynamic decoder (v2v_amd/hyper.py; kernels in v2v_amd/csrc/v2v_hyper.hpp) ---------------------------------------------
def hyper_context_nhwc8(events, prev):
    """cat(events [B, C <= 7, H, W] float32 of any strides, prev [B,1,H,W] float32) bilinearly downsampled by 4 -> bfloat16 [B,H/4,W/4,8],
    channels zero-padded to 8: f.interpolate(cat, scale_factor=0.25, mode='bilinear', align_corners=False) of
    ConvolutionalContextFusion.forward (model/hyper/hyper_dynamic.py:19-21) in the head kernels' 8-channel input layout (context_conv_nhwc reads it)."""
    _lib.require_gpu()
    if not events.is_cuda or events.dtype != torch.float32 or events.dim() != 4 or events.shape[1] > 7:
        raise ValueError("events must be a float32 CUDA tensor [B, C <= 7, H, W]")
    b, c, h, w = events.shape
    need("prev", prev, torch.float32, shape=(b, 1, h, w), device=events.device, owner="events")
    if h % 4 != 0 or w % 4 != 0:
        raise ValueError("H and W must be multiples of 4")
    out = torch.empty((b, h // 4, w // 4, 8), dtype=torch.bfloat16, device=events.device)
    launch("v2v_hyper_context_hip", events.device, ptr(events), *events.stride(), ptr(prev), b, c, h, w, ptr(out))
    return out


def context_conv_nhwc(x8, weight, bias):
    """out = conv3x3(x8, pad 1) + bias: x8 [B,h,w,8] bfloat16 (hyper_context_nhwc8) -> [B,h,w,32] bfloat16, any h and w;
    ConvolutionalContextFusion.conv (model/hyper/hyper_dynamic.py:22).  weight float32 [32, Cin <= 8, 3, 3], read as it is (no packing)."""
    _lib.require_gpu()
    need("x8", x8, dims="[B,h,w,8]", last=8)
    if weight.dtype != torch.float32 or weight.dim() != 4 or weight.shape[0] != 32 or weight.shape[1] > 8 or tuple(weight.shape[2:]) != (3, 3) \
            or bias.numel() != 32 or weight.device != x8.device:
        raise ValueError("weight must be float32 [32, Cin <= 8, 3, 3] on x8's device, bias [32]")
    b, h, w, _ = x8.shape
    out = torch.empty((b, h, w, 32), dtype=torch.bfloat16, device=x8.device)
    launch("v2v_hyper_context_conv_hip", x8.device, ptr(x8), ptr(weight.detach().contiguous()), ptr(bias.detach().float().contiguous()), b, h, w,
           weight.shape[1], ptr(out))
    return out


def tanh_bf16_(x):
    """In-place tanh of a contiguous bfloat16 CUDA tensor (numel % 8 == 0): the activation the convolution kernel's epilogue does not have."""
    _lib.require_gpu()
    if not x.is_cuda or x.dtype != torch.bfloat16 or not x.is_contiguous() or x.numel() % 8 != 0:
        raise ValueError("x must be a contiguous bfloat16 CUDA tensor with a multiple of 8 elements")
    launch("v2v_tanh_bf16_hip", x.device, ptr(x), x.numel(), ptr(x))
    return x


def hyper_atoms(coeff, bases):
    """coeff bfloat16 [B,h,w,128] (the 72 PRE-activation basis coefficients of bases_net's last convolution + BatchNorm, index m * 12 + k,
    zero-padded to the convolution kernel's 128 columns), bases float32 [12,25] -> atoms float32 [B,h,w,25,6]:
    atoms[..., l, m] = sum_k tanh(coeff[..., m * 12 + k]) * bases[k, l] (DynamicAtomGeneration.forward, model/hyper/hyper_dynamic.py:54-56)."""
    _lib.require_gpu()
    need("coeff", coeff, dims="[B,h,w,128]", last=128)
    need("bases", bases, torch.float32, shape=(12, 25), device=coeff.device, owner="coeff")
    b, h, w, _ = coeff.shape
    atoms = torch.empty((b, h, w, 25, 6), dtype=torch.float32, device=coeff.device)
    launch("v2v_hyper_atoms_hip", coeff.device, ptr(coeff), ptr(bases), b * h * w, ptr(atoms))
    return atoms


def pack_dynconv_weights(weight):
    """DynamicConv.compositional_coefficients float32 [128, 256 * 6, 1, 1] -> the dynamic-convolution kernel's packed bfloat16 stream
    (atom-major K: every 64-wide chunk is one atom over 64 channels)."""
    _lib.require_gpu()
    if not weight.is_cuda or weight.dtype != torch.float32 or weight.dim() != 4 or tuple(weight.shape[2:]) != (1, 1):
        raise ValueError("weight must be a float32 CUDA tensor [Cout, Cin * atoms, 1, 1]")
    cout, k = weight.shape[0], weight.shape[1]
    n = _lib.lib().v2v_hyper_dynconv_packed_elems(k // 6, cout, 6, 5) if k % 6 == 0 else -1
    if n < 0:
        raise ValueError(f"the dynamic convolution takes 256 -> 128 channels with 6 atoms (got weight {tuple(weight.shape)})")
    packed = torch.empty((n,), dtype=torch.bfloat16, device=weight.device)
    launch("v2v_hyper_dynconv_pack_weights_hip", weight.device, ptr(weight.detach().contiguous()), k // 6, cout, 6, ptr(packed))
    return packed


def dynconv_nhwc(x, atoms, packed, bias, relu=True):
    """out = [relu](DynamicConv(x, atoms) + bias) on NHWC bfloat16: x [B,H,W,256], atoms float32 [B,H,W,25,6] (hyper_atoms) -> [B,H,W,128];
    neither the unfolded input nor the intermediate features of model/hyper/hyper_dynamic.py:87-91 are written anywhere."""
    _lib.require_gpu()
    need("x", x, dims="[B,H,W,Cin]")
    b, h, w, cin = x.shape
    cout = bias.numel()
    need("atoms", atoms, torch.float32, shape=(b, h, w, 25, 6), device=x.device)
    if bias.dtype != torch.float32 or packed.dtype != torch.bfloat16 or packed.numel() != _lib.lib().v2v_hyper_dynconv_packed_elems(cin, cout, 6, 5):
        raise ValueError("bias must be float32 [128] and packed the output of pack_dynconv_weights (256 -> 128 channels, 6 atoms)")
    out = torch.empty((b, h, w, cout), dtype=torch.bfloat16, device=x.device)
    launch("v2v_hyper_dynconv_nhwc_hip", x.device, ptr(x), ptr(atoms), ptr(packed), ptr(bias.detach().contiguous()), int(bool(relu)), b, h, w, cin, cout,
           6, 5, ptr(out))
    return out


# ---- the dynamic decoder's backward and BatchNorm on batch statistics (kernels: the training section of v2v_amd/csrc/v2v_hyper.hpp) ---------
def pack_dynconv_weights_t(weight):
    """compositional_coefficients float32 [128, 1536, 1, 1] -> the transposed bfloat16 stream dynconv_df_nhwc reads ([1536 feature columns in
    dF's order][128])."""
    _lib.require_gpu()
    if not weight.is_cuda or weight.dtype != torch.float32 or tuple(weight.shape) != (128, 1536, 1, 1):
        raise ValueError("weight must be a float32 CUDA tensor [128, 1536, 1, 1]")
    packed = torch.empty((128 * 1536,), dtype=torch.bfloat16, device=weight.device)
    launch("v2v_hyper_dynconv_pack_t_hip", weight.device, ptr(weight.detach().contiguous()), ptr(packed))
    return packed


def dynconv_df_nhwc(dz, packed_t):
    """dz bf16 [B,H,W,128] (the ReLU backward applied) -> dF bf16 [B,H,W,4,6,64]: dF[p][cb][m][k] = sum_o dz[p][o] * W[o][(cb*64+k)*6+m],
    float32 accumulation on the matrix cores, one rounding."""
    need("dz", dz, dims="[B,H,W,128]", last=128)
    if packed_t.dtype != torch.bfloat16 or packed_t.numel() != 128 * 1536 or packed_t.device != dz.device:
        raise ValueError("packed_t must be the output of pack_dynconv_weights_t on dz's device")
    b, h, w, _ = dz.shape
    df = torch.empty((b, h, w, 4, 6, 64), dtype=torch.bfloat16, device=dz.device)
    launch("v2v_hyper_dynconv_df_hip", dz.device, ptr(dz), ptr(packed_t), b * h * w, ptr(df))
    return df


def dynconv_datoms_nhwc(x, df):
    """x bf16 [B,H,W,256] (the dynamic convolution's input), dF (dynconv_df_nhwc) -> dAtoms float32 [B,H,W,25,6]:
    dAtoms[p][l][m] = sum_c x[p + offset_l][c] * dF[p][c][m] over the zero-padded 5 x 5 window."""
    need("x", x, dims="[B,H,W,256]", last=256)
    b, h, w, _ = x.shape
    need("df", df, shape=(b, h, w, 4, 6, 64), device=x.device)
    out = torch.empty((b, h, w, 25, 6), dtype=torch.float32, device=x.device)
    launch("v2v_hyper_dynconv_datoms_hip", x.device, ptr(x), ptr(df), b, h, w, ptr(out))
    return out


def dynconv_dx_nhwc(atoms, df):
    """atoms float32 [B,H,W,25,6], dF -> dX bf16 [B,H,W,256]: dX[q][c] = sum_l sum_m atoms[q - offset_l][l][m] * dF[q - offset_l][c][m]."""
    if atoms.dim() != 5:
        raise ValueError("atoms must be float32 [B,H,W,25,6]")
    b, h, w = atoms.shape[:3]
    need("atoms", atoms, torch.float32, shape=(b, h, w, 25, 6))
    need("df", df, shape=(b, h, w, 4, 6, 64), device=atoms.device, owner="atoms")
    out = torch.empty((b, h, w, 256), dtype=torch.bfloat16, device=atoms.device)
    launch("v2v_hyper_dynconv_dx_hip", atoms.device, ptr(atoms), ptr(df), b, h, w, ptr(out))
    return out


def dynconv_wgrad_nhwc(dz, x, atoms):
    """(dW float32 [128, 1536, 1, 1], db float32 [128]) of the dynamic convolution: dW[o][c*6+m] = sum_p dz[p][o] * bf16(F[p][c][m]) with the
    features F recomputed from x and atoms exactly as dynconv_nhwc computes and rounds them (they are never stored)."""
    need("dz", dz, dims="[B,H,W,128]", last=128)
    b, h, w, _ = dz.shape
    need("x", x, shape=(b, h, w, 256), device=dz.device, owner="dz")
    need("atoms", atoms, torch.float32, shape=(b, h, w, 25, 6), device=dz.device, owner="dz")
    ws = _workspace(_lib.lib().v2v_hyper_dynconv_wgrad_workspace_bytes(b, h, w), dz.device)
    dw = torch.empty((128, 1536, 1, 1), dtype=torch.float32, device=dz.device)
    db = torch.empty((128,), dtype=torch.float32, device=dz.device)
    launch("v2v_hyper_dynconv_wgrad_hip", dz.device, ptr(dz), ptr(x), ptr(atoms), b, h, w, ptr(ws), ptr(dw), ptr(db))
    return dw, db


def hyper_bn_stats(z, eps: float = 1e-5):
    """z bf16 [B,h,w,Cs] -> (mean, biased variance, rstd = 1 / sqrt(var + eps)), float32 [Cs] each, over the B*h*w rows."""
    need("z", z, dims="[B,h,w,Cs]")
    cs = z.shape[3]
    mean, var, rstd = (torch.empty((cs,), dtype=torch.float32, device=z.device) for _ in range(3))
    launch("v2v_hyper_bn_stats_hip", z.device, ptr(z), z.numel() // cs, cs, C.c_float(eps), ptr(mean), ptr(var), ptr(rstd))
    return mean, var, rstd


def _bn_affine(z, gamma, beta):
    cs, cv = z.shape[3], gamma.numel()
    if cv > cs or beta.numel() != cv or gamma.device != z.device:
        raise ValueError("gamma / beta must hold Cv <= Cs values on z's device")
    return cs, cv, gamma.detach().float().contiguous(), beta.detach().float().contiguous()


def hyper_bn_apply(z, mean, rstd, gamma, beta, tanh: bool):
    """gamma * (z - mean) * rstd + beta [-> tanh] -> bf16 [B,h,w,Cs]; gamma / beta hold the Cv valid columns, the rest come out zero."""
    need("z", z, dims="[B,h,w,Cs]")
    cs, cv, g, b = _bn_affine(z, gamma, beta)
    out = torch.empty_like(z)
    launch("v2v_hyper_bn_apply_hip", z.device, ptr(z), ptr(mean), ptr(rstd), ptr(g), ptr(b), z.numel() // cs, cs, cv, int(bool(tanh)), ptr(out))
    return out


def hyper_bn_bwd(dy, z, mean, rstd, gamma, beta, tanh: bool):
    """Backward of hyper_bn_apply on batch statistics: dy bf16 or float32 [B,h,w,Cs] -> (dz bf16 [B,h,w,Cs], dgamma [Cv], dbeta [Cv],
    dz_sum [Cv] = the row sum of dz before its bf16 rounding: the bias gradient of the convolution in front, zero in exact arithmetic)."""
    need("z", z, dims="[B,h,w,Cs]")
    cs, cv, g, b = _bn_affine(z, gamma, beta)
    if dy.dtype not in _DTYPES:
        raise ValueError("dy must be float32 or bfloat16")
    need("dy", dy, dy.dtype, shape=z.shape, device=z.device, owner="z")
    sums = torch.empty((4, cs), dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z)
    launch("v2v_hyper_bn_bwd_hip", z.device, ptr(dy), int(dy.dtype == torch.float32), ptr(z), ptr(mean), ptr(rstd), ptr(g), ptr(b), z.numel() // cs,
           cs, cv, int(bool(tanh)), ptr(sums), ptr(dz))
    return dz, sums[1, :cv], sums[0, :cv], sums[2, :cv]


def hyper_atoms_bwd(datoms, pre, bases):
    """Adjoint of hyper_atoms: datoms float32 [B,h,w,25,6], pre bf16 [B,h,w,128] (what hyper_atoms read) -> dpre float32 [B,h,w,128],
    dpre[..., m*12+k] = (1 - tanh(pre)^2) * sum_l datoms[..., l, m] * bases[k, l]; columns 72..127 zero."""
    need("pre", pre, dims="[B,h,w,128]", last=128)
    b, h, w, _ = pre.shape
    need("datoms", datoms, torch.float32, shape=(b, h, w, 25, 6), device=pre.device, owner="pre")
    need("bases", bases, torch.float32, shape=(12, 25), device=pre.device, owner="pre")
    out = torch.empty((b, h, w, 128), dtype=torch.float32, device=pre.device)
    launch("v2v_hyper_atoms_bwd_hip", pre.device, ptr(datoms), ptr(pre), ptr(bases), b * h * w, ptr(out))
    return out
