"""NER-Net's learned event voxelisation on the device (v2v_nernet.hpp; C ABI in include/v2v_nernet.h).

Drop-ins for model/nernet/representation_modules.py of the reference -- `ValueLayer`, `QuantizationLayer_trail`,
`QuantizationLayer_trail_combined`, `RepresentationCNN`, `Voxelization` -- with the reference's constructors and state_dict keys
(`quantization_layer.value_layer.mlp.{i}.{weight,bias}`, `ConvLayer.cnn.*`), so its checkpoints load with strict=True.  Every event row
(x, y, t, p, b) adds t_n * MLP(t_n - bin) to each of the C bins of its pixel; the quantisation layers run that as two launches (a
statistics pre-pass and one fused kernel: normalisation, MLP in registers, float32 atomics) instead of C passes of nn.Linear and C put_ calls.
`v2v_amd.testh5.TestH5EventDataset` hands out exactly the rows this layer takes.

Inference only: there is no backward kernel for the MLP, so a call under grad with parameters (or rows) that require it raises.
`RepresentationCNN` stays stock torch.nn.  `RepresentationRecurrent` puts the recurrent network of v2v_amd/nernet_unet.py behind the
voxelisation, the reference's whole model.  No CPU fallback.

Deliberate differences from the reference:
  * the reference normalises t IN PLACE through views of its argument (:204, :213), so it changes the caller's tensor and a second call on
    the same tensor gives a different answer; these layers leave their input untouched;
  * a flat index below -numel, where put_ raises, drops that term."""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib
from ._lib import launch, ptr

MAX_WIDTH = 128


def check_mlp_layers(mlp_layers):
    """3 to 6 entries, first and last 1, hidden widths 1..128 -- what the fused kernel takes; anything else raises here, before any launch."""
    layers = [int(v) for v in mlp_layers]
    if not 3 <= len(layers) <= 6:
        raise ValueError(f"mlp_layers needs 3 to 6 entries (got {layers})")
    if layers[0] != 1 or layers[-1] != 1:
        raise ValueError(f"mlp_layers must start and end with 1 (got {layers})")
    if any(not 1 <= w <= MAX_WIDTH for w in layers[1:-1]):
        raise ValueError(f"hidden widths must be 1..{MAX_WIDTH} (got {layers})")
    return layers


def activation_slope(activation):
    """LeakyReLU(slope) of any slope, or ReLU (slope 0)."""
    if isinstance(activation, nn.LeakyReLU):
        return float(activation.negative_slope)
    if isinstance(activation, nn.ReLU):
        return 0.0
    raise ValueError(f"the fused value layer takes nn.LeakyReLU or nn.ReLU, not {type(activation).__name__}")


def _layers_of(weights, biases):
    if len(weights) != len(biases) or len(weights) < 2:
        raise ValueError("weights and biases are the MLP's Linear layers in order: at least two of each")
    layers = [1] + [int(w.shape[0]) for w in weights]
    for i, (w, b) in enumerate(zip(weights, biases)):
        if w.dim() != 2 or int(w.shape[1]) != layers[i] or tuple(b.shape) != (layers[i + 1],):
            raise ValueError(f"Linear {i}: weight {tuple(w.shape)} / bias {tuple(b.shape)} do not continue widths {layers[:i + 1]}")
    return check_mlp_layers(layers)


def padded_width(layers):
    return (max(layers[1:-1]) + 15) // 16 * 16


def pack_mlp(weights, biases):
    """The kernel's parameter block (layout in v2v_nernet.hpp), float32 on the weights' device.  Device work only: no synchronisation."""
    layers = _layers_of(weights, biases)
    kp = padded_width(layers)
    dev = weights[0].device

    def vec(v):
        v = v.detach().reshape(-1).to(torch.float32)
        return torch.nn.functional.pad(v, (0, kp - v.numel()))

    parts = [vec(weights[0]), vec(biases[0])]
    for w, b in zip(weights[1:-1], biases[1:-1]):
        w = w.detach().to(torch.float32)
        parts += [torch.nn.functional.pad(w, (0, kp - w.shape[1], 0, kp - w.shape[0])).reshape(-1), vec(b)]
    parts += [vec(weights[-1]), vec(biases[-1])]
    packed = torch.cat(parts).to(dev).contiguous()
    assert packed.numel() == 4 * kp + (len(layers) - 3) * (kp * kp + kp)
    return packed


def _check_grad(events, params, who):
    if torch.is_grad_enabled() and (events.requires_grad or any(p.requires_grad for p in params)):
        raise RuntimeError(f"{who} is inference-only (the fused value layer has no backward kernel): call it under torch.no_grad()")


def learned_voxel(events, weights, biases, dim, slope, normalize=False, combined=False, batch_size=None, offsets=None, return_t=False, packed=None):
    """The raw operator.  events [n, 5] rows (x, y, t, p, b), float64 or float32; weights / biases the MLP's Linear layers in order;
    dim = (C, H, W); slope the LeakyReLU slope (0: ReLU).  Returns float32 [B, 2C, H, W] with the positive-polarity half first
    (combined: [B, C, H, W]); with `offsets` (int64 [T + 1] row offsets, one interval each with statistics of its own) a leading T.

    batch_size=None reads B from the last row as the reference does (:191) -- one synchronisation; with batch_size given nothing waits on
    the device.  The output is cleared by a memset on the stream.  return_t=True also returns the normalised t (float32 [n]).  `packed` is
    pack_mlp(weights, biases) when the caller has it at hand.  The rows are not modified (the reference changes them in place)."""
    layers = _layers_of(weights, biases)
    Cb, H, W = (int(v) for v in dim)
    if events.dim() != 2 or events.shape[1] != 5:
        raise ValueError(f"events must be [n, 5] rows (x, y, t, p, b), got {tuple(events.shape)}")
    if events.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"event rows are float32 or float64, not {events.dtype}")
    if combined and events.dtype != torch.float32:
        raise TypeError("the combined layer takes float32 rows only: the reference itself fails on float64 rows, with a dtype mismatch in nn.Linear "
                        "(its time stays float64 there)")
    _check_grad(events, list(weights) + list(biases), "v2v_amd.nernet.learned_voxel")
    _lib.require_gpu()
    dev = weights[0].device
    if dev.type != "cuda":
        raise RuntimeError("v2v_amd.nernet: the MLP's parameters must be on the GPU; there is no CPU fallback")
    n = int(events.shape[0])
    if batch_size is None:
        if n == 0:
            raise ValueError("batch_size=None reads the batch size from the last row: there is none")
        batch_size = int((1 + events[-1, -1]).item())
    B = int(batch_size)
    ev = events.detach().to(dev).contiguous()
    T = 1
    seg = None
    if offsets is not None:
        seg = torch.as_tensor(offsets, dtype=torch.int64).to(dev).contiguous()
        T = int(seg.numel()) - 1
    if packed is None:
        packed = pack_mlp(weights, biases)
    with torch.cuda.device(dev):
        ws_bytes = _lib.lib().v2v_learned_voxel_workspace_bytes(T, B)
        if ws_bytes < 0:
            _lib.check(int(ws_bytes))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        out = torch.empty((T, B, Cb if combined else 2 * Cb, H, W), dtype=torch.float32, device=dev)
        t_n = torch.zeros(n, dtype=torch.float32, device=dev) if return_t else None
    dt = _lib.DTYPE_CODES[ev.dtype]
    ev_p = ptr(ev) if n else ptr(ws)          # an empty tensor has no address; n == 0 reads nothing
    host_layers = (C.c_int * len(layers))(*layers)
    launch("v2v_learned_voxel_stats_hip", dev, ev_p, dt, n, ptr(seg), T, B, ptr(ws))
    launch("v2v_learned_voxel_hip", dev, ev_p, dt, n, ptr(seg), T, B, Cb, H, W, ptr(packed), host_layers, len(layers), float(slope),
           int(bool(normalize)), int(bool(combined)), ptr(ws), ptr(out), ptr(t_n) if n else None)
    if offsets is None:
        out = out[0]
    return (out, t_n) if return_t else out


class ValueLayer(nn.Module):
    """The MLP  Linear(1, h1) - act - ... - Linear(h_last, 1)  (:12-54).  forward(x) is plain torch: it is the reference's training-time
    object; the quantisation layers below run the same parameters inside the fused kernel."""

    def __init__(self, mlp_layers, activation=nn.ReLU(), num_channels=9):
        assert mlp_layers[-1] == 1, "Last layer of the mlp must have 1 input channel."
        assert mlp_layers[0] == 1, "First layer of the mlp must have 1 output channel"
        super().__init__()
        self.mlp = nn.ModuleList(nn.Linear(i, o) for i, o in zip([1] + list(mlp_layers[1:-1]), mlp_layers[1:]))
        self.activation = activation

    def forward(self, x):
        x = x[None, ..., None]
        for layer in self.mlp[:-1]:
            x = self.activation(layer(x))
        return self.mlp[-1](x).squeeze()


class _Quantization(nn.Module):
    combined = False

    def __init__(self, dim, mlp_layers=[1, 100, 100, 1], activation=nn.LeakyReLU(negative_slope=0.1), normalize=False):
        super().__init__()
        check_mlp_layers(mlp_layers)
        self.slope = activation_slope(activation)
        self.value_layer = ValueLayer(mlp_layers, activation=activation, num_channels=dim[0])
        self.dim = dim
        self.normalize = normalize
        self._packed = (None, None)

    def _params(self):
        mlp = self.value_layer.mlp
        return [m.weight for m in mlp], [m.bias for m in mlp]

    def packed(self):
        """pack_mlp of the current parameters, rebuilt when one of them was written or moved"""
        w, b = self._params()
        key = tuple((p.data_ptr(), p._version) for p in w + b)
        if self._packed[0] != key:
            self._packed = (key, pack_mlp(w, b))
        return self._packed[1]

    def forward(self, events, batch_size=None, offsets=None):
        w, b = self._params()
        if self.combined and events.dtype == torch.float64:
            raise TypeError("QuantizationLayer_trail_combined takes float32 rows only: the reference itself fails on float64 rows, with a dtype "
                            "mismatch in nn.Linear")
        _check_grad(events, w + b, f"v2v_amd.nernet.{type(self).__name__}")
        _lib.require_gpu()
        packed = self.packed() if w[0].is_cuda else None
        return learned_voxel(events, w, b, self.dim, self.slope, self.normalize, self.combined, batch_size, offsets, packed=packed)


class QuantizationLayer_trail(_Quantization):
    """[n, 5] rows -> [B, 2C, H, W], positive-polarity half first (:175-261)."""


class QuantizationLayer_trail_combined(_Quantization):
    """[n, 5] float32 rows -> [B, C, H, W]; p * t_n is the MLP's input and the factor (:91-172)."""
    combined = True


class RepresentationCNN(nn.Module):
    """Conv - ReLU - (Conv - BatchNorm - ReLU) x (layers - 2) - Conv, all bias-free (:264-284).  Stock torch.nn."""

    def __init__(self, channels, net_kwargs):
        super().__init__()
        k, pad, feat = net_kwargs["RepCNN_kernel_size"], net_kwargs["RepCNN_padding"], net_kwargs["RepCNN_channel"]
        layers = [nn.Conv2d(channels, feat, k, padding=pad, bias=False), nn.ReLU(inplace=True)]
        for _ in range(net_kwargs["RepCNN_num_layers"] - 2):
            layers += [nn.Conv2d(feat, feat, k, padding=pad, bias=False), nn.BatchNorm2d(feat), nn.ReLU(inplace=True)]
        layers.append(nn.Conv2d(feat, channels, k, padding=pad, bias=False))
        self.cnn = nn.Sequential(*layers)

    def forward(self, x):
        return self.cnn(x)


class Voxelization(nn.Module):
    """The front of NER-Net (:287-313; model/nernet_model.py:57, :96): the quantisation layer, then RepresentationCNN if asked for."""

    def __init__(self, net_kwargs, use_cnn_representation, voxel_dimension=(5, 720, 1280), mlp_layers=[1, 30, 30, 1],
                 activation=nn.LeakyReLU(negative_slope=0.1), pretrained=True, normalize=False, combine_voxel=False):
        super().__init__()
        cls = QuantizationLayer_trail_combined if combine_voxel else QuantizationLayer_trail
        self.quantization_layer = cls(voxel_dimension, mlp_layers, activation, normalize)
        self.use_cnn_representation = use_cnn_representation
        if use_cnn_representation:
            self.ConvLayer = RepresentationCNN(voxel_dimension[0] * (1 if combine_voxel else 2), net_kwargs)

    def forward(self, x):
        """x: [n, 5] event rows; the batch size is read from the last row.  Returns what the reference returns; x is left untouched."""
        vox = self.quantization_layer(x)
        return self.ConvLayer(vox) if self.use_cnn_representation else vox

    def forward_sequence(self, events, batch_size=1):
        """A list of T event tensors (one per image interval, e.g. a TestH5EventDataset sequence) -> [T, B, 2C, H, W] from one upload and
        one launch pair; every interval has statistics of its own.  Equal to forward() per interval up to the order of float32 sums."""
        if len(events) == 0:
            raise ValueError("forward_sequence needs at least one interval")
        counts = [int(e.shape[0]) for e in events]
        offsets = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0)
        rows = torch.cat(list(events), 0)
        vox = self.quantization_layer(rows, batch_size=batch_size, offsets=offsets)
        if not self.use_cnn_representation:
            return vox
        T, B = vox.shape[:2]
        return self.ConvLayer(vox.flatten(0, 1)).unflatten(0, (T, B))


def crop_sizes(height, width, num_encoders=3):
    """CropParameters(width, height, num_encoders) of the reference (model/model_util.py:195-225) in four integers: the frame padded to
    multiples of 2^num_encoders, the ceil half of the padding on top / left -> (padded height, padded width, top, left)."""
    f = 1 << int(num_encoders)
    ph, pw = -(-int(height) // f) * f, -(-int(width) // f) * f
    return ph, pw, (ph - height + 1) // 2, (pw - width + 1) // 2


class RepresentationRecurrent(nn.Module):
    """Drop-in for model/nernet_model.py:RepresentationRecurrent (:23-99) with `recurrent_network: NIAM_STcell_GCB`: the learned voxelisation
    (`representation`, rebuilt by set_resolution, its learned weights kept), the zero padding to multiples of 8 and the recurrent network
    (`unetrecurrent`, v2v_amd.nernet_unet) -- the reference's module tree and state_dict keys.  YAML: target: v2v_amd.nernet.RepresentationRecurrent.
    Inference only.  forward(events) -> (output_dict, event_tensor) as the reference; forward_sequence is what its test loop does with it."""

    def __init__(self, unet_kwargs):
        super().__init__()
        from .nernet_unet import UNetNIAM_STcell_GCB
        self.unet_kwargs = dict(unet_kwargs)
        self.num_bins, self.num_encoders = unet_kwargs["num_bins"], unet_kwargs["num_encoders"]
        self.mlp_layers, self.normalize = unet_kwargs["mlp_layers"], unet_kwargs["normalize"]
        self.network = unet_kwargs["recurrent_network"]
        self.unetrecurrent = UNetNIAM_STcell_GCB(unet_kwargs)
        self.height = self.width = self.representation = None
        self.set_resolution(256, 256)             # a placeholder, as in the reference, so that weights can be loaded

    def set_resolution(self, H, W):
        if (H, W) == (self.height, self.width):
            return
        old = None if self.representation is None else self.representation.state_dict()
        k = self.unet_kwargs
        self.height, self.width = int(H), int(W)
        rep = Voxelization(k, k["use_cnn_representation"], voxel_dimension=(self.num_bins, self.height, self.width), mlp_layers=self.mlp_layers,
                           activation=nn.LeakyReLU(negative_slope=0.1), pretrained=True, normalize=self.normalize, combine_voxel=k["combine_voxel"])
        self.representation = rep.to(next(self.unetrecurrent.parameters()).device)
        if old is not None:
            self.representation.load_state_dict(old, strict=True)
        self.crop = crop_sizes(self.height, self.width, self.num_encoders)

    @property
    def states(self):
        return self.unetrecurrent.states

    @states.setter
    def states(self, states):
        self.unetrecurrent.states = states

    def reset_states(self):
        self.unetrecurrent.reset_states()

    def _pad(self, vox):
        ph, pw, top, left = self.crop
        return torch.nn.functional.pad(vox, (left, pw - self.width - left, top, ph - self.height - top))

    def forward(self, x):
        """x: [n, 5] event rows -> ({'image': [B,1,H8,W8]} on the frame padded to multiples of 8, the padded event tensor)"""
        event_tensor = self._pad(self.representation(x))
        return self.unetrecurrent(event_tensor), event_tensor

    def forward_sequence(self, events, H, W):
        """What ModelInterface.forward_sequence_nernet (model/train_utils.py:350-378) does: T event tensors of one sequence (batch 1) ->
        [1, T, 1, H, W]; every output is cut at the top left, [:H, :W], as that caller cuts it.  The states are the caller's to reset.
        The whole sequence is voxelised with one upload and one launch pair, as Voxelization.forward_sequence does it; RepresentationCNN
        (stock torch.nn) then runs per step on a batch of one, the call forward() makes, so that a library's choice of another algorithm
        for another batch size cannot tell the two paths apart."""
        self.set_resolution(H, W)
        events, rep = list(events), self.representation
        if len(events) == 0:
            raise ValueError("forward_sequence needs at least one interval")
        offsets = torch.tensor([0] + [int(e.shape[0]) for e in events], dtype=torch.int64).cumsum(0)
        vox = rep.quantization_layer(torch.cat(events, 0), batch_size=1, offsets=offsets)         # [T, 1, 2C, H, W]
        imgs = []
        for t in range(vox.shape[0]):
            v = rep.ConvLayer(vox[t]) if rep.use_cnn_representation else vox[t]
            imgs.append(self.unetrecurrent(self._pad(v))["image"][0, :, :H, :W])
        return torch.stack(imgs)[None]
