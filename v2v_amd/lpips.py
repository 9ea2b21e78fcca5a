"""LPIPS-VGG, the perceptual loss of training (PerceptualSimilarity/models/networks_basic.py:PNetLin with pnet_type='vgg', version '0.1',
spatial=False; model/loss.py:95-119), forward and backward on the device kernels.

    LPIPSVGG()                                   the network under the reference's 33 state_dict keys (a PNetLin state dict loads strict):
                                                 scaling_layer.shift / scale, net.slice{1..5}.{idx}.{weight,bias}, lin{0..4}.model.1.weight
    LPIPSVGG.forward(pred, target, normalize)    float32 [B]: sum over the five taps of mean_pixels sum_c w_c (n0_c - n1_c)^2

Frozen and always in eval mode (the reference's DistModel calls .eval(), so its Dropout never acts; the backbone is never tuned).  The
gradient goes to pred only, float32.  Twelve of the thirteen VGG convolutions run on conv_nhwc (bf16 NHWC, fp32 accumulation) and their
data gradients on the same kernel with the dgrad-packed stream -- what conv_dgrad_nhwc launches at stride 1 -- inside tile_like_batch, so
that the kernel instance, and with it every sample's bits, does not depend on how many images share a launch.  Stem, 2x2 max-pool and
the normalise / compare step are the kernels of v2v_amd/csrc/v2v_lpips.hpp (raw operators: v2v_amd/loss_ops.py).  The batch is cut into
chunks; pred and target of a chunk go through the backbone as one batch of 2 * chunk images; the backward runs the pred half only.

Deviation from autograd, stated: at a pixel whose pred features are ALL zero at a tap the reference's gradient is NaN (sqrt' at 0); here
the norm's derivative is taken as 0 there (loss_ops.lpips_compare_bwd)."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib, loss_ops
from .nhwc_ops import conv_nhwc, pack_conv_weights, pack_dgrad_weights, packed_weights, relu_bwd_nhwc, tile_like_batch

# torchvision's vgg16().features cut where PerceptualSimilarity/models/pretrained_networks.py:97-135 cuts it: (slice, [(index, Cin, Cout)]);
# a 2x2 max-pool opens every slice but the first, a ReLU follows every convolution, the tap is the slice's last ReLU
SLICES = ((1, ((0, 3, 64), (2, 64, 64))),
          (2, ((5, 64, 128), (7, 128, 128))),
          (3, ((10, 128, 256), (12, 256, 256), (14, 256, 256))),
          (4, ((17, 256, 512), (19, 512, 512), (21, 512, 512))),
          (5, ((24, 512, 512), (26, 512, 512), (28, 512, 512))))
CHANNELS = (64, 128, 256, 512, 512)
DEFAULT_CHUNK = 12                  # the training batch: one launch per layer for a time step
_LIKE_FWD, _LIKE_BWD = 2 * DEFAULT_CHUNK, DEFAULT_CHUNK            # tile_like_batch: every launch runs the instance of the default chunk


def check_size(h: int, w: int) -> None:
    """ValueError unless the convolution kernels take every level of an H x W image: H, W multiples of 16, (H/16 * W/16) % 4 == 0."""
    if h < 16 or w < 16 or h % 16 or w % 16 or ((h // 16) * (w // 16)) % 4:
        raise ValueError(f"LPIPSVGG needs H and W multiples of 16 whose 1/16-scale map has a multiple of 4 pixels (32x32, 16x64, 48x64, 128x128); got {h}x{w}")


class _Lin(nn.Module):
    """NetLinLayer (networks_basic.py:113-120): Dropout (never active) + 1x1 convolution to one channel without bias, key `model.1.weight`."""

    def __init__(self, c):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(c, 1, 1, stride=1, padding=0, bias=False))


class _Scaling(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.tensor([.458, .448, .450])[None, :, None, None])


class _Backbone(nn.Module):
    def __init__(self):
        super().__init__()
        for s, convs in SLICES:
            seq = nn.Sequential()
            if s > 1:
                seq.add_module(str(convs[0][0] - 1), nn.MaxPool2d(2, 2))
            for idx, cin, cout in convs:
                seq.add_module(str(idx), nn.Conv2d(cin, cout, 3, padding=1))
                seq.add_module(str(idx + 1), nn.ReLU())
            setattr(self, f"slice{s}", seq)


class LPIPSVGG(nn.Module):
    def __init__(self, net: str = "vgg", spatial: bool = False, pnet_tune: bool = False, chunk: int = DEFAULT_CHUNK):
        super().__init__()
        if net not in ("vgg", "vgg16"):
            raise ValueError(f"LPIPSVGG runs the vgg backbone only (got net={net!r}); alex is v2v_amd.lpips_alex.LPIPSAlex, squeeze stays the reference's")
        if spatial or pnet_tune:
            raise ValueError("LPIPSVGG has no spatial=True map and a frozen backbone (pnet_tune=False)")
        if int(chunk) < 1:
            raise ValueError("chunk must be at least 1")
        self.scaling_layer = _Scaling()
        self.net = _Backbone()
        for k, c in enumerate(CHANNELS):
            setattr(self, f"lin{k}", _Lin(c))
        self.chunk = int(chunk)
        self._packed = {}                                              # nhwc_ops.packed_weights' cache
        for p in self.parameters():
            p.requires_grad_(False)
        super().train(False)

    def train(self, mode: bool = True):
        """Always in eval mode, as under the reference's DistModel."""
        return super().train(False)

    def _conv(self, s, idx):
        return getattr(getattr(self.net, f"slice{s}"), str(idx))

    def _lin(self, k):
        return getattr(self, f"lin{k}").model[1].weight

    def _weights(self, backward: bool = False):
        """Everything a pass needs packed, now (on the current stream): {(slice, index): (packed stream, float32 bias)}; backward: the
        dgrad-packed stream and a zero bias of Cin."""
        out = {}
        for s, convs in SLICES:
            for idx, cin, cout in convs:
                if idx == 0:
                    continue
                conv = self._conv(s, idx)
                if backward:
                    out[s, idx] = (packed_weights(self._packed, f"dgrad{idx}", conv.weight, pack_dgrad_weights),
                                   packed_weights(self._packed, f"zero{idx}", conv.weight, lambda w, n=cin: torch.zeros(n, dtype=torch.float32, device=w.device)))
                else:
                    out[s, idx] = (packed_weights(self._packed, f"conv{idx}", conv.weight, pack_conv_weights), conv.bias)
        return out

    # ---- one chunk ------------------------------------------------------------------------------------------------------------------------
    def _chunk_forward(self, pred, target, normalize, dist, save):
        """dist float32 [c] (zeros) += the five taps; save: returns what _chunk_backward reads (the pred half's post-ReLU activations, the
        taps in both halves)."""
        c, _, h, w = pred.shape
        stem, sc = self._conv(1, 0), self.scaling_layer
        weights = self._weights()
        x = torch.empty((2 * c, h, w, 64), dtype=torch.bfloat16, device=pred.device)
        for half, img in ((x[:c], pred), (x[c:], target)):
            loss_ops.lpips_stem(img, stem.weight, stem.bias, sc.shift, sc.scale, normalize, out=half)
        acts, taps = {(1, 0): x[:c]}, []
        with tile_like_batch(_LIKE_FWD):
            for k, (s, convs) in enumerate(SLICES):
                if s > 1:
                    x = loss_ops.lpips_pool(x)
                for idx, _, _ in convs:
                    if idx == 0:
                        continue
                    x = conv_nhwc(x, *weights[s, idx], 3, relu=True)
                    acts[s, idx] = x[:c]
                loss_ops.lpips_compare_fwd(x[:c], x[c:], self._lin(k), dist)
                taps.append((x[:c], x[c:]))
        return (acts, taps) if save else None

    def _chunk_backward(self, saved, ddist, cin, normalize):
        acts, taps = saved
        weights = self._weights(backward=True)
        dpool = None
        with tile_like_batch(_LIKE_BWD):
            for k in range(len(SLICES) - 1, -1, -1):
                s, convs = SLICES[k]
                f0, f1 = taps[k]
                df = loss_ops.lpips_compare_bwd(f0, f1, self._lin(k), ddist)
                # the tap's gradient: the compare term + what comes back through the next slice's pool, through the tap's ReLU
                dz = relu_bwd_nhwc(df, f0) if dpool is None else loss_ops.lpips_pool_bwd(dpool, f0, dtap=df, relu_mask=True)
                for j in range(len(convs) - 1, -1, -1):
                    idx = convs[j][0]
                    if idx == 0:
                        stem = self._conv(1, 0)
                        return loss_ops.lpips_stem_bwd(dz, stem.weight, self.scaling_layer.scale, cin, normalize)
                    dx = conv_nhwc(dz, *weights[s, idx], 3)
                    if j > 0:
                        dz = relu_bwd_nhwc(dx, acts[s, convs[j - 1][0]])
                    else:
                        dpool = dx
        raise AssertionError("unreachable: the first slice ends in the stem")

    def forward(self, pred, target, normalize: bool = False, chunk: int | None = None):
        """pred, target float32 / bfloat16 [B,1|3,H,W] -> dist float32 [B].  chunk: images per backbone launch (default: the module's);
        per-sample results do not depend on it, bit for bit."""
        for name, t in (("pred", pred), ("target", target)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] not in (1, 3) or t.dtype not in (torch.float32, torch.bfloat16):
                raise ValueError(f"{name} must be a float32 or bfloat16 tensor [B,1|3,H,W]")
        if pred.shape[0] != target.shape[0] or pred.shape[2:] != target.shape[2:]:
            raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} must agree in batch and image size")
        check_size(pred.shape[2], pred.shape[3])
        if target.requires_grad:
            raise ValueError("LPIPSVGG has no gradient to target: detach it")
        chunk = self.chunk if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError("chunk must be at least 1")
        _lib.require_gpu()
        if not pred.is_cuda or target.device != pred.device or self.scaling_layer.shift.device != pred.device:
            raise ValueError("pred, target and the module must be on one CUDA device (v2v_amd has no CPU fallback)")
        return _LPIPSFn.apply(pred, target, self, bool(normalize), chunk)


class _LPIPSFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, model, normalize, chunk):
        b = pred.shape[0]
        dist = torch.zeros((b,), dtype=torch.float32, device=pred.device)
        save = ctx.needs_input_grad[0]
        ctx.saved = []
        for i in range(0, b, chunk):
            ctx.saved.append(model._chunk_forward(pred[i:i + chunk].detach(), target[i:i + chunk].detach(), normalize, dist[i:i + chunk], save))
        ctx.cfg = (model, normalize, chunk, tuple(pred.shape))
        return dist

    @staticmethod
    def backward(ctx, ddist):
        model, normalize, chunk, shape = ctx.cfg
        ddist = ddist.detach().to(torch.float32).contiguous()
        dpred = torch.empty(shape, dtype=torch.float32, device=ddist.device)
        for n, i in enumerate(range(0, shape[0], chunk)):
            dpred[i:i + chunk] = model._chunk_backward(ctx.saved[n], ddist[i:i + chunk], shape[1], normalize)
        return dpred, None, None, None, None
