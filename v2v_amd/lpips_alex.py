"""LPIPS-AlexNet, the third metric of the reference's test loop (PerceptualSimilarity/models/networks_basic.py:PNetLin with pnet_type='alex',
version '0.1', spatial=False; ModelInterface.compute_metrics, model/train_utils.py:198, 236; as a training loss model/loss.py:95-119 with
net='alex'), on the device kernels of v2v_amd/csrc/v2v_alex.hpp (include/v2v_lpips_alex.h) and, for the backward to pred, of
v2v_amd/csrc/v2v_alex_train.hpp (include/v2v_alex_train.h).

    LPIPSAlex()                                  the network under the reference's 17 state_dict keys (PerceptualLoss(net="alex").model.net's
                                                 state dict loads strict): scaling_layer.shift / scale, net.slice{1..5}.{idx}.{weight,bias},
                                                 lin{0..4}.model.1.weight
    LPIPSAlex.forward(pred, target, normalize)   float32 [B,1,1,1] as the reference returns it: a drop-in `lpips_fn`; differentiable with
                                                 respect to pred when pred requires grad (the loss: v2v_amd.losses.perceptual_loss_alex)
    LPIPSAlex.sequence(pred, frame, ...)         all T frames of a sequence: float32 [T] on the device (and the float64 tap means [T,5]), a
                                                 handful of launches per chunk, no host synchronisation
    stem / conv / pool / compare / tap_sum       the raw operators, one per kernel
    compare_bwd / conv_dgrad / pool_bwd / stem_bwd   the raw operators of the backward; pack_dgrad_weights
    tap_sizes(h, w)                              the five (H, W) of the taps

A metric, so float32 end to end: float32 NHWC activations, float32 weights, float32 accumulation on the float32-input matrix-core
instruction (a k-ordered fmaf chain), norms and sums in float64.  No split-K and nothing that depends on how many images share a launch:
per-frame results do not depend on T or on the chunk, bit for bit.  Frozen and always in eval mode.  No CPU path.  The gradient goes to
pred only, float32, through kernels under the same rules (one fixed summation order per element, no atomics): two backward runs agree
bit for bit, for any chunk.  sequence() is a metric and records no gradient.  The path that records the gradient cuts the batch into
chunks of grad_chunk images (default 480, fewer for large frames: GRAD_CHUNK_ELEMS), the metric paths into chunks of `chunk` (40).

Deviation from autograd, stated (as v2v_amd/lpips.py does for vgg): at a pixel whose pred features are ALL zero at a tap the reference's
gradient is NaN (sqrt' at 0); here the norm's derivative is taken as 0 there."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import launch, need, ptr
from .nhwc_ops import packed_weights

# torchvision's alexnet().features cut where PerceptualSimilarity/models/pretrained_networks.py:57-95 cuts it:
# (slice, index of the convolution, Cin, Cout, kernel, stride, padding, a 3x3 / stride-2 max-pool opens the slice)
CONVS = ((1, 0, 3, 64, 11, 4, 2, False), (2, 3, 64, 192, 5, 1, 2, True), (3, 6, 192, 384, 3, 1, 1, True), (4, 8, 384, 256, 3, 1, 1, False),
         (5, 10, 256, 256, 3, 1, 1, False))
CHANNELS = (64, 192, 384, 256, 256)
MIN_SIDE = 31                       # 31 -> 7 -> 3 -> 1
DEFAULT_CHUNK = 40                  # the frames of a test sequence: one launch per layer
DEFAULT_GRAD_CHUNK = 480            # as a loss: the 12 x 40 images of a training sequence, one launch per layer (40 images leave the GPU half idle)
GRAD_CHUNK_ELEMS = 1 << 28          # ... but no more images than keep the first tap of a chunk (pred and target) within 2^28 floats


def tap_sizes(h: int, w: int):
    """The five (H, W) of the taps of an h x w image; ValueError below 31."""
    if h < MIN_SIDE or w < MIN_SIDE:
        raise ValueError(f"LPIPS-alex needs H and W >= {MIN_SIDE} (got {h}x{w})")
    s1 = ((h - 7) // 4 + 1, (w - 7) // 4 + 1)
    s2 = ((s1[0] - 3) // 2 + 1, (s1[1] - 3) // 2 + 1)
    s3 = ((s2[0] - 3) // 2 + 1, (s2[1] - 3) // 2 + 1)
    return (s1, s2, s3, s3, s3)


# ---- raw operators -----------------------------------------------------------------------------------------------------------------------
def pack_stem_weights(w: torch.Tensor) -> torch.Tensor:
    """[64,3,11,11] -> float32 [3,122,64]: [c][ky * 11 + kx][o], row 121 zero (the k-step of the instruction is 2)."""
    out = torch.zeros((3, 122, 64), dtype=torch.float32, device=w.device)
    out[:, :121] = w.detach().to(torch.float32).reshape(64, 3, 121).permute(1, 2, 0)
    return out


def pack_conv_weights(w: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,KS,KS] -> float32 [KS*KS*Cin, Cout] with k = (ky * KS + kx) * Cin + ci: NHWC channel runs are contiguous in k."""
    cout, cin, ks, _ = w.shape
    return w.detach().to(torch.float32).permute(2, 3, 1, 0).reshape(ks * ks * cin, cout).contiguous()


def _vec(name, t, n, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.device != dev or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 CUDA tensor of {n} elements on the input's device")
    return t


def stem(frames: torch.Tensor, frame_stride: int, packed, bias, shift, scale, divisor: float = 1.0, normalize: bool = False, out=None):
    """frames float32 [n,1|3,H,W], every frame contiguous, frame_stride elements apart -> float32 NHWC [n,OH,OW,64]"""
    _lib.require_gpu()
    n, c, h, w = frames.shape
    (oh, ow) = tap_sizes(h, w)[0]
    dev = frames.device
    if out is None:
        out = torch.empty((n, oh, ow, 64), dtype=torch.float32, device=dev)
    need("out", out, torch.float32, shape=(n, oh, ow, 64), device=dev, owner="frames")
    need("packed", packed, torch.float32, shape=(3, 122, 64), device=dev, owner="frames")
    launch("v2v_lpips_alex_stem_hip", dev, ptr(frames), int(frame_stride), n, c, h, w, float(divisor), int(bool(normalize)), ptr(_vec("shift", shift, 3, dev)),
           ptr(_vec("scale", scale, 3, dev)), ptr(packed), ptr(_vec("bias", bias, 64, dev)), ptr(out))
    return out


def conv(x: torch.Tensor, packed: torch.Tensor, bias: torch.Tensor, ks: int, relu: bool = True):
    """x float32 NHWC [n,H,W,Cin], packed [ks*ks*Cin, Cout] -> float32 NHWC [n,H,W,Cout]: stride 1, pad ks // 2, + bias, ReLU"""
    _lib.require_gpu()
    need("x", x, torch.float32)
    n, h, w, cin = x.shape
    if packed.dim() != 2 or packed.shape[0] != ks * ks * cin:
        raise ValueError(f"packed must be [{ks * ks * cin}, Cout] (got {tuple(packed.shape)})")
    cout = packed.shape[1]
    need("packed", packed, torch.float32, shape=(ks * ks * cin, cout), device=x.device)
    y = torch.empty((n, h, w, cout), dtype=torch.float32, device=x.device)
    launch("v2v_lpips_alex_conv_hip", x.device, ptr(x), ptr(packed), ptr(_vec("bias", bias, cout, x.device)), n, h, w, cin, cout, int(ks), int(bool(relu)), ptr(y))
    return y


def pool(x: torch.Tensor):
    """x float32 NHWC [n,H,W,C] -> [n,(H-3)//2+1,(W-3)//2+1,C]: 3x3 / stride 2 max-pool, floor mode"""
    _lib.require_gpu()
    need("x", x, torch.float32)
    n, h, w, c = x.shape
    if h < 3 or w < 3:
        raise ValueError(f"the 3x3 pool needs H, W >= 3 (got {h}x{w})")
    y = torch.empty((n, (h - 3) // 2 + 1, (w - 3) // 2 + 1, c), dtype=torch.float32, device=x.device)
    launch("v2v_lpips_alex_pool_hip", x.device, ptr(x), n, h, w, c, ptr(y))
    return y


def compare(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor, tap: int, taps: torch.Tensor):
    """f0, f1 float32 NHWC [n,H,W,C], w [C] -> taps[:, tap] (float64 [n,5]) = mean over the pixels of sum_c w_c (n0_c - n1_c)^2"""
    _lib.require_gpu()
    need("f0", f0, torch.float32)
    need("f1", f1, torch.float32, shape=tuple(f0.shape), device=f0.device, owner="f0")
    n, h, wd, c = f0.shape
    need("taps", taps, torch.float64, shape=(n, 5), device=f0.device, owner="f0")
    nbytes = _lib.lib().v2v_lpips_alex_compare_workspace_bytes(n, h * wd)
    _lib.check(min(nbytes, 0))
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=f0.device)
    launch("v2v_lpips_alex_compare_hip", f0.device, ptr(f0), ptr(f1), ptr(_vec("w", w, c, f0.device)), n, h * wd, c, int(tap), ptr(ws), ptr(taps))
    return taps


def tap_sum(taps: torch.Tensor, out=None):
    """taps float64 [n,5] -> float32 [n]: the five means, each rounded to float32, added in tap order"""
    _lib.require_gpu()
    if not isinstance(taps, torch.Tensor) or taps.dim() != 2 or taps.shape[1] != 5:
        raise ValueError("taps must be float64 [n,5]")
    need("taps", taps, torch.float64, shape=tuple(taps.shape))
    n = taps.shape[0]
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=taps.device)
    need("out", out, torch.float32, shape=(n,), device=taps.device, owner="taps")
    launch("v2v_lpips_alex_sum_hip", taps.device, ptr(taps), n, ptr(out))
    return out


# ---- raw operators of the backward to pred (include/v2v_alex_train.h) --------------------------------------------------------------------
def pack_dgrad_weights(w: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,KS,KS] -> float32 [KS*KS*Cout, Cin]: row (ky * KS + kx) * Cout + co holds w[co][:][KS-1-ky][KS-1-kx] -- the forward's
    implicit GEMM run over dy gives the input gradient."""
    cout, cin, ks, _ = w.shape
    return w.detach().to(torch.float32).flip(2, 3).permute(2, 3, 0, 1).reshape(ks * ks * cout, cin).contiguous()


def compare_bwd(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor, ddist: torch.Tensor, relu_mask: bool = False):
    """f0 (pred), f1 (target) float32 NHWC [n,H,W,C], w [C], ddist float32 [n] or [n,1,1,1] -> float32 [n,H,W,C]: the gradient of
    sum_i ddist_i * (tap mean of image i) at f0, per pixel in float64, rounded once; relu_mask: 0 where f0 is not > 0.  Always a fresh
    buffer: a tap's gradient joins the chain as the `dtap` of conv_dgrad / pool_bwd, nothing accumulates in place."""
    _lib.require_gpu()
    need("f0", f0, torch.float32)
    need("f1", f1, torch.float32, shape=tuple(f0.shape), device=f0.device, owner="f0")
    n, h, wd, c = f0.shape
    if not isinstance(ddist, torch.Tensor) or tuple(ddist.shape) not in ((n,), (n, 1, 1, 1)):
        raise ValueError(f"ddist must be float32 [{n}] or [{n},1,1,1]")
    dz = torch.empty_like(f0)
    launch("v2v_alex_train_compare_bwd_hip", f0.device, ptr(f0), ptr(f1), ptr(_vec("w", w, c, f0.device)), ptr(_vec("ddist", ddist, n, f0.device)), n, h * wd, c,
           int(bool(relu_mask)), ptr(dz))
    return dz


def conv_dgrad(dy: torch.Tensor, packed: torch.Tensor, ks: int, dtap=None, mask=None):
    """dy float32 NHWC [n,H,W,Cout], packed = pack_dgrad_weights(w) [ks*ks*Cout, Cin] -> dx float32 [n,H,W,Cin] = the input gradient of the
    stride-1 convolution + dtap, 0 where mask (the post-ReLU activation that fed the convolution) is not > 0; both optional, [n,H,W,Cin]."""
    _lib.require_gpu()
    need("dy", dy, torch.float32)
    n, h, w, cout = dy.shape
    if packed.dim() != 2 or packed.shape[0] != ks * ks * cout:
        raise ValueError(f"packed must be [{ks * ks * cout}, Cin] (got {tuple(packed.shape)})")
    cin = packed.shape[1]
    need("packed", packed, torch.float32, shape=(ks * ks * cout, cin), device=dy.device, owner="dy")
    for name, t in (("dtap", dtap), ("mask", mask)):
        if t is not None:
            need(name, t, torch.float32, shape=(n, h, w, cin), device=dy.device, owner="dy")
    dx = torch.empty((n, h, w, cin), dtype=torch.float32, device=dy.device)
    launch("v2v_alex_train_conv_dgrad_hip", dy.device, ptr(dy), ptr(packed), ptr(dtap), ptr(mask), n, h, w, cin, cout, int(ks), ptr(dx))
    return dx


def pool_bwd(x: torch.Tensor, dy: torch.Tensor, dtap=None, relu_mask: bool = False):
    """x float32 NHWC [n,H,W,C] (the pool's input), dy [n,(H-3)//2+1,(W-3)//2+1,C] -> dx [n,H,W,C]: dy gathered at each window's first
    maximum, + dtap (optional, like x), 0 where x is not > 0 when relu_mask."""
    _lib.require_gpu()
    need("x", x, torch.float32)
    n, h, w, c = x.shape
    if h < 3 or w < 3:
        raise ValueError(f"the 3x3 pool needs H, W >= 3 (got {h}x{w})")
    need("dy", dy, torch.float32, shape=(n, (h - 3) // 2 + 1, (w - 3) // 2 + 1, c), device=x.device)
    if dtap is not None:
        need("dtap", dtap, torch.float32, shape=tuple(x.shape), device=x.device)
    dx = torch.empty_like(x)
    launch("v2v_alex_train_pool_bwd_hip", x.device, ptr(x), ptr(dy), ptr(dtap), n, h, w, c, int(bool(relu_mask)), ptr(dx))
    return dx


def stem_bwd(dz: torch.Tensor, packed: torch.Tensor, scale: torch.Tensor, cin: int, h: int, w: int, divisor: float = 1.0, normalize: bool = False, out=None):
    """dz float32 NHWC [n,OH,OW,64] (the gradient at the stem's pre-activation), packed = pack_stem_weights(w) -> float32 [n,cin,h,w]: the
    gradient at the frames stem() read with the same divisor / normalize."""
    _lib.require_gpu()
    need("dz", dz, torch.float32)
    n = dz.shape[0]
    (oh, ow) = tap_sizes(h, w)[0]
    dev = dz.device
    need("dz", dz, torch.float32, shape=(n, oh, ow, 64))
    need("packed", packed, torch.float32, shape=(3, 122, 64), device=dev, owner="dz")
    if cin not in (1, 3):
        raise ValueError(f"cin must be 1 or 3 (got {cin})")
    if out is None:
        out = torch.empty((n, cin, h, w), dtype=torch.float32, device=dev)
    need("out", out, torch.float32, shape=(n, cin, h, w), device=dev, owner="dz")
    launch("v2v_alex_train_stem_bwd_hip", dev, ptr(dz), ptr(packed), ptr(_vec("scale", scale, 3, dev)), n, int(cin), int(h), int(w), float(divisor),
           int(bool(normalize)), ptr(out))
    return out


# ---- the module --------------------------------------------------------------------------------------------------------------------------
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
        for s, idx, cin, cout, ks, stride, pad, pooled in CONVS:
            seq = nn.Sequential()
            if pooled:
                seq.add_module(str(idx - 1), nn.MaxPool2d(3, 2))
            seq.add_module(str(idx), nn.Conv2d(cin, cout, ks, stride=stride, padding=pad))
            seq.add_module(str(idx + 1), nn.ReLU())
            setattr(self, f"slice{s}", seq)


def _images(name, t):
    """t as [B, 1|3, H, W]: float32, CUDA, every image contiguous.  -> (tensor, image stride)"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 (got {t.dtype})")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA tensor (v2v_amd has no CPU fallback)")
    if t.dim() != 4 or t.shape[1] not in (1, 3):
        raise ValueError(f"{name} must be [B,1|3,H,W] (got {tuple(t.shape)})")
    t = t.detach()
    _, c, h, w = t.shape
    if t.stride()[1:] != (h * w, w, 1) or t.stride(0) < 0:
        t = t.contiguous()
    return t, t.stride(0)


class LPIPSAlex(nn.Module):
    def __init__(self, net: str = "alex", spatial: bool = False, chunk: int = DEFAULT_CHUNK, grad_chunk: int = DEFAULT_GRAD_CHUNK):
        super().__init__()
        if net != "alex":
            raise ValueError(f"LPIPSAlex runs the alex backbone only (got net={net!r}); vgg is v2v_amd.lpips.LPIPSVGG")
        if spatial:
            raise ValueError("LPIPSAlex has no spatial=True map")
        if int(chunk) < 1 or int(grad_chunk) < 1:
            raise ValueError("chunk and grad_chunk must be at least 1")
        self.scaling_layer = _Scaling()
        self.net = _Backbone()
        for k, c in enumerate(CHANNELS):
            setattr(self, f"lin{k}", _Lin(c))
        self.chunk = int(chunk)                                         # images per backbone launch of the metric paths
        self.grad_chunk = int(grad_chunk)                               # ... of the path that records the gradient (results do not depend on either)
        self._packed = {}                                              # nhwc_ops.packed_weights' cache
        for p in self.parameters():
            p.requires_grad_(False)
        super().train(False)

    def train(self, mode: bool = True):
        """Always in eval mode, as under the reference's DistModel."""
        return super().train(False)

    def _conv(self, s, idx):
        return getattr(getattr(self.net, f"slice{s}"), str(idx))

    def _weights(self):
        """Everything a pass needs, packed now (on the current stream): [(packed weight, bias)] per convolution, the five lin vectors,
        shift and scale as [3]."""
        convs = []
        for s, idx, *_ in CONVS:
            c = self._conv(s, idx)
            convs.append((packed_weights(self._packed, f"conv{idx}", c.weight, pack_stem_weights if idx == 0 else pack_conv_weights),
                          packed_weights(self._packed, f"bias{idx}", c.bias, lambda b: b.to(torch.float32).contiguous())))
        lins = [packed_weights(self._packed, f"lin{k}", getattr(self, f"lin{k}").model[1].weight, lambda w: w.to(torch.float32).reshape(-1).contiguous())
                for k in range(5)]
        sc = self.scaling_layer
        shift = packed_weights(self._packed, "shift", sc.shift, lambda v: v.to(torch.float32).reshape(-1).contiguous())
        scale = packed_weights(self._packed, "scale", sc.scale, lambda v: v.to(torch.float32).reshape(-1).contiguous())
        return convs, lins, shift, scale

    def _chunk(self, pred, ps, target, ts, divisor, normalize, taps, save=False):
        """taps float64 [c,5] <- the five tap means of c image pairs; both images of a pair go through the backbone in one batch of 2 c.
        save: returns the five (pred, target) post-ReLU taps, what _chunk_backward reads."""
        c, _, h, w = pred.shape
        convs, lins, shift, scale = self._weights()
        (oh, ow) = tap_sizes(h, w)[0]
        x = torch.empty((2 * c, oh, ow, 64), dtype=torch.float32, device=pred.device)
        for half, img, stride in ((x[:c], pred, ps), (x[c:], target, ts)):
            stem(img, stride, *convs[0], shift, scale, divisor, normalize, out=half)
        saved = []
        for k, (_, _, _, _, ks, _, _, pooled) in enumerate(CONVS):
            if k:
                if pooled:
                    x = pool(x)
                x = conv(x, *convs[k], ks, relu=True)
            compare(x[:c], x[c:], lins[k], k, taps)
            if save:
                saved.append((x[:c], x[c:]))
        return saved

    def _chunk_backward(self, saved, ddist, cin, h, w, divisor, normalize, out):
        """out float32 [c,cin,h,w] <- the gradient of sum_i ddist_i * dist_i at the c predictions of a chunk.  A tap's compare gradient is
        a buffer of its own (`dtap`) that the kernel of the layer above adds in its epilogue, where the tap's ReLU is applied too."""
        convs, lins, _, scale = self._weights()
        dgrad = [None] + [packed_weights(self._packed, f"dgrad{idx}", self._conv(s, idx).weight, pack_dgrad_weights) for s, idx, *_ in CONVS[1:]]
        tap = lambda k, relu=False: compare_bwd(*saved[k], lins[k], ddist, relu_mask=relu)   # noqa: E731
        d = tap(4, relu=True)                                           # at conv5's pre-activation
        d = conv_dgrad(d, dgrad[4], 3, dtap=tap(3), mask=saved[3][0])   # at conv4's
        d = conv_dgrad(d, dgrad[3], 3, dtap=tap(2), mask=saved[2][0])   # at conv3's
        d = conv_dgrad(d, dgrad[2], 3)                                  # at the second pool's output
        d = pool_bwd(saved[1][0], d, dtap=tap(1), relu_mask=True)       # at conv2's pre-activation
        d = conv_dgrad(d, dgrad[1], 5)                                  # at the first pool's output
        d = pool_bwd(saved[0][0], d, dtap=tap(0), relu_mask=True)       # at the stem's pre-activation
        return stem_bwd(d, convs[0][0], scale, cin, h, w, divisor, normalize, out=out)

    def _run(self, pred, ps, target, ts, divisor, normalize, chunk, save=False):
        if pred.shape != target.shape:
            raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
        if pred.device != target.device or self.scaling_layer.shift.device != pred.device:
            raise ValueError("pred, target and the module must be on one CUDA device (v2v_amd has no CPU fallback)")
        tap_sizes(pred.shape[2], pred.shape[3])
        if not (divisor == divisor and abs(divisor) != float("inf") and divisor != 0):
            raise ValueError(f"divisor must be finite and non-zero (got {divisor})")
        if chunk < 1:
            raise ValueError("chunk must be at least 1")
        n = pred.shape[0]
        taps = torch.empty((n, 5), dtype=torch.float64, device=pred.device)
        dist = torch.empty((n,), dtype=torch.float32, device=pred.device)
        saved = [self._chunk(pred[i:i + chunk], ps, target[i:i + chunk], ts, divisor, normalize, taps[i:i + chunk], save) for i in range(0, n, chunk)]
        if n:
            tap_sum(taps, out=dist)
        return (dist, taps, saved) if save else (dist, taps)

    def forward(self, pred, target, normalize: bool = False):
        """pred, target float32 CUDA [1|3,H,W] or [B,1|3,H,W] -> float32 [B,1,1,1], as PerceptualLoss.forward(pred, target, normalize).
        With gradient recording on and a pred that requires grad the result carries the gradient to pred (the same kernels and the same
        bits forward); target must not require grad."""
        _lib.require_gpu()
        pred, target = (t.unsqueeze(0) if isinstance(t, torch.Tensor) and t.dim() == 3 else t for t in (pred, target))
        if isinstance(pred, torch.Tensor) and pred.requires_grad and torch.is_grad_enabled():
            if isinstance(target, torch.Tensor) and target.requires_grad:
                raise ValueError("LPIPSAlex has no gradient to target: detach it")
            _images("pred", pred)
            _images("target", target)
            (oh, ow) = tap_sizes(pred.shape[2], pred.shape[3])[0]
            chunk = max(1, min(self.grad_chunk, GRAD_CHUNK_ELEMS // (2 * 64 * oh * ow)))
            return _LPIPSAlexFn.apply(pred, target, self, bool(normalize), chunk).reshape(-1, 1, 1, 1)
        pred, ps = _images("pred", pred)
        target, ts = _images("target", target)
        dist, _ = self._run(pred, ps, target, ts, 1.0, bool(normalize), self.chunk)
        return dist.reshape(-1, 1, 1, 1)

    def sequence(self, pred, frame, divisor: float = 255.0, normalize: bool = True, chunk: int | None = None, taps: bool = False):
        """pred, frame float32 CUDA [T,1|3,H,W] or [1,T,1|3,H,W] -> float32 [T] on the device: LPIPS of `pred / divisor` against
        `frame / divisor` (2x - 1 first when normalize, as the reference's test loop asks); with taps also the float64 tap means [T,5].
        chunk: frames per backbone launch (default: the module's); per-frame results do not depend on it, bit for bit.  Nothing is copied
        to the host."""
        _lib.require_gpu()
        pred, frame = (t[0] if isinstance(t, torch.Tensor) and t.dim() == 5 and t.shape[0] == 1 else t for t in (pred, frame))
        pred, ps = _images("pred", pred)
        frame, fs = _images("frame", frame)
        dist, tp = self._run(pred, ps, frame, fs, float(divisor), bool(normalize), self.chunk if chunk is None else int(chunk))
        return (dist, tp) if taps else dist


class _LPIPSAlexFn(torch.autograd.Function):
    """forward: LPIPSAlex._run as it is, keeping every chunk's taps; backward: LPIPSAlex._chunk_backward chunk by chunk, no host
    synchronisation."""

    @staticmethod
    def forward(ctx, pred, target, model, normalize, chunk):
        p, ps = _images("pred", pred)
        t, ts = _images("target", target)
        dist, _, ctx.saved = model._run(p, ps, t, ts, 1.0, normalize, chunk, save=True)
        ctx.cfg = (model, normalize, chunk, tuple(p.shape))
        return dist

    @staticmethod
    def backward(ctx, ddist):
        model, normalize, chunk, (n, cin, h, w) = ctx.cfg
        ddist = ddist.detach().to(torch.float32).reshape(-1).contiguous()
        dpred = torch.empty((n, cin, h, w), dtype=torch.float32, device=ddist.device)
        for k, i in enumerate(range(0, n, chunk)):
            model._chunk_backward(ctx.saved[k], ddist[i:i + chunk], cin, h, w, 1.0, normalize, dpred[i:i + chunk])
        return dpred, None, None, None, None
