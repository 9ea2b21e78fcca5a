"""Drop-ins for the image-loss classes of the reference's model/loss.py on the device kernels (v2v_amd/loss_ops.py): same class names (so
ModelInterface.calc_loss's log keys stay), same constructors, same __call__ signatures and the same image0 / processed0 carry-over of
temporal_consistency_loss, including the negated flow.  A V2V user switches with one import line in model/train_utils.py:

    from v2v_amd.losses import l1_loss, l2_loss, temporal_consistency_loss, perceptual_loss

perceptual_loss is LPIPS with the vgg backbone (v2v_amd/lpips.py: backbone, normalise / compare and the gradient to pred on the device
kernels).  perceptual_loss_alex is the same class for `lpips_type: alex` (v2v_amd/lpips_alex.py, float32); a configuration that trains
with it imports `perceptual_loss_alex as perceptual_loss`.  'squeeze' stays the reference's.  loss_ops.sequence_losses evaluates all T steps of the three image losses at once,
bit-identically; LPIPS has no state in time, a sequence is a batch of N*T images (loss_ops.lpips_vgg)."""
from __future__ import annotations

from .loss_ops import L1, L2, TC, MAPS, PairLossFn, sequence_losses  # noqa: F401
from .lpips import LPIPSVGG
from .lpips_alex import LPIPSAlex


def _pointwise(row, weight, pred, target, reduce_batch):
    weights = [0.0, 0.0, 0.0]
    weights[row] = float(weight)
    loss = PairLossFn.apply(None, pred, None, target, None, 50.0, tuple(weights), 1.0, False)[row]
    return loss.mean() if reduce_batch else loss


class l2_loss():
    def __init__(self, weight=1.0):
        self.weight = weight

    def __call__(self, pred, target, reduce_batch=True):
        """weight * mean((pred - target)^2): over everything, or per sample [B] with reduce_batch=False."""
        return _pointwise(L2, self.weight, pred, target, reduce_batch)


class l1_loss():
    def __init__(self, weight=1.0):
        self.weight = weight

    def __call__(self, pred, target, reduce_batch=True):
        """weight * mean(|pred - target|): over everything, or per sample [B] with reduce_batch=False."""
        return _pointwise(L1, self.weight, pred, target, reduce_batch)


class temporal_consistency_loss():
    def __init__(self, weight=1.0, L0=1):
        assert L0 > 0
        self.weight = weight
        self.L0 = L0

    def __call__(self, i, image1, processed1, flow, output_images=False, reduce_batch=True):
        """
        flow is from image0 to image1 (reversed when passed to the kernel).  Step i < L0 returns 0 and only remembers its images.
        """
        if i >= self.L0:
            out = PairLossFn.apply(self.processed0, processed1, self.image0, image1, flow, 50.0, (float(self.weight), 0.0, 0.0), -1.0, bool(output_images))
            loss = (out[0] if output_images else out)[TC]
            if reduce_batch:
                loss = loss.mean()
            if output_images:
                loss = (loss, dict(image0=self.image0, image1=image1, **dict(zip(MAPS, out[1:]))))
        else:
            loss = 0
        self.image0 = image1
        self.processed0 = processed1
        return loss


def _reference_lpips_state():
    """The weights the reference's train.py runs with: torchvision's pretrained vgg16 features under PNetLin's `net.slice*` keys + the five
    linear layers of PerceptualSimilarity/models/weights/v0.1/vgg.pth.  RuntimeError naming what is missing."""
    import os

    import torch
    from .lpips import SLICES
    try:
        from torchvision import models as tv
    except ImportError as e:
        raise RuntimeError("perceptual_loss(state_dict=None) takes the backbone from torchvision.models.vgg16(pretrained=True), and torchvision is "
                           "not importable here; pass state_dict= (a PNetLin state dict) instead") from e
    try:
        import PerceptualSimilarity
    except ImportError as e:
        raise RuntimeError("perceptual_loss(state_dict=None) takes the linear layers from the PerceptualSimilarity package's "
                           "models/weights/v0.1/vgg.pth, and that package is not importable here; pass state_dict= (a PNetLin state dict) instead") from e
    path = os.path.join(os.path.dirname(os.path.abspath(PerceptualSimilarity.__file__)), "models", "weights", "v0.1", "vgg.pth")
    if not os.path.exists(path):
        raise RuntimeError(f"perceptual_loss(state_dict=None): {path} is missing; pass state_dict= (a PNetLin state dict) instead")
    features = tv.vgg16(pretrained=True).features.state_dict()
    state = {f"net.slice{s}.{idx}.{p}": features[f"{idx}.{p}"] for s, convs in SLICES for idx, _, _ in convs for p in ("weight", "bias")}
    state.update(torch.load(path, map_location="cpu"))
    return state


class perceptual_loss():
    def __init__(self, weight=1.0, net='vgg', use_gpu=True, state_dict=None):
        """
        model/loss.py:95-119 on the device kernels, vgg only (the reference's default is net='alex'; its configs say lpips_type: vgg).
        state_dict: a PNetLin state dict (33 keys; without scaling_layer.* the reference's constants stay); None assembles the
        reference's own weights from torchvision and the PerceptualSimilarity package.
        """
        self.model = LPIPSVGG(net=net)
        state = dict(_reference_lpips_state() if state_dict is None else state_dict)
        for k, v in self.model.scaling_layer.state_dict().items():
            state.setdefault(f"scaling_layer.{k}", v)
        self.model.load_state_dict(state, strict=True)
        if use_gpu:
            self.model.cuda()
        self.weight = weight

    def __call__(self, pred, target, normalize=True, reduce_batch=True):
        """
        pred and target are Tensors with shape N x C x H x W (C {1, 3}); one channel stands for three equal ones
        normalize scales images from [0, 1] to [-1, 1] (default: True)
        returns weight * mean over the batch, or weight * dist [N] with reduce_batch=False
        """
        dist = self.model(pred, target, normalize=normalize)
        if reduce_batch:
            return self.weight * dist.mean()
        return self.weight * dist


def _reference_lpips_alex_state():
    """The weights the reference trains with under lpips_type: alex: torchvision's pretrained alexnet features under PNetLin's `net.slice*`
    keys + the five linear layers of PerceptualSimilarity/models/weights/v0.1/alex.pth.  RuntimeError naming what is missing."""
    import os

    import torch
    from .lpips_alex import CONVS
    hint = "pass state_dict= (a PNetLin state dict) instead"
    try:
        from torchvision import models as tv
    except ImportError as e:
        raise RuntimeError("perceptual_loss_alex(state_dict=None) takes the backbone from torchvision.models.alexnet(pretrained=True), and "
                           f"torchvision is not importable here; {hint}") from e
    try:
        import PerceptualSimilarity
    except ImportError as e:
        raise RuntimeError("perceptual_loss_alex(state_dict=None) takes the linear layers from the PerceptualSimilarity package's "
                           f"models/weights/v0.1/alex.pth, and that package is not importable here; {hint}") from e
    path = os.path.join(os.path.dirname(os.path.abspath(PerceptualSimilarity.__file__)), "models", "weights", "v0.1", "alex.pth")
    if not os.path.exists(path):
        raise RuntimeError(f"perceptual_loss_alex(state_dict=None): {path} is missing; {hint}")
    features = tv.alexnet(pretrained=True).features.state_dict()
    state = {f"net.slice{s}.{idx}.{p}": features[f"{idx}.{p}"] for s, idx, *_ in CONVS for p in ("weight", "bias")}
    state.update(torch.load(path, map_location="cpu"))
    return state


class perceptual_loss_alex():
    def __init__(self, weight=1.0, net='alex', use_gpu=True, state_dict=None):
        """
        model/loss.py:95-119 with net='alex' (the reference's default, and what its `lpips_type: alex` configurations train with) on the
        device kernels, float32, gradient to pred only.
        state_dict: a PNetLin state dict (17 keys; without scaling_layer.* the reference's constants stay); None assembles the
        reference's own weights from torchvision and the PerceptualSimilarity package.
        """
        self.model = LPIPSAlex(net=net)
        state = dict(_reference_lpips_alex_state() if state_dict is None else state_dict)
        for k, v in self.model.scaling_layer.state_dict().items():
            state.setdefault(f"scaling_layer.{k}", v)
        self.model.load_state_dict(state, strict=True)
        if use_gpu:
            self.model.cuda()
        self.weight = weight

    def __call__(self, pred, target, normalize=True, reduce_batch=True):
        """
        pred and target are float32 Tensors with shape N x C x H x W (C {1, 3}, H and W >= 31); one channel stands for three equal ones
        normalize scales images from [0, 1] to [-1, 1] (default: True)
        returns weight * mean over the batch, or weight * dist [N] with reduce_batch=False
        """
        dist = self.model(pred, target, normalize=normalize)
        if reduce_batch:
            return self.weight * dist.mean()
        return self.weight * dist.reshape(-1)
