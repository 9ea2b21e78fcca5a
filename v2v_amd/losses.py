"""Drop-ins for the image-loss classes of the reference's model/loss.py on the device kernels (v2v_amd/loss_ops.py): same class names (so
ModelInterface.calc_loss's log keys stay), same constructors, same __call__ signatures and the same image0 / processed0 carry-over of
temporal_consistency_loss, including the negated flow.  A V2V user switches with one import line in model/train_utils.py:

    from v2v_amd.losses import l1_loss, l2_loss, temporal_consistency_loss

perceptual_loss (LPIPS) needs the vendored network and stays the reference's.  loss_ops.sequence_losses evaluates all T steps of these three
at once, bit-identically."""
from __future__ import annotations

from .loss_ops import L1, L2, TC, MAPS, PairLossFn, sequence_losses  # noqa: F401


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
