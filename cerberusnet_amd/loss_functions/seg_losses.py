"""Drop-in for the segmentation losses of ``nnet_training/loss_functions/seg_losses.py`` (:121-190).

``FocalLoss2D`` and ``SegCrossEntropy`` keep their names, constructor signatures, defaults and ``forward(predictions,
targets)`` with the ``'seg'`` keys.  Both are ``weight * focal(F.cross_entropy(logits, target, weight=w, ignore_index=i))``
with ``focal(ce) = (1 - exp(-ce))^gamma * ce`` applied to the scalar MEAN, as the reference does (:150-154; gamma = 0 for
``SegCrossEntropy``), and ``w`` either ones or the reference's dynamic class-balance weights.

With ``backend='hip'`` fp32 CUDA logits take ONE fused HIP forward and one fused backward (``cerberus::seg_cross_entropy``,
``csrc/seg_loss.hip``): the (B,C,H,W) logits are read once forward, read once and written once backward, against the stock
chain's log_softmax / nll_loss2d and their backwards.  The dynamic weights come from ``cerberus::class_histogram`` and a
``torch.where`` on the (C,) counts -- no ``unique``, no host synchronisation, so the whole loss can be captured in a graph.
``backend='torch'`` restates the reference in its own operation order.

Differences from the reference, both supersets: the class weights follow the logits' device (the reference's
``.get_device()`` call breaks on CPU tensors), and a ``(B,1,H,W)`` target is squeezed in both classes (the reference does it
in ``SegCrossEntropy`` only).
"""
from typing import Dict

import torch
import torch.nn.functional as F

from .. import ops as _ops

__all__ = ["seg_cross_entropy", "class_balance_weights", "FocalLoss2D", "SegCrossEntropy"]


def _focal(ce, gamma):
    return ce if gamma == 0 else torch.pow(1 - torch.exp(-ce), gamma) * ce


def _fusable(logits, target, weight):
    """What cerberus::seg_cross_entropy takes: fp32 CUDA logits (B,C,H,W) with C >= 2 and a pixel, an int64 (B,H,W) target on
    the same device, fp32 class weights (or none) that want no gradient."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4 and logits.shape[1] >= 2 and logits.numel() > 0):
        return False
    if not (target.dtype == torch.int64 and target.device == logits.device
            and tuple(target.shape) == (logits.shape[0],) + tuple(logits.shape[2:])):
        return False
    if weight is None:
        return True
    if not (weight.dtype == torch.float32 and weight.device == logits.device and tuple(weight.shape) == (logits.shape[1],)):
        return False
    return not (torch.is_grad_enabled() and weight.requires_grad)


def _weighted_ce_of_stock_parts(logits, target, weight, ignore_index):
    """``F.cross_entropy(logits, target, weight=weight, ignore_index=ignore_index)`` written out in stock ops that carry a
    gradient to ``weight``: PyTorch's nll_loss kernels declare their weight non-differentiable and refuse one that requires grad."""
    valid = target != ignore_index
    safe = torch.where(valid, target, torch.zeros_like(target))
    nll = -F.log_softmax(logits, 1).gather(1, safe.unsqueeze(1)).squeeze(1)
    picked = weight[safe]
    zero = torch.zeros((), dtype=nll.dtype, device=nll.device)
    return torch.where(valid, picked * nll, zero).sum() / torch.where(valid, picked, zero).sum()


def seg_cross_entropy(logits, target, weight=None, ignore_index=255, gamma=0.0):
    """``focal(F.cross_entropy(logits, target, weight=weight, ignore_index=ignore_index))`` as a 0-dim tensor, with
    ``focal(ce) = (1 - exp(-ce))^gamma * ce`` on the mean and exactly ``ce`` for ``gamma == 0``.  ``logits`` (B,C,H,W),
    ``target`` (B,H,W) int64, ``weight`` (C,) or None.  fp32 CUDA logits with an int64 target on the same device and fp32
    weights that need no gradient take the fused HIP op (``cerberus::seg_cross_entropy``); 16-bit or CPU logits and a single
    class take ``F.cross_entropy``; a weight that requires grad takes the same mean written out in stock ops that give it a
    gradient (``F.cross_entropy`` refuses such a weight)."""
    if _fusable(logits, target, weight):
        w = weight if weight is not None else torch.ones(logits.shape[1], dtype=torch.float32, device=logits.device)
        return torch.ops.cerberus.seg_cross_entropy(logits, target, w, int(ignore_index), float(gamma))[0]
    if weight is not None and weight.dtype != logits.dtype:
        weight = weight.to(logits.dtype)
    if weight is not None and torch.is_grad_enabled() and weight.requires_grad:
        return _focal(_weighted_ce_of_stock_parts(logits, target, weight, ignore_index), gamma)
    return _focal(F.cross_entropy(logits, target, weight=weight, ignore_index=ignore_index), gamma)


def _balance_weights_stock(target, num_classes, ignore_index, scale_factor, device):
    # the reference's chain (:143-147): unique() sorts every label and synchronises with the host
    weights = torch.ones(num_classes).to(device)
    class_ids, counts = target[target != ignore_index].unique(return_counts=True)
    weights[class_ids] = scale_factor / (scale_factor + counts / float(target.nelement()))
    return weights


def class_balance_weights(target, num_classes, ignore_index=255, scale_factor=0.125):
    """The reference's dynamic class weights (:143-147): ones, and ``scale_factor / (scale_factor + count / target.nelement())``
    for every class with ``count > 0`` labels other than ``ignore_index`` (``nelement`` counts the ignored pixels too, as
    upstream).  A CUDA int64 target takes ``cerberus::class_histogram`` (``torch.bincount`` above its 2048 classes) and a
    ``torch.where`` on the (C,) counts: no ``unique``, no synchronisation.  Anything else takes the reference's chain."""
    if not (target.is_cuda and target.dtype == torch.int64 and target.numel() > 0):
        return _balance_weights_stock(target, num_classes, ignore_index, scale_factor, target.device)
    if num_classes <= _ops.HISTOGRAM_MAX_CLASSES:
        counts = torch.ops.cerberus.class_histogram(target, int(num_classes), int(ignore_index))
    else:
        keep = (target != ignore_index) & (target >= 0) & (target < num_classes)
        counts = torch.bincount(target[keep], minlength=num_classes)
    balanced = scale_factor / (scale_factor + counts / float(target.nelement()))
    return torch.where(counts > 0, balanced.to(torch.float32), torch.ones_like(balanced, dtype=torch.float32))


def _seg_pair(predictions, targets):
    assert all('seg' in dict_ for dict_ in [predictions.keys(), targets.keys()])
    logits, seg_gt = predictions['seg'], targets['seg']
    if len(seg_gt.shape) == 4:
        if seg_gt.shape[1] == 1:
            seg_gt = seg_gt.squeeze(1)
        else:
            raise ValueError(f"Invalid ground truth shape {seg_gt.shape}")
    return logits, seg_gt


class _SegLoss(torch.nn.Module):
    gamma = 0.0

    def _setup(self, weight, ignore_index, dynamic_weights, scale_factor, backend):
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        self.weight = weight
        self.ignore_index = ignore_index
        self.dynamic_weights = dynamic_weights
        self.scale_factor = scale_factor
        self.backend = backend

    def forward(self, predictions: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor]) -> torch.Tensor:
        logits, seg_gt = _seg_pair(predictions, targets)
        num_classes = logits.shape[1]
        if self.backend == "hip":
            weights = None
            if self.dynamic_weights:
                weights = class_balance_weights(seg_gt, num_classes, self.ignore_index, self.scale_factor).to(logits.device)
            return self.weight * seg_cross_entropy(logits, seg_gt, weights, self.ignore_index, self.gamma)

        # the reference's operation order
        if self.dynamic_weights:
            weights = _balance_weights_stock(seg_gt, num_classes, self.ignore_index, self.scale_factor, logits.device)
        else:
            weights = torch.ones(num_classes).to(logits.device)
        ce_loss = F.cross_entropy(logits, seg_gt, ignore_index=self.ignore_index, weight=weights.to(logits.dtype))
        return self._finish(ce_loss)


class FocalLoss2D(_SegLoss):
    """Focal loss of the mean cross-entropy with optional dynamic class weights (reference :121-157).

    ``backend='hip'`` (default): ``weight * seg_cross_entropy(..., gamma)``, the fused HIP op for fp32 CUDA logits.
    ``backend='torch'``: the stock-op formulation in the reference's operation order."""

    def __init__(self, weight=1.0, gamma=2.0, ignore_index=255, dynamic_weights=False, scale_factor=0.125, backend="hip",
                 **kwargs):
        super().__init__()
        self._setup(weight, ignore_index, dynamic_weights, scale_factor, backend)
        self.gamma = gamma

    def _finish(self, ce_loss):
        focal_loss = torch.pow(1 - torch.exp(-ce_loss), self.gamma) * ce_loss
        return self.weight * focal_loss.mean()


class SegCrossEntropy(_SegLoss):
    """Weighted cross-entropy with optional dynamic class weights (reference :159-190).

    ``backend='hip'`` (default): ``weight * seg_cross_entropy(..., gamma=0)``, the fused HIP op for fp32 CUDA logits.
    ``backend='torch'``: the stock-op formulation in the reference's operation order."""

    def __init__(self, weight=1.0, ignore_index=255, dynamic_weights=False, scale_factor=0.125, backend="hip", **kwargs):
        super().__init__()
        self._setup(weight, ignore_index, dynamic_weights, scale_factor, backend)

    def _finish(self, ce_loss):
        return self.weight * ce_loss


# The rest of the reference's seg_losses.py lives in ohem_losses.py (which imports this module); the names are reachable
# from here as well, where the reference keeps them.
_OHEM_NAMES = ("seg_ohem_cross_entropy", "MixSoftmaxCrossEntropyLoss", "SoftmaxCrossEntropyOHEMLoss", "MixSoftmaxCrossEntropyOHEMLoss")


def __getattr__(name):
    if name in _OHEM_NAMES:
        from . import ohem_losses
        return getattr(ohem_losses, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
