"""Drop-in for the F-SCNN losses of ``nnet_training/loss_functions/seg_losses.py`` (:16-119): ``MixSoftmaxCrossEntropyLoss``,
``SoftmaxCrossEntropyOHEMLoss`` and ``MixSoftmaxCrossEntropyOHEMLoss``.  The names are also reachable as attributes of
``loss_functions.seg_losses``, where the reference keeps them.

Online hard example mining (OHEM): of the pixels with a label, keep those whose target probability is at most ``thresh``, and at
least the ``min_kept`` hardest ones; the loss is the weighted cross-entropy over the kept pixels.  The reference (:56-95)
copies the logits to the host, computes a softmax in numpy, argsorts every valid pixel, rewrites the target on the host and
copies it back.  Here fp32 CUDA logits take ONE fused HIP forward and one fused backward
(``cerberus::seg_ohem_cross_entropy``, ``csrc/seg_ohem.hip``): the ``min_kept``-th smallest probability comes from a radix
select on the device, nothing is sorted, nothing is read on the host, and the whole loss can be captured in a graph.
Everything else takes the same selection written in stock ops on the logits' own device.

Semantics: a pixel is valid when its label is not ``ignore_index`` and lies in [0, C);
``prob = softmax(logits)[target]``; with ``num_valid`` valid pixels, ``min_kept >= num_valid`` keeps every valid pixel;
otherwise ``threshold = max(thresh, kth)`` with ``kth`` the ``min_kept``-th smallest ``prob`` (``thresh`` alone for
``min_kept <= 0`` or a NaN ``kth``); ``kept = valid & (prob <= threshold)``, ties included.

Differences from the reference: ``use_weight=True`` needs ``class_weights`` (the reference takes a 19-entry table written in its
source, which is not copied); no ``print``, no ``.cuda()``: the result lives where the logits live; the aux forward takes
the heads as a sequence (the reference wraps them in a list of one and fails on more than one head).
"""
import torch
import torch.nn.functional as F

from .. import ops as _ops  # noqa: F401  (registers the ops)
from .seg_losses import _fusable, seg_cross_entropy

__all__ = ["seg_ohem_cross_entropy", "MixSoftmaxCrossEntropyLoss", "SoftmaxCrossEntropyOHEMLoss", "MixSoftmaxCrossEntropyOHEMLoss"]


def _ohem_selection(logits, target, ignore_index, thresh, min_kept):
    """(kept mask, threshold, num_valid) of the stock-op route: ``softmax``, ``gather``, ``kthvalue``, ``where``.  No host read:
    ``num_valid`` stays a tensor and every branch is a ``where``."""
    C = logits.shape[1]
    with torch.no_grad():
        valid = (target != ignore_index) & (target >= 0) & (target < C)
        safe = torch.where(valid, target, torch.zeros_like(target))
        prob = F.softmax(logits.detach().float(), 1).gather(1, safe.unsqueeze(1)).squeeze(1)
        num_valid = valid.sum()
        th = torch.tensor(thresh, dtype=torch.float32, device=logits.device)
        inf = torch.full_like(th, float("inf"))
        threshold = th
        if min_kept > 0 and prob.numel() > 0:
            # NaN orders above every number, the pixels that are not valid above that: they get +inf and a NaN kth is told
            # from the count of the valid numbers
            nan = torch.isnan(prob)
            keys = torch.where(valid & ~nan, prob, inf).reshape(-1)
            kth = keys.kthvalue(min(int(min_kept), keys.numel())).values
            kth_is_nan = (valid & ~nan).sum() < min_kept
            threshold = torch.where(kth_is_nan | ~(kth > th), th, kth)
        keep_all = num_valid <= min_kept
        threshold = torch.where(keep_all, inf, threshold)
        kept = valid & ((prob <= threshold) | keep_all)
    return kept, threshold, num_valid


def _ohem_stock(logits, target, weight, ignore_index, thresh, min_kept, cross_entropy):
    kept, threshold, num_valid = _ohem_selection(logits, target, ignore_index, thresh, min_kept)
    # a label outside [0, C) that is not the ignore value stays in the target: the stock loss reports it as it always does
    stray = (target != ignore_index) & ((target < 0) | (target >= logits.shape[1]))
    new_target = torch.where(kept | stray, target, torch.full_like(target, ignore_index))
    return cross_entropy(logits, new_target, weight, ignore_index), threshold, num_valid, kept.sum()


def _stock_ce(logits, target, weight, ignore_index):
    if weight is not None and weight.dtype != logits.dtype:
        weight = weight.to(logits.dtype)
    return F.cross_entropy(logits, target, weight=weight, ignore_index=ignore_index)


def seg_ohem_cross_entropy(logits, target, weight=None, ignore_index=-1, thresh=0.7, min_kept=256, return_stats=False):
    """OHEM cross-entropy as a 0-dim tensor: the weighted mean of ``lse - x_t`` over the kept pixels (module docstring).
    ``logits`` (B,C,H,W), ``target`` (B,H,W) int64, ``weight`` (C,) or None.  fp32 CUDA logits with an int64 target on the same
    device and fp32 weights that need no gradient take the fused HIP op; CPU tensors, 16-bit logits, a single class and a weight
    that requires grad take the stock-op restatement on the logits' device, then ``seg_cross_entropy``.  With
    ``return_stats=True`` the result is ``(loss, threshold, num_valid, num_kept)``, all device tensors, no synchronisation."""
    thresh, min_kept = float(thresh), int(min_kept)
    if _fusable(logits, target, weight):
        w = weight if weight is not None else torch.ones(logits.shape[1], dtype=torch.float32, device=logits.device)
        loss, _prob, _lse, state, counts = torch.ops.cerberus.seg_ohem_cross_entropy(logits, target, w, int(ignore_index), thresh,
                                                                                  min_kept)
        return (loss, state[3], counts[0], counts[1]) if return_stats else loss
    out = _ohem_stock(logits, target, weight, ignore_index, thresh, min_kept, seg_cross_entropy)
    return out if return_stats else out[0]


def _heads(preds):
    return [preds] if isinstance(preds, torch.Tensor) else list(preds)


class MixSoftmaxCrossEntropyLoss(torch.nn.Module):
    """Cross-entropy of the first head plus ``aux_weight`` times that of every later head (reference :16-37), each a
    ``seg_cross_entropy`` call.  ``forward(preds, target)`` with ``preds`` a tensor or a sequence of (B,C,H,W) heads; with
    ``aux=False`` there is one head."""

    def __init__(self, aux=True, aux_weight=0.2, ignore_label=255, **kwargs):
        super().__init__()
        self.aux = aux
        self.aux_weight = aux_weight
        self.ignore_index = ignore_label

    def forward(self, preds, target):
        heads = _heads(preds)
        if not self.aux and len(heads) != 1:
            raise ValueError("MixSoftmaxCrossEntropyLoss(aux=False) takes one head, got %d" % len(heads))
        loss = seg_cross_entropy(heads[0], target, None, self.ignore_index)
        for head in heads[1:]:
            loss = loss + self.aux_weight * seg_cross_entropy(head, target, None, self.ignore_index)
        return loss


class SoftmaxCrossEntropyOHEMLoss(torch.nn.Module):
    """OHEM cross-entropy (reference :40-95).  ``use_weight=True`` needs ``class_weights``, a (C,) tensor or sequence;
    ``use_weight=False`` weighs every class 1.

    ``backend='hip'`` (default): ``seg_ohem_cross_entropy``, the fused HIP op for fp32 CUDA logits.
    ``backend='torch'``: the selection in stock ops and ``F.cross_entropy`` on the rewritten target, on the logits' device."""

    def __init__(self, ignore_label=-1, thresh=0.7, min_kept=256, use_weight=True, backend="hip", class_weights=None, **kwargs):
        super().__init__()
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        if use_weight and class_weights is None:
            raise ValueError("use_weight=True needs class_weights, one weight per class (the reference's Cityscapes table is not "
                             "part of this package); use_weight=False weighs every class 1")
        self.ignore_label = ignore_label
        self.thresh = float(thresh)
        self.min_kept = int(min_kept)
        self.backend = backend
        weight = torch.as_tensor(class_weights, dtype=torch.float32).detach().clone() if use_weight else None
        if weight is not None and weight.dim() != 1:
            raise ValueError("class_weights must hold one weight per class, got shape %s" % (tuple(weight.shape),))
        self.register_buffer("weight", weight, persistent=False)

    def _one_head(self, predict, target):
        assert not target.requires_grad
        assert predict.dim() == 4
        assert target.dim() == 3
        assert predict.size(0) == target.size(0), "{0} vs {1} ".format(predict.size(0), target.size(0))
        assert predict.size(2) == target.size(1), "{0} vs {1} ".format(predict.size(2), target.size(1))
        assert predict.size(3) == target.size(2), "{0} vs {1} ".format(predict.size(3), target.size(2))
        weight = self.weight
        if weight is not None and weight.device != predict.device:
            weight = weight.to(predict.device)
        if self.backend == "hip":
            return seg_ohem_cross_entropy(predict, target, weight, self.ignore_label, self.thresh, self.min_kept)
        return _ohem_stock(predict, target, weight, self.ignore_label, self.thresh, self.min_kept, _stock_ce)[0]

    def forward(self, predict, target):
        return self._one_head(predict, target)


class MixSoftmaxCrossEntropyOHEMLoss(SoftmaxCrossEntropyOHEMLoss):
    """``SoftmaxCrossEntropyOHEMLoss`` of the first head plus ``aux_weight`` times that of every later head (reference
    :98-119).  ``forward(preds, target)`` with ``preds`` a tensor or a sequence of heads; with ``aux=False`` there is one head."""

    def __init__(self, aux=False, aux_weight=0.2, ignore_index=255, **kwargs):
        super().__init__(ignore_label=ignore_index, **kwargs)
        self.aux = aux
        self.aux_weight = aux_weight

    def forward(self, preds, target):
        heads = _heads(preds)
        if not self.aux and len(heads) != 1:
            raise ValueError("MixSoftmaxCrossEntropyOHEMLoss(aux=False) takes one head, got %d" % len(heads))
        loss = self._one_head(heads[0], target)
        for head in heads[1:]:
            loss = loss + self.aux_weight * self._one_head(head, target)
        return loss
