"""Drop-in for ``nnet_training/loss_functions/panoptic_loss.py``: the centre / offset regression loss of the panoptic head.

``DeeplabPanopticLoss`` keeps its name, its constructor arguments (``weight``, ``ignore_index``, ``center_weight`` and
``offset_weight`` through ``kwargs``) and ``forward(predictions, targets)`` with the keys ``'center'``, ``'offset'``,
``'center_mask'`` and ``'offset_mask'`` (each mask optional).  As in the reference the semantic cross-entropy it constructs is
never part of the result.

What the reference computes (``masking='reference'``, the default): its ``nn.MSELoss()`` and ``nn.L1Loss()`` reduce to the
MEAN before the mask is applied, so a "masked" term is ``mean * mask`` summed and divided by ``mask.sum()`` -- the unmasked
mean, gated by "the mask is not empty" (a host read in the reference, ``if mask.sum() > 0``; a ``torch.where`` or the kernel's
own select here: no host read, capturable).  ``masking='pixel'`` is Panoptic-DeepLab's rule, which the reference cannot
express: ``sum(m * f) / sum(m)`` over the term's elements, ``f = d^2`` for the centre and ``|d|`` for the offsets, 0 for an
empty mask; an element with ``m == 0`` is skipped by selection (a NaN predicted there changes nothing, its gradient is 0).

``backend='hip'`` (default): fp32 CUDA tensors whose targets need no gradient take ``cerberus::panoptic_loss``
(``csrc/panoptic_train.hip``: one pass per term and a one-workgroup finish forward, ONE launch backward).  16-bit, 64-bit and
CPU tensors, targets that require grad and ``backend='torch'`` take the stock-op chain below.
"""
import torch

from .. import ops

__all__ = ["deeplab_panoptic_loss", "DeeplabPanopticLoss"]

MASKINGS = ("reference", "pixel")


def _term_stock(pred, tgt, mask, weight, absolute, pixel):
    d = pred - tgt
    f = d.abs() if absolute else d * d
    if mask is None:
        return weight * f.mean()
    m = mask[:, None, :, :].expand_as(pred)
    total = m.sum()
    on = total > 0
    safe = torch.where(on, total, torch.ones_like(total))
    if pixel:
        # the selection sits on d, before anything is computed from it: the gradient under m == 0 is 0 even for a NaN there
        d = torch.where(m != 0, d, torch.zeros_like(d))
        value = (m * (d.abs() if absolute else d * d)).sum() / safe
    else:
        value = (f.mean() * m).sum() / safe
    return torch.where(on, weight * value, torch.zeros_like(value))


def _stock(predictions, targets, center_weight, offset_weight, masking):
    pixel = masking == "pixel"
    return (_term_stock(predictions["center"], targets["center"], targets.get("center_mask"), center_weight, False, pixel) +
            _term_stock(predictions["offset"], targets["offset"], targets.get("offset_mask"), offset_weight, True, pixel))


def _fusable(predictions, targets):
    """What cerberus::panoptic_loss takes: fp32 tensors on one GPU, (B,1,H,W) / (B,2,H,W) / (B,H,W), no gradient wanted by a
    target or a mask."""
    c = predictions["center"]
    tensors = [c, predictions["offset"], targets["center"], targets["offset"]]
    masks = [targets[k] for k in ("center_mask", "offset_mask") if k in targets]
    if not all(torch.is_tensor(t) and t.is_cuda and t.device == c.device and t.dtype == torch.float32 for t in tensors + masks):
        return False
    if c.dim() != 4 or c.shape[1] != 1 or c.numel() == 0 or 2 * c.numel() > 0x7fffffff - 1024:
        return False
    B, _, H, W = c.shape
    if tuple(predictions["offset"].shape) != (B, 2, H, W) or targets["center"].shape != c.shape or \
            targets["offset"].shape != predictions["offset"].shape or any(tuple(m.shape) != (B, H, W) for m in masks):
        return False
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors[2:] + masks))


def deeplab_panoptic_loss(predictions, targets, center_weight=200., offset_weight=.1, masking="reference", backend="hip"):
    """``center_weight * centre term + offset_weight * offset term`` of ``predictions['center']`` (B,1,H,W) and
    ``predictions['offset']`` (B,2,H,W) against ``targets['center']``, ``targets['offset']`` and the optional (B,H,W) weights
    ``targets['center_mask']``, ``targets['offset_mask']``; see the module text for the two ``masking`` rules.  No host read
    on either backend."""
    if masking not in MASKINGS:
        raise ValueError("masking must be 'reference' or 'pixel', got %r" % (masking,))
    if backend not in ("hip", "torch"):
        raise ValueError("backend must be 'hip' or 'torch'")
    if backend == "hip" and _fusable(predictions, targets):
        loss, _state = torch.ops.cerberus.panoptic_loss(predictions["center"], targets["center"], targets.get("center_mask"),
                                                        predictions["offset"], targets["offset"], targets.get("offset_mask"),
                                                        float(center_weight), float(offset_weight), ops.PANOPTIC_LOSS_MODES[masking])
        return loss
    return _stock(predictions, targets, center_weight, offset_weight, masking)


class DeeplabPanopticLoss(torch.nn.Module):
    """The reference's module: ``weight * (center_weight * centre term + offset_weight * offset term)``."""

    def __init__(self, weight=1.0, ignore_index=255, masking="reference", backend="hip", **kwargs):
        super().__init__()
        if masking not in MASKINGS:
            raise ValueError("masking must be 'reference' or 'pixel', got %r" % (masking,))
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        self.weight = weight
        self.ignore_index = ignore_index
        self.masking = masking
        self.backend = backend
        self.center_weight = kwargs.get('center_weight', 200.)
        self.offset_weight = kwargs.get('offset_weight', .1)

    def forward(self, predictions, targets):
        return self.weight * deeplab_panoptic_loss(predictions, targets, self.center_weight, self.offset_weight, self.masking,
                                                   self.backend)
