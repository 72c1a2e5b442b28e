"""The DETR set criterion (reference: nnet_training/loss_functions/detr_loss.py) with its per-step work on the device.

``backend='hip'``: the main output and every auxiliary decoder layer are stacked into N = L B images; ONE ``hungarian_match`` launch
assigns them all, ONE ``set_loss`` launch (and its one-workgroup finish) forms loss_ce, loss_bbox, loss_giou and cardinality_error
of every layer, and one launch writes both gradients.  Nothing is read on the host -- ``num_boxes`` stays a device tensor -- so the
criterion can be captured in a graph.  ``backend='torch'`` is the reference's route in stock ops with a host solver; CPU tensors,
16-bit tensors and sizes past the fused limits take it under either setting.

Not here: the mask losses (``'masks'`` raises NotImplementedError) and ``class_error``, which the reference's forward never enables.
"""
from typing import Dict

import torch
import torch.nn.functional as F

from .. import ops_detr
from ..nnet_models.detr import box_ops
from ..nnet_models.detr.matcher import HungarianMatcher, pad_targets

TERMS = ("loss_ce", "loss_bbox", "loss_giou", "cardinality_error")         # the columns of ops_detr.set_loss
_TERMS_OF = {"labels": ("loss_ce",), "boxes": ("loss_bbox", "loss_giou"), "cardinality": ("cardinality_error",)}


def _key(term, layer):
    """The reference's name of ``term`` at stacked layer ``layer``: the main output first, then auxiliary layer i as ``_{i}``."""
    return term if layer == 0 else "%s_%d" % (term, layer - 1)


def _world_num_boxes(count, device):
    """(1,) float32 on the device: the number of target boxes averaged over the ranks, at least 1 (no ``.item()``)."""
    num_boxes = torch.as_tensor([count], dtype=torch.float, device=device)
    world = 1
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.all_reduce(num_boxes)
        world = torch.distributed.get_world_size()
    return torch.clamp(num_boxes / world, min=1)


def detr_set_loss(logits, boxes, tgt_labels, tgt_boxes, tgt_count, empty_weight, num_boxes, cost_class=1.0, cost_bbox=1.0,
                  cost_giou=1.0):
    """The per-layer terms of the criterion on the fused route, as a dict of 0-dim tensors under the reference's names
    (``loss_ce``, ``loss_bbox``, ``loss_giou``, ``cardinality_error``, and ``..._{i}`` for auxiliary layer i).

    logits (N,Q,C1) / boxes (N,Q,4): the L = N / B decoder outputs stacked layer-major, the main output first; the targets padded as
    ``pad_targets`` returns them; ``empty_weight`` (C1,) the class weights; ``num_boxes`` a (1,) float32 device tensor."""
    match, _status = ops_detr.hungarian_match(logits.detach(), boxes.detach(), tgt_labels, tgt_boxes, tgt_count, cost_class, cost_bbox,
                                              cost_giou)
    losses = ops_detr.set_loss(logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, empty_weight, num_boxes)
    return {_key(term, layer): losses[layer, k] for layer in range(losses.shape[0]) for k, term in enumerate(TERMS)}


class DetrLoss(torch.nn.Module):
    """The loss for DETR: a Hungarian assignment between the ground-truth boxes and the predictions, then the class and box terms
    of every matched pair.  Arguments as the reference's; ``backend`` selects the fused route ('hip') or the stock ops ('torch')."""

    def __init__(self, num_classes, weight_dict, eos_coef, losses, weight=1.0, backend="hip", **kwargs):
        super().__init__()
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch', got %r" % (backend,))
        if "masks" in losses:
            raise NotImplementedError("DetrLoss: the mask losses of DetrSegmHead are not part of this package")
        for loss in losses:
            assert loss in _TERMS_OF, f'do you really want to compute {loss} loss?'
        self.num_classes = num_classes
        matcher_cfg = dict(kwargs.get("matcher_cfg", {}))
        matcher_cfg.setdefault("backend", backend)
        self.matcher = HungarianMatcher(**matcher_cfg)
        self.weight = weight
        self.weight_dict = weight_dict
        self.eos_coef = eos_coef
        self.losses = losses
        self.backend = backend
        empty_weight = torch.ones(self.num_classes + 1)
        empty_weight[-1] = self.eos_coef
        self.register_buffer('empty_weight', empty_weight)
        self._coef = {}                # (L, device) -> the (L,4) weights of the terms, built once

    def _terms(self):
        return [t for loss in self.losses for t in _TERMS_OF[loss]]

    def _coefficients(self, L, device):
        key = (L, str(device))
        if key not in self._coef:
            active = set(self._terms())
            rows = [[float(self.weight_dict.get(_key(t, layer), 0.0)) if t in active else 0.0 for t in TERMS] for layer in range(L)]
            self._coef[key] = torch.tensor(rows, dtype=torch.float32, device=device)
        return self._coef[key]

    # ---- the fused route ----------------------------------------------------------------------------------------------------
    def _forward_hip(self, layers, padded, count):
        logits = torch.cat([o["logits"] for o in layers]) if len(layers) > 1 else layers[0]["logits"]
        boxes = torch.cat([o["bboxes"] for o in layers]) if len(layers) > 1 else layers[0]["bboxes"]
        tgt_labels, tgt_boxes, tgt_count = padded
        num_boxes = _world_num_boxes(count, logits.device)
        match, _status = ops_detr.hungarian_match(logits.detach(), boxes.detach(), tgt_labels, tgt_boxes, tgt_count,
                                                  self.matcher.cost_class, self.matcher.cost_bbox, self.matcher.cost_giou)
        losses = ops_detr.set_loss(logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, self.empty_weight, num_boxes)
        return self.weight * (losses * self._coefficients(losses.shape[0], logits.device)).sum()

    # ---- the reference's route in stock ops -----------------------------------------------------------------------------
    def loss_labels(self, outputs, targets, indices, _num_boxes=None):
        src_logits = outputs['logits']
        idx = self._get_src_permutation_idx(indices)
        target_classes_o = torch.cat([t.reshape(-1)[J] for t, (_, J) in zip(targets["labels"], indices)]).to(
            device=src_logits.device, dtype=torch.int64)
        target_classes = torch.full(src_logits.shape[:2], self.num_classes, dtype=torch.int64, device=src_logits.device)
        target_classes[idx] = target_classes_o
        return {'loss_ce': F.cross_entropy(src_logits.transpose(1, 2), target_classes, self.empty_weight.to(src_logits.dtype))}

    @staticmethod
    @torch.no_grad()
    def loss_cardinality(outputs, targets, *_args):
        pred_logits = outputs['logits']
        tgt_lengths = torch.as_tensor([len(v) for v in targets["labels"]], device=pred_logits.device)
        card_pred = (pred_logits.argmax(-1) != pred_logits.shape[-1] - 1).sum(1)
        return {'cardinality_error': F.l1_loss(card_pred.float(), tgt_lengths.float())}

    def loss_boxes(self, outputs, targets, indices, num_boxes):
        idx = self._get_src_permutation_idx(indices)
        src_boxes = outputs['bboxes'][idx]
        target_boxes = torch.cat([t.reshape(-1, 4)[i] for t, (_, i) in zip(targets['bboxes'], indices)], dim=0).to(src_boxes)
        loss_bbox = F.l1_loss(src_boxes, target_boxes, reduction='none')
        loss_giou = 1 - torch.diag(box_ops.generalized_box_iou(box_ops.box_cxcywh_to_xyxy(src_boxes),
                                                               box_ops.box_cxcywh_to_xyxy(target_boxes)))
        return {'loss_bbox': loss_bbox.sum() / num_boxes, 'loss_giou': loss_giou.sum() / num_boxes}

    @staticmethod
    def _get_src_permutation_idx(indices):
        batch_idx = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)])
        src_idx = torch.cat([src for (src, _) in indices])
        return batch_idx, src_idx

    def get_loss(self, loss, outputs, targets, indices, num_boxes):
        loss_map = {'labels': self.loss_labels, 'cardinality': self.loss_cardinality, 'boxes': self.loss_boxes}
        assert loss in loss_map, f'do you really want to compute {loss} loss?'
        return loss_map[loss](outputs, targets, indices, num_boxes)

    def _forward_torch(self, layers, targets, count):
        num_boxes = _world_num_boxes(count, layers[0]["logits"].device)
        losses = {}
        for layer, outputs in enumerate(layers):
            indices = self.matcher(outputs, targets)
            for loss in self.losses:
                for k, v in self.get_loss(loss, outputs, targets, indices, num_boxes).items():
                    losses[_key(k, layer)] = v.reshape(())
        return self.weight * sum([losses[k] * self.weight_dict[k] for k in losses if k in self.weight_dict.keys()])

    def forward(self, predictions: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor]) -> torch.Tensor:
        """``predictions``: 'logits' (B,Q,C1), 'bboxes' (B,Q,4) and optionally 'aux_outputs', a list of such dicts; ``targets``:
        'labels' and 'bboxes', lists of one tensor per image."""
        main = {k: v for k, v in predictions.items() if k in ('logits', 'bboxes')}
        layers = [main] + list(predictions.get('aux_outputs', []))
        counts = [len(t) for t in targets["labels"]]
        logits = main['logits']
        if self.backend == "hip" and all(ops_detr.detr_fused_ok(o["logits"], o["bboxes"], max(counts, default=0)) for o in layers):
            return self._forward_hip(layers, pad_targets(targets["labels"], targets["bboxes"], logits.device), sum(counts))
        return self._forward_torch(layers, targets, sum(counts))
