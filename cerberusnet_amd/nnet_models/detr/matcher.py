"""The Hungarian matcher of the DETR head (reference: nnet_models/detr/matcher.py) with the assignment on the device.

``backend='hip'`` (the default) computes the cost matrix and solves the assignment in one launch for every image of every decoder
layer (``torch.ops.cerberus_detr.hungarian_match``); ``forward`` then makes ONE device-to-host copy to build the reference's list of
index pairs, and ``match`` makes none.  ``backend='torch'`` is the reference's route in stock ops -- cost matrix on the inputs' device,
one ``.cpu()`` copy, a host solver per image -- and is what CPU tensors, 16-bit tensors and sizes past the fused limits take under
either setting.  The host solver is scipy's where scipy imports and ``_lsap_host`` otherwise.
"""
import numpy as np
import torch
from torch import nn

from ... import ops_detr
from .box_ops import box_cxcywh_to_xyxy, generalized_box_iou

try:
    from scipy.optimize import linear_sum_assignment as _scipy_lsap
except ImportError:          # scipy is optional: _lsap_host solves the same problem
    _scipy_lsap = None


def _lsap_host(cost):
    """Rectangular linear sum assignment on the host: (rows, cols) int64 arrays of min(nr, nc) pairs with minimal total cost, rows
    ascending.  Shortest augmenting paths with dual variables, the algorithm csrc/detr_loss.hip runs per image: every row in turn
    grows a tree of alternating paths over the reduced costs until it reaches a free column, the duals move by the distances found,
    and the path is flipped.  The lowest column index wins a tie."""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.ndim != 2:
        raise ValueError("expected a matrix, got shape %s" % (cost.shape,))
    if cost.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    if not np.isfinite(cost).all():
        raise ValueError("cost matrix holds non-finite entries")
    flipped = cost.shape[0] > cost.shape[1]
    c = cost.T if flipped else cost
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    row_of, col_of = np.full(nc, -1, dtype=np.int64), np.full(nr, -1, dtype=np.int64)
    for start in range(nr):
        dist = np.full(nc, np.inf)
        prev = np.full(nc, -1, dtype=np.int64)
        closed = np.zeros(nc, dtype=bool)
        reach, i, sink = 0.0, start, -1
        for _ in range(nc):
            r = reach + c[i] - u[i] - v
            better = ~closed & (r < dist)
            dist[better] = r[better]
            prev[better] = i
            j = int(np.argmin(np.where(closed, np.inf, dist)))
            reach = dist[j]
            closed[j] = True
            if row_of[j] < 0:
                sink = j
                break
            i = row_of[j]
        u[start] += reach
        inner = closed & (row_of >= 0)
        u[row_of[inner]] += reach - dist[inner]
        v[closed] -= reach - dist[closed]
        j = sink
        for _ in range(nr + 1):
            i = prev[j]
            row_of[j] = i
            col_of[i], j = j, col_of[i]
            if i == start:
                break
    rows, cols = np.arange(nr, dtype=np.int64), col_of
    if flipped:
        order = np.argsort(cols, kind="stable")
        rows, cols = cols[order], rows[order]
    return rows, cols


def _solve_host(cost):
    if _scipy_lsap is not None:
        i, j = _scipy_lsap(cost)
        return np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    return _lsap_host(cost)


def pad_targets(labels_list, boxes_list, device):
    """(tgt_labels (B,Tmax) int64, tgt_boxes (B,Tmax,4) float32, tgt_count (B,) int32) on ``device`` from the reference's
    ``targets['labels']`` / ``targets['bboxes']`` lists.  The counts come from the lists' lengths (host metadata): nothing is read
    back from the device."""
    counts = [int(t.shape[0]) for t in labels_list]
    if [int(t.shape[0]) for t in boxes_list] != counts:
        raise ValueError("labels and bboxes disagree on the number of targets per image")
    B, Tmax = len(counts), max(counts, default=0)
    tgt_count = torch.tensor(counts, dtype=torch.int32, device=device)
    if Tmax == 0:
        return (torch.zeros((B, 0), dtype=torch.int64, device=device), torch.zeros((B, 0, 4), dtype=torch.float32, device=device),
                tgt_count)
    labels = [t.reshape(-1).to(device=device, dtype=torch.int64) for t in labels_list]
    boxes = [t.reshape(-1, 4).to(device=device, dtype=torch.float32) for t in boxes_list]
    return (nn.utils.rnn.pad_sequence(labels, batch_first=True), nn.utils.rnn.pad_sequence(boxes, batch_first=True), tgt_count)


class HungarianMatcher(nn.Module):
    """Assignment between the targets and the predictions of the network (see the reference for the conventions): the targets
    hold no no-object entry, so with more predictions than targets the best predictions are matched one to one and the rest stay
    unmatched."""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1, backend: str = "hip"):
        super().__init__()
        self.cost_class = cost_class
        self.cost_bbox = cost_bbox
        self.cost_giou = cost_giou
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch', got %r" % (backend,))
        self.backend = backend

    def fused(self, logits, boxes, Tmax):
        """Whether these predictions take the fused route."""
        return self.backend == "hip" and ops_detr.detr_fused_ok(logits, boxes, Tmax)

    @torch.no_grad()
    def match(self, outputs, targets, aux_outputs=None):
        """The device-side form, with no synchronisation: ``(match (N,Q) int32, (tgt_labels, tgt_boxes, tgt_count), status (N,))``
        for the N = L B images of ``outputs`` and every entry of ``aux_outputs`` stacked layer-major (``outputs`` is layer 0).
        ``targets`` is the reference's dict of lists, or an already padded triple."""
        layers = [outputs] + list(aux_outputs or [])
        logits = torch.cat([o["logits"] for o in layers]) if len(layers) > 1 else outputs["logits"]
        boxes = torch.cat([o["bboxes"] for o in layers]) if len(layers) > 1 else outputs["bboxes"]
        padded = targets if isinstance(targets, (tuple, list)) else pad_targets(targets["labels"], targets["bboxes"], logits.device)
        tgt_labels, tgt_boxes, tgt_count = padded
        match, status = ops_detr.hungarian_match(logits, boxes, tgt_labels, tgt_boxes, tgt_count, self.cost_class, self.cost_bbox,
                                                 self.cost_giou)
        return match, (tgt_labels, tgt_boxes, tgt_count), status

    @torch.no_grad()
    def forward(self, outputs, targets):
        """A list of size batch_size of ``(index_i, index_j)`` int64 CPU tensors: the selected predictions (ascending) and their
        targets, ``len(index_i) = len(index_j) = min(num_queries, num_target_boxes)``."""
        logits, boxes = outputs["logits"], outputs["bboxes"]
        sizes = [int(v.shape[0]) for v in targets["bboxes"]]
        if self.fused(logits, boxes, max(sizes, default=0)):
            match, _, _ = self.match(outputs, targets)
            rows = match.cpu()                              # the one copy
            out = []
            for row in rows:
                i = torch.nonzero(row >= 0).reshape(-1)
                out.append((i, row[i].to(torch.int64)))
            return out
        return self._forward_torch(logits, boxes, targets, sizes)

    def _forward_torch(self, logits, boxes, targets, sizes):
        bs, num_queries = logits.shape[:2]
        empty = torch.zeros(0, dtype=torch.int64)
        if sum(sizes) == 0:
            return [(empty, empty.clone()) for _ in range(bs)]
        out_prob = logits.flatten(0, 1).float().softmax(-1)
        out_bbox = boxes.flatten(0, 1).float()
        tgt_ids = torch.cat([t.reshape(-1) for t in targets["labels"]]).to(device=logits.device, dtype=torch.int64)
        tgt_bbox = torch.cat([t.reshape(-1, 4) for t in targets["bboxes"]]).to(device=logits.device, dtype=torch.float32)
        cost_class = -out_prob[:, tgt_ids]
        cost_bbox = torch.cdist(out_bbox, tgt_bbox, p=1)
        cost_giou = -generalized_box_iou(box_cxcywh_to_xyxy(out_bbox), box_cxcywh_to_xyxy(tgt_bbox))
        cost = self.cost_bbox * cost_bbox + self.cost_class * cost_class + self.cost_giou * cost_giou
        cost = cost.view(bs, num_queries, -1).cpu()         # the one copy
        out = []
        for b, c in enumerate(cost.split(sizes, -1)):
            i, j = _solve_host(c[b].numpy())
            out.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
        return out
