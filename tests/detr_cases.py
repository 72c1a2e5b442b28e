"""Shared inputs and yardsticks of the DETR set-loss tests (tests/test_detr_loss_cpu.py, tests/test_detr_loss_gpu.py,
tests/detr_op_cases.py).

Inputs come from a hash (cerberusnet_amd.synth.hash_uniform, as tests/op_cases.py uses): logits in [-3, 3), boxes with centres in
[0.1, 0.9) and sizes in [0.02, 0.32) -- never degenerate -- and DETR's own cost weights (class 1, bbox 5, giou 2).

The yardstick is a restatement of the reference's HungarianMatcher cost matrix and of DetrLoss.loss_labels / loss_boxes /
loss_cardinality written here in torch ops at float64 (``dtype=torch.float64``); the same functions at float32 are the "stock fp32
chain" whose own error against float64 sets the bounds of the GPU tests.  ``stock_cost`` is that chain for the cost matrix, through
the package's box_ops, softmax and cdist.  ``brute_force`` enumerates the assignments of a small matrix."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from cerberusnet_amd.synth import hash_uniform

W_CLASS, W_BBOX, W_GIOU = 1.0, 5.0, 2.0
EOS_COEF = 0.1


def make_boxes(shape, seed):
    """cxcywh boxes of ``shape + (4,)``."""
    centre = hash_uniform(tuple(shape) + (2,), seed, 0.1, 0.9)
    size = hash_uniform(tuple(shape) + (2,), seed + 1, 0.02, 0.32)
    return np.concatenate([centre, size], axis=-1).astype(np.float32)


def make_case(L, B, Q, C1, counts, seed):
    """One step's inputs: L layers over a batch of B, ``counts[b]`` targets for image b, padded with zeros to Tmax."""
    assert len(counts) == B
    N, Tmax = L * B, max(counts)
    labels = np.zeros((B, Tmax), dtype=np.int64)
    tboxes = np.zeros((B, Tmax, 4), dtype=np.float32)
    if Tmax:
        draw = np.floor(hash_uniform((B, Tmax), seed + 4, 0.0, float(C1 - 1))).astype(np.int64).clip(0, C1 - 2)
        full = make_boxes((B, Tmax), seed + 5)
        for b, c in enumerate(counts):
            labels[b, :c] = draw[b, :c]
            tboxes[b, :c] = full[b, :c]
    weight = np.ones(C1, dtype=np.float32)
    weight[-1] = EOS_COEF
    return {"L": L, "B": B, "Q": Q, "C1": C1, "counts": tuple(counts), "Tmax": Tmax,
            "logits": hash_uniform((N, Q, C1), seed, -3.0, 3.0), "boxes": make_boxes((N, Q), seed + 2),
            "tgt_labels": labels, "tgt_boxes": tboxes, "tgt_count": np.asarray(counts, dtype=np.int32), "weight": weight,
            "num_boxes": np.asarray([max(float(sum(counts)), 1.0)], dtype=np.float32)}


# name -> (L, B, Q, C1, counts): the smallest shapes at which each path of the kernels can go wrong
CASES = {
    "1x1": (1, 1, 1, 2, (1,)),
    "5x0": (1, 1, 5, 4, (0,)),
    "3x5_swapped": (1, 1, 3, 4, (5,)),                 # more targets than queries: the queries become the rows
    "7x7": (1, 1, 7, 5, (7,)),                         # against the brute force
    "100x37": (1, 1, 100, 20, (37,)),                  # more than one column per lane
    "130x126": (1, 1, 130, 20, (126,)),                # at the LDS cap: 16380 entries
    "256x64": (1, 1, 256, 20, (64,)),                  # at the LDS cap: 16384 entries, four columns per lane
    "batch_0_Tmax_1": (1, 3, 10, 6, (0, 6, 1)),        # an empty image, a full one, a single target
    "layers_3x2": (3, 2, 12, 7, (5, 3)),               # layer-major stacking: image n reads target row n % B
}


def case(name):
    L, B, Q, C1, counts = CASES[name]
    return make_case(L, B, Q, C1, counts, 4000 + 37 * sorted(CASES).index(name))


# ---- the float64 restatement (and, at float32, the stock chain of the loss terms) ---------------------------------------------------
def _xyxy(b):
    return torch.stack([b[..., 0] - 0.5 * b[..., 2], b[..., 1] - 0.5 * b[..., 3], b[..., 0] + 0.5 * b[..., 2],
                        b[..., 1] + 0.5 * b[..., 3]], dim=-1)


def giou_pairs(p, t):
    """GIoU of broadcastable cxcywh boxes ``p`` and ``t``."""
    a, b = _xyxy(p), _xyxy(t)
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a + area_b - inter
    hull_wh = (torch.max(a[..., 2:], b[..., 2:]) - torch.min(a[..., :2], b[..., :2])).clamp(min=0)
    hull = hull_wh[..., 0] * hull_wh[..., 1]
    return inter / union - (hull - union) / hull


def cost_matrix(c, dtype=torch.float64, weights=(W_CLASS, W_BBOX, W_GIOU)):
    """(N,Q,Tmax): C = w_bbox |p - t|_1 - w_class softmax(logits)[label] - w_giou GIoU, padding columns zero."""
    wc, wb, wg = weights
    logits, boxes = torch.from_numpy(c["logits"]).to(dtype), torch.from_numpy(c["boxes"]).to(dtype)
    N, Q, _ = logits.shape
    out = torch.zeros((N, Q, c["Tmax"]), dtype=dtype)
    prob = logits.softmax(-1)
    for n in range(N):
        b = n % c["B"]
        T = int(c["tgt_count"][b])
        if T == 0:
            continue
        lab = torch.from_numpy(c["tgt_labels"][b, :T])
        tb = torch.from_numpy(c["tgt_boxes"][b, :T]).to(dtype)
        l1 = (boxes[n][:, None, :] - tb[None, :, :]).abs().sum(-1)
        out[n, :, :T] = wb * l1 - wc * prob[n][:, lab] - wg * giou_pairs(boxes[n][:, None, :], tb[None, :, :])
    return out


def stock_cost(c, weights=(W_CLASS, W_BBOX, W_GIOU)):
    """The reference's chain at float32 in stock ops: softmax, cdist and the package's box_ops."""
    from cerberusnet_amd.nnet_models.detr.box_ops import box_cxcywh_to_xyxy, generalized_box_iou
    wc, wb, wg = weights
    logits, boxes = torch.from_numpy(c["logits"]), torch.from_numpy(c["boxes"])
    N, Q, _ = logits.shape
    out = torch.zeros((N, Q, c["Tmax"]), dtype=torch.float32)
    for n in range(N):
        b = n % c["B"]
        T = int(c["tgt_count"][b])
        if T == 0:
            continue
        lab, tb = torch.from_numpy(c["tgt_labels"][b, :T]), torch.from_numpy(c["tgt_boxes"][b, :T])
        prob = logits[n].softmax(-1)
        out[n, :, :T] = (wb * torch.cdist(boxes[n], tb, p=1) + wc * (-prob[:, lab])
                         + wg * (-generalized_box_iou(box_cxcywh_to_xyxy(boxes[n]), box_cxcywh_to_xyxy(tb))))
    return out


def loss_terms(c, match, logits, boxes):
    """(L,4) = loss_ce, loss_bbox, loss_giou, cardinality_error per layer, from ``match`` (N,Q) (target index or -1), in the dtype
    of ``logits`` / ``boxes`` (torch tensors, differentiable)."""
    dtype = logits.dtype
    L, B, Q, C1 = c["L"], c["B"], c["Q"], c["C1"]
    weight = torch.from_numpy(c["weight"]).to(dtype)
    num_boxes = torch.from_numpy(c["num_boxes"]).to(dtype)[0]
    match = torch.as_tensor(np.asarray(match), dtype=torch.int64)
    rows = []
    for layer in range(L):
        classes = torch.full((B, Q), C1 - 1, dtype=torch.int64)
        src, tgt = [], []
        for b in range(B):
            n = layer * B + b
            q = torch.nonzero(match[n] >= 0).reshape(-1)
            t = match[n][q]
            classes[b, q] = torch.from_numpy(c["tgt_labels"][b])[t]
            src.append(boxes[n][q])
            tgt.append(torch.from_numpy(c["tgt_boxes"][b]).to(dtype)[t])
        lg = logits[layer * B:(layer + 1) * B]
        loss_ce = F.cross_entropy(lg.transpose(1, 2), classes, weight)
        src, tgt = torch.cat(src), torch.cat(tgt)
        loss_bbox = F.l1_loss(src, tgt, reduction="none").sum() / num_boxes
        loss_giou = (1 - giou_pairs(src, tgt)).sum() / num_boxes
        card = (lg.detach().argmax(-1) != C1 - 1).sum(1).to(dtype)
        card_err = F.l1_loss(card, torch.from_numpy(c["tgt_count"]).to(dtype))
        rows.append(torch.stack([loss_ce, loss_bbox, loss_giou, card_err]))
    return torch.stack(rows)


def loss_and_grads(c, match, upstream, dtype):
    """(losses (L,4), grad_logits, grad_boxes) of ``(loss_terms * upstream).sum()`` at ``dtype`` on the CPU."""
    logits = torch.from_numpy(c["logits"]).to(dtype).requires_grad_(True)
    boxes = torch.from_numpy(c["boxes"]).to(dtype).requires_grad_(True)
    losses = loss_terms(c, match, logits, boxes)
    gl, gb = torch.autograd.grad((losses * torch.as_tensor(upstream).to(dtype)).sum(), [logits, boxes], allow_unused=True)
    gb = torch.zeros_like(boxes) if gb is None else gb
    return losses.detach(), gl, gb


def upstream_of(c, seed=77):
    return hash_uniform((c["L"], 4), seed, 0.5, 2.0)


# ---- assignments --------------------------------------------------------------------------------------------------------------------
def brute_force(cost):
    """The minimal total of min(nr, nc) pairs of a small matrix, by enumeration."""
    cost = np.asarray(cost, dtype=np.float64)
    nr, nc = cost.shape
    if nr > nc:
        cost, nr, nc = cost.T, nc, nr
    assert nc <= 7
    if nr == 0:
        return 0.0
    rows = np.arange(nr)
    return min(float(cost[rows, list(p)].sum()) for p in itertools.permutations(range(nc), nr))


def total_of(cost, match_row, T):
    """The float64 total of the pairs of one image's ``match`` row over the first ``T`` columns of its cost matrix."""
    cost = np.asarray(cost, dtype=np.float64)
    q = np.nonzero(np.asarray(match_row) >= 0)[0]
    return float(cost[q, np.asarray(match_row)[q]].sum()) if T else 0.0


def check_matching(match_row, Q, T):
    """A valid matching: targets in [0, T), each at most once, exactly min(Q, T) queries matched."""
    m = np.asarray(match_row)
    assert m.shape == (Q,)
    used = m[m >= 0]
    assert ((m >= -1) & (m < max(T, 1))).all() and (T > 0 or (m == -1).all()), m
    assert len(used) == min(Q, T) and len(set(used.tolist())) == len(used), (m, Q, T)
