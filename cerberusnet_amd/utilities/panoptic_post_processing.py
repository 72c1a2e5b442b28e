"""Post-processing of a Panoptic-DeepLab head: instance centres from the centre heat map, an instance id per pixel from the
offset map, and the merge with the semantic labels -- the reference's ``nnet_training/utilities/panoptic_post_processing.py``
with its names, argument order and ``ValueError``s, plus a trailing ``backend`` keyword.

``backend='hip'`` (default): float32 CUDA inputs take the fused ops ``cerberus::center_peaks`` (threshold + non-maximum
suppression in one pass, written to a new tensor) and ``cerberus::group_pixels`` (the argmin over the centres, held in LDS;
nothing of size K x H*W is stored).  Everything else -- ``backend='torch'``, CPU tensors, other dtypes, a thing class of 64 or
more, more centres than ``ops.GROUP_PIXELS_MAX_CENTERS`` -- takes a stock-op restatement in the reference's operation order,
which also runs on the CPU.  ``merge_semantic_and_instance`` is stock ops only.

Quirks of the reference that are kept:
  * ``top_k`` keeps only the scores STRICTLY GREATER than the k-th score: at most ``top_k - 1`` centres come back, and NONE
    when the best ``top_k`` peaks tie (40 ground-truth peaks of value 1.0 with ``top_k=10`` give 0 centres);
  * peaks are counted with ``> 0``, whatever ``threshold`` is;
  * centres come in row-major order, and an instance id is that order + 1;
  * a NaN in the heat map passes the threshold and is the maximum of every window that holds it (``max_pool2d``'s rule): the NaN
    pixel and its neighbours within the window's reach are no peaks.
Deliberate differences:
  * inputs are never mutated (the reference thresholds and suppresses ``ctr_hmp`` in place, which writes through to the
    model's own output when given a view);
  * a heat map with H == 1 or W == 1 works (the reference's ``squeeze()`` assertion fails there).
"""
import torch
import torch.nn.functional as F

from .. import ops as _ops
from ..statistics.base import BACKENDS

__all__ = ["get_semantic_segmentation", "find_instance_center", "group_pixels", "get_instance_segmentation",
           "merge_semantic_and_instance", "get_panoptic_segmentation", "compare_centers"]


def _check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError("backend must be one of %s, got %r" % (BACKENDS, backend))


def _fusable(backend, *tensors):
    first = tensors[0]
    return (backend == "hip" and first.is_cuda and first.numel() > 0
            and all(t.dtype == torch.float32 and t.device == first.device for t in tensors))


# ---- the batched building blocks (also what statistics.PanopticMetric runs) -------------------------------------------------------
def peaks_stock(ctr_hmp, threshold, nms_kernel):
    """The reference's chain (post_processing.py:52-59) out of place, for any batch: ``F.threshold(.., -1)``, ``max_pool2d``
    with stride 1 and padding ``(nms_kernel - 1) // 2``, and -1 wherever the two differ.  (B,1,H,W) or (B,H,W), any device."""
    v = F.threshold(ctr_hmp, threshold, -1)
    pooled = F.max_pool2d(v, kernel_size=nms_kernel, stride=1, padding=(nms_kernel - 1) // 2)
    return torch.where(v != pooled, torch.full_like(v, -1), v)


def center_peaks(ctr_hmp, threshold=0.1, nms_kernel=3, backend="hip"):
    """The heat map after thresholding and non-maximum suppression: its own value at a peak, -1 elsewhere.  A new tensor."""
    if (_fusable(backend, ctr_hmp) and nms_kernel % 2 == 1 and 1 <= nms_kernel <= _ops.CENTER_PEAKS_MAX_KERNEL
            and (ctr_hmp.dim() == 3 or (ctr_hmp.dim() == 4 and ctr_hmp.shape[1] == 1))):
        return torch.ops.cerberus.center_peaks(ctr_hmp, float(threshold), int(nms_kernel))
    return peaks_stock(ctr_hmp, threshold, nms_kernel)


def select_centers(peaks, top_k):
    """The reference's selection rule (post_processing.py:65-75) for a whole batch without a host synchronisation:
    ``peaks`` (B,H,W) -> centres (B,top_k,2) int64 (y, x) in row-major order and counts (B,) int64; rows at and past
    ``counts[b]`` hold (H, 0).  All peaks (``> 0``) of an image that has fewer than ``top_k``; else those strictly greater
    than the ``top_k``-th largest value of the map."""
    B, H, W = peaks.shape
    flat = peaks.reshape(B, H * W)
    positive = flat > 0
    kth = torch.topk(flat, min(top_k, H * W), dim=1).values[:, -1:]
    few = positive.sum(dim=1, keepdim=True) < top_k
    keep = torch.where(few, positive, flat > kth)
    index = torch.arange(H * W, device=peaks.device).expand(B, -1)
    first = torch.topk(torch.where(keep, index, torch.full_like(index, H * W)), min(top_k, H * W), dim=1, largest=False).values
    if first.shape[1] < top_k:
        first = F.pad(first, (0, top_k - first.shape[1]), value=H * W)
    return torch.stack((first // W, first % W), dim=2), keep.sum(dim=1)


def group_stock(offsets, centers, counts):
    """The reference's ``group_pixels`` chain (post_processing.py:95-114) for image after image in stock ops: (B,H,W) int64,
    zeros for an image without a centre.  No host synchronisation: every image computes the distances to all Kmax rows and
    the rows at and past ``counts[b]`` are set to +inf before the argmin, which leaves the first minimal valid row."""
    B, _, H, W = offsets.shape
    if centers.shape[1] == 0:
        return torch.zeros((B, H, W), dtype=torch.int64, device=offsets.device)
    rows = torch.arange(centers.shape[1], device=offsets.device)
    out = []
    for b in range(B):
        distance = _distances(centers[b], offsets[b])
        distance = torch.where((rows < counts[b])[:, None], distance, torch.full_like(distance, float("inf")))
        out.append((torch.argmin(distance, dim=0).reshape(H, W) + 1) * (counts[b] > 0))
    return torch.stack(out)


def _distances(ctr, offsets):
    """(K,2) centres, (2,H,W) offsets -> (K, H*W) distances: the coordinate map plus the offsets, the (K, H*W, 2) difference
    to the centres, its norm."""
    height, width = offsets.shape[1:]
    y_coord = torch.arange(height, dtype=offsets.dtype, device=offsets.device)[:, None].expand(height, width)
    x_coord = torch.arange(width, dtype=offsets.dtype, device=offsets.device)[None, :].expand(height, width)
    ctr_loc = (torch.stack((y_coord, x_coord)) + offsets).reshape(2, height * width).transpose(1, 0)
    return torch.norm(ctr.unsqueeze(1) - ctr_loc.unsqueeze(0), dim=-1)


def _group_one(ctr, offsets):
    """(K,2) centres, (2,H,W) offsets -> (H,W) int64 ids: argmin of the distances + 1."""
    return torch.argmin(_distances(ctr, offsets), dim=0).reshape(offsets.shape[1:]) + 1


def thing_map(sem_seg, thing_list):
    """1 where ``sem_seg`` holds a thing class, 0 elsewhere, in ``sem_seg``'s dtype (post_processing.py:139-143)."""
    thing_seg = torch.zeros_like(sem_seg)
    for thing_class in thing_list:
        thing_seg = torch.where(sem_seg == thing_class, torch.ones_like(sem_seg), thing_seg)
    return thing_seg


def group_things(offsets, centers, counts, sem, thing_list, backend="hip"):
    """Batched instance ids: ``group_pixels`` times the thing map of ``sem`` (B,H,W) -- one fused launch where the inputs
    allow it, else ``group_stock`` and a product."""
    mask = _ops.thing_mask_of(thing_list)
    if (_fusable(backend, offsets) and mask is not None and sem.dtype == torch.int64 and sem.device == offsets.device
            and centers.shape[1] <= _ops.GROUP_PIXELS_MAX_CENTERS):
        signed = mask - (1 << 64) if mask >= 1 << 63 else mask
        return torch.ops.cerberus.group_pixels(offsets, centers.to(torch.int64), counts.to(torch.int64), sem, signed)
    return thing_map(sem, thing_list) * group_stock(offsets, centers, counts)


# ---- the reference's functions ---------------------------------------------------------------------------------------------------
def get_semantic_segmentation(sem, backend="hip"):
    """Semantic labels of raw [1, C, H, W] scores: [1, H, W] (argmax over the classes).  ValueError if the batch is not 1."""
    _check_backend(backend)
    if sem.size(0) != 1:
        raise ValueError('Only supports inference for batch size = 1')
    return torch.argmax(sem.squeeze(0), dim=0, keepdim=True)


def find_instance_center(ctr_hmp, threshold=0.1, nms_kernel=3, top_k=None, backend="hip"):
    """The centre points of a [1, 1, H, W] (or [1, H, W]) centre heat map: a [K, 2] int64 tensor of (y, x) in row-major
    order.  Scores at or below ``threshold`` are dropped, then everything that is not the maximum of its ``nms_kernel``
    window.  With ``top_k`` and at least that many peaks, only the peaks strictly greater than the ``top_k``-th score are
    kept: at most ``top_k - 1``, none when the best ``top_k`` tie (the reference's rule).  ``ctr_hmp`` is not written."""
    _check_backend(backend)
    if len(ctr_hmp.shape) == 4 and ctr_hmp.size(0) != 1:
        raise ValueError('Only supports inference for batch size = 1')
    if len(ctr_hmp.shape) == 3:
        ctr_hmp = ctr_hmp.unsqueeze(0)
    peaks = center_peaks(ctr_hmp, threshold, nms_kernel, backend)
    peaks = peaks.reshape(peaks.shape[-2:])                # the last two dimensions, whatever their sizes
    ctr_all = torch.nonzero(peaks > 0)
    if top_k is None:
        return ctr_all
    if ctr_all.size(0) < top_k:
        return ctr_all
    top_k_scores, _ = torch.topk(torch.flatten(peaks), top_k)
    return torch.nonzero(peaks > top_k_scores[-1])


def group_pixels(ctr, offsets, backend="hip"):
    """An instance id for every pixel: 1 + the index of the centre of ``ctr`` [K, 2] (y, x) nearest to the pixel's position
    plus its offset (``offsets`` [1, 2, H, W] in (dy, dx) order); the first of equally near centres.  [1, H, W] int64."""
    _check_backend(backend)
    if offsets.size(0) != 1:
        raise ValueError('Only supports inference for batch size = 1')
    if (_fusable(backend, offsets) and not ctr.is_floating_point() and ctr.device == offsets.device
            and 0 < ctr.shape[0] <= _ops.GROUP_PIXELS_MAX_CENTERS):
        counts = torch.full((1,), ctr.shape[0], dtype=torch.int64, device=offsets.device)
        return torch.ops.cerberus.group_pixels(offsets, ctr.to(torch.int64).unsqueeze(0), counts, None, -1)
    return _group_one(ctr, offsets.squeeze(0)).unsqueeze(0)


def get_instance_segmentation(sem_seg, ctr_hmp, offsets, thing_list, threshold=0.1, nms_kernel=3, top_k=None, thing_seg=None,
                              backend="hip"):
    """The class-agnostic instance id map [1, H, W] of semantic labels ``sem_seg`` [1, H, W], a centre heat map and an offset
    map, and the centres [1, K, 2]: ``group_pixels`` where ``thing_seg`` (default: the pixels of a class of ``thing_list``)
    is set, 0 elsewhere; all zeros without a centre.  No input is written."""
    _check_backend(backend)
    ctr = find_instance_center(ctr_hmp, threshold=threshold, nms_kernel=nms_kernel, top_k=top_k, backend=backend)
    if ctr.size(0) == 0:
        return torch.zeros_like(sem_seg), ctr.unsqueeze(0)
    mask = _ops.thing_mask_of(thing_list)
    if (thing_seg is None and offsets.size(0) == 1 and _fusable(backend, offsets) and mask is not None and sem_seg.dtype == torch.int64
            and sem_seg.device == offsets.device and sem_seg.numel() == offsets[0, 0].numel()
            and ctr.shape[0] <= _ops.GROUP_PIXELS_MAX_CENTERS):
        counts = torch.full((1,), ctr.shape[0], dtype=torch.int64, device=offsets.device)
        signed = mask - (1 << 64) if mask >= 1 << 63 else mask
        ins_seg = torch.ops.cerberus.group_pixels(offsets, ctr.unsqueeze(0), counts, sem_seg.reshape((1,) + tuple(offsets.shape[2:])),
                                                  signed)
        return ins_seg.reshape(sem_seg.shape) if sem_seg.dim() == 3 else ins_seg, ctr.unsqueeze(0)
    if thing_seg is None:
        thing_seg = thing_map(sem_seg, thing_list)
    ins_seg = group_pixels(ctr, offsets, backend=backend)
    return thing_seg * ins_seg, ctr.unsqueeze(0)


def merge_semantic_and_instance(sem_seg, ins_seg, label_divisor, thing_list, stuff_area, void_label, backend="hip"):
    """The panoptic map [1, H, W]: ``class * label_divisor + instance`` for things (the class by majority vote inside the
    instance's thing pixels, the instance numbered per class in the order of the ids), ``class * label_divisor`` for stuff
    regions of at least ``stuff_area`` pixels outside every instance, ``void_label`` elsewhere.  Stock ops only (it loops
    over the instances and synchronises for each, as the reference does)."""
    _check_backend(backend)
    pan_seg = torch.zeros_like(sem_seg) + void_label
    thing_seg = ins_seg > 0
    semantic_thing_seg = thing_map(sem_seg, thing_list)
    class_id_tracker = {}
    for ins_id in torch.unique(ins_seg):
        if ins_id == 0:
            continue
        thing_mask = (ins_seg == ins_id) & (semantic_thing_seg == 1)       # the vote counts thing pixels only
        if torch.nonzero(thing_mask).size(0) == 0:
            continue
        class_id, _ = torch.mode(sem_seg[thing_mask].view(-1, ))
        key = class_id.item()
        if key in class_id_tracker:
            new_ins_id = class_id_tracker[key]
        else:
            class_id_tracker[key] = 1
            new_ins_id = 1
        class_id_tracker[key] += 1
        pan_seg = torch.where(thing_mask, class_id * label_divisor + new_ins_id, pan_seg)
    for class_id in torch.unique(sem_seg):
        if class_id.item() in thing_list:
            continue
        stuff_mask = (sem_seg == class_id) & (~thing_seg)
        if torch.nonzero(stuff_mask).size(0) >= stuff_area:
            pan_seg = torch.where(stuff_mask, class_id * label_divisor, pan_seg)
    return pan_seg


def get_panoptic_segmentation(sem, ctr_hmp, offsets, thing_list, label_divisor, stuff_area, void_label, threshold=0.1, nms_kernel=3,
                              top_k=None, foreground_mask=None, backend="hip"):
    """Panoptic map [1, H, W] int64 and centres [1, K, 2] of raw [1, C, H, W] semantic scores (or [1, H, W] labels), a centre
    heat map [1, 1, H, W] and offsets [1, 2, H, W]; ``foreground_mask`` ([1, 2, H, W] scores or a [1, H, W] mask) replaces
    the thing map derived from the labels.  ValueError for a batch other than 1 or an unsupported rank."""
    _check_backend(backend)
    if sem.dim() != 4 and sem.dim() != 3:
        raise ValueError(f'Semantic prediction with un-supported dimension: {sem.dim()}.')
    if sem.dim() == 4 and sem.size(0) != 1:
        raise ValueError('Only supports inference for batch size = 1')
    if ctr_hmp.size(0) != 1:
        raise ValueError('Only supports inference for batch size = 1')
    if offsets.size(0) != 1:
        raise ValueError('Only supports inference for batch size = 1')
    if foreground_mask is not None:
        if foreground_mask.dim() != 4 and foreground_mask.dim() != 3:
            raise ValueError(f'Foreground prediction with un-supported dimension: {sem.dim()}.')
    semantic = get_semantic_segmentation(sem, backend=backend) if sem.dim() == 4 else sem
    thing_seg = None
    if foreground_mask is not None:
        thing_seg = get_semantic_segmentation(foreground_mask, backend=backend) if foreground_mask.dim() == 4 else foreground_mask
    instance, center = get_instance_segmentation(semantic, ctr_hmp, offsets, thing_list, threshold=threshold, nms_kernel=nms_kernel,
                                                 top_k=top_k, thing_seg=thing_seg, backend=backend)
    panoptic = merge_semantic_and_instance(semantic, instance, label_divisor, thing_list, stuff_area, void_label, backend=backend)
    return panoptic, center


def assignment_cost(center_preds, center_gt):
    """The costs of the minimum-cost (Hungarian) assignment between predicted and ground-truth centres: a float32 tensor of
    ``min(len(center_preds), len(center_gt))`` Euclidean distances.  Needs scipy."""
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError as exc:
        raise ImportError("cerberusnet_amd: comparing centre lists needs scipy (scipy.optimize.linear_sum_assignment), which "
                          "is not installed") from exc
    cost_mat = torch.cdist(center_preds, center_gt, p=2).cpu()
    return cost_mat[linear_sum_assignment(cost_mat)]


def compare_centers(center_list, center_heatmap, backend="hip"):
    """Mean (over the images that have both) of the mean assignment distance between each image's ground-truth centre list
    and the peaks of its heat map (``nms_kernel=7``, no ``top_k``), and the summed variance.  ``center_heatmap`` [B, 1, H, W]
    with a list of lists, or [1, H, W] with one list.  Prints both, as the reference; like it, fails when no image counts."""
    _check_backend(backend)
    if len(center_heatmap.shape) == 4:
        batch_size = center_heatmap.shape[0]
    else:
        batch_size = 1
        center_list = [center_list]
    divisor = batch_size
    total_mse = 0
    total_var = 0
    for idx in range(batch_size):
        if not center_list[idx]:
            divisor -= 1
            continue
        center_preds = find_instance_center(center_heatmap[idx], nms_kernel=7, backend=backend).type(torch.float32)
        if not center_preds.shape[0]:
            divisor -= 1
            continue
        center_gt = torch.as_tensor(center_list[idx], device=center_preds.device, dtype=torch.float32)
        costs = assignment_cost(center_preds, center_gt)
        total_mse += costs.mean()
        total_var += costs.var()
    center_mse = total_mse.item() / divisor
    center_var = total_var.item()
    print(f"MSE Between Centers and Heatmap: {center_mse:.2f}, {center_var}")
    return center_mse, center_var
