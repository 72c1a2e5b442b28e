"""``PanopticMetric``: panoptic / segmentation / recognition quality and the centre and offset errors of a Panoptic-DeepLab head."""
import numpy as np
import torch

from .. import ops as _ops
from ..utilities import panoptic_post_processing as _pp
from .base import MetricBase, fusable, host_copy

__all__ = ["PanopticMetric"]

CITYSCAPES_THINGS = (11, 12, 13, 14, 15, 16, 17, 18)       # person .. bicycle: the reference's CityScapesDataset.cityscapes_things
NMS_KERNEL, TOP_K = 7, 100                                  # what the reference's metric passes to get_instance_segmentation


def overlap_stock(pred_inst, tgt_inst, pred_seg, tgt_seg, max_ids, num_classes):
    """``cerberus::instance_overlap`` in stock ops, on the maps' device and without a host synchronisation: (B,M,M), (B,M,C),
    (B,M,C) int64.  The cells are counted by ``scatter_add_`` into one row per image with an extra cell for the pixels that do
    not count, as ``semantic.confusion_stock``."""
    B = pred_inst.shape[0]
    M, C = int(max_ids), int(num_classes)
    dev = pred_inst.device
    pi, ti, ps, ts = (t.reshape(B, -1).to(torch.int64) for t in (pred_inst, tgt_inst, pred_seg, tgt_seg))
    both = (pi >= 0) & (pi < M) & (ti >= 0) & (ti < M)

    def count(valid, cell, cells):
        cell = torch.where(valid, cell, torch.full_like(cell, cells)) + torch.arange(B, device=dev)[:, None] * (cells + 1)
        out = torch.zeros(B * (cells + 1), dtype=torch.int64, device=dev)
        out.scatter_add_(0, cell.reshape(-1), torch.ones_like(cell).reshape(-1))
        return out.view(B, cells + 1)[:, :cells]

    inter = count(both, pi * M + ti, M * M).reshape(B, M, M)
    pred_cls = count(both & (ps >= 0) & (ps < C), pi * C + ps, M * C).reshape(B, M, C)
    tgt_cls = count(both & (ts >= 0) & (ts < C), ti * C + ts, M * C).reshape(B, M, C)
    return inter, pred_cls, tgt_cls


def quality_from_counts(inter, pred_cls, tgt_cls, ids=None):
    """(PQ, SQ, RQ) of one image from its intersection matrix [pred row, target row] and the two class histograms
    [row, class], with the reference's bookkeeping (panoptic.py:34-78) in float64; ``ids[r]`` is the instance id of row r
    (default: r itself).  A row counts as present if it has a pixel."""
    inter = np.asarray(inter, dtype=np.int64)
    ids = np.arange(inter.shape[0]) if ids is None else np.asarray(ids)
    pred_areas, tgt_areas = inter.sum(axis=1), inter.sum(axis=0)
    pred_rows, tgt_rows = np.flatnonzero(pred_areas), np.flatnonzero(tgt_areas)
    if pred_rows.size == 1 and tgt_rows.size == 1:
        return np.nan, np.nan, np.nan                       # neither side has an instance (one id each: the background)
    matched = []
    iou_sum = np.float64(0)
    true_positives = 0
    for i in pred_rows:
        if not ids[i]:
            continue
        for j in np.flatnonzero(inter[i]):                  # every target id it touches, the background (id 0) included
            iou = inter[i, j] / (pred_areas[i] + tgt_areas[j] - inter[i, j])
            if iou > 0.5:
                true_positives += 1
                iou_sum += iou
                matched.append((i, j))
    # "minus one" removes the background from each difference, whether or not it is there (the reference's count)
    false_positives = len(set(pred_rows.tolist()) - set(i for i, _ in matched)) - 1
    false_negatives = len(set(tgt_rows.tolist()) - set(j for _, j in matched)) - 1
    # a match whose majority classes differ becomes a false positive; its IoU stays in the sum
    for i, j in matched:
        if np.argmax(pred_cls[i]) != np.argmax(tgt_cls[j]):
            true_positives -= 1
            false_positives += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        denominator = np.float64(true_positives + 0.5 * false_positives + 0.5 * false_negatives)
        panoptic_quality = iou_sum / denominator
        segmentation_quality = iou_sum / true_positives if true_positives != 0 else true_positives
        recognition_quality = true_positives / denominator
    return panoptic_quality, segmentation_quality, recognition_quality


def counts_from_maps(pred_inst, pred_seg, target_inst, target_seg):
    """The matrices ``quality_from_counts`` takes, from four numpy maps of one image, with ``np.bincount``: ids and classes
    are ranked jointly first, so that any integer values will do.  Returns (inter, pred_cls, tgt_cls, ids)."""
    n = np.asarray(pred_inst).size
    ids, rank = np.unique(np.concatenate([np.ravel(pred_inst), np.ravel(target_inst)]), return_inverse=True)
    classes, crank = np.unique(np.concatenate([np.ravel(pred_seg), np.ravel(target_seg)]), return_inverse=True)
    rank, crank = rank.reshape(-1), crank.reshape(-1)
    pi, ti, ps, ts = rank[:n], rank[n:], crank[:n], crank[n:]
    M, C = ids.size, classes.size
    inter = np.bincount(pi * M + ti, minlength=M * M).reshape(M, M)
    pred_cls = np.bincount(pi * C + ps, minlength=M * C).reshape(M, C)
    tgt_cls = np.bincount(ti * C + ts, minlength=M * C).reshape(M, C)
    return inter, pred_cls, tgt_cls, ids


class PanopticMetric(MetricBase):
    """Panoptic, segmentation and recognition quality (``Batch_PQ`` / ``Batch_SQ`` / ``Batch_RQ``: one entry per image that
    has an instance on either side), the per-image offset error ``norm(pred - target, dim=1).mean()`` (``Batch_Offset_MSE``)
    and the mean assignment distance between the predicted peaks and ``targets['center_points']`` (``Batch_Center_MSE``) of
    ``predictions`` / ``targets`` with the keys ``seg`` ((B,C,H,W) scores / (B,H,W) labels), ``center`` ((B,1,H,W) heat maps)
    and ``offset`` ((B,2,H,W), (dy, dx)): the reference's ``PanopticMetric``.  Instances are found as the reference does: NMS
    kernel 7, threshold 0.1, ``top_k=100`` (so at most 99 centres, see ``utilities.panoptic_post_processing``), for the
    prediction and for the target.

    ``backend='hip'``: float32 CUDA tensors take ``cerberus::center_peaks``, ``cerberus::group_pixels`` and
    ``cerberus::instance_overlap`` for the whole batch at once (and ``cerberus::flow_metric_sums`` for the offset error); the
    centres are selected on the device with stock ops; the qualities are finished in float64 on the host from the (B,101,101)
    intersection matrices and the class histograms.  Everything else takes the stock-op restatements.  Either way there are at
    most two synchronisations per ``add_sample``, whatever B: the one host copy, and -- only when some image has ground-truth
    ``center_points`` -- one ``torch.nonzero`` over the batch's predicted peak map, whose result travels in that same copy.

    Quirks of the reference that are kept: IoU > 0.5 pairs count whatever the target id, the background (id 0) included; false
    positives and negatives are set differences "minus one"; a true positive whose majority classes differ is demoted to a
    false positive without its IoU leaving the sum; an image with no instance on either side gives NaNs and is left out.
    Deliberate differences from the reference:
      * ``thing_list`` is a constructor argument (default: the Cityscapes things 11..18, which the reference takes from its
        dataset class); classes outside ``[0, num_classes)`` vote as ONE extra class in the majority vote;
      * nothing in ``predictions`` / ``targets`` is written (the reference thresholds the centre maps in place);
      * the offset error of the fused path is accumulated in float64.
    ``base_dir`` / ``savefile`` are accepted and ignored (see ``MetricBase``).
    """

    def __init__(self, num_classes, main_metric="PQ", mode="training", base_dir=None, savefile="", thing_list=None, backend="hip",
                 **kwargs):
        super().__init__(savefile=savefile, base_dir=base_dir, main_metric=main_metric, mode=mode, backend=backend)
        self._n_classes = int(num_classes)
        self.thing_list = list(CITYSCAPES_THINGS if thing_list is None else thing_list)
        self._reset_metric()
        assert self.main_metric in self.metric_data.keys()

    # ---- the reference's static methods --------------------------------------------------------------------------------------
    @staticmethod
    def calculate_pq(pred_inst, pred_seg, target_inst, target_seg):
        """(PQ, SQ, RQ) of one prediction / target pair of numpy id and class maps; NaNs when neither has an instance."""
        inter, pred_cls, tgt_cls, ids = counts_from_maps(pred_inst, pred_seg, target_inst, target_seg)
        return quality_from_counts(inter, pred_cls, tgt_cls, ids)

    @staticmethod
    def batch_process_pq(predictions, targets, thing_list=None, backend="hip"):
        """Image by image, as the reference: three arrays (PQ, SQ, RQ) over the images that have an instance."""
        things = list(CITYSCAPES_THINGS if thing_list is None else thing_list)
        results = ([], [], [])
        seg_pred = torch.argmax(predictions["seg"], dim=1)
        for idx in range(predictions["center"].shape[0]):
            pred_inst, _ = _pp.get_instance_segmentation(seg_pred[idx].unsqueeze(0), predictions["center"][idx].unsqueeze(0),
                                                         predictions["offset"][idx].unsqueeze(0), things, nms_kernel=NMS_KERNEL,
                                                         top_k=TOP_K, backend=backend)
            tgt_inst, _ = _pp.get_instance_segmentation(targets["seg"][idx], targets["center"][idx].unsqueeze(0),
                                                        targets["offset"][idx].unsqueeze(0), things, nms_kernel=NMS_KERNEL,
                                                        top_k=TOP_K, backend=backend)
            quality = PanopticMetric.calculate_pq(pred_inst.cpu().numpy(), seg_pred[idx].cpu().numpy(), tgt_inst.cpu().numpy(),
                                                  targets["seg"][idx].cpu().numpy())
            if not any(np.isnan(quality)):
                for store, value in zip(results, quality):
                    store.append(value)
        return tuple(np.asarray(r) for r in results)

    @staticmethod
    def batch_process_center_mse(predictions, targets, backend="hip"):
        """The mean assignment distance between each image's predicted peaks (NMS kernel 7, no ``top_k``) and its
        ``center_points``, over the images that have both."""
        results = []
        for idx in range(predictions["center"].shape[0]):
            if not targets["center_points"][idx]:
                continue
            center_preds = _pp.find_instance_center(predictions["center"][idx], nms_kernel=NMS_KERNEL, backend=backend).type(torch.float32)
            if not center_preds.shape[0]:
                continue
            center_gt = torch.as_tensor(targets["center_points"][idx], device=center_preds.device, dtype=torch.float32)
            results.append(_pp.assignment_cost(center_preds, center_gt).mean())
        return np.asarray(results)

    # ---- one add_sample ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _maps(t):
        return t.reshape((t.shape[0],) + tuple(t.shape[-2:]))

    def _device_part(self, predictions, targets):
        """Everything an ``add_sample`` does on the device before its copies, without a synchronisation (capturable): the
        packed (B, n) int64 tensor -- intersection matrix, the two class histograms and the bits of the float64 offset
        error of each image -- and the predicted peak map (B,H,W)."""
        backend, C, M = self.backend, self._n_classes, TOP_K + 1
        seg_pred = torch.argmax(predictions["seg"].detach(), dim=1)
        seg_tgt = self._maps(targets["seg"]).to(device=seg_pred.device, dtype=torch.int64)
        insts, peaks = [], []
        for side, sem in ((predictions, seg_pred), (targets, seg_tgt)):
            heat, offset = self._maps(side["center"].detach()), side["offset"].detach()
            peak = self._maps(_pp.center_peaks(heat, 0.1, NMS_KERNEL, backend))
            centers, counts = _pp.select_centers(peak, TOP_K)
            insts.append(_pp.group_things(offset, centers, counts, sem, self.thing_list, backend))
            peaks.append(peak)
        # classes outside [0, C) (an ignore label) vote as class C
        cls = [torch.where((s >= 0) & (s < C), s, torch.full_like(s, C)) for s in (seg_pred, seg_tgt)]
        if (backend == "hip" and seg_pred.is_cuda and seg_tgt.device == seg_pred.device and seg_pred.numel() > 0
                and M * (M + 2 * (C + 1)) <= _ops.INSTANCE_OVERLAP_MAX_BINS):
            counts3 = torch.ops.cerberus.instance_overlap(insts[0], insts[1], cls[0], cls[1], M, C + 1)
        else:
            counts3 = overlap_stock(insts[0], insts[1], cls[0], cls[1], M, C + 1)
        p_off, t_off = predictions["offset"].detach(), targets["offset"]
        B = p_off.shape[0]
        if backend == "hip" and fusable(p_off, t_off) and p_off.numel() > 0:
            ones = torch.ones((B,) + tuple(p_off.shape[2:]), dtype=torch.float32, device=p_off.device)
            sums, _ = torch.ops.cerberus.flow_metric_sums(p_off, t_off, ones)          # sum of norm(dy, dx) per image, float64
            error = sums[:, 0] / float(p_off.shape[2] * p_off.shape[3])
        else:
            error = torch.linalg.norm(p_off - t_off, dim=1).mean(dim=(1, 2)).to(torch.float64)
        packed = torch.cat([c.reshape(B, -1) for c in counts3] + [error.reshape(B, 1).view(torch.int64)], dim=1)
        return packed, peaks[0]

    def _record(self, host, center_points=None):
        """The host part: ``host`` is the flat int64 array of the sample -- B packed rows, then, if ``center_points`` is
        given, the (N,3) indices (image, y, x) of the predicted peaks."""
        C1, M = self._n_classes + 1, TOP_K + 1
        row = M * M + 2 * M * C1 + 1
        B = len(center_points) if center_points is not None else host.size // row
        rows = host[:B * row].reshape(B, row)
        results = ([], [], [])
        for r in rows:
            inter = r[:M * M].reshape(M, M)
            pred_cls = r[M * M:M * M + M * C1].reshape(M, C1)
            tgt_cls = r[M * M + M * C1:row - 1].reshape(M, C1)
            quality = quality_from_counts(inter, pred_cls, tgt_cls)
            if not any(np.isnan(quality)):
                for store, value in zip(results, quality):
                    store.append(value)
        for key, store in zip(("Batch_PQ", "Batch_SQ", "Batch_RQ"), results):
            self.metric_data[key].append(np.asarray(store))
        self.metric_data["Batch_Offset_MSE"].append(np.ascontiguousarray(rows[:, -1]).view(np.float64))
        errors = []
        if center_points is not None:
            found = torch.from_numpy(np.ascontiguousarray(host[B * row:].reshape(-1, 3)))
            for idx, points in enumerate(center_points):
                preds = found[found[:, 0] == idx][:, 1:].type(torch.float32)
                if not points or not preds.shape[0]:
                    continue
                errors.append(_pp.assignment_cost(preds, torch.as_tensor(points, dtype=torch.float32)).mean())
        self.metric_data["Batch_Center_MSE"].append(np.asarray(errors))

    def add_sample(self, predictions, targets, loss=0, **kwargs):
        assert all(key in predictions for key in ['center', 'offset', 'seg']), \
            "Missing key in predictions required for panoptic caluclations."
        assert all(key in targets for key in ['center', 'offset', 'seg', 'center_points']), \
            "Missing key in targets required for panoptic caluclations."
        self.metric_data["Batch_Loss"].append(loss)
        packed, peaks = self._device_part(predictions, targets)
        B = packed.shape[0]
        center_points = [targets["center_points"][idx] for idx in range(B)]
        packed = packed.reshape(-1)
        if any(center_points):
            packed = torch.cat([packed, torch.nonzero(peaks > 0).reshape(-1)])        # the second synchronisation
        else:
            center_points = None
        self._record(host_copy(packed), center_points)

    def _reset_metric(self):
        self.metric_data = dict(Batch_Loss=[], Batch_Center_MSE=[], Batch_Offset_MSE=[], Batch_PQ=[], Batch_SQ=[], Batch_RQ=[])
