"""``SegmentationMetric``: pixel accuracy and IoU of the segmentation head from a per-image confusion matrix."""
import numpy as np
import torch

from .. import ops as _ops
from .base import MetricBase, host_copy

__all__ = ["SegmentationMetric"]


def confusion_stock(logits, target, ignore_index):
    """The reference's chain (semantic.py:41-48, :190-194: argmax, the label mask, ``C * label + prediction``, a count per
    cell) for the whole batch in stock ops, on the logits' device: (B,C,C) int64.  The cells are counted by ``scatter_add_``
    into one row of C*C + 1 cells per image -- the extra cell takes the pixels that do not count -- where the reference indexes
    with a boolean mask and calls ``bincount`` per image: both synchronise with the host, this does not."""
    B, C = logits.shape[:2]
    pred = torch.argmax(logits, dim=1).reshape(B, -1)
    labels = target.to(device=logits.device, dtype=torch.int64).reshape(B, -1)
    counted = (labels != ignore_index) & (labels >= 0) & (labels < C)
    cells = C * C + 1
    cell = torch.where(counted, labels * C + pred, C * C) + torch.arange(B, device=logits.device)[:, None] * cells
    conf = torch.zeros(B * cells, dtype=torch.int64, device=logits.device)
    conf.scatter_add_(0, cell.reshape(-1), torch.ones_like(cell).reshape(-1))
    return conf.view(B, cells)[:, :C * C].reshape(B, C, C)


class SegmentationMetric(MetricBase):
    """Pixel-wise accuracy (``Batch_PixelAcc``, (B,1) per batch) and class-wise intersection over union (``Batch_IoU``, (B,C)
    per batch) of ``predictions['seg']`` (B,C,H,W) logits against ``targets['seg']`` (B,H,W) labels, and the epoch's summed
    ``Confusion_Mat`` [label, prediction], as the reference's ``SegmentationMetric``.

    ``backend='hip'``: float32 CUDA logits with int64 labels on the same device and at most 64 classes take ONE fused launch
    (``cerberus::seg_confusion``: the argmax is streamed over the class planes, no index map is written) and one device-to-host
    copy of the (B,C,C) matrices; accuracy and IoU are finished in float64 on the host.  Everything else (``backend='torch'``,
    other dtypes, CPU tensors, more classes) takes ``confusion_stock`` and the same single copy.

    Deliberate differences from the reference:
      * the ignore label is the constructor argument ``ignore_index`` (default 255, which the reference hard-codes); labels
        outside ``[0, num_classes)`` are skipped as well (the reference would corrupt the matrix or raise);
      * ``Confusion_Mat`` is an int64 tensor (the reference: int32);
      * nothing is moved to a GPU: the labels follow the logits' device;
      * the pixel accuracy of an image with no counted pixel is NaN (0 / 0, as in the reference), and so is its IoU row.
    ``base_dir`` / ``savefile`` are accepted and ignored (see ``MetricBase``).
    """

    def __init__(self, num_classes, main_metric="IoU", mode="training", base_dir=None, savefile="", ignore_index=255, backend="hip",
                 **kwargs):
        super().__init__(savefile=savefile, base_dir=base_dir, main_metric=main_metric, mode=mode, backend=backend)
        self._n_classes = int(num_classes)
        self.ignore_index = int(ignore_index)
        self._reset_metric()
        assert self.main_metric in self.metric_data.keys()

    def _fused(self, logits, target):
        return (self.backend == "hip" and logits.is_cuda and logits.dtype == torch.float32 and target.dtype == torch.int64
                and target.device == logits.device and logits.dim() == 4 and 2 <= logits.shape[1] <= _ops.SEG_CONFUSION_MAX_CLASSES
                and logits.numel() > 0)

    def _device_part(self, predictions, targets):
        """Everything an ``add_sample`` does on the device: the (B,C,C) int64 confusion matrices (capturable)."""
        logits, target = predictions["seg"].detach(), targets["seg"]
        if self._fused(logits, target):
            return torch.ops.cerberus.seg_confusion(logits, target, self.ignore_index)
        return confusion_stock(logits, target, self.ignore_index)

    def _record(self, conf):
        """The host part: ``conf`` is the (B,C,C) int64 numpy array of the batch."""
        conf = conf.astype(np.int64, copy=False)
        self.metric_data["Confusion_Mat"] += torch.from_numpy(conf.sum(axis=0))
        hits = np.diagonal(conf, axis1=1, axis2=2).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            pix_acc = hits.sum(axis=1) / conf.sum(axis=(1, 2)).astype(np.float64)
            iou = hits / (conf.sum(axis=2) + conf.sum(axis=1) - np.diagonal(conf, axis1=1, axis2=2)).astype(np.float64)
        self.metric_data["Batch_PixelAcc"].append(pix_acc.reshape(-1, 1))
        self.metric_data["Batch_IoU"].append(iou)

    def add_sample(self, predictions, targets, loss=0, **kwargs):
        assert "seg" in predictions.keys() and "seg" in targets.keys()
        assert predictions["seg"].shape[1] == self._n_classes
        self.metric_data["Batch_Loss"].append(loss)
        self._record(host_copy(self._device_part(predictions, targets)))

    @staticmethod
    def _confmat_cls_iou(conf_mat):
        """Class-wise IoU of a confusion matrix (tensor or array): the diagonal over row sum + column sum - diagonal."""
        if isinstance(conf_mat, torch.Tensor):
            conf_mat = conf_mat.detach().cpu().numpy()
        if not isinstance(conf_mat, np.ndarray):
            raise NotImplementedError(type(conf_mat))
        hits = np.diag(conf_mat)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.true_divide(hits, conf_mat.sum(axis=1) + conf_mat.sum(axis=0) - hits)

    def _epoch_miou(self):
        return np.nanmean(self._confmat_cls_iou(self.metric_data["Confusion_Mat"]))

    def print_epoch_statistics(self):
        conf = self.metric_data["Confusion_Mat"].numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            pixel_acc = np.true_divide(np.diag(conf).sum(), conf.sum())
        loss = np.asarray(self.metric_data["Batch_Loss"]).mean()
        print("Pixel Accuracy: %.4f\tmIoU: %.4f\tLoss: %.4f" % (pixel_acc, self._epoch_miou(), loss))

    def get_current_statistics(self, main_only=True, return_loss=True):
        """As the reference: the IoU entry is the mean class IoU of the epoch's summed confusion matrix, with the mean over the
        images of the variance over the classes; every other entry is the mean and sample variance of the recorded values."""
        means, variances = (), ()
        if main_only:
            keys = [self.main_metric] + (["Batch_Loss"] if return_loss else [])
        else:
            keys = [k for k in sorted(self.metric_data) if k.startswith("Batch") and (return_loss or k != "Batch_Loss")]
        for key in keys:
            if key == "Batch_IoU":
                means += (self._epoch_miou(),)
                per_image = np.concatenate(self.metric_data[key]).reshape(-1, self._n_classes)
                variances += (np.nanvar(per_image, axis=1).mean(),)
            else:
                data = self._flat(self.metric_data[key])
                means += (data.mean(),)
                variances += (data.var(ddof=1),)
        return means, variances

    def get_last_batch(self, main_metric=True):
        if main_metric:
            last = self.metric_data[self.main_metric][-1]
            return np.nanmean(last) if self.main_metric == "Batch_IoU" else last
        out = ()
        for key in sorted(self.metric_data):
            if key == "Batch_IoU":
                out += (np.nanmean(self.metric_data[key][-1]),)
            elif key != "Batch_Loss":
                out += (self.metric_data[key][-1],)
        return out

    def _reset_metric(self):
        self.metric_data = {
            "Batch_Loss": [],
            "Batch_PixelAcc": [],
            "Batch_IoU": [],
            "Confusion_Mat": torch.zeros((self._n_classes, self._n_classes), dtype=torch.int64),
        }
