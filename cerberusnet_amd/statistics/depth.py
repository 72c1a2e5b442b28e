"""``DepthMetric``: the error and accuracy statistics of the depth head, per image."""
import numpy as np
import torch

from .base import MetricBase, fusable, host_copy, pack_rows, unpack_rows

__all__ = ["DepthMetric"]

KEYS = ("Batch_Absolute_Relative", "Batch_Squared_Relative", "Batch_RMSE_Linear", "Batch_RMSE_Log", "Batch_Invariant",
        "Batch_a1", "Batch_a2", "Batch_a3")


def depth_metrics_stock(pred, gt, min_depth=0.0, max_depth=80.0):
    """The reference's chain (depth.py:35-78) in stock ops and its operation order, out of place, on the tensors' device: the
    eight per-image metrics in the order of ``KEYS``, each a (B,) tensor."""
    if pred.dim() == 4:
        pred = pred.squeeze(dim=1)
    pred = torch.where(pred == 0, pred + 1e-7, pred)                    # the reference adds in place, into the model's output
    valid = (gt < max_depth) & (gt > min_depth)
    n_valid = torch.sum(valid, dim=(1, 2))
    skip = ~valid
    difference = (pred - gt).masked_fill(skip, 0.)
    squared_diff = difference.pow(2)
    log_diff = (torch.log(pred) - torch.log(gt)).masked_fill(skip, 0.)
    sq_log_diff = torch.sum(log_diff.pow(2), dim=(1, 2)) / n_valid
    abs_rel = torch.sum((difference.abs() / gt).masked_fill(skip, 0.), dim=(1, 2)) / n_valid
    sqr_rel = torch.sum((squared_diff / gt).masked_fill(skip, 0.), dim=(1, 2)) / n_valid
    rmse = torch.sqrt(torch.sum(squared_diff, dim=(1, 2)) / n_valid)
    rmse_log = torch.sqrt(sq_log_diff)
    invariant = sq_log_diff - torch.sum(log_diff.abs(), dim=(1, 2)) ** 2 / n_valid ** 2     # the SUM of |log| squared, as the reference
    ratio = torch.max(pred / gt, gt / pred).masked_fill(skip, 1.25 ** 3)
    acc = [torch.sum(ratio < 1.25 ** k, dim=(1, 2)) / n_valid for k in (1, 2, 3)]
    return [abs_rel, sqr_rel, rmse, rmse_log, invariant] + acc


def depth_metrics_from_sums(sums, counts):
    """The eight metrics, in the order of ``KEYS``, in float64 on the host from the (B,5) sums and (B,4) counts of
    ``cerberus::depth_metric_sums``."""
    sums = np.asarray(sums, dtype=np.float64)
    n = np.asarray(counts, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        sq_log = sums[:, 3] / n[:, 0]
        return [sums[:, 0] / n[:, 0], sums[:, 1] / n[:, 0], np.sqrt(sums[:, 2] / n[:, 0]), np.sqrt(sq_log),
                sq_log - sums[:, 4] ** 2 / n[:, 0] ** 2, n[:, 1] / n[:, 0], n[:, 2] / n[:, 0], n[:, 3] / n[:, 0]]


class DepthMetric(MetricBase):
    """Absolute and squared relative error, linear and log RMSE, the reference's "invariant" term and the a1 / a2 / a3
    accuracies of ``predictions['depth']`` ((B,1,h,w) or (B,h,w); of a list its element 0) against ``targets['disparity']``
    (B,h,w), one (B,) array per key and batch, over the pixels with ``min_depth < gt < max_depth``: the reference's
    ``DepthMetric``.

    ``backend='hip'``: float32 CUDA tensors take ONE fused op (``cerberus::depth_metric_sums``: one read of prediction and
    ground truth, five float64 sums and four counts per image) and one device-to-host copy; the divisions and square roots are
    finished in float64 on the host (float64 arrays).  Everything else takes ``depth_metrics_stock`` (arrays in the tensors'
    precision, float32 for 16-bit tensors) and the same single copy.

    Deliberate differences from the reference:
      * no mutation: the reference writes ``+= 1e-7`` into the zeros of the model's prediction; here the prediction is read only;
      * an image without a valid pixel gets NaN in every metric (the reference's 0 / 0), the other images are not affected.
    ``base_dir`` / ``savefile`` are accepted and ignored (see ``MetricBase``).
    """

    def __init__(self, main_metric="RMSE_Linear", mode="training", base_dir=None, savefile="", min_depth=0.0, max_depth=80.0,
                 backend="hip", **kwargs):
        super().__init__(savefile=savefile, base_dir=base_dir, main_metric=main_metric, mode=mode, backend=backend)
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self._reset_metric()
        assert self.main_metric in self.metric_data.keys()

    def _device_part(self, predictions, targets):
        """Everything an ``add_sample`` does on the device (capturable): one 2-D tensor and what ``_record`` needs to read it."""
        pred = predictions["depth"][0] if isinstance(predictions["depth"], list) else predictions["depth"]
        pred, gt = pred.detach(), targets["disparity"]
        if (self.backend == "hip" and fusable(pred, gt) and pred.numel() > 0 and gt.dim() == 3
                and (pred.dim() == 3 or (pred.dim() == 4 and pred.shape[1] == 1))):
            sums, counts = torch.ops.cerberus.depth_metric_sums(pred, gt, self.min_depth, self.max_depth)
            return torch.cat([sums, counts.to(torch.float64)], dim=1), None       # counts < 2^31: exact in float64
        return pack_rows(depth_metrics_stock(pred, gt, self.min_depth, self.max_depth))

    def _record(self, host, back):
        rows = depth_metrics_from_sums(host[:, :5], host[:, 5:]) if back is None else unpack_rows(host, back)
        for key, row in zip(KEYS, rows):
            self.metric_data[key].append(row)

    def add_sample(self, predictions, targets, loss=0, **kwargs):
        assert "depth" in predictions.keys() and "disparity" in targets.keys()
        self.metric_data["Batch_Loss"].append(loss)
        packed, back = self._device_part(predictions, targets)
        self._record(host_copy(packed), back)

    def _reset_metric(self):
        self.metric_data = {key: [] for key in ("Batch_Loss",) + KEYS}
