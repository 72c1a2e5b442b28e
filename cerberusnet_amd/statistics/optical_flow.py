"""``OpticFlowMetric``: end-point error, outlier rate and the warped sequence's absolute difference, per image."""
import numpy as np
import torch
import torch.nn.functional as F

from ..loss_functions.UnFlowLoss import mesh_grid, norm_grid
from .base import MetricBase, fusable, host_copy, pack_rows, unpack_rows

__all__ = ["OpticFlowMetric"]


def flow_metrics_stock(flow_pred, flow_gt, mask):
    """The reference's chain (optical_flow.py:28-37, :53-63) in stock ops and its operation order, on the tensors' device: the
    per-image end-point error and outlier rate, (B,) each.  ``mask`` is (B,H,W)."""
    n_valid = torch.sum(mask, dim=(1, 2))
    diff = flow_pred - flow_gt
    norm_diff = (diff[:, 0, :, :] ** 2 + diff[:, 1, :, :] ** 2) ** 0.5
    masked = norm_diff * mask
    epe = torch.sum(masked, dim=(1, 2)) / n_valid
    magnitude = torch.sqrt(torch.sum(torch.square(flow_gt), dim=1))
    # the reference's float32 torch.tensor([1e-10]), filled on the device (the reference asks .get_device(): GPU tensors only)
    floor = torch.full((1,), 1e-10, dtype=torch.float32, device=flow_gt.device)
    bad = torch.logical_and(masked > 3, masked / torch.maximum(magnitude, floor) > 0.05)
    return epe, torch.sum(bad, dim=(1, 2)) / n_valid


def sad_stock(image, source, flow):
    """mean |image - flow_warp(source, flow)| per image (optical_flow.py:68-70) with the stock ``grid_sample``; the pixel grid
    is built on the tensors' device (no host-to-device copy: capturable)."""
    b, _, h, w = source.shape
    grid = norm_grid(mesh_grid(b, h, w, device=source.device).type_as(source) + flow)
    warped = F.grid_sample(source, grid, mode="bilinear", padding_mode="border", align_corners=False)
    return (image - warped).abs().mean(dim=(1, 2, 3))


class OpticFlowMetric(MetricBase):
    """End-point error (``Batch_EPE``), the outlier rate (``Batch_Fl_all``: EPE > 3 px and > 5 % of the ground truth's
    magnitude) and the mean absolute difference between ``targets['l_img']`` and ``targets['l_seq']`` warped by the flow
    (``Batch_SAD``) of ``predictions['flow']`` ((B,2,H,W); of a list its element 0), one (B,) array per key and batch: the
    reference's ``OpticFlowMetric``.  Without ``targets['flow']`` / ``targets['flow_mask']`` EPE and Fl are (B,1) zeros, as in
    the reference.

    ``backend='hip'``: float32 CUDA tensors take two fused ops (``cerberus::flow_metric_sums`` and ``cerberus::warp_sad``: the
    warped image is never stored) and one device-to-host copy; the divisions are finished in float64 on the host (float64
    arrays).  Everything else takes ``flow_metrics_stock`` / ``sad_stock`` (arrays in the tensors' precision, float32 for 16-bit
    tensors) and the same single copy.

    Deliberate differences from the reference:
      * no mutation: the reference replaces ``targets['flow_mask']`` by its squeezed form; here a (B,1,H,W) mask keeps its shape;
      * the stock path follows its tensors' device (the reference's ``error_rate`` breaks on CPU tensors).
    ``base_dir`` / ``savefile`` are accepted and ignored (see ``MetricBase``).
    """

    def __init__(self, main_metric="EPE", mode="training", base_dir=None, savefile="", backend="hip", **kwargs):
        super().__init__(savefile=savefile, base_dir=base_dir, main_metric=main_metric, mode=mode, backend=backend)
        self._reset_metric()
        assert self.main_metric in self.metric_data.keys()

    def _device_part(self, predictions, targets):
        """Everything an ``add_sample`` does on the device (capturable): one 2-D tensor and what ``_record`` needs to read it."""
        flow = predictions["flow"][0] if isinstance(predictions["flow"], list) else predictions["flow"]
        flow = flow.detach()
        image, source = targets["l_img"], targets["l_seq"]
        supervised = all(key in targets.keys() for key in ("flow", "flow_mask"))
        mask = None
        if supervised:
            mask = targets["flow_mask"]
            mask = mask.squeeze(1) if mask.dim() == 4 else mask           # out of place: the dict keeps its tensor
        tensors = (flow, image, source) + ((targets["flow"], mask) if supervised else ())
        if self.backend == "hip" and fusable(*tensors) and flow.numel() > 0 and image.numel() > 0:
            sad = torch.ops.cerberus.warp_sad(image, source, flow)
            if not supervised:
                return sad[None], ("sums", False, image[0].numel())
            sums, counts = torch.ops.cerberus.flow_metric_sums(flow, targets["flow"], mask)
            packed = torch.cat([sums, counts.to(torch.float64), sad[:, None]], dim=1).t()     # counts < 2^31: exact in float64
            return packed, ("sums", True, image[0].numel())
        rows = [sad_stock(image, source, flow)]
        if supervised:
            rows = list(flow_metrics_stock(flow, targets["flow"], mask)) + rows
        packed, back = pack_rows(rows)
        return packed, ("rows", supervised, back)

    def _record(self, host, how):
        kind, supervised, extra = how
        batch = host.shape[1]
        if kind == "sums":
            with np.errstate(divide="ignore", invalid="ignore"):
                rows = [host[-1] / float(extra)]
                if supervised:
                    rows = [host[0] / host[1], host[2] / host[1]] + rows
        else:
            rows = unpack_rows(host, extra)
        if supervised:
            self.metric_data["Batch_EPE"].append(rows[0])
            self.metric_data["Batch_Fl_all"].append(rows[1])
        else:
            self.metric_data["Batch_EPE"].append(np.zeros((batch, 1)))
            self.metric_data["Batch_Fl_all"].append(np.zeros((batch, 1)))
        self.metric_data["Batch_SAD"].append(np.ascontiguousarray(rows[-1]))

    def add_sample(self, predictions, targets, loss=0, **kwargs):
        self.metric_data["Batch_Loss"].append(loss if loss is not None else 0)
        packed, how = self._device_part(predictions, targets)
        self._record(host_copy(packed), how)

    def _reset_metric(self):
        self.metric_data = {"Batch_Loss": [], "Batch_SAD": [], "Batch_Fl_all": [], "Batch_EPE": []}
