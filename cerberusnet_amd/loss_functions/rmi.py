"""Drop-in for the region mutual information losses of ``nnet_training/loss_functions/rmi.py`` (:33-258).

``RMILoss``, ``RMILossAux`` and ``MultiScaleRMILoss`` keep their names, constructor arguments, defaults, assertions and
``forward`` signatures (``do_rmi``, the ``'seg'`` / ``'seg_aux'`` and ``'pred'`` / ``'aux'`` keys).  The loss is

    loss = lambda * bce + (1 - lambda) * rmi          (``lambda_way=1``; otherwise ``bce + lambda * rmi``; ``bce`` alone with
                                                       ``do_rmi=False``)

with ``bce`` the sigmoid cross-entropy of the valid pixels over ``n_valid + 1`` and ``rmi`` the lower bound of the region mutual
information: pooled one-hot and probability maps, their ``radius^2`` shifted slices as points of dimension ``radius^2``, the
covariance matrices of those points per (image, class), and ``0.5 logdet(la_cov - la_pr_cov inv(pr_cov) la_pr_cov^T)``.

With ``backend='hip'`` (the default) fp32 CUDA logits with ``rmi_radius=3`` and average pooling of 1..8 take the fused route:
``cerberus::rmi_moments`` (``csrc/rmi_loss.hip``) reads the logits once and returns ``bce`` and the three (N,C,9,9) float64
matrices; the 9 x 9 algebra runs in ``torch`` float64 ops on those; one backward launch writes the logits' gradient.  No
one-hot tensor, no permuted logits, no (N,C,9,P) float64 stacks.  Every other setting -- other radii, max pooling,
interpolation, 16-bit or CPU tensors, a pooled map smaller than the radius -- takes ``backend='torch'``, the reference's
operation order with ``.double()`` in place of its CUDA-only tensor type, so that it runs on any device.

Differences from the reference:
 * a label is valid if ``0 <= label < num_classes``; the reference tests only ``label < num_classes`` and fails inside
   ``one_hot`` on a negative one.  Negative labels are ignored here, on both backends (a superset);
 * the fused route inverts and factorises with ``torch.linalg.inv_ex`` / ``cholesky_ex`` and does not look at their error flags
   (that would copy them to the host; the loss ops of this package never synchronise): a matrix that is not positive definite
   gives NaN where the reference raises.
"""
from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops as _ops

__all__ = ["rmi_loss", "RMILoss", "RMILossAux", "MultiScaleRMILoss"]

_CLIP_MIN = 1e-6     # added to the probabilities after the mask
_POS_ALPHA = 5e-4    # added to the diagonals to keep the matrices positive definite


def _fusable(logits, target, radius, pool_way, pool):
    """What cerberus::rmi_moments takes (see the module docstring)."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4 and logits.shape[0] > 0):
        return False
    if not (target.dtype == torch.int64 and target.device == logits.device
            and tuple(target.shape) == (logits.shape[0],) + tuple(logits.shape[2:])):
        return False
    return pool_way == 1 and logits.shape[0] <= 65535 and _ops.rmi_fused_shape_ok(*logits.shape[1:], radius, pool)


def _log_det_by_cholesky(matrix, checked):
    chol = torch.linalg.cholesky(matrix) if checked else torch.linalg.cholesky_ex(matrix, check_errors=False)[0]
    return 2.0 * torch.sum(torch.log(torch.diagonal(chol, dim1=-2, dim2=-1) + 1e-8), dim=-1)


def _rmi_from_cov(la_cov, pr_cov, la_pr_cov, num_classes, half_d, checked):
    """rmi.py:168-206 from the three covariance matrices (float64, (N,C,d,d))."""
    diag_matrix = torch.eye(half_d, dtype=pr_cov.dtype, device=pr_cov.device).unsqueeze(dim=0).unsqueeze(dim=0)
    if checked:
        pr_cov_inv = torch.inverse(pr_cov + diag_matrix * _POS_ALPHA)
    else:
        pr_cov_inv = torch.linalg.inv_ex(pr_cov + diag_matrix * _POS_ALPHA, check_errors=False)[0]
    appro_var = la_cov - torch.matmul(la_pr_cov.matmul(pr_cov_inv), la_pr_cov.transpose(-2, -1))
    rmi_now = 0.5 * _log_det_by_cholesky(appro_var + diag_matrix * _POS_ALPHA, checked)
    rmi_per_class = rmi_now.view([-1, num_classes]).mean(dim=0).float()
    rmi_per_class = torch.div(rmi_per_class, float(half_d))
    return torch.sum(rmi_per_class)


def _combine(bce_loss, rmi, weight_lambda, lambda_way):
    if lambda_way:
        return weight_lambda * bce_loss + rmi * (1 - weight_lambda)
    return bce_loss + rmi * weight_lambda


def _rmi_loss_stock(logits_4D, labels_4D, num_classes, rmi_radius, rmi_pool_way, rmi_pool_size, rmi_pool_stride, weight_lambda,
                    lambda_way, do_rmi):
    """The reference's chain (rmi.py:72-207) in its own operation order."""
    label_mask_3d = (labels_4D < num_classes) & (labels_4D >= 0)
    valid_onehot_labels_4d = F.one_hot(labels_4D.long() * label_mask_3d.long(), num_classes=num_classes).float()
    label_mask_3d = label_mask_3d.float()
    label_mask_flat = label_mask_3d.view([-1, ])
    valid_onehot_labels_4d = valid_onehot_labels_4d * label_mask_3d.unsqueeze(dim=3)

    # the sigmoid binary cross entropy of the valid pixels
    valid_onehot_label_flat = valid_onehot_labels_4d.view([-1, num_classes])
    logits_flat = logits_4D.permute(0, 2, 3, 1).contiguous().view([-1, num_classes])
    valid_pixels = torch.sum(label_mask_flat)
    binary_loss = F.binary_cross_entropy_with_logits(logits_flat, target=valid_onehot_label_flat,
                                                     weight=label_mask_flat.unsqueeze(dim=1), reduction='sum')
    bce_loss = torch.div(binary_loss, valid_pixels + 1.0)
    if not do_rmi:
        return bce_loss

    probs_4D = logits_4D.sigmoid() * label_mask_3d.unsqueeze(dim=1) + _CLIP_MIN
    labels_4D = valid_onehot_labels_4d.permute(0, 3, 1, 2)
    p, s, half_d = rmi_pool_size, rmi_pool_stride, rmi_radius * rmi_radius
    if s > 1:
        if rmi_pool_way == 0:
            labels_4D = F.max_pool2d(labels_4D, kernel_size=p, stride=s, padding=p // 2)
            probs_4D = F.max_pool2d(probs_4D, kernel_size=p, stride=s, padding=p // 2)
        elif rmi_pool_way == 1:
            labels_4D = F.avg_pool2d(labels_4D, kernel_size=p, stride=s, padding=p // 2)
            probs_4D = F.avg_pool2d(probs_4D, kernel_size=p, stride=s, padding=p // 2)
        elif rmi_pool_way == 2:
            shape = labels_4D.size()
            new_h, new_w = shape[2] // s, shape[3] // s
            labels_4D = F.interpolate(labels_4D, size=(new_h, new_w), mode='nearest')
            probs_4D = F.interpolate(probs_4D, size=(new_h, new_w), mode='bilinear', align_corners=True)
        else:
            raise NotImplementedError("Pool way of RMI is not defined!")
    n, c, h, w = labels_4D.size()
    new_h, new_w = h - (rmi_radius - 1), w - (rmi_radius - 1)
    la_ns, pr_ns = [], []
    for y in range(0, rmi_radius, 1):
        for x in range(0, rmi_radius, 1):
            la_ns.append(labels_4D[:, :, y:y + new_h, x:x + new_w])
            pr_ns.append(probs_4D[:, :, y:y + new_h, x:x + new_w])
    la_vectors = torch.stack(la_ns, dim=2).view([n, c, half_d, -1]).double()
    pr_vectors = torch.stack(pr_ns, dim=2).view([n, c, half_d, -1]).double()

    la_vectors = la_vectors - la_vectors.mean(dim=3, keepdim=True)
    la_cov = torch.matmul(la_vectors, la_vectors.transpose(2, 3))
    pr_vectors = pr_vectors - pr_vectors.mean(dim=3, keepdim=True)
    pr_cov = torch.matmul(pr_vectors, pr_vectors.transpose(2, 3))
    la_pr_cov = torch.matmul(la_vectors, pr_vectors.transpose(2, 3))
    rmi = _rmi_from_cov(la_cov, pr_cov, la_pr_cov, num_classes, half_d, checked=True)
    return _combine(bce_loss, rmi, weight_lambda, lambda_way)


def rmi_loss(logits, target, num_classes=21, rmi_radius=3, rmi_pool_way=1, rmi_pool_size=4, rmi_pool_stride=4,
             loss_weight_lambda=0.5, lambda_way=1, do_rmi=True, backend="hip"):
    """``RMILoss.forward`` as a function: ``logits`` (N,C,H,W) with ``C == num_classes``, ``target`` (N,H,W) or (N,1,H,W),
    returns a 0-dim fp32 tensor.  As the reference, the logits are taken to fp32 and autocast is off inside."""
    if backend not in ("hip", "torch"):
        raise ValueError("backend must be 'hip' or 'torch'")
    if len(target.shape) == 4:
        target = target.squeeze(1)
    fused = (backend == "hip" and rmi_pool_size == rmi_pool_stride and logits.shape[1] == num_classes
             and _fusable(logits, target, rmi_radius, rmi_pool_way, rmi_pool_size))
    with torch.autocast(device_type=logits.device.type, enabled=False):
        if not fused:
            return _rmi_loss_stock(logits.float(), target.long(), num_classes, rmi_radius, rmi_pool_way, rmi_pool_size,
                                   rmi_pool_stride, loss_weight_lambda, lambda_way, do_rmi)
        bce, la_cov, pr_cov, la_pr_cov = torch.ops.cerberus.rmi_moments(logits, target, rmi_radius, rmi_pool_size, bool(do_rmi))[:4]
        if not do_rmi:
            return bce
        rmi = _rmi_from_cov(la_cov, pr_cov, la_pr_cov, num_classes, rmi_radius * rmi_radius, checked=False)
        return _combine(bce, rmi, loss_weight_lambda, lambda_way)


class RMILoss(nn.Module):
    """Region mutual information loss, I(A, B) = H(A) + H(B) - H(A, B) (reference :33-207).

    ``backend='hip'`` (default): the fused HIP route where it applies (module docstring), the stock ops elsewhere.
    ``backend='torch'``: the stock-op formulation in the reference's operation order."""

    def __init__(self, num_classes=21, rmi_radius=3, rmi_pool_way=1, rmi_pool_size=4,
                 rmi_pool_stride=4, loss_weight_lambda=0.5, lambda_way=1, ignore_index=255, backend="hip"):
        super().__init__()
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        self.num_classes = num_classes
        assert rmi_radius in [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
        self.rmi_radius = rmi_radius
        assert rmi_pool_way in [0, 1, 2, 3]
        self.rmi_pool_way = rmi_pool_way

        assert rmi_pool_size == rmi_pool_stride
        self.rmi_pool_size = rmi_pool_size
        self.rmi_pool_stride = rmi_pool_stride
        self.weight_lambda = loss_weight_lambda
        self.lambda_way = lambda_way

        self.half_d = self.rmi_radius * self.rmi_radius
        self.d = 2 * self.half_d
        self.kernel_padding = self.rmi_pool_size // 2
        self.ignore_index = ignore_index      # kept for the signature: as in the reference, every label >= num_classes is ignored
        self.backend = backend

    def forward(self, logits_4D: torch.FloatTensor, labels_4D: torch.LongTensor, do_rmi=True) -> torch.Tensor:
        return rmi_loss(logits_4D, labels_4D, self.num_classes, self.rmi_radius, self.rmi_pool_way, self.rmi_pool_size,
                        self.rmi_pool_stride, self.weight_lambda, self.lambda_way, do_rmi, self.backend)


class MultiScaleRMILoss(nn.Module):
    """RMI on the main prediction, BCE (or RMI with ``ocr_aux_rmi``) on the OCR auxiliary head (reference :209-239)."""

    def __init__(self, ocr_aux_rmi=False, supervised_mscale_wt=0.0, alpha=0.4, **kwargs):
        super().__init__()
        self.alpha = alpha
        self.ocr_aux_rmi = ocr_aux_rmi
        self.supervised_mscale_wt = supervised_mscale_wt
        self.rmi = RMILoss(**kwargs)

    def forward(self, seg_pred: Dict[str, torch.Tensor], seg_gt: torch.Tensor, **kwargs):
        aux_loss = self.rmi(seg_pred['aux'], seg_gt, do_rmi=self.ocr_aux_rmi)
        main_loss = self.rmi(seg_pred['pred'], seg_gt, do_rmi=True)
        loss = self.alpha * aux_loss + main_loss

        if self.supervised_mscale_wt:
            # the reference passes a slice of the tensor itself as the size (:229-231), which cannot run; its shape is meant
            scaled_pred_05x = F.interpolate(seg_pred['pred_05x'], size=tuple(seg_pred['pred_10x'].shape[2:]), mode='bilinear',
                                            align_corners=True)
            loss_lo = self.rmi(scaled_pred_05x, seg_gt, do_rmi=False)
            loss_hi = self.rmi(seg_pred['pred_10x'], seg_gt, do_rmi=False)
            loss = loss + self.supervised_mscale_wt * loss_lo
            loss = loss + self.supervised_mscale_wt * loss_hi
        return loss


class RMILossAux(nn.Module):
    """``weight * (rmi(seg) + aux_weight * rmi(seg_aux))`` (reference :241-258)."""

    def __init__(self, weight=1., aux_weight=0.4, **kwargs):
        super().__init__()
        self.rmi = RMILoss(**kwargs)
        self.aux_weight = aux_weight
        self.weight = weight

    def forward(self, predictions: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor]) -> torch.Tensor:
        assert all('seg' in dict_ for dict_ in [predictions.keys(), targets.keys()])
        seg_gt = targets['seg']
        seg_loss = self.rmi(predictions['seg'], seg_gt)
        if 'seg_aux' in predictions.keys():
            seg_loss = seg_loss + (self.aux_weight * self.rmi(predictions['seg_aux'], seg_gt))
        return self.weight * seg_loss
