"""Drop-in for the stereo reconstruction loss of ``nnet_training/loss_functions/depth_losses.py`` (:112-206).

``BackprojectDepth``, ``Project3D`` and ``DepthReconstructionLossV1`` keep their names, constructor signatures and
``forward`` arguments.  The three are restated here in stock ops that follow their tensors' device and dtype (no ``.cuda()``
calls); with ``backend='hip'`` (default) the chain back-project -> project -> normalise -> ``grid_sample`` runs as ONE HIP
launch (``cerberus::reproject_warp``, ``csrc/reproject.hip``) with a one-launch gather backward to the depth, followed by
``photometric_loss`` -- the loss is ``photometric_loss(r_img, warp(l_img), 0.15, 0.85)``.

The sampling rule is ``flow_warp``'s: positions are normalised by (W-1), (H-1) and sampled with ``align_corners=False``
(quirk Q2), bilinear, border padding.

The supervised losses of the same file (:16-110) keep their names, constructor signatures and ``forward(predictions,
targets)`` with the keys ``'depth'`` and ``'disparity'``.  ``InvHuberLoss`` (the one a reference config trains with) and
``InvHuberLossPyr`` have a fused HIP path (``cerberus::inv_huber``, ``csrc/depth_loss.hip``: two passes and a finish forward,
one launch backward, the gradient through the data-dependent cutoff included); ``ScaleInvariantError`` and ``DepthAwareLoss``
are restated in stock ops so that they can be differentiated at all (the reference's in-place ``+= 0.001`` makes its
backward raise).
"""
import torch
import torch.nn.functional as F

from .UnFlowLoss import _ssim_distance, photometric_loss

__all__ = ["BackprojectDepth", "Project3D", "DepthReconstructionLossV1", "reproject_warp",
           "inv_huber_loss", "InvHuberLoss", "InvHuberLossPyr", "ScaleInvariantError", "DepthAwareLoss"]


class BackprojectDepth(torch.nn.Module):
    """Depth image -> homogeneous point cloud (B,4,H*W) in the camera frame (reference :112-141)."""

    def __init__(self, batch_size, height, width):
        super().__init__()
        self.batch_size, self.height, self.width = batch_size, height, width
        ys, xs = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32), indexing="ij")
        # (1,3,N): x, y, 1 of every pixel, row-major; broadcast over the batch
        self.register_buffer("pix_coords", torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(height * width)], 0).unsqueeze(0),
                             persistent=False)

    def forward(self, depth, inv_K):
        batch = depth.shape[0]
        pix = self.pix_coords.to(device=depth.device, dtype=depth.dtype)
        cam_points = torch.matmul(inv_K[:, :3, :3].to(device=depth.device, dtype=depth.dtype), pix)
        cam_points = depth.reshape(batch, 1, -1) * cam_points
        return torch.cat([cam_points, pix[:, 2:].expand(batch, 1, -1)], 1)


class Project3D(torch.nn.Module):
    """Points (B,4,N) -> sample positions (B,H,W,2) of a camera with intrinsics K at pose T, normalised by (W-1), (H-1)
    (reference :143-165)."""

    def __init__(self, batch_size, height, width, eps=1e-7):
        super().__init__()
        self.batch_size, self.height, self.width, self.eps = batch_size, height, width, eps

    def forward(self, points, K, T):
        P = torch.matmul(K.to(points), T.to(points))[:, :3, :]
        cam_points = torch.matmul(P, points)
        pix_coords = cam_points[:, :2, :] / (cam_points[:, 2, :].unsqueeze(1) + self.eps)
        pix_coords = pix_coords.view(points.shape[0], 2, self.height, self.width).permute(0, 2, 3, 1)
        pix_coords = torch.stack([pix_coords[..., 0] / (self.width - 1), pix_coords[..., 1] / (self.height - 1)], -1)
        return (pix_coords - 0.5) * 2


def _depth4(image, depth):
    return depth.reshape(image.shape[0], 1, image.shape[2], image.shape[3])


def _reproject_stock(image, depth, inv_K, K, T, eps):
    b, _, h, w = image.shape
    points = BackprojectDepth(b, h, w)(_depth4(image, depth), inv_K)
    grid = Project3D(b, h, w, eps)(points, K, T)
    return F.grid_sample(image, grid, padding_mode="border", align_corners=False)


def _fusable(image, depth, mats):
    """What cerberus::reproject_warp takes: fp32 tensors on one GPU, H, W >= 2, a gradient wanted by the depth alone."""
    tensors = (image, depth) + tuple(mats)
    if not all(t.is_cuda and t.device == image.device and t.dtype == torch.float32 for t in tensors):
        return False
    if image.dim() != 4 or image.numel() == 0 or min(image.shape[2:]) < 2 or depth.numel() != image.numel() // image.shape[1]:
        return False
    return not (torch.is_grad_enabled() and (image.requires_grad or any(m.requires_grad for m in mats)))


def reproject_warp(image, depth, inv_K, K, T, eps=1e-7):
    """The image seen from the other camera of a rig: pixel (x, y) with depth d is back-projected with ``inv_K``, moved by
    ``T``, projected with ``K`` and the image sampled there (bilinear, border padding, the rule of ``flow_warp``).
    ``image`` (B,C,H,W), ``depth`` (B,1,H,W), ``inv_K`` / ``K`` / ``T`` (B,4,4).  fp32 CUDA tensors take ONE HIP launch
    (``cerberus::reproject_warp``) and a one-launch gather backward to the depth; an image or a matrix that requires grad,
    16-bit, 64-bit or CPU tensors take the stock-op formulation."""
    if _fusable(image, depth, (inv_K, K, T)):
        proj = torch.matmul(K, T)[:, :3, :].contiguous()
        return torch.ops.cerberus.reproject_warp(image, _depth4(image, depth), inv_K[:, :3, :3].contiguous(), proj, float(eps))
    return _reproject_stock(image, depth, inv_K, K, T, eps)


class DepthReconstructionLossV1(torch.nn.Module):
    """Photometric stereo loss of the depth head: ``l_img`` warped into the right camera by the predicted depth against
    ``r_img``, 0.15 L1 + 0.85 SSIM distance (L1 alone with ``ssim=False``) (reference :167-206).

    ``backend='hip'`` (default): ``reproject_warp`` + ``photometric_loss``, the HIP ops for fp32 CUDA tensors whose image
    needs no gradient.  ``backend='torch'``: the stock-op formulation in the reference's operation order."""

    def __init__(self, batch_size, height, width, pred_type="disparity", ssim=True, backend="hip"):
        super().__init__()
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        self.pred_type = pred_type
        self.backend = backend
        self.use_ssim = bool(ssim)
        self.back_proj_depth = BackprojectDepth(batch_size, height, width)
        self.project_3d = Project3D(batch_size, height, width)

    @staticmethod
    def depth_from_disparity(disparity):
        return (0.209313 * 2262.52) / ((disparity - 1) / 256)

    def forward(self, predictions, targets):
        assert all(key in targets.keys() for key in ['camera', 'l_img', 'r_img'])
        if self.pred_type == "depth":
            depth = predictions['depth']
        elif self.pred_type == "disparity":
            depth = self.depth_from_disparity(predictions['depth'])
        else:
            raise NotImplementedError(self.pred_type)
        camera, l_img, r_img = targets['camera'], targets['l_img'], targets['r_img']
        inv_K, K, T = (camera[k].to(device=depth.device, dtype=depth.dtype) for k in ("inv_K", "K", "baseline_T"))

        if self.backend == "hip":
            source_img = reproject_warp(l_img, depth, inv_K, K, T, self.project_3d.eps)
            weights = (0.15, 0.85) if self.use_ssim else (1.0, 0.0)
            return photometric_loss(r_img, source_img, *weights)

        cam_points = self.back_proj_depth(depth, inv_K)
        pix_coords = self.project_3d(cam_points, K, T)
        source_img = F.grid_sample(l_img, pix_coords, padding_mode="border", align_corners=False)
        abs_diff = (r_img - source_img).abs()
        if self.use_ssim:
            loss = 0.15 * abs_diff.mean(1, True) + 0.85 * _ssim_distance(source_img, r_img).mean(1, True)
        else:
            loss = abs_diff.mean(1, True)
        return loss.mean()


# ---- the supervised depth losses (reference :16-110) --------------------------------------------------------------------
def _map3(t, name):
    """A (B,1,h,w) map as (B,h,w); a (B,h,w) one as it is."""
    if t.dim() == 4 and t.shape[1] == 1:
        return t.squeeze(1)
    if t.dim() == 3:
        return t
    raise ValueError(f"Invalid {name} shape {tuple(t.shape)}: (B,1,h,w) or (B,h,w)")


def _nearest(gt, size):
    return F.interpolate(gt.unsqueeze(1), tuple(size), mode="nearest").squeeze(1)


def _inv_huber_stock(pred, gt):
    """The reference's ``InvHuberLoss.forward`` (:78-87) without ``weight``, in its operation order; ``pred`` and ``gt`` (B,h,w)."""
    pred_relu = F.relu(pred)
    diff = pred_relu - gt
    mask = gt > 0
    err = (diff * mask.float()).abs()
    c = 0.2 * err.max()
    err2 = (diff**2 + c**2) / (2. * c)
    mask_err = err <= c
    mask_err2 = err > c
    return (err * mask_err.float() + err2 * mask_err2.float()).mean()


def _inv_huber_fusable(pred, gt):
    """What cerberus::inv_huber takes: fp32 tensors on one GPU, at least a pixel, a ground truth that wants no gradient."""
    if not (pred.is_cuda and gt.device == pred.device and pred.dtype == torch.float32 and gt.dtype == torch.float32):
        return False
    if pred.numel() == 0 or gt.numel() == 0 or pred.shape[0] != gt.shape[0]:
        return False
    return not (torch.is_grad_enabled() and gt.requires_grad)


def inv_huber_loss(pred, gt):
    """The inverse Huber (berHu) loss of ``InvHuberLoss`` (reference :64-88) as a 0-dim tensor.  ``pred`` (B,1,h,w) or
    (B,h,w), ``gt`` (B,H,W) (or (B,1,H,W)); a ground truth of another size is compared as
    ``F.interpolate(gt, (h, w), mode='nearest')``.  With ``d = relu(pred) - gt`` and ``err = |d|`` where ``gt > 0``, else 0::

        c = 0.2 * err.max();   loss = mean(err if err <= c else (d*d + c*c) / (2*c))     over ALL pixels

    The cutoff ``c`` depends on the data and carries a gradient, into the pixel(s) that hold the maximum.

    fp32 CUDA tensors on one device take ONE fused HIP forward and one fused backward (``cerberus::inv_huber``,
    ``csrc/depth_loss.hip``); for integer ratios H / h and W / w the kernels read ``gt[b, y*(H/h), x*(W/w)]`` themselves, for
    any other ratio the ground truth is resized first.  16-bit, 64-bit and CPU tensors, and a ``gt`` that requires grad, take
    the reference's chain of stock ops.

    The fused op differs from the reference where the reference fails: pixels with ``gt <= 0`` (or NaN) are skipped by
    selection, so a NaN or an infinity predicted there changes nothing (the reference multiplies by the mask and returns
    NaN); and ``c == 0`` (no valid pixel, or every valid pixel exact) gives 0 with a zero gradient, the limit of the formula,
    where the reference divides by ``2*c`` and returns NaN."""
    pred, gt = _map3(pred, "prediction"), _map3(gt, "ground truth")
    h, w = pred.shape[1:]
    H, W = gt.shape[1:]
    fused = _inv_huber_fusable(pred, gt)
    if (H, W) != (h, w) and not (fused and H % h == 0 and W % w == 0):
        gt = _nearest(gt, (h, w))
    if fused:
        return torch.ops.cerberus.inv_huber(pred, gt)[0]
    return _inv_huber_stock(pred, gt)


def _depth_pair(predictions, targets):
    assert 'depth' in predictions.keys() and 'disparity' in targets.keys()
    return predictions['depth'], targets['disparity']


def _check_backend(backend):
    if backend not in ("hip", "torch"):
        raise ValueError("backend must be 'hip' or 'torch'")
    return backend


class InvHuberLoss(torch.nn.Module):
    """Inverse Huber (berHu) loss for depth / disparity training (reference :64-88): ``weight * inv_huber_loss(
    predictions['depth'], targets['disparity'])``.

    ``backend='hip'`` (default): the fused HIP op for fp32 CUDA tensors (see ``inv_huber_loss``, also for the two corners
    where it returns a number and the reference NaN).  ``backend='torch'``: the stock-op formulation in the reference's
    operation order."""

    def __init__(self, weight=1.0, backend="hip", **kwargs):
        super().__init__()
        self.weight = weight
        self.backend = _check_backend(backend)

    def forward(self, predictions, targets):
        disp_pred, disp_gt = _depth_pair(predictions, targets)
        if self.backend == "hip":
            return self.weight * inv_huber_loss(disp_pred, disp_gt)
        return self.weight * _inv_huber_stock(disp_pred.squeeze(dim=1), disp_gt)


class InvHuberLossPyr(torch.nn.Module):
    """``weight * sum_l lvl_weights[l] * inv_huber_loss(level_l, gt)`` over a list ``predictions['depth']`` of (B,1,h_l,w_l)
    levels, the ground truth ``targets['disparity']`` (B,H,W) nearest-resized to each level.

    This is the evident intent of the reference's class (:90-110), whose own ``forward`` cannot run: it passes tensors to a
    ``forward`` that asserts on dict keys, and subtracts a (B,1,h,w) map from a (B,h,w) one.  With ``backend='hip'`` (default)
    a level whose size divides the ground truth's needs no resized map: the kernels gather.  ``backend='torch'``: the stock
    chain on the resized ground truth."""

    def __init__(self, lvl_weights, weight=1.0, backend="hip", **kwargs):
        super().__init__()
        self.lvl_weights = lvl_weights
        self.weight = weight
        self.backend = _check_backend(backend)

    def forward(self, predictions, targets):
        disp_pred, disp_gt = _depth_pair(predictions, targets)
        loss = 0
        for lvl, pred in enumerate(disp_pred):
            if self.backend == "hip":
                lvl_loss = inv_huber_loss(pred, disp_gt)
            else:
                lvl_loss = _inv_huber_stock(pred.squeeze(dim=1), _nearest(disp_gt, pred.size()[2:]))
            loss = loss + lvl_loss * self.lvl_weights[lvl]
        return self.weight * loss


def _positive_prediction(disp_pred):
    """The reference's ``relu`` and ``disp_pred[disp_pred == 0] += 0.001`` (:27-28, :54-55) out of place: the in-place form on
    the output of relu makes the reference's backward raise."""
    disp_pred = F.relu(disp_pred.squeeze(dim=1))
    return torch.where(disp_pred > 0, disp_pred, 0.001)


class ScaleInvariantError(torch.nn.Module):
    """Scale-invariant log error over the pixels with ``gt > 0`` (reference :42-62), in stock ops.

    A restatement that can be trained with: the reference's in-place ``+= 0.001`` makes its backward raise, and its
    boolean-mask indexing synchronises with the host.  Here the mask is applied with ``torch.where`` and a valid count: the
    same forward value, differentiable, capturable.  Not on the HIP path: no reference config trains with it."""

    def __init__(self, weight=1.0, lmda=1, **kwargs):
        super().__init__()
        self.lmda = lmda
        self.weight = weight

    def forward(self, predictions, targets):
        disp_pred, disp_gt = _depth_pair(predictions, targets)
        disp_pred = _positive_prediction(disp_pred)
        mask = disp_gt > 0
        count = mask.sum()
        log_diff = torch.where(mask, torch.log(disp_pred) - torch.log(torch.where(mask, disp_gt, 1.0)), 0.0)
        element_wise = torch.pow(log_diff, 2).sum() / count
        scaled_error = self.lmda * (log_diff.sum()**2) / (count**2)
        return self.weight * (element_wise - scaled_error)


class DepthAwareLoss(torch.nn.Module):
    """Depth-aware smooth-L1 loss over the pixels with ``gt > 0`` (reference :16-40), in stock ops.

    A restatement that can be trained with, as ``ScaleInvariantError``: the ``+ 0.001`` out of place, ``torch.where`` and a
    valid count instead of boolean-mask indexing.  Not on the HIP path: no reference config trains with it."""

    def __init__(self, weight=1.0, **kwargs):
        super().__init__()
        self.weight = weight

    def forward(self, predictions, targets):
        disp_pred, disp_gt = _depth_pair(predictions, targets)
        disp_pred = _positive_prediction(disp_pred)
        mask = disp_gt > 0
        count = mask.sum()
        safe_gt = torch.where(mask, disp_gt, 2.0)      # log(2) != 0: no 0 / 0 in the ratio below, whose backward would give NaN
        l_disp_pred = torch.log(disp_pred)
        l_disp_gt = torch.log(safe_gt)
        regularization = 1 - torch.min(l_disp_pred, l_disp_gt) / torch.max(l_disp_pred, l_disp_gt)
        l_loss = torch.where(mask, F.smooth_l1_loss(disp_pred, safe_gt, reduction='none'), 0.0).sum() / count
        depth_aware_attention = disp_gt / torch.where(mask, disp_gt, -float("inf")).max()
        return self.weight * torch.where(mask, (depth_aware_attention + regularization) * l_loss, 0.0).sum() / count
