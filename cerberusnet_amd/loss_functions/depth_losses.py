"""Drop-in for the stereo reconstruction loss of ``nnet_training/loss_functions/depth_losses.py`` (:112-206).

``BackprojectDepth``, ``Project3D`` and ``DepthReconstructionLossV1`` keep their names, constructor signatures and
``forward`` arguments.  The three are restated here in stock ops that follow their tensors' device and dtype (no ``.cuda()``
calls); with ``backend='hip'`` (default) the chain back-project -> project -> normalise -> ``grid_sample`` runs as ONE HIP
launch (``cerberus::reproject_warp``, ``csrc/reproject.hip``) with a one-launch gather backward to the depth, followed by
``photometric_loss`` -- the loss is ``photometric_loss(r_img, warp(l_img), 0.15, 0.85)``.

The sampling rule is ``flow_warp``'s: positions are normalised by (W-1), (H-1) and sampled with ``align_corners=False``
(quirk Q2), bilinear, border padding.
"""
import torch
import torch.nn.functional as F

from .UnFlowLoss import _ssim_distance, photometric_loss

__all__ = ["BackprojectDepth", "Project3D", "DepthReconstructionLossV1", "reproject_warp"]


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
