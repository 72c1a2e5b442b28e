"""Drop-in for the flow-warp part of ``nnet_training/loss_functions/UnFlowLoss.py``.

``flow_warp(image, flow12, pad='border', mode='bilinear')`` (reference :83-94)
keeps its name, signature, defaults and semantics -- including quirk Q2 (the
grid is normalised by (W-1),(H-1) but sampled with align_corners=False, so zero
flow is not the identity) -- but runs as ONE fused HIP kernel per direction
(``cerberus::flow_warp``): no CPU-built mesh, no H2D copy, no grid tensor.
Gradients flow to both the image and the flow.

``mesh_grid`` / ``norm_grid`` (:11-32) are kept for importers; they are not on
the hot path any more.

The occlusion handling of the reference -- ``get_corresponding_map`` (:34-81), ``get_occu_mask_backward`` (:108-117),
``get_occu_mask_bidirection`` (:96-106), the masked ``loss_photometric`` (:225-241) and the mask schedule of ``forward``
(:286-295) -- is here under the same names: fp32 CUDA tensors take the HIP ops of ``csrc/occlusion.hip`` (a bit-reproducible
splat, a one-launch bidirectional check), everything else a stock-op formulation; ``unFlowLoss(occlusion=True)`` switches
the schedule on.
"""
import torch

from .. import ops as _ops

__all__ = ["flow_warp", "mesh_grid", "norm_grid", "area_resize", "area_pyramid", "photometric_loss", "edge_smoothness",
           "TernaryLoss", "census_loss", "get_corresponding_map", "get_occu_mask_backward", "get_occu_mask_bidirection",
           "unFlowLoss"]


def area_resize(image, size):
    """``F.interpolate(image, size, mode='area')`` as one HIP launch: how the photometric loss
    brings the target images to every flow scale (reference :279-280).  Forward only."""
    return torch.ops.cerberus.area_resize(image, int(size[0]), int(size[1]))


def area_pyramid(image, sizes):
    """``[F.interpolate(image, size, mode='area') for size in sizes]`` with ONE pass over the image for all
    integer-ratio scales; a scale of the image's own size is the image itself (reference :279-280, per scale)."""
    flat = [int(v) for size in sizes for v in size]
    return list(torch.ops.cerberus.area_pyramid(image, flat))


def mesh_grid(batch_sz, height, width, device=None):
    """Pixel-coordinate grid, (B,2,H,W), channel 0 = x, channel 1 = y (``device``: where to build it; default CPU)."""
    xs = torch.arange(0, width, device=device).view(1, 1, width).expand(batch_sz, height, width)
    ys = torch.arange(0, height, device=device).view(1, height, 1).expand(batch_sz, height, width)
    return torch.stack([xs, ys], 1)


def norm_grid(v_grid):
    """Scale pixel coordinates to [-1, 1] by (W-1), (H-1); returns (B,H,W,2)."""
    _, _, height, width = v_grid.size()
    v_grid_norm = torch.zeros_like(v_grid)
    v_grid_norm[:, 0, :, :] = 2.0 * v_grid[:, 0, :, :] / (width - 1) - 1.0
    v_grid_norm[:, 1, :, :] = 2.0 * v_grid[:, 1, :, :] / (height - 1) - 1.0
    return v_grid_norm.permute(0, 2, 3, 1)


def flow_warp(image, flow12, pad='border', mode='bilinear'):
    '''
    Warps an image given a flow prediction (fused HIP grid_sample)
    '''
    if pad not in _ops.PAD_MODES:
        raise ValueError("nn.functional.grid_sample(): expected padding_mode to be 'zeros', "
                         "'border', or 'reflection', but got: '%s'" % pad)
    if mode not in _ops.INTERP_MODES:
        raise ValueError("flow_warp: mode must be 'bilinear' or 'nearest', got '%s'" % mode)
    modes = (_ops.PAD_MODES[pad], _ops.INTERP_MODES[mode])
    if torch.is_grad_enabled() and image.requires_grad:
        # training: the forward also saves the sample positions for the backward (what
        # autograd's save_for_backward is to grid_sample in the reference)
        return torch.ops.cerberus.flow_warp_ctx(image, flow12, *modes)[0]
    # inference, and training warps of an image that carries no gradient (the photometric loss's target
    # images, :282-283): the positions are only needed by grad_image's tiles -- grad_flow recomputes them from
    # the flow -- so no context is written (2 floats per pixel at full resolution)
    return torch.ops.cerberus.flow_warp(image, flow12, *modes)


# ---- the photometric flow loss: a CALLER of the warp (host model of the hot path) ---------------
def _torch_flow_warp(image, flow12, pad="border", mode="bilinear"):
    """The reference op sequence (:83-94) in stock torch ops -- CPU wiring tests only."""
    import torch.nn.functional as F
    b, _, h, w = image.size()
    grid = norm_grid(mesh_grid(b, h, w).type_as(image) + flow12)
    return F.grid_sample(image, grid, mode=mode, padding_mode=pad, align_corners=False)


def _ssim_distance(x, y):
    """(1 - SSIM) / 2 on 3x3 windows with reflection padding, clamped to [0, 1]
    (``loss_functions.py:47-77``)."""
    import torch.nn.functional as F
    # the reference's op sequence: both images padded once, products of the padded images pooled (the same forward bits as
    # pooling padded products, and the reference's summation order in the backward as well)
    x, y = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    pool = lambda t: F.avg_pool2d(t, 3, 1)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mu_x, mu_y = pool(x), pool(y)
    var_x = pool(x ** 2) - mu_x ** 2
    var_y = pool(y ** 2) - mu_y ** 2
    cov = pool(x * y) - mu_x * mu_y
    num = (2 * mu_x * mu_y + c1) * (2 * cov + c2)
    den = (mu_x ** 2 + mu_y ** 2 + c1) * (var_x + var_y + c2)
    return torch.clamp((1 - num / den) / 2, 0, 1)


def TernaryLoss(im, im_warp, max_distance=1):
    """The census ("ternary") distance map of two RGB images, (B,1,H,W), zero within ``max_distance`` of the border
    (reference :119-156, same name, signature and return value) in stock ops: the soft ternary transform
    ``t = x / sqrt(0.81 + x^2)`` of every gray difference ``x`` inside a ``2 * max_distance + 1`` window, and the mean over
    the window of ``D / (0.1 + D)``, ``D = (t(im) - t(im_warp))^2``.  The formulation ``census_loss`` falls back to, the
    CPU path and the tests' yardstick."""
    import torch.nn.functional as F
    patch_size = 2 * max_distance + 1
    out_channels = patch_size * patch_size
    weights = torch.eye(out_channels).view((out_channels, 1, patch_size, patch_size)).type_as(im)

    def transform(image):
        gray = image[:, 0, :, :] * 0.2989 + image[:, 1, :, :] * 0.5870 + image[:, 2, :, :] * 0.1140
        intensities = gray.unsqueeze(1) * 255
        transf = F.conv2d(intensities, weights, padding=max_distance) - intensities
        return transf / torch.sqrt(0.81 + torch.pow(transf, 2))

    dist = torch.pow(transform(im) - transform(im_warp), 2)
    dist_mean = torch.mean(dist / (0.1 + dist), 1, keepdim=True)
    n, _, h, w = im.size()
    inner = torch.ones(n, 1, h - 2 * max_distance, w - 2 * max_distance).type_as(im)
    return dist_mean * F.pad(inner, [max_distance] * 4)


def _edge_aware_smoothness(flow, image, alpha, degree):
    """First / second order smoothness of the flow, damped across image edges (:162-187)."""
    dx = lambda t: t[:, :, :, 1:] - t[:, :, :, :-1]
    dy = lambda t: t[:, :, 1:] - t[:, :, :-1]
    wx = torch.exp(-dx(image).abs().mean(1, keepdim=True) * alpha)
    wy = torch.exp(-dy(image).abs().mean(1, keepdim=True) * alpha)
    if degree == 1:
        return ((wx * dx(flow).abs() / 2.).mean() + (wy * dy(flow).abs() / 2).mean()) / 2.
    if degree == 2:
        return ((wx[:, :, :, 1:] * dx(dx(flow)).abs()).mean() +
                (wy[:, :, 1:, :] * dy(dy(flow)).abs()).mean()) / 2.
    raise NotImplementedError(degree)


def _photometric_stock(im_orig, im_recons, l1_weight, ssim_weight):
    """The photometric term in stock ops (``loss_photometric`` below without a mask); a weight of None or 0 skips its term."""
    terms = []
    if l1_weight:
        terms.append(l1_weight * (im_orig - im_recons).abs())
    if ssim_weight:
        terms.append(ssim_weight * _ssim_distance(im_recons, im_orig))
    if not terms:
        return (im_recons * 0).sum()
    return sum(t.mean() for t in terms)


def _fusable(a, b):
    """What the scalar HIP ops take: fp32 NCHW tensors on one GPU."""
    return (a.is_cuda and b.is_cuda and a.device == b.device and a.dim() == 4 and b.dim() == 4
            and a.dtype == torch.float32 and b.dtype == torch.float32 and a.numel() > 0)


def photometric_loss(im_orig, im_recons, l1_weight=0.15, ssim_weight=0.85):
    """mean(l1_weight * |im_orig - im_recons| + ssim_weight * clamp((1 - SSIM(im_recons, im_orig)) / 2, 0, 1)) as a 0-dim
    tensor: ``unFlowLoss.loss_photometric`` (reference :225-241) without a mask as ONE fused HIP forward and one fused
    backward (``cerberus::photometric_loss``), differentiable in both images, reductions in a fixed order without
    atomics.  A weight of None or 0 skips its term.  fp32 CUDA tensors with H, W >= 2 take the HIP op; anything else
    (16-bit tensors, CPU tensors) the stock-op formulation.  An occlusion mask is applied by the caller:
    ``photometric_loss(im_orig * m, im_recons * m, ...) / m.mean()`` is the masked term for a 0 / 1 mask ``m``."""
    l1_weight, ssim_weight = float(l1_weight or 0.0), float(ssim_weight or 0.0)
    if (_fusable(im_orig, im_recons) and im_orig.shape == im_recons.shape and min(im_orig.shape[2:]) >= 2
            and (l1_weight or ssim_weight)):
        return torch.ops.cerberus.photometric_loss(im_orig, im_recons, l1_weight, ssim_weight)
    return _photometric_stock(im_orig, im_recons, l1_weight, ssim_weight)


def edge_smoothness(flow, image, alpha, degree):
    """``_edge_aware_smoothness`` (reference :162-187; degree 1 or 2) as one fused HIP forward and one gather backward
    (``cerberus::edge_smoothness``), differentiable in the flow.  An image that requires grad, 16-bit or CPU tensors and
    maps smaller than the degree needs take the stock-op formulation."""
    if degree not in (1, 2):
        raise NotImplementedError(degree)
    if (_fusable(flow, image) and flow.shape[0] == image.shape[0] and flow.shape[2:] == image.shape[2:]
            and min(flow.shape[2:]) > degree and not (torch.is_grad_enabled() and image.requires_grad)):
        return torch.ops.cerberus.edge_smoothness(flow, image, float(alpha), int(degree))
    return _edge_aware_smoothness(flow, image, alpha, degree)


def census_loss(im, im_warp, max_distance=1):
    """``TernaryLoss(im, im_warp, max_distance).mean()`` as a 0-dim tensor: the census term of ``loss_photometric``
    (reference :237-239; a mask multiplies both images before the call) as ONE fused HIP forward and one fused backward (``cerberus::census_loss``),
    differentiable in both images, reduced in a fixed order without atomics.  fp32 CUDA tensors of equal shape with 3
    channels, ``max_distance`` 1, 2 or 3 and H, W >= 2 * max_distance + 1 take the HIP op; anything else (16-bit or CPU
    tensors, other windows) the stock-op formulation."""
    if (_fusable(im, im_warp) and im.shape == im_warp.shape and im.shape[1] == 3
            and max_distance in _ops.CENSUS_MAX_DISTANCES and min(im.shape[2:]) >= 2 * max_distance + 1):
        return torch.ops.cerberus.census_loss(im, im_warp, int(max_distance))
    return TernaryLoss(im, im_warp, max_distance).mean()


# ---- occlusion masks (reference :34-81, :96-117) ---------------------------------------------------------------------
def _corresponding_map_stock(data):
    """``get_corresponding_map`` in stock ops, differentiable through the weights: every source pixel adds
    ``(1 - |x - xt|)(1 - |y - yt|)`` to the taps ``floor`` / ``floor + 1`` of its target ``(x, y)``; a tap outside the map is
    dropped, judged on the unclamped integer.  Taps are added in the reference's order (both ``+ 1``, then x ``+ 1``, then y
    ``+ 1``, then both ``floor``) by one ``scatter_add_``.  A non-finite target adds nothing."""
    B, _, H, W = data.shape
    x, y = data[:, 0].reshape(B, -1), data[:, 1].reshape(B, -1)
    x1, y1 = torch.floor(x), torch.floor(y)
    index, values = [], []
    for xt, yt in ((x1 + 1, y1 + 1), (x1 + 1, y1), (x1, y1 + 1), (x1, y1)):
        inside = (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)          # False for NaN and +-Inf
        weight = (1 - torch.abs(x - xt)) * (1 - torch.abs(y - yt))
        values.append(torch.where(inside, weight, torch.zeros_like(weight)))
        zero = torch.zeros_like(xt)
        index.append(torch.where(inside, xt, zero).long() + torch.where(inside, yt, zero).long() * W)
    out = torch.zeros(B, H * W, dtype=data.dtype, device=data.device)
    out = out.scatter_add(1, torch.cat(index, 1), torch.cat(values, 1))
    return out.view(B, 1, H, W)


def _flow_fusable(flow):
    """What the occlusion ops take: one fp32 (B,2,H,W) tensor on a GPU."""
    return _fusable(flow, flow) and flow.shape[1] == 2


def get_corresponding_map(data):
    """
    :param data: unnormalized coordinates Bx2xHxW
    :return: Bx1xHxW

    How many source pixels land on every pixel: the bilinear forward splat of ones (reference :34-81).  fp32 CUDA
    coordinates that carry no gradient take ``cerberus::corresponding_map`` (64-bit fixed-point sums: the same bits on
    every run); anything else -- CPU or 16-bit tensors, coordinates that require grad (the map is differentiable through
    its weights) -- the stock-op formulation."""
    if _flow_fusable(data) and not (torch.is_grad_enabled() and data.requires_grad):
        return torch.ops.cerberus.corresponding_map(data, False)
    return _corresponding_map_stock(data)


def _occu_mask_backward_stock(flow21, theta):
    B, _, H, W = flow21.shape
    base_grid = mesh_grid(B, H, W, device=flow21.device).type_as(flow21)
    corr_map = _corresponding_map_stock(base_grid + flow21)
    return (corr_map.clamp(min=0., max=1.) < theta).float()


def get_occu_mask_backward(flow21, theta=0.2):
    '''
    Get an occlusion mask using backward propagation: 1 where fewer than ``theta`` pixels of the other frame land
    (reference :108-117).  A constant: no gradient reaches the flow.  fp32 CUDA flows take ``cerberus::corresponding_map``
    (which forms pixel + flow itself) and one comparison; anything else the stock-op formulation.
    '''
    flow21 = flow21.detach()
    if _flow_fusable(flow21):
        corr_map = torch.ops.cerberus.corresponding_map(flow21, True)
        return (corr_map.clamp(min=0., max=1.) < theta).float()
    return _occu_mask_backward_stock(flow21, theta)


def _occu_mask_bidirection_stock(flow12, flow21, scale, bias):
    import torch.nn.functional as F
    b, _, h, w = flow12.shape
    grid = norm_grid(mesh_grid(b, h, w, device=flow12.device).type_as(flow12) + flow12)
    warped = F.grid_sample(flow21, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    diff = flow12 + warped
    mag = (flow12 * flow12).sum(1, keepdim=True) + (warped * warped).sum(1, keepdim=True)
    return ((diff * diff).sum(1, keepdim=True) > scale * mag + bias).float()


def get_occu_mask_bidirection(flow12, flow21, scale=0.01, bias=0.5):
    '''
    Get an occlusion mask using both flows such that they match each other: 1 where
    ``|flow12 + warp(flow21)|^2 > scale (|flow12|^2 + |warp(flow21)|^2) + bias`` (reference :96-106).  A constant: no
    gradient reaches either flow.  fp32 CUDA flows of equal shape take ``cerberus::occlusion_mask_bidirection`` (one
    launch, the warped flow is never written); anything else the stock-op formulation.
    '''
    flow12, flow21 = flow12.detach(), flow21.detach()
    if _flow_fusable(flow12) and _flow_fusable(flow21) and flow12.shape == flow21.shape and flow12.device == flow21.device:
        return torch.ops.cerberus.occlusion_mask_bidirection(flow12, flow21, float(scale), float(bias))
    return _occu_mask_bidirection_stock(flow12, flow21, scale, bias)


class unFlowLoss(torch.nn.Module):
    """Counterpart of ``unFlowLoss`` (:189-322) for the terms the Cerberus configs use: L1 and SSIM
    photometric terms on the image pair warped by the predicted flow at every pyramid scale,
    edge-aware smoothness, forward / backward consistency.  Same constructor keywords, same
    ``forward(predictions, targets)`` with ``predictions['flow'|'flow_b']`` (lists, full resolution
    first) and ``targets['l_img'|'l_seq']``.

    ``occlusion=True`` (opt-in) runs the mask schedule the reference carries commented out (:286-295): at the first used
    scale ``occlusion_masks(flow12, flow21)`` -- ``1 - get_occu_mask_backward`` of the opposite flow when
    ``back_occ_only`` else ``1 - get_occu_mask_bidirection``, argument order as upstream --, at every further used scale the
    previous scale's masks resized with ``nearest``; each photometric term is then the masked one of ``loss_photometric``.
    Masks are constants (no gradient flows through them); override ``occlusion_masks`` for masks of your own.  The default
    ``False`` builds no mask and keeps every result as it was.

    ``weights`` may carry ``"ternary"``, the census term (``TernaryLoss`` above, added to the photometric term as in the
    reference, :237-239), with ``fused=True`` (``census_loss``, the HIP op) or ``backend='torch'`` (stock ops).  With the
    defaults (``backend='hip'``, ``fused=False``) a ternary weight raises ``NotImplementedError``.

    ``backend='hip'`` (default): the two warps per scale are ``cerberus::flow_warp`` and the area
    resizes of the targets ``cerberus::area_resize``; ``'torch'``: stock ops, CPU tests only.

    ``fused=True`` (opt-in, ``backend='hip'`` only): what follows each warp -- the photometric term and the edge-aware
    smoothness -- runs as ``photometric_loss`` / ``edge_smoothness`` above (one HIP launch pair each instead of ~35 / ~15
    stock launches, reductions in a fixed order), per call where the op applies.  The default ``False`` keeps every
    result as it was."""

    def __init__(self, weight=1.0, weights=None, consistency=True, back_occ_only=False,
                 backend="hip", fused=False, occlusion=False, **kwargs):
        super().__init__()
        weights = weights or {"l1": 0.15, "ssim": 0.85}
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        if "ternary" in weights and not (fused or backend == "torch"):
            raise NotImplementedError("the census (ternary) term runs as the fused HIP op census_loss: pass fused=True "
                                      "(or backend='torch' for the stock-op formulation)")
        self.weight = weight
        self.l1_weight = weights.get("l1")
        self.ssim_weight = weights.get("ssim")
        self.ternary_weight = weights.get("ternary")
        self.smooth_args = kwargs.get("smooth", {"degree": 2, "alpha": 0.2, "weighting": 75.0})
        self.w_sm_scales = kwargs.get("w_sm_scales", [1.0, 0.0, 0.0, 0.0, 0.0])
        self.w_wrp_scales = kwargs.get("w_wrp_scales", [1.0, 1.0, 1.0, 1.0, 0.0])
        self.consistency = consistency
        self.back_occ_only = back_occ_only
        if fused and backend != "hip":
            raise ValueError("fused=True needs backend='hip' (the fused terms are HIP ops)")
        self.backend = backend
        self.fused = bool(fused)
        self.occlusion = bool(occlusion)

    def _fused(self):
        # `backend` may be reassigned on a live object: fused has no effect unless the backend is 'hip' at call time
        return self.fused and self.backend == "hip"

    def _pyramid(self, image, sizes):
        if self.backend == "hip":
            return area_pyramid(image, sizes)
        return [torch.nn.functional.interpolate(image, size, mode="area") for size in sizes]

    def _warp(self, image, flow):
        return flow_warp(image, flow, pad="border") if self.backend == "hip" \
            else _torch_flow_warp(image, flow, pad="border")

    def occlusion_masks(self, flow12, flow21):
        """The non-occluded masks ``(mask1, mask2)`` (1 = visible, (B,1,H,W)) of the two photometric terms, from the flows of
        the first used scale (reference :286-292).  ``backend='hip'``: the public functions above (HIP ops for fp32 CUDA
        flows); ``'torch'``: their stock formulations."""
        f12, f21 = flow12.detach(), flow21.detach()
        if self.backend == "hip":
            backward, bidirection = get_occu_mask_backward, get_occu_mask_bidirection
        else:
            backward = lambda f: _occu_mask_backward_stock(f, 0.2)
            bidirection = lambda a, b: _occu_mask_bidirection_stock(a, b, 0.01, 0.5)
        if self.back_occ_only:
            return 1 - backward(f21), 1 - backward(f12)
        return 1 - bidirection(f12, f21), 1 - bidirection(f21, f12)

    def _loss_photometric_masked(self, im_orig, im_recons, occu_mask):
        """Reference :225-241: every term masked, the sum of the means over the mask's mean; an all-zero mask counts as
        all ones.  That rule is applied on the device (no host comparison: the step stays capturable)."""
        occu_mask = occu_mask.detach()
        mean = occu_mask.mean()
        empty = mean == 0
        occu_mask = torch.where(empty, torch.ones_like(occu_mask), occu_mask)
        mean = torch.where(empty, torch.ones_like(mean), mean)
        if self._fused():
            # for a 0 / 1 mask |a m - b m| and |a - b| m are the same floats: the fused ops serve unchanged
            orig_m, recons_m = im_orig * occu_mask, im_recons * occu_mask
            loss = photometric_loss(orig_m, recons_m, self.l1_weight, self.ssim_weight)
            if self.ternary_weight is not None:
                census = self.ternary_weight * census_loss(recons_m, orig_m)
                loss = loss + census if (self.l1_weight or self.ssim_weight) else census
            return loss / mean
        terms = []
        if self.l1_weight is not None:
            terms.append(self.l1_weight * (im_orig - im_recons).abs() * occu_mask)
        if self.ssim_weight is not None:
            terms.append(self.ssim_weight * _ssim_distance(im_recons * occu_mask, im_orig * occu_mask))
        if self.ternary_weight is not None:
            if self.backend != "torch":        # `backend` may be reassigned on a live object
                raise NotImplementedError("the census (ternary) term needs fused=True or backend='torch'")
            terms.append(self.ternary_weight * TernaryLoss(im_recons * occu_mask, im_orig * occu_mask))
        return sum(t.mean() for t in terms) / mean

    def loss_photometric(self, im_orig, im_recons, occu_mask=None):
        """The photometric term of one direction at one scale.  ``occu_mask`` (B,1,H,W) or (B,C,H,W), 1 = visible: the
        masked term of the reference (:225-241); ``None``: the unmasked term (the reference's all-ones mask)."""
        if occu_mask is not None:
            return self._loss_photometric_masked(im_orig, im_recons, occu_mask)
        if self._fused():
            loss = photometric_loss(im_orig, im_recons, self.l1_weight, self.ssim_weight)
            if self.ternary_weight is not None:
                if not (self.l1_weight or self.ssim_weight):
                    return self.ternary_weight * census_loss(im_recons, im_orig)
                loss = loss + self.ternary_weight * census_loss(im_recons, im_orig)
            return loss
        terms = []
        if self.l1_weight is not None:
            terms.append(self.l1_weight * (im_orig - im_recons).abs())
        if self.ssim_weight is not None:
            terms.append(self.ssim_weight * _ssim_distance(im_recons, im_orig))
        if self.ternary_weight is not None:
            if self.backend != "torch":        # `backend` may be reassigned on a live object
                raise NotImplementedError("the census (ternary) term needs fused=True or backend='torch'")
            terms.append(self.ternary_weight * TernaryLoss(im_recons, im_orig))
        return sum(t.mean() for t in terms)          # (no mask: the reference divides by the mean of ones)

    def loss_smooth(self, flow, image):
        fn = edge_smoothness if self._fused() else _edge_aware_smoothness
        return fn(flow, image, self.smooth_args["alpha"], self.smooth_args["degree"])

    def forward(self, predictions, targets):
        total_warp, total_smooth, s = 0., 0., 1.
        used = [i for i in range(min(len(predictions["flow"]), len(predictions["flow_b"]))) if self.w_wrp_scales[i] != 0]
        sizes = [tuple(predictions["flow"][i].shape[2:]) for i in used]
        # both target images at every scale the loss uses: one pass over each image (reference: one
        # F.interpolate per scale and image, :279-280)
        pyr1 = dict(zip(used, self._pyramid(targets["l_img"], sizes)))
        pyr2 = dict(zip(used, self._pyramid(targets["l_seq"], sizes)))
        mask1 = mask2 = None
        for i, (f12, f21) in enumerate(zip(predictions["flow"], predictions["flow_b"])):
            if self.w_wrp_scales[i] == 0:
                continue
            size = tuple(f12.shape[2:])
            im1, im2 = pyr1[i], pyr2[i]
            if i == 0:
                s = min(size)
            if self.occlusion:
                if mask1 is None:
                    mask1, mask2 = self.occlusion_masks(f12, f21)
                else:
                    mask1 = torch.nn.functional.interpolate(mask1, size, mode="nearest")
                    mask2 = torch.nn.functional.interpolate(mask2, size, mode="nearest")
            warp = self.loss_photometric(im1, self._warp(im2, f12), mask1)
            smooth = self.loss_smooth(f12 / s, im1)
            if self.consistency:
                warp = (warp + self.loss_photometric(im2, self._warp(im1, f21), mask2)) / 2.
                smooth = (smooth + self.loss_smooth(f21 / s, im2)) / 2.
            total_warp = total_warp + warp * self.w_wrp_scales[i]
            total_smooth = total_smooth + smooth * self.w_sm_scales[i]
        return self.weight * (total_warp + self.smooth_args["weighting"] * total_smooth)
