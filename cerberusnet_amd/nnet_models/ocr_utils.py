"""The object-contextual representation (OCR) modules of the segmentation head: the reference's ``nnet_models/ocr_utils.py`` with
its constructor arguments, attribute names and ``forward`` signatures (so the ``segmentation.ocr.*`` entries of a reference
checkpoint load), written for this package.

The convolutions, BatchNorm and the resizes are stock dense ops.  The two steps that make the head an OCR head have a fused HIP
route (``cerberus_ocr::spatial_gather`` / ``cerberus_ocr::object_attention``, csrc/ocr_head.hip):

* ``SpatialGather_Module``: the softmax over all pixels of each class plane, times the features -- one pooling pass over the
  features instead of a softmax pass and a (K x HW)(HW x C) matmul.
* ``ObjectAttentionBlock``: ``softmax(q . k / sqrt(Kc))`` over the regions, times the values -- the context written in
  (B, Kc, H, W) order with no (B, HW, Kc) intermediate and no ``permute(0, 2, 1).contiguous()`` copy of it.

``backend='hip'`` takes the fused ops for fp32 CUDA tensors outside autocast with 1..32 regions; everything else (CPU, 16-bit,
autocast, more than 32 classes) takes the reference's operation order in stock ops, which is all ``backend='torch'`` ever does.  A
``backend='hip'`` module on CPU tensors therefore works, as the loss classes do.  ``backend=None`` (the default) is each step's own
default: 'hip' for the attention, 'torch' for the gather (see below).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops_ocr

# The defaults follow the measurement (tools/prof_ocr_head.py, profiles/ocr_head_fused.txt): a step's fused route is
# its default where it beat the stock chain, forward + backward, at both measured shapes.  The attention did (1.38 x and 1.06 x, one run); the
# gather did not at the model's shape (0.99 x; 1.05 x at the smaller one), so it stays opt-in, as warp_correlation_leaky does.
DEFAULT_GATHER_BACKEND = "torch"
DEFAULT_ATTENTION_BACKEND = "hip"


def _backend(backend, default):
    """``None``: the step's own default."""
    backend = default if backend is None else backend
    if backend not in ("hip", "torch"):
        raise ValueError("backend must be 'hip' or 'torch'")
    return backend


def BNReLU(ch):
    """BatchNorm2d + ReLU (multi-GPU training needs the synchronised BatchNorm: ``nn.SyncBatchNorm.convert_sync_batchnorm``)."""
    return nn.Sequential(nn.BatchNorm2d(ch), nn.ReLU())


def scale_as(x, y):
    """``x`` resized (bilinear, align_corners) to the height and width of ``y``."""
    return F.interpolate(x, size=(y.size(2), y.size(3)), mode="bilinear", align_corners=True)


def _projection(*widths):
    """Bias-free 1 x 1 convolutions ``widths[i] -> widths[i + 1]``, each followed by BatchNorm + ReLU (keys ``0.*``, ``1.0.*``,
    ``2.*``, ``3.0.*``)."""
    layers = []
    for c_in, c_out in zip(widths, widths[1:]):
        layers += [nn.Conv2d(c_in, c_out, 1, bias=False), BNReLU(c_out)]
    return nn.Sequential(*layers)


def _gather_stock(feats, logits, scale):
    """The gather in stock ops, in the reference's operation order: the softmax of ``scale * logits`` over each plane's pixels,
    then one (K x HW)(HW x C) matmul per image.  (B, C, K)."""
    weights = F.softmax(scale * logits.flatten(2), dim=2)                                   # (B, K, HW)
    return torch.matmul(weights, feats.flatten(2).transpose(1, 2)).transpose(1, 2)


def _attention_stock(query, key, value, scale):
    """The attention core in stock ops, in the reference's operation order: (HW x Kc)(Kc x R), times ``scale``, softmax over
    the regions, (HW x R)(R x Kc), and the copy back into (B, Kc, H, W) order."""
    weights = F.softmax(scale * torch.matmul(query.flatten(2).transpose(1, 2), key), dim=-1)             # (B, HW, R)
    per_pixel = torch.matmul(weights, value.transpose(1, 2))                                            # (B, HW, Kc)
    return per_pixel.transpose(1, 2).contiguous().view(query.shape)


class SpatialGather_Module(nn.Module):
    """The context of every class: ``softmax`` of ``scale * probs`` (B,K,H,W) over the pixels, times ``feats`` (B,C,H,W).
    Returns (B, C, K, 1)."""

    def __init__(self, cls_num=0, scale=1, backend=None):
        super().__init__()
        self.cls_num = cls_num
        self.scale = scale
        self.backend = _backend(backend, DEFAULT_GATHER_BACKEND)

    def forward(self, feats, probs):
        if self.backend == "hip" and feats.dim() == 4 and ops_ocr.ocr_fused_ok(feats, probs, regions=probs.size(1)):
            return ops_ocr.spatial_gather(feats, probs, self.scale).unsqueeze(3)
        return _gather_stock(feats, probs, self.scale).unsqueeze(3)


class ObjectAttentionBlock(nn.Module):
    """Pixel-to-region attention: ``x`` (B,C,H,W) attends to the region representations ``proxy`` (B,C,R,1); returns (B,C,H,W).
    ``scale`` > 1 max-pools the pixels first and resizes the result back."""

    def __init__(self, in_channels, key_channels, scale=1, backend=None):
        super().__init__()
        self.scale = scale
        self.in_channels = in_channels
        self.key_channels = key_channels
        self.backend = _backend(backend, DEFAULT_ATTENTION_BACKEND)
        self.pool = nn.MaxPool2d(kernel_size=(scale, scale))

        self.f_pixel = _projection(in_channels, key_channels, key_channels)
        self.f_object = _projection(in_channels, key_channels, key_channels)
        self.f_down = _projection(in_channels, key_channels)
        self.f_up = _projection(key_channels, in_channels)

    def forward(self, x, proxy):
        full_size = x.shape[2:]
        if self.scale > 1:
            x = self.pool(x)
        query = self.f_pixel(x)
        key, value = self.f_object(proxy).flatten(2), self.f_down(proxy).flatten(2)         # (B, Kc, R) each
        softmax_scale = self.key_channels ** -0.5
        if self.backend == "hip" and ops_ocr.ocr_fused_ok(query, key, value, regions=key.size(2)):
            context = ops_ocr.object_attention(query, key, value, softmax_scale)
        else:
            context = _attention_stock(query, key, value, softmax_scale)
        context = self.f_up(context)
        if self.scale > 1:
            context = F.interpolate(context, size=tuple(full_size), mode="bilinear", align_corners=True)
        return context


class SpatialOCR_Module(nn.Module):
    """The OCR module: the object context of every pixel, concatenated with the pixel's features and projected."""

    def __init__(self, in_channels, key_channels, out_channels, scale=1, dropout=0.1, backend=None, **kwargs):
        super().__init__()
        if "OCR_ASPP" in kwargs:
            raise NotImplementedError("SpatialOCR_Module: the OCR_ASPP variant is not implemented (nor is the reference's get_aspp)")
        self.object_context_block = ObjectAttentionBlock(in_channels, key_channels, scale, backend=backend)
        self.conv_bn_dropout = _projection(2 * in_channels, out_channels)       # context and features, side by side
        self.conv_bn_dropout.append(nn.Dropout2d(dropout))

    def forward(self, feats, proxy_feats):
        attended = self.object_context_block(feats, proxy_feats)
        return self.conv_bn_dropout(torch.cat((attended, feats), dim=1))
