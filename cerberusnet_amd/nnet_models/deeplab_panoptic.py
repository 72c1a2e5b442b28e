"""The Panoptic-DeepLab decoder head: the reference's ``nnet_models/deeplab_panoptic.py`` with its constructor arguments, its
``forward(features)`` and its state-dict keys (so the ``segmentation.*`` entries of a reference checkpoint load), written for this
package in stock ``torch.nn``.

``PanopticDeepLabDecoder`` is used on what ``HighResolutionNet`` returns, directly, as ``OCRNetHead`` is: ``forward`` consumes
``features[1]``, the list of maps from the lowest resolution up, and returns ``seg`` and, with ``has_instance``, ``center`` and
``offset`` -- what ``DeeplabPanopticLoss`` and the segmentation losses train.  ``CerberusBase`` does not build it (it still refuses
a ``segmentation_config``).

A decoder stage is ``interpolate(x, size, bilinear, align_corners=True)`` -> ``cat((x, l), 1)`` -> depthwise 5 x 5 convolution ->
BatchNorm, ReLU, 1 x 1 convolution, BatchNorm, ReLU, and every classifier starts with the same depthwise 5 x 5.  That step has a
fused HIP route (``cerberus_pdl::upcat_dwconv5x5`` / ``cerberus_pdl::dwconv5x5``, csrc/pdl_head.hip): the upsampled
map and the concatenation are never written.  The depthwise ``nn.Conv2d`` stays in place as the holder of the weights.  BatchNorm,
ReLU, the 1 x 1 convolutions and the ASPP are stock ops on every route.

``backend='hip'`` takes the fused ops for fp32 CUDA tensors outside autocast; everything else (CPU, 16-bit, autocast) takes the
reference's operation order in stock ops, which is all ``backend='torch'`` ever does.  ``backend=None`` (the default) is each op's
own default, decided by the measurement (see below).
"""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops_pdl
from .aspp import ASPP

__all__ = ["SinglePanopticDeepLabDecoder", "SinglePanopticDeepLabHead", "PanopticDeepLabDecoder"]

# The defaults follow the measurement (tools/prof_pdl_head.py, profiles/pdl_head_fused.txt): an op's fused route is
# its default where it was at least as fast as the stock chain, forward + backward, at both measured shapes.  Both were: the last
# decoder stage at 4 pairs of 1024 x 512 took 5228 -> 646 us (8.1 x), a classifier's convolution 4064 -> 403 us (10.1 x); one run.
DEFAULT_UPCAT_BACKEND = "hip"       # the decoder stages: upsample + concat + depthwise 5 x 5
DEFAULT_DWCONV_BACKEND = "hip"      # the classifiers: the depthwise 5 x 5 alone


def _backend(backend, default):
    """``None``: the op's own default."""
    backend = default if backend is None else backend
    if backend not in ("hip", "torch"):
        raise ValueError("backend must be 'hip' or 'torch'")
    return backend


class _SeparableConv5x5(nn.Sequential):
    """Depthwise 5 x 5 convolution, BatchNorm, ReLU, then a 1 x 1 convolution to ``out_planes``, BatchNorm, ReLU, nested as the
    reference nests them: keys ``0.0.0.weight`` (depthwise), ``0.0.1.*``, ``0.1.weight`` (pointwise), ``0.2.*``.

    ``forward(x)`` convolves ``x``; ``forward(x, low)`` convolves ``cat(interpolate(low, x's size), x)``."""

    def __init__(self, in_planes, out_planes, backend):
        depthwise = nn.Sequential(nn.Conv2d(in_planes, in_planes, 5, padding=2, groups=in_planes, bias=False),
                                  nn.BatchNorm2d(in_planes), nn.ReLU())
        super().__init__(nn.Sequential(depthwise, nn.Conv2d(in_planes, out_planes, 1, bias=False), nn.BatchNorm2d(out_planes), nn.ReLU()))
        self.backend = backend

    def forward(self, x, low=None):
        depthwise, pointwise = self[0][0], self[0][1:]
        conv = depthwise[0]
        tensors = (x, conv.weight) if low is None else (low, x, conv.weight)
        if self.backend == "hip" and ops_pdl.pdl_fused_ok(*tensors):
            x = ops_pdl.dwconv5x5(x, conv.weight) if low is None else ops_pdl.upcat_dwconv5x5(low, x, conv.weight)
        else:
            if low is not None:
                low = F.interpolate(low, size=x.shape[2:], mode="bilinear", align_corners=True)
                x = torch.cat((low, x), dim=1)
            x = conv(x)
        return pointwise(depthwise[2](depthwise[1](x)))


class SinglePanopticDeepLabDecoder(nn.Module):
    """ASPP on the lowest-resolution map, then one stage per higher-resolution map: project that map with a 1 x 1 convolution,
    upsample the running features to its size, concatenate, fuse with a depthwise-separable 5 x 5 convolution."""

    def __init__(self, in_channels, low_level_channels_project, decoder_channels, atrous_rates, aspp_channels=None, backend=None):
        super().__init__()
        backend = _backend(backend, DEFAULT_UPCAT_BACKEND)
        if aspp_channels is None:
            aspp_channels = decoder_channels
        self.aspp = ASPP(in_channels[-1], out_channels=aspp_channels, atrous_rates=atrous_rates)
        self.decoder_stage = len(in_channels) - 1
        if self.decoder_stage != len(low_level_channels_project):
            raise ValueError("%d maps above the lowest need %d projection widths, got %r"
                             % (self.decoder_stage, self.decoder_stage, low_level_channels_project))
        project, fuse = [], []
        running = aspp_channels
        for i, width in enumerate(low_level_channels_project):       # top-down: from the largest stride
            project.append(nn.Sequential(nn.Conv2d(in_channels[-2 - i], width, 1, bias=False), nn.BatchNorm2d(width), nn.ReLU()))
            fuse.append(_SeparableConv5x5(running + width, decoder_channels, backend))
            running = decoder_channels
        self.project = nn.ModuleList(project)
        self.fuse = nn.ModuleList(fuse)
        self.backend = backend

    def set_image_pooling(self, pool_size):
        self.aspp.set_image_pooling(pool_size)

    def forward(self, features):
        x = self.aspp(features[0])
        for idx in range(self.decoder_stage):
            x = self.fuse[idx](self.project[idx](features[idx + 1]), low=x)
        return x


class SinglePanopticDeepLabHead(nn.Module):
    """One classifier per entry of ``class_key``: a depthwise-separable 5 x 5 convolution to ``head_channels`` and a 1 x 1
    convolution (with bias) to ``num_classes[i]``."""

    def __init__(self, decoder_channels, head_channels, num_classes, class_key, backend=None):
        super().__init__()
        backend = _backend(backend, DEFAULT_DWCONV_BACKEND)
        self.num_head = len(num_classes)
        if self.num_head != len(class_key):
            raise ValueError("%d class counts for %d keys" % (self.num_head, len(class_key)))
        self.classifier = nn.ModuleDict({key: nn.Sequential(_SeparableConv5x5(decoder_channels, head_channels, backend),
                                                            nn.Conv2d(head_channels, n, 1))
                                         for key, n in zip(class_key, num_classes)})
        self.class_key = class_key
        self.backend = backend

    def forward(self, x):
        return OrderedDict((key, self.classifier[key](x)) for key in self.class_key)


class PanopticDeepLabDecoder(nn.Module):
    """The semantic decoder and head (``seg``) and, with ``has_instance=True``, the instance decoder and head (the keys of
    ``instance_class_key``: ``center`` and ``offset``), both on ``features[1]``."""

    def __init__(self, in_channels, low_level_channels_project, decoder_channels, atrous_rates, num_classes, backend=None, **kwargs):
        super().__init__()
        if backend is not None:
            _backend(backend, None)
        self.semantic_decoder = SinglePanopticDeepLabDecoder(in_channels, low_level_channels_project, decoder_channels, atrous_rates,
                                                             backend=backend)
        self.semantic_head = SinglePanopticDeepLabHead(decoder_channels, decoder_channels, [num_classes], ["seg"], backend=backend)
        self.instance_decoder = None
        self.instance_head = None
        if kwargs.get("has_instance", False):
            self.instance_decoder = SinglePanopticDeepLabDecoder(in_channels, kwargs["instance_low_level_channels_project"],
                                                                 kwargs["instance_decoder_channels"], atrous_rates,
                                                                 aspp_channels=kwargs["instance_aspp_channels"], backend=backend)
            self.instance_head = SinglePanopticDeepLabHead(kwargs["instance_decoder_channels"], kwargs["instance_head_channels"],
                                                           kwargs["instance_num_classes"], kwargs["instance_class_key"], backend=backend)

    def set_image_pooling(self, pool_size):
        self.semantic_decoder.set_image_pooling(pool_size)
        if self.instance_decoder is not None:
            self.instance_decoder.set_image_pooling(pool_size)

    def forward(self, features):
        pred = OrderedDict()
        pred.update(self.semantic_head(self.semantic_decoder(features[1])))
        if self.instance_decoder is not None:
            pred.update(self.instance_head(self.instance_decoder(features[1])))
        return pred
