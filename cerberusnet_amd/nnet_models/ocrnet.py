"""The OCR segmentation head: ``OCR_block`` (counterpart of the reference's ``nnet_models/ocrnet.py``) and ``OCRNetHead`` (of its
``nnet_models/ocrnet_sfd.py``).  Constructor arguments, attribute names, ``forward`` signatures and ``state_dict`` keys are the
reference's, so its checkpoints load; the code is this package's.  ``backend='hip' | 'torch'`` is passed down to the two OCR steps
(nnet_models/ocr_utils.py; ``None``, the default, leaves each step its own measured default); everything else is stock dense ops.

``CerberusBase`` does not take a ``segmentation_config`` yet (a later change wires the head in).  Until then backbone and head run
by hand:

    head = OCRNetHead(backbone.output_ch, mid_channels=512, key_channels=256, classes=19)
    out = head(backbone(image))          # HighResolutionNet(concat_features=True); out['seg'], out['seg_aux']
"""
from typing import List

import torch
from torch import nn

from .ocr_utils import BNReLU, SpatialGather_Module, SpatialOCR_Module


def _reset_decoder(root):
    """What ``init_decoder`` asks for: He-normal weights and zero biases in every convolution under ``root``, and every
    BatchNorm back at the identity (weight 1, bias 0)."""
    with torch.no_grad():
        for layer in root.modules():
            if isinstance(layer, (nn.Conv2d, nn.Linear)):
                nn.init.kaiming_normal_(layer.weight)
            elif isinstance(layer, nn.BatchNorm2d):
                nn.init.ones_(layer.weight)
            else:
                continue
            if layer.bias is not None:
                nn.init.zeros_(layer.bias)


def _conv_bn_relu(c_in, c_out, kernel_size):
    """Biased 'same' convolution, BatchNorm, ReLU: keys ``0.*`` (convolution) and ``1.0.*`` (BatchNorm)."""
    return [nn.Conv2d(c_in, c_out, kernel_size, padding=kernel_size // 2), BNReLU(c_out)]


class OCR_block(nn.Module):
    """3 x 3 projection, auxiliary class logits, the class contexts gathered under them, the object attention, the class logits.
    ``forward`` returns (cls_out, aux_out, ocr_feats)."""

    def __init__(self, high_level_ch, backend=None, **kwargs):
        super().__init__()
        mid, key, classes = kwargs['mid_channels'], kwargs['key_channels'], kwargs['classes']

        self.conv3x3_ocr = nn.Sequential(*_conv_bn_relu(high_level_ch, mid, 3))
        self.ocr_gather_head = SpatialGather_Module(classes, backend=backend)
        self.ocr_distri_head = SpatialOCR_Module(mid, key, mid, scale=1, dropout=0.05, backend=backend)
        self.cls_head = nn.Conv2d(mid, classes, 1)
        self.aux_head = nn.Sequential(*_conv_bn_relu(high_level_ch, high_level_ch, 1), nn.Conv2d(high_level_ch, classes, 1))
        if 'init_decoder' in kwargs:
            _reset_decoder(self)

    def forward(self, high_level_features):
        x = high_level_features[0] if isinstance(high_level_features, tuple) else high_level_features
        coarse = self.aux_head(x)                                   # the auxiliary logits are the gather's soft regions
        pixels = self.conv3x3_ocr(x)
        regions = self.ocr_gather_head(pixels, coarse)              # (B, mid, classes, 1)
        augmented = self.ocr_distri_head(pixels, regions)
        return self.cls_head(augmented), coarse, augmented


class OCRNetHead(nn.Module):
    """The self-contained OCR head of the multi-task model: ``features_in`` is what ``HighResolutionNet(concat_features=True)``
    returns; the result holds ``'seg'`` and ``'seg_aux'`` at the features' resolution."""

    def __init__(self, channels_in: List[int], backend=None, **kwargs):
        super().__init__()
        self.ocr = OCR_block(sum(channels_in), backend=backend, **kwargs)

    def forward(self, features_in: List[torch.Tensor]):
        seg, seg_aux = self.ocr(features_in)[:2]
        return {'seg': seg, 'seg_aux': seg_aux}
