"""Atrous spatial pyramid pooling as the Panoptic-DeepLab decoders use it: the reference's ``nnet_models/aspp.py`` with its
constructor arguments and state-dict keys (``convs.0.0.weight`` .. ``convs.4.aspp_pooling.1.weight``, ``project.*``), written for
this package in stock ``torch.nn``.  Dense and dilated convolutions, BatchNorm and a resize: nothing here has a fused route.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ["ASPP"]


def _conv_bn_relu(in_channels, out_channels, kernel_size, dilation=1):
    """A bias-free convolution that keeps the map's size, BatchNorm, ReLU: keys ``0.weight``, ``1.*``."""
    padding = dilation * (kernel_size // 2)
    return nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding, dilation=dilation, bias=False),
                         nn.BatchNorm2d(out_channels), nn.ReLU())


class ASPPPooling(nn.Module):
    """The image-level branch: average pooling (global, or a fixed window once ``set_image_pooling`` was called), a 1 x 1
    convolution, ReLU, and a bilinear resize back to the input's size."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.aspp_pooling = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(in_channels, out_channels, 1, bias=False), nn.ReLU())

    def set_image_pooling(self, pool_size=None):
        self.aspp_pooling[0] = nn.AdaptiveAvgPool2d(1) if pool_size is None else nn.AvgPool2d(kernel_size=pool_size, stride=1)

    def forward(self, x):
        return F.interpolate(self.aspp_pooling(x), size=x.shape[-2:], mode="bilinear", align_corners=True)


class ASPP(nn.Module):
    """Five branches over the same input -- a 1 x 1 convolution, three 3 x 3 convolutions at ``atrous_rates`` and the image
    pooling -- concatenated and projected to ``out_channels`` (1 x 1 convolution, BatchNorm, ReLU, Dropout 0.5)."""

    def __init__(self, in_channels, out_channels, atrous_rates):
        super().__init__()
        rates = tuple(atrous_rates)
        if len(rates) != 3:
            raise ValueError("ASPP takes three atrous rates, got %r" % (atrous_rates,))
        branches = [_conv_bn_relu(in_channels, out_channels, 1)]
        branches += [_conv_bn_relu(in_channels, out_channels, 3, dilation=rate) for rate in rates]
        branches.append(ASPPPooling(in_channels, out_channels))
        self.convs = nn.ModuleList(branches)
        self.project = nn.Sequential(nn.Conv2d(5 * out_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(),
                                     nn.Dropout(0.5))

    def set_image_pooling(self, pool_size):
        self.convs[-1].set_image_pooling(pool_size)

    def forward(self, x):
        return self.project(torch.cat([branch(x) for branch in self.convs], dim=1))
