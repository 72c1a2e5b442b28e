"""cerberusnet_amd -- MI355X-native (gfx950) correlation + flow-warp hot path for
CerberusNet, behind the reference's own ``correlation_package`` /
``flow_warp`` surface.  Importing the package registers ``torch.ops.cerberus.*``.
"""
__version__ = "0.1.0"

from . import ops  # noqa: F401  (registers torch.ops.cerberus.*)
from .correlation_package.correlation import (Correlation, CorrelationFunction,
                                              CorrelationTorch)
from .loss_functions.depth_losses import (BackprojectDepth, DepthAwareLoss, DepthReconstructionLossV1, InvHuberLoss,
                                          InvHuberLossPyr, Project3D, ScaleInvariantError, inv_huber_loss, reproject_warp)
from .loss_functions.ohem_losses import (MixSoftmaxCrossEntropyLoss, MixSoftmaxCrossEntropyOHEMLoss,
                                         SoftmaxCrossEntropyOHEMLoss, seg_ohem_cross_entropy)
from .loss_functions.panoptic_loss import DeeplabPanopticLoss, deeplab_panoptic_loss
from .loss_functions.rmi import MultiScaleRMILoss, RMILoss, RMILossAux, rmi_loss
from .loss_functions.seg_losses import FocalLoss2D, SegCrossEntropy, class_balance_weights, seg_cross_entropy
from .loss_functions.UnFlowLoss import (TernaryLoss, area_pyramid, area_resize, census_loss, edge_smoothness, flow_warp,
                                         get_corresponding_map, get_occu_mask_backward, get_occu_mask_bidirection, mesh_grid,
                                         norm_grid, photometric_loss)
from . import ops_ocr  # noqa: F401  (registers torch.ops.cerberus_ocr.*)
from .nnet_models.ocr_utils import BNReLU, ObjectAttentionBlock, SpatialGather_Module, SpatialOCR_Module, scale_as
from .nnet_models.ocrnet import OCR_block, OCRNetHead
from .ops_ocr import object_attention, spatial_gather
from . import ops_detr  # noqa: F401  (registers torch.ops.cerberus_detr.*)
from .loss_functions.detr_loss import DetrLoss, detr_set_loss
from .nnet_models.detr import HungarianMatcher, pad_targets
from . import ops_pdl  # noqa: F401  (registers torch.ops.cerberus_pdl.*)
from .nnet_models.aspp import ASPP
from .nnet_models.deeplab_panoptic import PanopticDeepLabDecoder, SinglePanopticDeepLabDecoder, SinglePanopticDeepLabHead
from .ops_pdl import dwconv5x5, upcat_dwconv5x5
from . import ops_attn  # noqa: F401  (registers torch.ops.cerberus_attn.*)
from .nnet_models.detr import (MLP, DetrSegmHead, PositionEmbeddingLearned, PositionEmbeddingSine, Transformer, TransformerDecoder,
                               TransformerDecoderLayer, TransformerEncoder, TransformerEncoderLayer, build_position_encoding)
from .ops_attn import detr_attention
from .statistics import DepthMetric, MetricBase, OpticFlowMetric, PanopticMetric, SegmentationMetric
from .utilities.panoptic_targets import PanopticTargetGenerator, panoptic_targets

__all__ = ["Correlation", "CorrelationFunction", "CorrelationTorch", "flow_warp",
           "mesh_grid", "norm_grid", "area_resize", "area_pyramid", "photometric_loss", "edge_smoothness", "TernaryLoss",
           "census_loss", "get_corresponding_map", "get_occu_mask_backward", "get_occu_mask_bidirection", "BackprojectDepth", "Project3D",
           "DepthReconstructionLossV1", "reproject_warp", "seg_cross_entropy", "class_balance_weights", "FocalLoss2D",
           "SegCrossEntropy", "seg_ohem_cross_entropy", "MixSoftmaxCrossEntropyLoss", "SoftmaxCrossEntropyOHEMLoss",
           "MixSoftmaxCrossEntropyOHEMLoss", "inv_huber_loss", "InvHuberLoss", "InvHuberLossPyr", "ScaleInvariantError", "DepthAwareLoss",
           "rmi_loss", "RMILoss", "RMILossAux", "MultiScaleRMILoss", "MetricBase", "SegmentationMetric", "DepthMetric", "OpticFlowMetric",
           "PanopticMetric", "deeplab_panoptic_loss", "DeeplabPanopticLoss", "panoptic_targets", "PanopticTargetGenerator", "ops",
           "BNReLU", "scale_as", "SpatialGather_Module", "ObjectAttentionBlock", "SpatialOCR_Module", "OCR_block", "OCRNetHead",
           "spatial_gather", "object_attention", "ops_ocr",
           "ops_detr", "DetrLoss", "detr_set_loss", "HungarianMatcher", "pad_targets",
           "ops_pdl", "dwconv5x5", "upcat_dwconv5x5", "ASPP", "SinglePanopticDeepLabDecoder", "SinglePanopticDeepLabHead",
           "PanopticDeepLabDecoder",
           "ops_attn", "detr_attention", "Transformer", "TransformerEncoder", "TransformerDecoder", "TransformerEncoderLayer",
           "TransformerDecoderLayer", "PositionEmbeddingSine", "PositionEmbeddingLearned", "build_position_encoding", "MLP",
           "DetrSegmHead"]
