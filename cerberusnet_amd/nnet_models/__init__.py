from .pwcnet_sfd import PWCNetHead
from .pwcnet_modules import FlowEstimatorDense, FlowEstimatorLite, ContextNetwork
from .hrnetv2 import HighResolutionNet, hrnet_config
from .cerberus import CerberusBase, cerberus_flow_config
from .ocr_utils import BNReLU, ObjectAttentionBlock, SpatialGather_Module, SpatialOCR_Module, scale_as
from .ocrnet import OCR_block, OCRNetHead
from .aspp import ASPP
from .deeplab_panoptic import PanopticDeepLabDecoder, SinglePanopticDeepLabDecoder, SinglePanopticDeepLabHead
from .detr import (MLP, DetrSegmHead, PositionEmbeddingLearned, PositionEmbeddingSine, Transformer, TransformerDecoder,
                   TransformerDecoderLayer, TransformerEncoder, TransformerEncoderLayer, build_position_encoding)

__all__ = ["PWCNetHead", "FlowEstimatorDense", "FlowEstimatorLite", "ContextNetwork",
           "HighResolutionNet", "hrnet_config", "CerberusBase", "cerberus_flow_config",
           "BNReLU", "scale_as", "SpatialGather_Module", "ObjectAttentionBlock", "SpatialOCR_Module", "OCR_block", "OCRNetHead",
           "ASPP", "SinglePanopticDeepLabDecoder", "SinglePanopticDeepLabHead", "PanopticDeepLabDecoder",
           "Transformer", "TransformerEncoder", "TransformerDecoder", "TransformerEncoderLayer", "TransformerDecoderLayer",
           "PositionEmbeddingSine", "PositionEmbeddingLearned", "build_position_encoding", "MLP", "DetrSegmHead"]
