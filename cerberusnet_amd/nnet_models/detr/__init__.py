from .box_ops import box_cxcywh_to_xyxy, box_iou, box_xyxy_to_cxcywh, generalized_box_iou
from .matcher import HungarianMatcher, pad_targets
from .position_encoding import PositionEmbeddingLearned, PositionEmbeddingSine, build_position_encoding
from .transformer import (Transformer, TransformerDecoder, TransformerDecoderLayer, TransformerEncoder,
                          TransformerEncoderLayer)
from .head import MLP, DetrSegmHead

__all__ = ["box_cxcywh_to_xyxy", "box_xyxy_to_cxcywh", "box_iou", "generalized_box_iou", "HungarianMatcher", "pad_targets",
           "PositionEmbeddingSine", "PositionEmbeddingLearned", "build_position_encoding", "Transformer", "TransformerEncoder",
           "TransformerDecoder", "TransformerEncoderLayer", "TransformerDecoderLayer", "MLP", "DetrSegmHead"]
