from .box_ops import box_cxcywh_to_xyxy, box_iou, box_xyxy_to_cxcywh, generalized_box_iou
from .matcher import HungarianMatcher, pad_targets

__all__ = ["box_cxcywh_to_xyxy", "box_xyxy_to_cxcywh", "box_iou", "generalized_box_iou", "HungarianMatcher", "pad_targets"]
