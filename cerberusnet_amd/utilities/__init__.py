"""Deployment-side helpers, the panoptic post-processing and the panoptic training
targets."""
from . import panoptic_post_processing
from .panoptic_targets import PanopticTargetGenerator, panoptic_targets      # the function, not the module of the same name

__all__ = ["panoptic_post_processing", "panoptic_targets", "PanopticTargetGenerator"]
