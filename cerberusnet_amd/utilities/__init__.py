"""Deployment-side helpers and the panoptic post-processing."""
from . import panoptic_post_processing

__all__ = ["panoptic_post_processing"]
