"""The reference's training-metric loggers (``nnet_training/statistics/``) on this package's surface: ``SegmentationMetric``,
``DepthMetric`` and ``OpticFlowMetric`` over a ``MetricBase``.  fp32 CUDA tensors take the fused HIP ops of ``csrc/metrics.hip``
(``backend='hip'``, the default) and ONE device-to-host copy per ``add_sample``; everything else takes a stock-op restatement in
the reference's operation order that makes the same single copy."""
from .base import MetricBase
from .depth import DepthMetric
from .optical_flow import OpticFlowMetric
from .panoptic import PanopticMetric
from .semantic import SegmentationMetric

__all__ = ["MetricBase", "SegmentationMetric", "DepthMetric", "OpticFlowMetric", "PanopticMetric"]
