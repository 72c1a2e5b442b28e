"""Inputs of the segmentation-loss tests, shared by tests/test_seg_loss_cpu.py, tests/test_seg_loss_gpu.py and the generator
of tests/golden/seg_loss.npz (tools/gen_golden_seg_loss.py): everything comes from ``hash_uniform`` seeds.

Logits are uniform in [-4, 4).  Labels are skewed as ``min(floor(u * u * C), C - 1)`` for u uniform in [0, 1), so the low
classes are frequent and the high ones rare or absent (what the dynamic class weights are for), and about 15 % of them are
set to the ignore value from a second hash field."""
import numpy as np

from cerberusnet_amd.synth import hash_uniform

IGNORE_SHARE = 0.15

# the golden cases: (class name, shape (B,C,H,W), constructor keywords, target given as (B,1,H,W))
GOLDEN_CASES = [
    ("FocalLoss2D", (1, 19, 9, 20), dict(gamma=2.0, ignore_index=-1, dynamic_weights=True, scale_factor=0.125), False),
    ("FocalLoss2D", (2, 7, 12, 20), dict(weight=0.5, gamma=2.0, ignore_index=255, dynamic_weights=False), False),
    ("FocalLoss2D", (2, 7, 12, 20), dict(gamma=0.5, ignore_index=255, dynamic_weights=True, scale_factor=0.25), False),
    ("FocalLoss2D", (2, 7, 12, 20), dict(gamma=0.5, ignore_index=-1, dynamic_weights=False), False),
    ("SegCrossEntropy", (1, 19, 9, 20), dict(ignore_index=255, dynamic_weights=True), False),
    ("SegCrossEntropy", (2, 7, 12, 20), dict(weight=2.0, ignore_index=-1, dynamic_weights=False), False),
    ("SegCrossEntropy", (2, 7, 12, 20), dict(ignore_index=-1, dynamic_weights=True), True),
]


def logits(shape, seed):
    return hash_uniform(shape, seed, -4.0, 4.0)


def labels(shape, seed, ignore_index, ignore_share=IGNORE_SHARE):
    """(B,H,W) int64 labels for logits of ``shape`` = (B,C,H,W)."""
    B, C, H, W = shape
    u = hash_uniform((B, H, W), seed, 0.0, 1.0, dtype=np.float64)
    t = np.minimum(np.floor(u * u * C), C - 1).astype(np.int64)
    drop = hash_uniform((B, H, W), seed + 1, 0.0, 1.0) < ignore_share
    t[drop] = ignore_index
    return t


def golden_inputs(i):
    """Logits (B,C,H,W) float32 and the target (int64; (B,1,H,W) where the case says so) of golden case ``i``."""
    _, shape, kwargs, four_d = GOLDEN_CASES[i]
    x = logits(shape, 700 + 10 * i)
    t = labels(shape, 705 + 10 * i, kwargs["ignore_index"])
    return x, (t[:, None] if four_d else t)
