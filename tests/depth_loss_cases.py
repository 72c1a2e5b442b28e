"""Inputs of the supervised depth-loss tests, shared by tests/test_depth_loss_cpu.py, tests/test_depth_loss_gpu.py and the
generator of tests/golden/depth_loss.npz (tools/gen_golden_depth_loss.py): everything comes from ``hash_uniform`` seeds.

Predictions are uniform in [-1, 6), so about 1/7 of them are non-positive (the ReLU's flat side).  The ground truth is uniform
in [0.01, 5), and about 40 % of it is set to 0 (no measurement: an invalid pixel) from a second hash field."""
import numpy as np

from cerberusnet_amd.synth import hash_uniform

INVALID_SHARE = 0.4

# the golden cases: (class name, prediction shape (B,1,h,w), constructor keywords, "tie" = the maximum is tied between two pixels)
GOLDEN_CASES = [
    ("InvHuberLoss", (1, 1, 9, 20), dict(), False),
    ("InvHuberLoss", (2, 1, 12, 20), dict(weight=0.5), False),
    ("InvHuberLoss", (2, 1, 12, 20), dict(), True),
    ("ScaleInvariantError", (2, 1, 12, 20), dict(), False),
    ("ScaleInvariantError", (2, 1, 12, 20), dict(weight=2.0, lmda=0.5), False),
    ("DepthAwareLoss", (2, 1, 12, 20), dict(), False),
    ("DepthAwareLoss", (1, 1, 9, 20), dict(weight=0.5), False),
]


def prediction(shape, seed):
    return hash_uniform(shape, seed, -1.0, 6.0)


def ground_truth(shape, seed, invalid_share=INVALID_SHARE):
    """(B,H,W) float32 ground truth for a prediction of ``shape`` = (B,1,H,W) or (B,H,W)."""
    shape = (shape[0],) + tuple(shape[-2:])
    g = hash_uniform(shape, seed, 0.01, 5.0)
    g[hash_uniform(shape, seed + 1, 0.0, 1.0) < invalid_share] = 0.0
    return g


def plant_tie(p, g):
    """Two valid pixels, far apart, whose errors are equal, larger than every other one and of opposite sign: prediction 10.5
    against 1.5 (d = +9) and 0.5 against 9.5 (d = -9), all exact in fp32."""
    p, g = p.copy(), g.copy()
    n = p.size
    for i, (pv, gv) in ((3, (10.5, 1.5)), (n - 5, (0.5, 9.5))):
        p.reshape(-1)[i], g.reshape(-1)[i] = pv, gv
    return p, g


def golden_inputs(i):
    """Prediction (B,1,h,w) float32 and ground truth (B,h,w) float32 of golden case ``i``."""
    _, shape, _, tie = GOLDEN_CASES[i]
    p, g = prediction(shape, 1700 + 10 * i), ground_truth(shape, 1705 + 10 * i)
    return plant_tie(p, g) if tie else (p, g)
