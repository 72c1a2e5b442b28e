"""Portable synthetic-input generator (no torch RNG, bit-identical everywhere).

SURVEY.md section 8(d): values in [-1, 1) from a counter hash so that this
container (where the reference can be imported to make golden vectors) and the
GPU box (where it cannot) regenerate exactly the same tensors.

    value(seed, i) = top24(splitmix64(seed * 2^40 + i)) / 2^23 - 1

Every value has at most 24 significant bits, so it is exact in float32.
"""
import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(z: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = (z + np.uint64(0x9E3779B97F4A7C15)) & _M64
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return z ^ (z >> np.uint64(31))


def hash_uniform(shape, seed: int, lo: float = -1.0, hi: float = 1.0,
                 dtype=np.float32) -> np.ndarray:
    """Deterministic array in [lo, hi); default [-1, 1) with 24-bit mantissas."""
    n = int(np.prod(shape)) if len(shape) else 1
    idx = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = (np.uint64(seed) << np.uint64(40)) + idx
    top = (_splitmix64(key) >> np.uint64(40)).astype(np.float64)  # 24 bits
    unit = top / float(1 << 23) - 1.0                              # [-1, 1)
    if lo != -1.0 or hi != 1.0:
        unit = (unit + 1.0) * (0.5 * (hi - lo)) + lo
    return unit.astype(dtype).reshape(shape)


# HRNetV2-W32 feature pyramid seen by the flow head at 1024x512 input
# (SURVEY.md section 3c): (C, H, W), low resolution first.
W32_PYRAMID_1024x512 = ((256, 16, 32), (128, 32, 64), (64, 64, 128),
                        (32, 128, 256))


def pyramid_shapes(width: int = 1024, height: int = 512, base_ch: int = 32):
    """(C,H,W) per level, coarse to fine, for an HRNetV2-W<base_ch> backbone
    (strides 32,16,8,4; channels 8w,4w,2w,w)."""
    return tuple((base_ch * (8 >> lvl), height // (32 >> lvl),
                  width // (32 >> lvl)) for lvl in range(4))


def fill_parameters(module, seed: int = 1000) -> None:
    """Deterministic, framework-RNG-free weights: parameter i (in named_parameters order) is
    hash_uniform(seed + i) scaled by 0.7/sqrt(fan_in) (weights) or 0.05 (biases).  Used to put
    identical weights into the reference's modules (in-container, for goldens) and into this
    repository's counterparts (anywhere)."""
    import math
    import torch
    for i, (_, p) in enumerate(module.named_parameters()):
        if p.dim() > 1:
            fan_in = int(np.prod(p.shape[1:]))
            scale = 0.7 / math.sqrt(fan_in)
        else:
            scale = 0.05
        with torch.no_grad():
            p.copy_(torch.from_numpy(hash_uniform(tuple(p.shape), seed + i) * scale))


# The stereo rig of the depth reconstruction loss (depth_losses.py:181): Cityscapes' focal length in pixels at 2048 columns
# and its baseline in metres.
STEREO_FOCAL_2048 = 2262.52
STEREO_BASELINE = 0.209313


def stereo_camera(batch: int, height: int, width: int, rig: str = "cityscapes"):
    """(inv_K, K, T), float32 (B,4,4) each: the Cityscapes rig scaled to `width` columns with an off-centre principal point
    and an x baseline ("cityscapes"), or the same with a small rotation and y / z translation ("rotated": the y and z
    terms of the projection are exercised).  Item b's focal length is 1 + b / 64 times the nominal one, so that a batch
    holds different matrices."""
    if rig not in ("cityscapes", "rotated"):
        raise ValueError(rig)
    inv_k, k, t = (np.zeros((batch, 4, 4)) for _ in range(3))
    for b in range(batch):
        f = STEREO_FOCAL_2048 * width / 2048.0 * (1.0 + b / 64.0)
        k[b] = np.array([[f, 0, 0.53 * (width - 1), 0], [0, f, 0.46 * (height - 1), 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        t[b] = np.eye(4)
        t[b, 0, 3] = STEREO_BASELINE
        if rig == "rotated":
            ay, ax = 0.004, -0.003          # radians about the y and x axes
            ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
            rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
            t[b, :3, :3] = ry @ rx
            t[b, 1, 3], t[b, 2, 3] = 0.02, 0.05
        inv_k[b] = np.linalg.inv(k[b])
    return inv_k.astype(np.float32), k.astype(np.float32), t.astype(np.float32)


def stereo_depth(batch: int, height: int, width: int, seed: int, lo_px: float = 1.0, hi_px: float = 6.0, pred_type: str = "depth"):
    """A (B,1,H,W) float32 prediction whose stereo shift under stereo_camera's nominal focal length is a smooth field in
    [lo_px, hi_px) pixels plus +-2 % noise: metres for "depth", what depth_from_disparity inverts for "disparity"."""
    import torch
    coarse = torch.from_numpy(hash_uniform((batch, 1, max(2, height // 8), max(2, width // 8)), seed, lo_px, hi_px, np.float64))
    shift = torch.nn.functional.interpolate(coarse, size=(height, width), mode="bilinear", align_corners=True).numpy()
    shift = shift * (1.0 + hash_uniform((batch, 1, height, width), seed + 1, -0.02, 0.02, np.float64))
    depth = STEREO_FOCAL_2048 * width / 2048.0 * STEREO_BASELINE / shift
    if pred_type == "depth":
        return depth.astype(np.float32)
    if pred_type == "disparity":
        return (1.0 + 256.0 * (STEREO_BASELINE * STEREO_FOCAL_2048) / depth).astype(np.float32)
    raise ValueError(pred_type)
