"""Inputs of the census (ternary) tests, shared by tests/test_census_cpu.py, tests/test_census_gpu.py and the generator of
tests/golden/census.npz (tools/gen_golden_census.py): everything comes from ``hash_uniform`` seeds, so the golden file
holds results only."""
import numpy as np
import torch

from cerberusnet_amd.synth import hash_uniform

FAMILIES = ["noise", "smooth", "unit"]


def _smooth_field(shape, seed, lo=-2.0, hi=2.0):
    B, C, H, W = shape
    coarse = torch.from_numpy(hash_uniform((B, C, max(2, H // 8), max(2, W // 8)), seed, lo, hi))
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).numpy()


def images(shape, family, seed=100):
    """noise / smooth: the families of test_photometric_gpu (two independent uniform fields in [-2, 2); a smooth field +
    small noise against a copy shifted by one column with noise of its own).  unit: an image in [0, 1] and a small
    perturbation of it, clipped to [0, 1]: what a well-warped image is to its target."""
    B, C, H, W = shape
    if family == "noise":
        return hash_uniform(shape, seed, -2.0, 2.0), hash_uniform(shape, seed + 1, -2.0, 2.0)
    if family == "unit":
        im = hash_uniform(shape, seed, 0.0, 1.0)
        return im, np.clip(im + hash_uniform(shape, seed + 1, -0.02, 0.02), 0.0, 1.0).astype(np.float32)
    field = _smooth_field((B, C, H, W + 1), seed)
    im = field[..., :-1] + hash_uniform(shape, seed + 2, -0.02, 0.02)
    im_warp = field[..., 1:] + hash_uniform(shape, seed + 3, -0.02, 0.02)
    return im.astype(np.float32), im_warp.astype(np.float32)


# ---- the golden file ------------------------------------------------------------------------------------------------
GOLDEN_SEED = 500
GOLDEN_CASES = [((2, 3, 16, 24), 1, "unit"), ((1, 3, 19, 23), 1, "smooth"), ((2, 3, 3, 9), 1, "noise"),      # H = 2d + 1
                ((1, 3, 16, 24), 3, "unit"), ((2, 3, 19, 23), 3, "noise"), ((1, 3, 11, 7), 3, "smooth")]     # W = 2d + 1
LOSS_WEIGHTS = (("l1", 0.15), ("ssim", 0.85), ("ternary", 0.5))


def _flows(B, H, W, seed):
    coarse = torch.from_numpy(hash_uniform((B, 2, max(2, H // 8), max(2, W // 8)), seed, -3.0, 3.0))
    up = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    return up + torch.from_numpy(hash_uniform((B, 2, H, W), seed + 1, -0.25, 0.25))


def loss_inputs(dtype=torch.float32):
    """A small whole-loss setup: images in [0, 1] at 64 x 96 and a 4-scale (+ one unused scale) flow pyramid."""
    B, H, W = 2, 64, 96
    l_img = torch.from_numpy(hash_uniform((B, 3, H, W), 601, 0.0, 1.0)).to(dtype)
    l_seq = torch.from_numpy(hash_uniform((B, 3, H, W), 602, 0.0, 1.0)).to(dtype)
    sizes = [(H, W), (H // 2, W // 2), (H // 4, W // 4), (H // 8, W // 8), (H // 16, W // 16)]
    mk = lambda s: [_flows(B, h, w, s + 2 * i).to(dtype).requires_grad_(True) for i, (h, w) in enumerate(sizes)]
    return l_img, l_seq, mk(610), mk(630)
