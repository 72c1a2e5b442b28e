"""Inputs of the photometric (L1 + SSIM) and smoothness tests that are held to the reference, shared by
tests/test_photometric_cpu.py, tests/test_photometric_gpu.py and the generator of tests/golden/photometric.npz
(tools/gen_golden_photometric.py): everything comes from ``hash_uniform`` seeds, so the golden file holds results only."""
import numpy as np
import torch

from cerberusnet_amd.synth import hash_uniform
from census_cases import _flows, _smooth_field, images

FAMILIES = ["noise", "smooth", "unit"]
WEIGHT_PAIRS = [(0.15, 0.85), (1.0, 0.0), (0.0, 1.0)]
DTYPES = (("f32", torch.float32), ("f64", torch.float64))

# ---- photometric: (shape, family); the kernels' tile is 16 rows x 64 columns, the reflected halo 1 forward, 2 backward ---
PHOTO_TILE = (16, 64)
# The seed of case i is PHOTO_SEED + 10 * i.  tools/gen_golden_photometric.py asserts ssim_margin >= SSIM_MARGIN for every
# case (no window's (1 - SSIM) / 2 within that of the clamp's corner at 1); advance PHOTO_SEED until it holds.
PHOTO_SEED = 1500
SSIM_MARGIN = 1e-3
PHOTO_CASES = [((1, 1, 2, 2), "noise"), ((1, 2, 3, 3), "unit"),       # every pixel a reflected border pixel
               ((2, 3, 19, 23), "smooth"),                            # one ragged tile, two items
               ((1, 3, 18, 66), "noise"), ((1, 3, 18, 66), "unit"),   # two pixels beyond a tile seam in both directions
               ((1, 1, 17, 130), "smooth")]                           # three tile columns, the last ragged


def photo_images(i):
    """(im_orig, im_recons) of photometric case i, fp32 numpy."""
    shape, family = PHOTO_CASES[i]
    return images(shape, family, PHOTO_SEED + 10 * i)


def photo_reference(golden, i, tag, l1_weight, ssim_weight):
    """Value and gradients (im_orig, im_recons) of ``l1_weight * L1 mean + ssim_weight * SSIM mean`` of case i as the golden
    file holds them for one dtype.  ``f64``: the two terms combined (the loss is linear in them).  ``f32``: the reference's
    own float32 result, stored for each pair of WEIGHT_PAIRS (``l1``, ``ssim``, and ``mix`` for the pair with both terms)."""
    if tag == "f32":
        assert (l1_weight, ssim_weight) in WEIGHT_PAIRS
        t = "mix" if l1_weight and ssim_weight else "l1" if l1_weight else "ssim"
        return float(golden["p%d_f32_%s" % (i, t)]), [golden["p%d_f32_%s_grad_%s" % (i, t, k)] for k in ("orig", "recons")]
    term = lambda t, key: golden["p%d_%s_%s%s" % (i, tag, t, key)].astype(np.float64)
    mix = lambda key: l1_weight * term("l1", key) + ssim_weight * term("ssim", key)
    return float(mix("")), [mix("_grad_orig"), mix("_grad_recons")]


# ---- smoothness: (flow shape, image channels, degree, alpha, family); the kernels' tile is 4 rows x 64 columns -----------
SMOOTH_TILE = (4, 64)
SMOOTH_SEED = 1700
SMOOTH_CASES = [((1, 2, 2, 2), 3, 1, 0.2, "noise"), ((2, 2, 6, 66), 3, 1, 10.0, "unit"), ((1, 2, 19, 23), 3, 1, 0.2, "smooth"),
                ((1, 2, 3, 3), 3, 2, 10.0, "noise"), ((2, 2, 6, 66), 3, 2, 0.2, "unit"), ((1, 2, 19, 23), 3, 2, 10.0, "smooth"),
                ((1, 3, 9, 70), 1, 2, 0.2, "noise")]


def smooth_inputs(i):
    """(flow, image) of smoothness case i, fp32 numpy.  noise: white +-6 px flow on a white image in [-2, 2); smooth: a
    smooth +-6 px flow + +-0.25 px noise on a smooth image + small noise; unit: the same flow on a white image in [0, 1]."""
    shape, channels, _, _, family = SMOOTH_CASES[i]
    seed = SMOOTH_SEED + 10 * i
    ishape = (shape[0], channels) + shape[2:]
    if family == "noise":
        return hash_uniform(shape, seed, -6.0, 6.0), hash_uniform(ishape, seed + 2, -2.0, 2.0)
    flow = (_smooth_field(shape, seed, -6.0, 6.0) + hash_uniform(shape, seed + 1, -0.25, 0.25)).astype(np.float32)
    if family == "unit":
        return flow, hash_uniform(ishape, seed + 2, 0.0, 1.0)
    return flow, (_smooth_field(ishape, seed + 2) + hash_uniform(ishape, seed + 3, -0.02, 0.02)).astype(np.float32)


# ---- the whole loss: one small setup, three configurations of keywords away from the defaults -------------------------
LOSS_SIZES = [(32, 48), (16, 24), (8, 12), (4, 6), (2, 3)]           # the fifth scale is unused (w_wrp_scales[4] == 0)
LOSS_CONFIGS = {
    "a": dict(weights={"l1": .15, "ssim": .85}, consistency=True, weight=0.5,
              smooth={"degree": 1, "alpha": 10.0, "weighting": 30.0}, w_sm_scales=[1, .5, .25, 0, 0]),
    "b": dict(weights={"l1": 1.0}, consistency=False, weight=1.0, w_wrp_scales=[1, 0, 1, 1, 0]),       # a skipped scale
    "c": dict(weights={"ssim": 1.0, "ternary": 0.5}, consistency=True, weight=1.0, w_sm_scales=[0, 1, 0, 0, 0],
              w_wrp_scales=[0, 1, 1, 1, 0]),                          # the first scale is off: the flow divisor s stays 1
}


def loss_used(name):
    """Indices into ``fw + bw`` (ten flows) of the flows a configuration's loss depends on."""
    cfg = LOSS_CONFIGS[name]
    wrp = cfg.get("w_wrp_scales", [1, 1, 1, 1, 0])
    fw = [i for i in range(5) if wrp[i] != 0]
    return fw + ([5 + i for i in fw] if cfg["consistency"] else [])


def loss_inputs(dtype=torch.float32):
    """(l_img, l_seq, forward flows, backward flows): B = 1, images in [0, 1] at 32 x 48, five flow scales."""
    H, W = LOSS_SIZES[0]
    l_img = torch.from_numpy(hash_uniform((1, 3, H, W), 1901, 0.0, 1.0)).to(dtype)
    l_seq = torch.from_numpy(hash_uniform((1, 3, H, W), 1902, 0.0, 1.0)).to(dtype)
    mk = lambda s: [_flows(1, h, w, s + 2 * i).to(dtype).requires_grad_(True) for i, (h, w) in enumerate(LOSS_SIZES)]
    return l_img, l_seq, mk(1910), mk(1930)
