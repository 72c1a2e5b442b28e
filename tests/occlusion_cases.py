"""Inputs of the occlusion tests, shared by tests/test_occlusion_cpu.py, tests/test_occlusion_gpu.py and the generator of
tests/golden/occlusion.npz (tools/gen_golden_occlusion.py): everything comes from ``hash_uniform`` seeds, so the golden
file holds results only."""
import numpy as np
import torch

from cerberusnet_amd.synth import hash_uniform

FAMILIES = ["independent", "consistent"]


def smooth_field(B, H, W, seed, amp):
    coarse = torch.from_numpy(hash_uniform((B, 2, max(2, H // 8), max(2, W // 8)), seed, -amp, amp))
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)


def noise(B, H, W, seed, amp):
    return torch.from_numpy(hash_uniform((B, 2, H, W), seed, -amp, amp))


def flow_pair(B, H, W, family, seed=900):
    """(flow12, flow21), fp32 (B,2,H,W).  independent: two independent smooth +-6 px fields + +-0.25 px noise.  consistent:
    flow21 = -flow12 + a smooth +-1.5 px disagreement + noise.  noisy: two fields of +-8 px white noise (no two neighbours land
    together).  outward: a smooth field whose amplitude exceeds the map, so sources leave it on every side."""
    if family == "independent":
        return (smooth_field(B, H, W, seed, 6.0) + noise(B, H, W, seed + 1, 0.25),
                smooth_field(B, H, W, seed + 2, 6.0) + noise(B, H, W, seed + 3, 0.25))
    if family == "consistent":
        f12 = smooth_field(B, H, W, seed, 6.0) + noise(B, H, W, seed + 1, 0.25)
        return f12, -f12 + smooth_field(B, H, W, seed + 2, 1.5) + noise(B, H, W, seed + 3, 0.25)
    if family == "noisy":
        return noise(B, H, W, seed, 8.0), noise(B, H, W, seed + 1, 8.0)
    if family == "outward":
        amp = 1.5 * max(H, W)
        return noise(B, H, W, seed, amp), noise(B, H, W, seed + 1, amp)
    raise ValueError(family)


def mesh(B, H, W):
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(B, 1, H, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1).expand(B, 1, H, W)
    return torch.cat([xs, ys], 1)


def collapse_flow(B, H, W, tx, ty):
    """The flow that sends every pixel to (tx, ty): the accumulator's worst case (one cell receives H * W sources)."""
    target = torch.tensor([tx, ty], dtype=torch.float32).view(1, 2, 1, 1)
    return (target - mesh(B, H, W)).contiguous()


def block_collapse_flow(B, H, W, seed):
    """A smooth field in which one block of the map (a quarter of each side) is sent to one pixel."""
    f = smooth_field(B, H, W, seed, 3.0).clone()
    h0, h1, w0, w1 = H // 4, H // 4 + max(1, H // 4), W // 4, W // 4 + max(1, W // 4)
    f[:, :, h0:h1, w0:w1] = collapse_flow(B, H, W, W / 2 + 0.25, H / 2 - 0.5)[:, :, h0:h1, w0:w1]
    return f


# ---- the golden file ------------------------------------------------------------------------------------------------
GOLDEN_SEED = 1200
# (B, H, W), family, theta, scale, bias
GOLDEN_CASES = [((2, 37, 53), "independent", 0.2, 0.01, 0.5), ((1, 19, 23), "consistent", 0.2, 0.01, 0.5),
                ((2, 1, 9), "noisy", 0.2, 0.01, 0.5), ((1, 7, 1), "noisy", 0.2, 0.01, 0.5), ((1, 2, 3), "independent", 0.2, 0.01, 0.5),
                ((2, 3, 2), "consistent", 0.35, 0.05, 0.25), ((1, 24, 40), "outward", 0.2, 0.01, 0.5),
                ((2, 32, 48), "block", 0.5, 0.02, 1.0), ((1, 33, 65), "noisy", 0.6, 0.002, 2.0)]
MASK_KINDS = ["random", "ones", "zeros"]
LOSS_WEIGHT_SETS = [(("l1", 0.15), ("ssim", 0.85)), (("l1", 0.15), ("ssim", 0.85), ("ternary", 0.5))]


def golden_flows(i):
    (B, H, W), family = GOLDEN_CASES[i][:2]
    seed = GOLDEN_SEED + 10 * i
    if family == "block":
        return smooth_field(B, H, W, seed + 5, 3.0), block_collapse_flow(B, H, W, seed)      # the map is built from flow21
    return flow_pair(B, H, W, family, seed)


def photometric_inputs():
    shape = (2, 3, 21, 34)
    a = torch.from_numpy(hash_uniform(shape, 1301, 0.0, 1.0))
    b = torch.from_numpy(np.clip(a.numpy() + hash_uniform(shape, 1302, -0.1, 0.1), 0.0, 1.0).astype(np.float32))
    masks = {"random": torch.from_numpy((hash_uniform((2, 1, 21, 34), 1303, 0.0, 1.0) > 0.4).astype(np.float32)),
             "ones": torch.ones(2, 1, 21, 34), "zeros": torch.zeros(2, 1, 21, 34)}
    return a, b, masks
