"""Shared inputs of the Panoptic-DeepLab head's tests: the tiny decoder of tests/golden/pdl_head.npz (tools/gen_golden_pdl.py), and
the shapes, seeded tensors and float64 yardstick of the two fused ops (csrc/pdl_head.hip).

The yardstick is the stock chain in float64 on the CPU -- ``interpolate`` + ``cat`` + ``conv2d`` and its autograd -- computed once
per case and shared (``reference``); nothing writes to what it returns.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from cerberusnet_amd.synth import fill_parameters, hash_uniform
from conftest import l2_err, rel_err  # noqa: F401  (the metrics of every comparison here)

# ---- the tiny decoder of the fixture ---------------------------------------------------------------------------------------------
CONFIG = dict(in_channels=[8, 16, 24], low_level_channels_project=[6, 4], decoder_channels=12, atrous_rates=[1, 2, 3], num_classes=5,
              has_instance=True, instance_low_level_channels_project=[4, 3], instance_decoder_channels=8, instance_aspp_channels=10,
              instance_head_channels=6, instance_num_classes=[1, 2], instance_class_key=["center", "offset"])
FEATURES = [(2, 24, 5, 7), (2, 16, 9, 13), (2, 8, 18, 25)]        # features[1]: low resolution first
OUTPUTS = {"seg": (2, 5, 18, 25), "center": (2, 1, 18, 25), "offset": (2, 2, 18, 25)}
SEED = 1000


def tensor(shape, seed, lo=-1.0, hi=1.0):
    return torch.from_numpy(np.array(hash_uniform(tuple(shape), seed, lo, hi), order="C"))


def features(device="cpu"):
    return [tensor(shape, 51 + i).to(device) for i, shape in enumerate(FEATURES)]


def make_decoder(cls, backend=None, mode="train"):
    """The decoder of ``cls`` with seeded parameters.  ``mode='train'``: BatchNorm uses its batch statistics and only the Dropout
    modules are in ``eval()``, so nothing is random."""
    kwargs = {} if backend is None else {"backend": backend}
    net = cls(**CONFIG, **kwargs)
    fill_parameters(net, SEED)
    net.train(mode == "train")
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    return net


def decoder_loss(pred):
    """One scalar that every output feeds."""
    return sum((pred[k] * pred[k]).mean() for k in ("seg", "center", "offset"))


def run_decoder(net, feats):
    """(outputs, loss, gradients of the features, {parameter: gradient norm}) of one forward + backward."""
    feats = [f.clone().requires_grad_(True) for f in feats]
    pred = net((None, feats))
    loss = decoder_loss(pred)
    loss.backward()
    return pred, loss, [f.grad for f in feats], {n: float(p.grad.double().norm()) for n, p in net.named_parameters()}


# ---- the two ops -----------------------------------------------------------------------------------------------------------------
# (B, Ca, Cb, h, w, H, W); Ca == 0 is the plain op.  The kernel's tile is 32 rows x 64 columns.
SHAPES = {
    "ratios": (2, 5, 3, 5, 7, 9, 13),               # 1: non-integer ratios in both axes
    "one_pixel": (1, 3, 2, 1, 1, 4, 3),             # 2: h = w = 1 (scale 0), an image smaller than the kernel
    "x2_tile_edge": (2, 4, 4, 17, 33, 33, 65),      # 3: exact x2 on 2n+1 grids; one row past a 32-row tile, one column past a 64-wide one
    "wide": (1, 2, 1, 3, 70, 5, 139),               # 4: three tiles in x, few rows, odd width
    "plain": (3, 0, 7, 0, 0, 21, 67),               # 5: the plain op
    "two_tile_rows": (2, 6, 2, 8, 8, 40, 40),       # 6: crosses the tile boundary in y (rows 32..39 are a second tile)
    "identity": (1, 2, 2, 6, 6, 6, 6),              # 7: h == H, the identity upsample
    "one_row": (2, 3, 2, 3, 5, 1, 9),               # 8a: H = 1 (scale_y 0 whatever h is)
    "two_columns": (1, 2, 3, 4, 3, 7, 2),           # 8b: W = 2
    # 9: grad_weight's finishing fold takes 256 partials per (channel, tap) and round; one partial per image and tile
    "fold_one_round": (256, 1, 1, 2, 2, 3, 3),      # 256 images x 1 tile: exactly one round
    "fold_two_rounds": (130, 1, 1, 2, 40, 3, 65),   # 130 images x 2 tiles = 260 partials: a second round
}
PARITY = list(SHAPES)
BOUND = 1e-5            # rel_err of the forward and of every gradient against the float64 chain


def op_inputs(name):
    """(low or None, skip, weight, grad_y): fp32 CPU tensors, uniform in [-1, 1]."""
    B, Ca, Cb, h, w, H, W = SHAPES[name]
    seed = 7000 + 10 * list(SHAPES).index(name)
    low = tensor((B, Ca, h, w), seed) if Ca else None
    return low, tensor((B, Cb, H, W), seed + 1), tensor((Ca + Cb, 1, 5, 5), seed + 2), tensor((B, Ca + Cb, H, W), seed + 3)


def stock_chain(low, skip, weight):
    """The decoder stage's step in stock ops, in the reference's order."""
    x = skip
    if low is not None:
        x = torch.cat((F.interpolate(low, size=skip.shape[2:], mode="bilinear", align_corners=True), skip), dim=1)
    return F.conv2d(x, weight, padding=2, groups=weight.shape[0])


@functools.lru_cache(maxsize=None)
def reference(name):
    """{'y', 'low', 'skip', 'weight'}: the float64 chain's output and gradients on the CPU as numpy arrays ('low' only with Ca > 0)."""
    low, skip, weight, gy = op_inputs(name)
    leaves = {k: t.double().requires_grad_(True) for k, t in (("low", low), ("skip", skip), ("weight", weight)) if t is not None}
    y = stock_chain(leaves.get("low"), leaves["skip"], leaves["weight"])
    grads = torch.autograd.grad(y, list(leaves.values()), grad_outputs=gy.double())
    out = {k: g.numpy() for k, g in zip(leaves, grads)}
    out["y"] = y.detach().numpy()
    return out


def fused(low, skip, weight):
    """The fused op through its differentiable wrapper."""
    import cerberusnet_amd as ca
    return ca.dwconv5x5(skip, weight) if low is None else ca.upcat_dwconv5x5(low, skip, weight)


def run_fused(low, skip, weight, gy, need=(True, True, True)):
    """(y, {'low' | 'skip' | 'weight': gradient}) on the tensors' device; ``need``: which of (low, skip, weight) require a gradient."""
    leaves = {}
    for k, t, n in (("low", low, need[0]), ("skip", skip, need[1]), ("weight", weight, need[2])):
        leaves[k] = None if t is None else t.detach().clone().requires_grad_(bool(n))
    y = fused(leaves["low"], leaves["skip"], leaves["weight"])
    wanted = {k: t for k, t in leaves.items() if t is not None and t.requires_grad}
    grads = torch.autograd.grad(y, list(wanted.values()), grad_outputs=gy)
    return y.detach(), dict(zip(wanted, grads))


def offset_view(t):
    """``t``'s values as a contiguous view at a storage offset of one element: the pointer is 4 bytes past a 16-byte boundary."""
    buf = t.new_empty(t.numel() + 1)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.storage_offset() == 1
    return v
