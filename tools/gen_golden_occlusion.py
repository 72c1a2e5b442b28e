#!/usr/bin/env python3
"""Generate tests/golden/occlusion.npz by running the REFERENCE's own occlusion functions and masked loss_photometric on
the CPU.

Runs only where the reference tree lies (as tools/gen_golden.py, whose import recipe it uses); nothing of the reference is
copied: its module is imported from where it lies and only results are saved.  Inputs come from
``cerberusnet_amd.synth.hash_uniform`` (tests/occlusion_cases.py names the seeds), so the file holds results, not inputs:

  * per case ``c<i>_``: shape, family, ``get_corresponding_map(mesh + flow21)``, ``get_occu_mask_backward(flow21, theta)``
    and ``get_occu_mask_bidirection(flow12, flow21, scale, bias)``;
  * ``p<w>_<mask>``: ``unFlowLoss(weights=...).loss_photometric(a, b, mask)`` for each weight set and mask kind.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import occlusion_cases as cases          # noqa: E402
from gen_golden import import_reference  # noqa: E402


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    _, unflow = import_reference()
    rec = {"n_cases": np.int64(len(cases.GOLDEN_CASES))}
    for i, (shape, family, theta, scale, bias) in enumerate(cases.GOLDEN_CASES):
        f12, f21 = cases.golden_flows(i)
        B, H, W = shape
        cmap = unflow.get_corresponding_map(unflow.mesh_grid(B, H, W).type_as(f21) + f21)
        back = unflow.get_occu_mask_backward(f21, theta=theta)
        bidir = unflow.get_occu_mask_bidirection(f12, f21, scale=scale, bias=bias)
        rec.update({"c%d_shape" % i: np.array(shape), "c%d_family" % i: np.array(family), "c%d_map" % i: cmap.numpy(),
                    "c%d_backward" % i: back.numpy(), "c%d_bidirection" % i: bidir.numpy()})
        print("case %d %s %s: map max %.4g, backward mean %.3f, bidirection mean %.3f" % (
            i, shape, family, float(cmap.max()), float(back.mean()), float(bidir.mean())))
    a, b, masks = cases.photometric_inputs()
    for w, weights in enumerate(cases.LOSS_WEIGHT_SETS):
        mod = unflow.unFlowLoss(weights=dict(weights))
        for kind in cases.MASK_KINDS:
            v = mod.loss_photometric(a, b, masks[kind])
            rec["p%d_%s" % (w, kind)] = v.detach().numpy()
            print("loss_photometric weights %d mask %s: %.9g" % (w, kind, float(v)))
    out = os.path.join(REPO, "tests", "golden", "occlusion.npz")
    np.savez_compressed(out, **rec)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
