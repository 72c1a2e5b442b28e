#!/usr/bin/env python3
"""Generate tests/golden/census.npz by running the REFERENCE's own TernaryLoss and unFlowLoss on the CPU.

Runs only where the reference tree lies (as tools/gen_golden.py, whose import recipe it uses); nothing of the reference is
copied: its module is imported from where it lies and only results are saved.  Inputs come from
``cerberusnet_amd.synth.hash_uniform`` (tests/census_cases.py names the seeds), so the file holds results, not inputs:

  * per case ``c<i>_``: shape, max_distance, family, the fp32 map ``TernaryLoss(im, im_warp, max_distance)``, its mean and
    the fp32 gradient of that mean with respect to im_warp;
  * ``loss_``: the reference ``unFlowLoss(weights={"l1", "ssim", "ternary"})`` on a small 4-scale flow pyramid: its value
    and the norms of the eight flow gradients.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import census_cases as cases            # noqa: E402
from gen_golden import import_reference  # noqa: E402


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    _, unflow = import_reference()
    rec = {"n_cases": np.int64(len(cases.GOLDEN_CASES))}
    for i, (shape, d, family) in enumerate(cases.GOLDEN_CASES):
        im, im_warp = (torch.from_numpy(a) for a in cases.images(shape, family, cases.GOLDEN_SEED + 10 * i))
        im_warp.requires_grad_(True)
        out = unflow.TernaryLoss(im, im_warp, d)
        mean = out.mean()
        grad, = torch.autograd.grad(mean, im_warp)
        rec.update({"c%d_shape" % i: np.array(shape), "c%d_max_distance" % i: np.int64(d), "c%d_family" % i: np.array(family),
                    "c%d_map" % i: out.detach().numpy(), "c%d_mean" % i: mean.detach().numpy(),
                    "c%d_grad_warp" % i: grad.numpy()})
        print("case %d %s d=%d %s: mean %.9g, |grad| max %.3e" % (i, shape, d, family, float(mean.detach()), float(grad.abs().max())))
    l_img, l_seq, fw, bw = cases.loss_inputs()
    loss_mod = unflow.unFlowLoss(weights=dict(cases.LOSS_WEIGHTS), consistency=True)
    loss = loss_mod({"flow": fw, "flow_b": bw}, {"l_img": l_img, "l_seq": l_seq})
    grads = torch.autograd.grad(loss, fw[:4] + bw[:4])
    rec["loss_value"] = loss.detach().numpy()
    rec["loss_flow_grad_norms"] = np.array([float(g.double().norm()) for g in grads])
    print("unFlowLoss %.9g, flow gradient norms %s" % (float(loss.detach()), rec["loss_flow_grad_norms"]))
    out = os.path.join(REPO, "tests", "golden", "census.npz")
    np.savez_compressed(out, **rec)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
