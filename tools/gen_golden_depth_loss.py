#!/usr/bin/env python3
"""Generate tests/golden/depth_loss.npz by running the REFERENCE's own InvHuberLoss, ScaleInvariantError and DepthAwareLoss on
the CPU.

Runs only where the reference tree is present; the fixture it writes is committed.  Nothing from the reference is copied:
its ``depth_losses.py`` is imported from where it lies (the load-by-path recipe of gen_golden_depth_recon.py) and only inputs
and outputs are saved.

Per case ``c<i>`` of tests/depth_loss_cases.py: ``pred`` (B,1,h,w) and ``gt`` (B,h,w), then
  InvHuberLoss (one case with weight=0.5, one whose maximum is tied between two pixels): ``f32_value`` / ``f32_grad`` /
      ``f64_value`` / ``f64_grad`` (the gradient of the prediction);
  ScaleInvariantError (lmda 1 and 0.5) and DepthAwareLoss: ``f32_value`` / ``f64_value`` only, taken under ``no_grad`` -- the
      reference's in-place ``disp_pred[disp_pred == 0] += 0.001`` on the output of relu makes its backward raise.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

sys.path.insert(0, os.path.join(gen_golden.REPO, "tests"))
import depth_loss_cases as cases  # noqa: E402


def main():
    gen_golden.import_reference()
    mod = gen_golden._load("nnet_training.loss_functions.depth_losses",
                           os.path.join(gen_golden.REF, "loss_functions", "depth_losses.py"))
    torch.set_num_threads(8)
    out = {}
    for i, (name, _shape, kwargs, _tie) in enumerate(cases.GOLDEN_CASES):
        p, g = cases.golden_inputs(i)
        out["c%d_pred" % i], out["c%d_gt" % i] = p, g
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            pred = torch.from_numpy(p).to(dtype)
            targets = {"disparity": torch.from_numpy(g).to(dtype)}
            fn = getattr(mod, name)(**kwargs)
            if name == "InvHuberLoss":
                pred.requires_grad_(True)
                loss = fn({"depth": pred}, targets)
                grad, = torch.autograd.grad(loss, pred)
                out["c%d_%s_grad" % (i, tag)] = grad.numpy()
            else:
                with torch.no_grad():
                    loss = fn({"depth": pred}, targets)
            assert loss.dtype == dtype and bool(torch.isfinite(loss))
            out["c%d_%s_value" % (i, tag)] = loss.detach().numpy().copy()
            print("case %d %s %s %s: %.12g" % (i, name, kwargs, tag, loss.item()))
    path = os.path.join(gen_golden.OUT, "depth_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
