#!/usr/bin/env python3
"""Generate tests/golden/seg_loss.npz by running the REFERENCE's own FocalLoss2D and SegCrossEntropy on the CPU.

Runs only where the reference tree is present; the fixture it writes is committed.  Nothing from the reference is copied:
its ``seg_losses.py`` is imported from where it lies (gen_golden.py's load-by-path recipe) and only inputs / outputs are saved.
The reference moves its class weights with ``.to(logits.get_device())``, which is -1 for a CPU tensor; ``torch.Tensor.get_device``
returns the tensor's device for the duration of the run.  The float64 results come from the same code with float64 logits and
float64 as the default dtype (the reference builds its weights with ``torch.ones``), also for the duration of the run only.

Per case ``c<i>`` of tests/seg_loss_cases.py (both classes, dynamic_weights on and off, gamma 2 and 0.5, ignore_index 255 and
-1, one (B,1,H,W) target): ``logits``, ``target``, and ``f32_value`` / ``f32_grad`` / ``f64_value`` / ``f64_grad`` (the
gradient of the logits).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

sys.path.insert(0, os.path.join(gen_golden.REPO, "tests"))
import seg_loss_cases as cases  # noqa: E402


def main():
    mod = gen_golden._load("reference_seg_losses", os.path.join(gen_golden.REF, "loss_functions", "seg_losses.py"))
    torch.set_num_threads(8)
    real_get_device, real_dtype = torch.Tensor.get_device, torch.get_default_dtype()
    torch.Tensor.get_device = lambda self: self.device
    out = {}
    try:
        for i, (name, shape, kwargs, _four_d) in enumerate(cases.GOLDEN_CASES):
            x, t = cases.golden_inputs(i)
            out["c%d_logits" % i], out["c%d_target" % i] = x, t
            for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                torch.set_default_dtype(dtype)
                logits = torch.from_numpy(x).to(dtype).requires_grad_(True)
                loss = getattr(mod, name)(**kwargs)({"seg": logits}, {"seg": torch.from_numpy(t)})
                grad, = torch.autograd.grad(loss, logits)
                assert loss.dtype == dtype and bool(torch.isfinite(loss))
                out["c%d_%s_value" % (i, tag)] = loss.detach().numpy().copy()
                out["c%d_%s_grad" % (i, tag)] = grad.numpy()
                print("case %d %s %s %s: %.12g" % (i, name, kwargs, tag, loss.item()))
    finally:
        torch.Tensor.get_device = real_get_device
        torch.set_default_dtype(real_dtype)
    path = os.path.join(gen_golden.OUT, "seg_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
