#!/usr/bin/env python3
"""Generate tests/golden/rmi_loss.npz by running the REFERENCE's own RMILoss, RMILossAux and MultiScaleRMILoss on the CPU.

Runs only where the reference tree is present; the fixture it writes is committed.  Nothing from the reference is copied:
its ``rmi.py`` (and the ``rmi_utils.py`` it imports) is imported from where it lies (gen_golden.py's load-by-path recipe, under
a stub package for the relative import) and only inputs / outputs are saved.  The reference converts its stacks with
``.type(torch.cuda.DoubleTensor)``; in this process ``torch.cuda.DoubleTensor`` is ``torch.DoubleTensor``, so it runs on the CPU.

Per case ``c<i>`` of tests/rmi_cases.py (all three classes, do_rmi on and off, lambda_way 0 and 1, pool sizes 1, 2 and 4, pool
ways 0, 1 and 2, radii 1, 2 and 3, one (N,1,H,W) target): ``logits<k>`` of every prediction, ``target``, ``value``, ``grad<k>``
(the gradient of every prediction), and per prediction the loss values of the case's own RMILoss with and without ``do_rmi``
(``full<k>``, ``bce<k>``: the two terms the tests scale their bound with).
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

sys.path.insert(0, os.path.join(gen_golden.REPO, "tests"))
import rmi_cases as cases  # noqa: E402

_RMI_KEYS = ("num_classes", "rmi_radius", "rmi_pool_way", "rmi_pool_size", "rmi_pool_stride", "loss_weight_lambda", "lambda_way",
             "ignore_index")


def _load_reference():
    pkg = types.ModuleType("reference_loss_functions")
    pkg.__path__ = [os.path.join(gen_golden.REF, "loss_functions")]
    sys.modules["reference_loss_functions"] = pkg
    gen_golden._load("reference_loss_functions.rmi_utils", os.path.join(gen_golden.REF, "loss_functions", "rmi_utils.py"))
    return gen_golden._load("reference_loss_functions.rmi", os.path.join(gen_golden.REF, "loss_functions", "rmi.py"))


def main():
    warnings.filterwarnings("ignore")
    torch.cuda.DoubleTensor = torch.DoubleTensor       # this process only
    mod = _load_reference()
    torch.set_num_threads(8)
    out = {}
    for i, (name, shape, kwargs, fwd, _four_d) in enumerate(cases.GOLDEN_CASES):
        xs, t = cases.golden_inputs(i)
        out["c%d_target" % i] = t
        leaves = [torch.from_numpy(x).requires_grad_(True) for x in xs]
        loss = cases.golden_call(getattr(mod, name)(**kwargs), name, fwd, leaves, torch.from_numpy(t))
        grads = torch.autograd.grad(loss, leaves)
        assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
        out["c%d_value" % i] = loss.detach().numpy().copy()
        plain = mod.RMILoss(**{k: v for k, v in kwargs.items() if k in _RMI_KEYS})
        for k, (x, g) in enumerate(zip(xs, grads)):
            out["c%d_logits%d" % (i, k)], out["c%d_grad%d" % (i, k)] = x, g.numpy()
            with torch.no_grad():
                out["c%d_full%d" % (i, k)] = plain(torch.from_numpy(x), torch.from_numpy(t), do_rmi=True).numpy().copy()
                out["c%d_bce%d" % (i, k)] = plain(torch.from_numpy(x), torch.from_numpy(t), do_rmi=False).numpy().copy()
        print("case %d %s %s %s: %.9g" % (i, name, kwargs, fwd, loss.item()))
    path = os.path.join(gen_golden.OUT, "rmi_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
