#!/usr/bin/env python3
"""Generate tests/golden/seg_ohem.npz by running the REFERENCE's own SoftmaxCrossEntropyOHEMLoss and
MixSoftmaxCrossEntropyOHEMLoss on the CPU.

Runs only where the reference tree is present; the fixture it writes is committed.  Nothing from the reference is copied: its
``seg_losses.py`` is imported from where it lies (gen_golden.py's load-by-path recipe) and only inputs / outputs are saved.
The reference ends its selection with ``.cuda()``; ``torch.Tensor.cuda`` is the identity for the duration of the run.  Its
``criterion`` is wrapped to record the target it was given (the rewritten one).  ``use_weight=True`` takes the 19-entry table
of the reference's constructor (so those cases have 19 classes); the weight the criterion held at run time is stored as data,
and the tests pass it back as ``class_weights``.  The aux case calls the
reference's ``_aux_forward(head0, head1, target)``: its ``forward`` wraps the heads in a list of one and cannot take two.

Per case ``c<i>`` of tests/seg_ohem_cases.py: ``value`` (float32), ``kept`` (uint8 (heads,B,H,W): the rewritten target is not
the ignore value), ``grad`` (float32, one per head, stacked), ``weight`` ((C,) float32; ones for use_weight=False).  The inputs
are regenerated from the seeds by the tests.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

sys.path.insert(0, os.path.join(gen_golden.REPO, "tests"))
import seg_ohem_cases as cases  # noqa: E402


def main():
    mod = gen_golden._load("reference_seg_losses", os.path.join(gen_golden.REF, "loss_functions", "seg_losses.py"))
    torch.set_num_threads(8)
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {}
    try:
        for i, (name, shape, kwargs, nheads) in enumerate(cases.GOLDEN_CASES):
            with contextlib.redirect_stdout(io.StringIO()):                 # the constructor prints
                fn = getattr(mod, name)(**kwargs)
            ignore = kwargs.get("ignore_label", kwargs.get("ignore_index"))
            seen, inner = [], fn.criterion

            def recording(predict, target, inner=inner, seen=seen):
                seen.append(target.numpy().copy())
                return inner(predict, target)
            fn.__dict__["criterion"] = recording                           # ahead of the registered child module
            heads = [torch.from_numpy(cases.inputs(shape, h)[0].copy()).requires_grad_(True) for h in range(nheads)]
            target = torch.from_numpy(cases.inputs(shape)[1].copy())
            with contextlib.redirect_stdout(io.StringIO()):                 # 'Labels: n' when min_kept >= num_valid
                loss = fn._aux_forward(*heads, target) if nheads > 1 else fn(heads[0], target)
            grads = torch.autograd.grad(loss, heads)
            assert len(seen) == nheads and bool(torch.isfinite(loss))
            out["c%d_value" % i] = loss.detach().numpy().copy()
            out["c%d_kept" % i] = np.stack([(s != ignore).astype(np.uint8) for s in seen])
            out["c%d_grad" % i] = np.stack([g.numpy() for g in grads])
            w = inner.weight
            out["c%d_weight" % i] = (w.numpy().copy() if w is not None else np.ones(shape[1])).astype(np.float32)
            print("case %d %s %s: %.9g, kept %s" % (i, name, kwargs, loss.item(), [int(s.sum()) for s in out["c%d_kept" % i]]))
    finally:
        torch.Tensor.cuda = real_cuda
    path = os.path.join(gen_golden.OUT, "seg_ohem.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
