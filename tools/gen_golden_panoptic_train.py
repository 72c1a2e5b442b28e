#!/usr/bin/env python3
"""Generate tests/golden/panoptic_train.npz by running the REFERENCE's own PanopticTargetGenerator and DeeplabPanopticLoss on
the CPU, on the inputs of tests/panoptic_train_cases.py.

Runs only where the reference tree is present; the fixture it writes is committed.  Nothing from the reference is copied:
``datasets/cityscapes_panoptic_transform.py`` and ``loss_functions/panoptic_loss.py`` are loaded by path (the recipe of
gen_golden.py) and only their outputs are saved.  The generator works on one image: a batch is one call per image, stacked.
Its list of centres becomes an (S,2) table with NaN in the rows that got none (a row got one if it is a thing with a pixel in
the map -- the order of the list is the order of those rows).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

sys.path.insert(0, os.path.join(gen_golden.REPO, "tests"))
import panoptic_train_cases as cases  # noqa: E402


def load_reference():
    gen = gen_golden._load("ref_cityscapes_panoptic_transform", os.path.join(gen_golden.REF, "datasets", "cityscapes_panoptic_transform.py"))
    loss = gen_golden._load("ref_panoptic_loss", os.path.join(gen_golden.REF, "loss_functions", "panoptic_loss.py"))
    return gen.PanopticTargetGenerator, loss.DeeplabPanopticLoss


def main():
    Generator, Loss = load_reference()
    out = {"numpy_version": np.asarray(np.__version__)}
    for name in cases.TARGET_CASES:
        ids, sid, cat, _crowd, count, segs, kwargs = cases.target_case(name)
        make = Generator(**kwargs)
        per_image = [make(cases.colour(ids[b]), segs[b]) for b in range(ids.shape[0])]
        for item in cases.ITEMS:
            out["tgt_%s_%s" % (name, item)] = np.concatenate([d[item].numpy() for d in per_image], 0)
        points = np.full((ids.shape[0], sid.shape[1], 2), np.nan)
        for b, d in enumerate(per_image):
            rows = [i for i, seg in enumerate(segs[b]) if seg["category_id"] in cases.THINGS and (ids[b] == seg["id"]).any()]
            assert len(rows) == len(d["center_points"]), (name, b)
            for i, pt in zip(rows, d["center_points"]):
                points[b, i] = pt
        out["tgt_%s_points" % name] = points
        print("targets %s %s: %d centres, heat map max %.6f" % (name, ids.shape, int((~np.isnan(points[..., 0])).sum()),
                                                                 out["tgt_%s_center" % name].max()))
    # the drop-in call: the reference's dict of the one-image case, list of centres included
    out["call_big_points"] = np.asarray(Generator(**cases.target_case("big")[6])(cases.colour(cases.target_case("big")[0][0]),
                                                                                  cases.target_case("big")[5][0])["center_points"])
    crit = Loss(weight=1.0, center_weight=cases.CENTER_WEIGHT, offset_weight=cases.OFFSET_WEIGHT)
    cp, ct, cm, op, ot, om = (torch.from_numpy(a.copy()) for a in cases.loss_inputs(cases.GOLDEN_LOSS_SHAPE))
    combos = [("%d%d" % (c, o), cm if c else None, om if o else None) for c, o in cases.MASK_COMBOS]
    combos.append(("empty", torch.zeros_like(cm), torch.zeros_like(om)))
    combos.append(("empty_center", torch.zeros_like(cm), om))
    for tag, mc, mo in combos:
        p = {"center": cp.clone().requires_grad_(True), "offset": op.clone().requires_grad_(True)}
        t = {"center": ct, "offset": ot}
        if mc is not None:
            t["center_mask"] = mc
        if mo is not None:
            t["offset_mask"] = mo
        loss = crit(p, t)
        if torch.is_tensor(loss) and loss.requires_grad:
            loss.backward()
        grads = [torch.zeros_like(v) if v.grad is None else v.grad for v in (p["center"], p["offset"])]
        out["loss_%s" % tag] = np.asarray(float(loss), dtype=np.float32)
        out["loss_%s_gc" % tag], out["loss_%s_go" % tag] = grads[0].numpy(), grads[1].numpy()
        print("loss %s: %.6f" % (tag, float(loss)))
    path = os.path.join(gen_golden.OUT, "panoptic_train.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
