#!/usr/bin/env python3
"""Generate tests/golden/panoptic.npz by running the REFERENCE's own panoptic post-processing and PanopticMetric on the CPU.

Runs only where the reference tree is present; the fixture it writes is committed.  Nothing from the reference is copied:
``utilities/panoptic_post_processing.py``, ``statistics/base.py`` and ``statistics/panoptic.py`` are imported from where they
lie (the load-by-path recipe of gen_golden.py) and only the seeded inputs of tests/panoptic_cases.py and the reference's
outputs are saved.  Modules that need not be installed here (``h5py``, ``matplotlib``) and the reference's dataset module get
an empty stand-in; the dataset stand-in carries the one attribute the metric reads, its list of thing classes, which is
checked against the reference's source text.  ``PanopticMetric.__init__`` fixes a file name, so the object is made without
it and ``MetricBase.__init__`` is called with ``savefile=""``: no file is touched.  The reference writes into the heat maps
it is given (and through views into the model's outputs): it always gets clones.
"""
import importlib
import os
import sys
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

sys.path.insert(0, os.path.join(gen_golden.REPO, "tests"))
import panoptic_cases as cases  # noqa: E402


def load_reference():
    for name in ("h5py", "matplotlib", "matplotlib.pyplot"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    for name, sub in (("nnet_training", ""), ("nnet_training.statistics", "statistics"), ("nnet_training.utilities", "utilities"),
                      ("nnet_training.datasets", "datasets")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(gen_golden.REF, sub)]
        sys.modules[name] = pkg
    dataset = types.ModuleType("nnet_training.datasets.cityscapes_dataset")
    dataset.CityScapesDataset = type("CityScapesDataset", (), {"cityscapes_things": list(cases.THINGS)})
    with open(os.path.join(gen_golden.REF, "datasets", "cityscapes_dataset.py")) as f:
        assert "cityscapes_things = %s" % list(cases.THINGS) in f.read()
    sys.modules[dataset.__name__] = dataset
    post = gen_golden._load("nnet_training.utilities.panoptic_post_processing",
                            os.path.join(gen_golden.REF, "utilities", "panoptic_post_processing.py"))
    base = gen_golden._load("nnet_training.statistics.base", os.path.join(gen_golden.REF, "statistics", "base.py"))
    metric = gen_golden._load("nnet_training.statistics.panoptic", os.path.join(gen_golden.REF, "statistics", "panoptic.py"))
    return post, base.MetricBase, metric.PanopticMetric


def tensors(d):
    return {k: (torch.from_numpy(v).clone() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def main():
    post, MetricBase, PanopticMetric = load_reference()
    torch.set_num_threads(8)
    tt = lambda a: torch.from_numpy(a).clone()
    out = {}
    for name, shape, seed, kwargs in cases.CENTER_CASES:
        x = cases.center_case_input(name, shape, seed)
        kwargs = dict(kwargs)
        if name == "top_equal":
            kwargs["top_k"] = int(post.find_instance_center(tt(x), nms_kernel=kwargs["nms_kernel"]).shape[0])
            out["ctr_top_equal_k"] = np.int64(kwargs["top_k"])
        given = tt(x)
        ctr = post.find_instance_center(given, **kwargs)
        out["ctr_%s_in" % name], out["ctr_%s_out" % name] = x, ctr.numpy()
        out["ctr_%s_map" % name] = given.numpy().reshape(shape)          # what the reference left in its input
        print("find_instance_center %s %s: %d centres" % (name, kwargs, ctr.shape[0]))
    for name, (H, W), K, kind, seed in cases.GROUP_CASES:
        ctr, off = cases.group_case_input(H, W, K, kind, seed)
        ids = post.group_pixels(tt(ctr), tt(off)).numpy()
        out["grp_%s_ctr" % name], out["grp_%s_off" % name], out["grp_%s_out" % name] = ctr, off, ids
        print("group_pixels %s: ids %s, ties %d" % (name, np.unique(ids).tolist(), cases.ties32(ctr, off[0])))
    # get_instance_segmentation / get_panoptic_segmentation on image 0 of the scene
    pred, tgt = cases.scene()
    sem = torch.argmax(tt(pred["seg"][:1]), dim=1)
    for tag, thing_seg in (("things", None), ("mask", (sem % 2 == 1).to(torch.int64))):
        inst, ctr = post.get_instance_segmentation(sem.clone(), tt(pred["center"][:1]), tt(pred["offset"][:1]), cases.THINGS, nms_kernel=7,
                                                   top_k=100, thing_seg=thing_seg)
        out["inst_%s_out" % tag], out["inst_%s_ctr" % tag] = inst.numpy(), ctr.numpy()
        print("get_instance_segmentation %s: ids %s" % (tag, np.unique(inst.numpy()).tolist()))
    pan, ctr = post.get_panoptic_segmentation(tt(pred["seg"][:1]), tt(pred["center"][:1]), tt(pred["offset"][:1]), cases.THINGS, 1000, 64,
                                              255, nms_kernel=7, top_k=100)
    out["pan_out"], out["pan_ctr"] = pan.numpy(), ctr.numpy()
    print("get_panoptic_segmentation: ids %s" % np.unique(pan.numpy()).tolist())
    for name in cases.PQ_CASES:
        maps = cases.pq_case_maps(name)
        out["pq_%s" % name] = np.asarray(PanopticMetric.calculate_pq(*maps), dtype=np.float64)
        print("calculate_pq %s: %s" % (name, out["pq_%s" % name].tolist()))
    # the reference indexes the target's labels with a (1,H,W) mask: it needs them as (B,1,H,W)
    tgt = dict(tgt, seg=np.ascontiguousarray(tgt["seg"][:, None]))
    quality = PanopticMetric.batch_process_pq(tensors(pred), tensors(tgt))
    for key, value in zip(("pq", "sq", "rq"), quality):
        out["batch_%s" % key] = np.asarray(value, dtype=np.float64)
    metric = PanopticMetric.__new__(PanopticMetric)
    MetricBase.__init__(metric, savefile="", base_dir=Path("."), main_metric="PQ")
    metric._n_classes = 19
    metric._reset_metric()
    metric.add_sample(tensors(pred), tensors(tgt), loss=0.25)
    for key, data in metric.metric_data.items():
        out["sample_%s" % key] = np.asarray([np.asarray(a) for a in data][0])
        print("add_sample %s: %s %s" % (key, out["sample_%s" % key].dtype, out["sample_%s" % key].tolist()))
    path = os.path.join(gen_golden.OUT, "panoptic.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
