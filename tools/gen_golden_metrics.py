#!/usr/bin/env python3
"""Generate tests/golden/metrics.npz by running the REFERENCE's own DepthMetric on the CPU, in float32 and float64.

Runs only where the reference tree is present; the fixture it writes is committed.  Nothing from the reference is copied:
``statistics/base.py`` and ``statistics/depth.py`` are imported from where they lie (the load-by-path recipe of gen_golden.py)
and only inputs and the recorded ``metric_data`` arrays are saved.  ``base.py`` imports modules that need not be installed here
(``h5py``): an empty stand-in module takes the place of each missing one.  ``DepthMetric.__init__`` fixes a file name, so the
object is made without it and ``MetricBase.__init__`` is called with ``savefile=""``: no file is touched.  The reference writes
``+= 1e-7`` into the prediction it is given: it gets a clone.

The reference's SegmentationMetric and OpticFlowMetric need a GPU (``.cuda()``, ``.get_device()``); their yardsticks are the
numpy restatements of tests/metrics_cases.py.

Per case ``d<i>`` of ``metrics_cases.GOLDEN_DEPTH_CASES``: ``pred``, ``gt``, and per precision ``f32`` / ``f64`` one array
``<precision>_<key>`` of shape (2, B) for every ``Batch_*`` key: the case's batch recorded twice (the second time with the two
halves of the prediction's rows swapped, so that the two entries differ).

    python tools/gen_golden_metrics.py --seeds     # print, per shape, the first seed whose inputs keep clear of the thresholds
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
import metrics_cases as cases  # noqa: E402


def second_batch(p):
    """The prediction of a case's second batch: its rows rolled by half the height."""
    return np.ascontiguousarray(np.roll(p, p.shape[-2] // 2, axis=-2))


def load_reference_depth_metric():
    for name in ("h5py", "matplotlib", "matplotlib.pyplot", "scipy", "scipy.stats"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    for name, sub in (("nnet_training", ""), ("nnet_training.statistics", "statistics")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(gen_golden.REF, sub)]
        sys.modules[name] = pkg
    base = gen_golden._load("nnet_training.statistics.base", os.path.join(gen_golden.REF, "statistics", "base.py"))
    depth = gen_golden._load("nnet_training.statistics.depth", os.path.join(gen_golden.REF, "statistics", "depth.py"))
    return base.MetricBase, depth.DepthMetric


def make_metric(MetricBase, DepthMetric, **kwargs):
    metric = DepthMetric.__new__(DepthMetric)
    MetricBase.__init__(metric, savefile="", base_dir=Path("."), **kwargs)
    metric._reset_metric()
    assert metric._path is None and metric.main_metric in metric.metric_data
    return metric


def find_seeds():
    for name, make, start in (("DEPTH_SEEDS", cases.depth_inputs, 3000), ("FLOW_SEEDS", cases.flow_inputs, 4000)):
        found = {}
        for shape in cases.SHAPES + [(2, 9, 20), (3, 12, 20), (3, 5, 7), (3, 37, 53)]:
            for seed in range(start, start + 4000, 10):
                try:
                    make(shape, seed)
                except AssertionError:
                    continue
                found[shape] = seed
                break
        print("%s = %s" % (name, found))


def main():
    if "--seeds" in sys.argv:
        return find_seeds()
    MetricBase, DepthMetric = load_reference_depth_metric()
    torch.set_num_threads(8)
    out = {}
    for i, (_shape, kwargs) in enumerate(cases.GOLDEN_DEPTH_CASES):
        p, g = cases.golden_depth_inputs(i)
        out["d%d_pred" % i], out["d%d_gt" % i] = p, g
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            metric = make_metric(MetricBase, DepthMetric, **kwargs)
            for k, pred in enumerate((p, second_batch(p))):
                given = torch.from_numpy(pred).to(dtype).clone()
                metric.add_sample({"depth": given}, {"disparity": torch.from_numpy(g).to(dtype)}, loss=0.5 + k)
            for key, data in metric.metric_data.items():
                out["d%d_%s_%s" % (i, tag, key)] = np.stack([np.asarray(a) for a in data])
            mean, var = metric.get_current_statistics(main_only=False)
            out["d%d_%s_summary" % (i, tag)] = np.asarray([mean, var], dtype=np.float64)
            out["d%d_%s_last" % (i, tag)] = np.float64(metric.get_last_batch())
            print("case %d %s %s: %s" % (i, kwargs, tag, {k: np.asarray(v[-1]).tolist() for k, v in metric.metric_data.items()}))
    path = os.path.join(gen_golden.OUT, "metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
