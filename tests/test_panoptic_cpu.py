"""CPU tests of the panoptic metric (cerberusnet_amd/utilities/panoptic_post_processing.py, statistics/panoptic.py,
csrc/panoptic.hip): both backends on CPU tensors against results of the reference's own code (tests/golden/panoptic.npz, written
by tools/gen_golden_panoptic.py), the batched building blocks against the per-image functions, the op / C-ABI layer as far as it
goes without a GPU, and the table of what the GPU tests' shapes and seeds cross.

Bounds.  Integer maps and centre lists: exact.  PQ / SQ / RQ and the centre error: 1e-12 relative in float64 (the same float64
operations in the same order).  The offset error: 1e-6 relative (a float32 mean in another blocking, as the seg tests' VALUE_TOL)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import panoptic_cases as cases
from cerberusnet_amd import _lib
from cerberusnet_amd import build as cbuild
from cerberusnet_amd import ops
from cerberusnet_amd import statistics as S
from cerberusnet_amd import utilities as U
from cerberusnet_amd.statistics import panoptic as SP
from cerberusnet_amd.utilities import panoptic_post_processing as pp
from conftest import REPO

BACKENDS = ["torch", "hip"]           # on CPU tensors 'hip' takes the stock ops
F64_TOL, VALUE_TOL = 1e-12, 1e-6
tt = torch.from_numpy


def close(got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    return bool(np.all(np.abs(got[~nan] - want[~nan]) <= tol * np.abs(want[~nan])))


def scene_tensors(four_d_seg=False):
    pred, tgt = cases.scene()
    pred = {k: tt(v) for k, v in pred.items()}
    tgt = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in tgt.items()}
    if four_d_seg:
        tgt["seg"] = tgt["seg"][:, None]
    return pred, tgt


# ---- against the reference's own results -------------------------------------------------------------------------------------------
def test_the_golden_file_holds_the_inputs_of_the_cases(golden):
    g = golden("panoptic")
    for name, shape, seed, _ in cases.CENTER_CASES:
        assert np.array_equal(g["ctr_%s_in" % name], cases.center_case_input(name, shape, seed))
    for name, (H, W), K, kind, seed in cases.GROUP_CASES:
        ctr, off = cases.group_case_input(H, W, K, kind, seed)
        assert np.array_equal(g["grp_%s_ctr" % name], ctr) and np.array_equal(g["grp_%s_off" % name], off, equal_nan=True)
    assert g["ctr_tied_out"].shape == (0, 2) and (cases.center_case_input(*cases.CENTER_CASES[6][:3]) == 1.0).sum() >= 40
    assert g["ctr_top_below_out"].shape[0] < 4 and g["ctr_top_equal_out"].shape[0] == int(g["ctr_top_equal_k"]) - 1
    assert np.isnan(g["pq_nan"]).all() and np.isnan(g["grp_nan_off"]).any()
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "panoptic.npz")) < 300 * 1024


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", cases.CENTER_CASES, ids=[c[0] for c in cases.CENTER_CASES])
def test_find_instance_center_reproduces_the_reference(golden, case, backend):
    g = golden("panoptic")
    name, shape, seed, kwargs = case
    kwargs = dict(kwargs)
    if name == "top_equal":
        kwargs["top_k"] = int(g["ctr_top_equal_k"])
    x = tt(g["ctr_%s_in" % name])
    before = x.clone()
    got = pp.find_instance_center(x, backend=backend, **kwargs)
    assert torch.equal(x, before)                                   # the reference writes the peak map into its input
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), g["ctr_%s_out" % name])
    peaks = pp.center_peaks(x, kwargs.get("threshold", 0.1), kwargs["nms_kernel"], backend)
    assert np.array_equal(peaks.numpy(), g["ctr_%s_map" % name])    # ... and this is that map
    # the batched selection gives the same centres in the same order
    k = kwargs.get("top_k")
    if k is not None:
        ctr, cnt = pp.select_centers(peaks.reshape((1,) + peaks.shape[-2:]), k)
        assert ctr.shape == (1, k, 2) and np.array_equal(ctr[0, :int(cnt[0])].numpy(), g["ctr_%s_out" % name])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", cases.GROUP_CASES, ids=[c[0] for c in cases.GROUP_CASES])
def test_group_pixels_reproduces_the_reference(golden, case, backend):
    g = golden("panoptic")
    name = case[0]
    ctr, off = tt(g["grp_%s_ctr" % name]), tt(g["grp_%s_off" % name])
    before = off.clone()
    got = pp.group_pixels(ctr, off, backend=backend)
    assert got.shape == g["grp_%s_out" % name].shape and np.array_equal(got.numpy(), g["grp_%s_out" % name])
    assert np.array_equal(off.numpy(), before.numpy(), equal_nan=True)
    # the batched form: padded rows and a count
    padded = torch.cat([ctr, torch.tensor([[off.shape[2], 0]] * 3)])[None]
    assert np.array_equal(pp.group_stock(off, padded, torch.tensor([ctr.shape[0]])).numpy(), g["grp_%s_out" % name])
    assert int(pp.group_stock(off, padded, torch.tensor([0])).abs().sum()) == 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_instance_and_panoptic_segmentation_reproduce_the_reference(golden, backend):
    g = golden("panoptic")
    pred, _ = scene_tensors()
    seg, ctr, off = pred["seg"][:1], pred["center"][:1], pred["offset"][:1]
    sem = torch.argmax(seg, dim=1)
    keep = [t.clone() for t in (seg, ctr, off, sem)]
    for tag, thing_seg in (("things", None), ("mask", (sem % 2 == 1).to(torch.int64))):
        inst, centers = pp.get_instance_segmentation(sem, ctr, off, cases.THINGS, nms_kernel=7, top_k=100, thing_seg=thing_seg,
                                                     backend=backend)
        assert np.array_equal(inst.numpy(), g["inst_%s_out" % tag]) and np.array_equal(centers.numpy(), g["inst_%s_ctr" % tag])
    pan, centers = pp.get_panoptic_segmentation(seg, ctr, off, cases.THINGS, 1000, 64, 255, nms_kernel=7, top_k=100, backend=backend)
    assert pan.dtype == torch.int64 and np.array_equal(pan.numpy(), g["pan_out"]) and np.array_equal(centers.numpy(), g["pan_ctr"])
    assert all(torch.equal(a, b) for a, b in zip((seg, ctr, off, sem), keep))
    # no centre at all: zeros and an empty list
    inst, centers = pp.get_instance_segmentation(sem, torch.zeros_like(ctr), off, cases.THINGS, backend=backend)
    assert int(inst.abs().sum()) == 0 and inst.shape == sem.shape and centers.shape == (1, 0, 2)


@pytest.mark.parametrize("name", cases.PQ_CASES)
def test_calculate_pq_reproduces_the_reference(golden, name):
    want = golden("panoptic")["pq_%s" % name]
    maps = cases.pq_case_maps(name)
    keep = [m.copy() for m in maps]
    got = ca.PanopticMetric.calculate_pq(*maps)
    print(name, got, want.tolist())
    assert close(got, want, F64_TOL) and all(np.array_equal(a, b) for a, b in zip(maps, keep))
    # the same numbers from the matrices the device builds (ids are rows, classes outside [0, C) vote as class C)
    pi, ps, ti, ts = maps
    C = 19
    fold = lambda s: np.where((s >= 0) & (s < C), s, C)
    if pi.max() < 8 and ti.max() < 8:
        inter, pc, tc = cases.overlap_ref(pi, ti, fold(ps), fold(ts), 8, C + 1)
        assert close(SP.quality_from_counts(inter[0], pc[0], tc[0]), want, F64_TOL)


@pytest.mark.parametrize("four_d_seg", [False, True])
@pytest.mark.parametrize("backend", BACKENDS)
def test_panoptic_metric_reproduces_the_reference(golden, backend, four_d_seg):
    g = golden("panoptic")
    pred, tgt = scene_tensors(four_d_seg)
    keep = {k: v.clone() for k, v in list(pred.items()) + [("t_" + k, v) for k, v in tgt.items() if isinstance(v, torch.Tensor)]}
    quality = ca.PanopticMetric.batch_process_pq(pred, tgt, backend=backend)
    for key, got in zip(("pq", "sq", "rq"), quality):
        assert close(got, g["batch_%s" % key], F64_TOL), key
    assert close(ca.PanopticMetric.batch_process_center_mse(pred, tgt, backend=backend), g["sample_Batch_Center_MSE"], F64_TOL)
    metric = ca.PanopticMetric(19, backend=backend)
    metric.add_sample(pred, tgt, loss=0.25)
    assert list(metric.metric_data) == ["Batch_Loss", "Batch_Center_MSE", "Batch_Offset_MSE", "Batch_PQ", "Batch_SQ", "Batch_RQ"]
    assert metric.metric_data["Batch_Loss"] == [0.25]
    for key in ("Batch_PQ", "Batch_SQ", "Batch_RQ", "Batch_Center_MSE"):
        print(backend, key, metric.metric_data[key][0], g["sample_" + key])
        assert close(metric.metric_data[key][0], g["sample_" + key], F64_TOL), key
    assert close(metric.metric_data["Batch_Offset_MSE"][0], g["sample_Batch_Offset_MSE"], VALUE_TOL)
    for k, v in keep.items():
        assert torch.equal(v, tgt[k[2:]] if k.startswith("t_") else pred[k]), k
    assert metric.get_last_batch() == np.nanmean(metric.metric_data["Batch_PQ"][-1])
    with pytest.raises(AssertionError):
        metric.add_sample(pred, {k: v for k, v in tgt.items() if k != "center_points"})
    with pytest.raises(AssertionError):
        metric.add_sample({k: v for k, v in pred.items() if k != "offset"}, tgt)


def test_images_without_instances_are_left_out_and_center_points_are_optional(monkeypatch):
    pred, tgt = scene_tensors()
    pred["center"] = pred["center"].clone()
    tgt["center"] = tgt["center"].clone()
    pred["center"][1] = 0.0
    tgt["center"][1] = 0.0                                          # image 1: no centre on either side -> NaN -> left out
    copies, finds = [], []
    real_copy, real_nonzero = SP.host_copy, torch.nonzero
    monkeypatch.setattr(SP, "host_copy", lambda t: (copies.append(tuple(t.shape)), real_copy(t))[1])
    monkeypatch.setattr(SP.torch, "nonzero", lambda *a, **k: (finds.append(1), real_nonzero(*a, **k))[1])
    metric = ca.PanopticMetric(19)
    metric.add_sample(pred, dict(tgt, center_points=[[], []]))
    assert len(copies) == 1 and finds == []
    assert metric.metric_data["Batch_PQ"][0].shape == (1,) and metric.metric_data["Batch_Center_MSE"][0].shape == (0,)
    assert metric.metric_data["Batch_Offset_MSE"][0].shape == (2,)
    metric.add_sample(pred, tgt)
    assert len(copies) == 2 and finds == [1] and metric.metric_data["Batch_Center_MSE"][1].shape == (1,)


# ---- the batched building blocks -----------------------------------------------------------------------------------------------------
def test_select_centers_equals_the_per_image_rule():
    x = np.concatenate([cases.heatmap((1, 1, 20, 30), 500), cases.heatmap((1, 1, 20, 30), 501, step=1.0 / 4),
                        np.zeros((1, 1, 20, 30), np.float32)])
    peaks = pp.peaks_stock(tt(x), 0.1, 3)[:, 0]
    for top_k in (1, 5, 40, 100, 700):
        ctr, cnt = pp.select_centers(peaks, top_k)
        assert ctr.shape == (3, top_k, 2) and ctr.dtype == torch.int64 and cnt.dtype == torch.int64
        for b in range(3):
            want = pp.find_instance_center(tt(x[b:b + 1]), nms_kernel=3, top_k=top_k)
            assert int(cnt[b]) == want.shape[0] < max(top_k, 2) and torch.equal(ctr[b, :want.shape[0]], want), (top_k, b)
            assert (ctr[b, want.shape[0]:, 0] == 20).all()
    assert int(pp.select_centers(peaks, 5)[1][1]) == 0              # coarse steps: the best 5 peaks tie, none is kept


def test_overlap_stock_equals_the_numpy_restatement():
    for shape, (M, C) in (((2, 9, 14), (4, 3)), ((1, 5, 7), (101, 19))):
        maps = cases.id_maps(shape, 600, M, C)
        got = SP.overlap_stock(*[tt(m) for m in maps], M, C)
        want = cases.overlap_ref(*maps, M, C)
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(got, want)) and want[0].sum() < maps[0].size


# ---- the surface -------------------------------------------------------------------------------------------------------------------
REFERENCE_SIGNATURES = {
    "get_semantic_segmentation": ["sem"],
    "find_instance_center": ["ctr_hmp", "threshold", "nms_kernel", "top_k"],
    "group_pixels": ["ctr", "offsets"],
    "get_instance_segmentation": ["sem_seg", "ctr_hmp", "offsets", "thing_list", "threshold", "nms_kernel", "top_k", "thing_seg"],
    "merge_semantic_and_instance": ["sem_seg", "ins_seg", "label_divisor", "thing_list", "stuff_area", "void_label"],
    "get_panoptic_segmentation": ["sem", "ctr_hmp", "offsets", "thing_list", "label_divisor", "stuff_area", "void_label", "threshold",
                                  "nms_kernel", "top_k", "foreground_mask"],
    "compare_centers": ["center_list", "center_heatmap"],
}


def test_signatures_are_the_references_plus_backend():
    for name, params in REFERENCE_SIGNATURES.items():
        sig = inspect.signature(getattr(pp, name))
        assert list(sig.parameters) == params + ["backend"] and sig.parameters["backend"].default == "hip", name
        assert name in pp.__all__
    d = {k: v.default for k, v in inspect.signature(pp.get_panoptic_segmentation).parameters.items()}
    assert (d["threshold"], d["nms_kernel"], d["top_k"], d["foreground_mask"]) == (0.1, 3, None, None)
    sig = inspect.signature(ca.PanopticMetric.__init__)
    assert list(sig.parameters)[:9] == ["self", "num_classes", "main_metric", "mode", "base_dir", "savefile", "thing_list", "backend",
                                        "kwargs"]
    assert list(inspect.signature(ca.PanopticMetric.calculate_pq).parameters) == ["pred_inst", "pred_seg", "target_inst", "target_seg"]
    assert ca.PanopticMetric(19).thing_list == cases.THINGS and ca.PanopticMetric(19, thing_list=[3]).thing_list == [3]
    assert "at most two synchronisations per ``add_sample``, whatever B" in " ".join(ca.PanopticMetric.__doc__.split())
    assert "STRICTLY GREATER" in pp.__doc__ and "never mutated" in pp.__doc__ and "H == 1" in pp.__doc__


def test_value_errors_and_backend_validation():
    x = torch.zeros(2, 1, 4, 4)
    with pytest.raises(ValueError, match="batch size = 1"):
        pp.find_instance_center(x)
    with pytest.raises(ValueError, match="batch size = 1"):
        pp.group_pixels(torch.zeros(1, 2, dtype=torch.int64), torch.zeros(2, 2, 4, 4))
    with pytest.raises(ValueError, match="batch size = 1"):
        pp.get_semantic_segmentation(torch.zeros(2, 3, 4, 4))
    with pytest.raises(ValueError, match="un-supported dimension"):
        pp.get_panoptic_segmentation(torch.zeros(4, 4), x[:1], torch.zeros(1, 2, 4, 4), [1], 1000, 4, 255)
    for fn, args in ((pp.find_instance_center, (x[:1],)), (pp.get_semantic_segmentation, (torch.zeros(1, 3, 4, 4),)),
                     (pp.compare_centers, ([[1, 1]], x[0]))):
        with pytest.raises(ValueError, match="backend"):
            fn(*args, backend="cuda")
    with pytest.raises(ValueError, match="backend"):
        ca.PanopticMetric(19, backend="cuda")
    with pytest.raises(AssertionError):
        ca.PanopticMetric(19, main_metric="NoSuchMetric")


def test_a_one_row_heat_map_works_and_compare_centers_runs(capsys):
    x = torch.tensor([[[[0.0, 0.5, 0.2, 0.0, 0.9, 0.0]]]])
    assert pp.find_instance_center(x, nms_kernel=3).tolist() == [[0, 1], [0, 4]]
    assert pp.find_instance_center(x.reshape(1, 1, 6, 1), nms_kernel=3).tolist() == [[1, 0], [4, 0]]
    heat = torch.zeros(2, 1, 8, 8)
    heat[0, 0, 2, 2], heat[0, 0, 6, 5] = 1.0, 0.8
    before = heat.clone()
    mse, var = pp.compare_centers([[[2, 3], [6, 5]], []], heat)
    assert mse == pytest.approx(0.5) and var == pytest.approx(0.5) and torch.equal(heat, before)
    assert "MSE Between Centers" in capsys.readouterr().out


def test_names_are_exported_and_the_source_is_built():
    assert "PanopticMetric" in S.__all__ and "PanopticMetric" in ca.__all__ and ca.PanopticMetric is S.PanopticMetric
    assert U.panoptic_post_processing is pp and "panoptic_post_processing" in U.__all__
    assert "panoptic.hip" in cbuild.SOURCES and "panoptic.hip" in cbuild.EXPERIMENT_SOURCES
    assert issubclass(ca.PanopticMetric, ca.MetricBase)


# ---- the op / C-ABI layer -----------------------------------------------------------------------------------------------------------
def test_op_schemas():
    s = lambda n: str(getattr(torch.ops.cerberus, n).default._schema)
    assert s("center_peaks") == "cerberus::center_peaks(Tensor heatmap, float threshold, int nms_kernel) -> Tensor"
    assert s("group_pixels") == ("cerberus::group_pixels(Tensor offsets, Tensor centers, Tensor counts, Tensor? sem, int thing_mask) "
                                 "-> Tensor")
    assert s("instance_overlap") == ("cerberus::instance_overlap(Tensor pred_inst, Tensor tgt_inst, Tensor pred_seg, Tensor tgt_seg, "
                                     "int max_ids, int num_classes) -> (Tensor inter, Tensor pred_cls, Tensor tgt_cls)")
    assert all(callable(getattr(ops, n)) for n in ("center_peaks", "group_pixels", "instance_overlap"))


def test_meta_implementations_give_the_shapes_and_dtypes():
    m = lambda *shape, dtype=torch.float32: torch.empty(*shape, device="meta", dtype=dtype)
    for h in (m(2, 1, 5, 7), m(2, 5, 7)):
        out = torch.ops.cerberus.center_peaks(h, 0.1, 7)
        assert out.shape == h.shape and out.dtype == torch.float32 and out.device.type == "meta"
    i64 = torch.int64
    for sem in (None, m(2, 5, 7, dtype=i64)):
        out = torch.ops.cerberus.group_pixels(m(2, 2, 5, 7), m(2, 100, 2, dtype=i64), m(2, dtype=i64), sem, -1)
        assert out.shape == (2, 5, 7) and out.dtype == i64
    inter, pc, tc = ops.instance_overlap(*[m(3, 5, 7, dtype=i64)] * 4, 101, 20)
    assert inter.shape == (3, 101, 101) and pc.shape == tc.shape == (3, 101, 20) and {inter.dtype, pc.dtype, tc.dtype} == {i64}


def test_cpu_tensors_through_the_raw_ops_raise():
    z = lambda *shape: torch.zeros(*shape, dtype=torch.int64)
    calls = [lambda: torch.ops.cerberus.center_peaks(torch.ones(1, 1, 4, 4), 0.1, 3),
             lambda: ops.group_pixels(torch.ones(1, 2, 4, 4), z(1, 3, 2), z(1)),
             lambda: ops.instance_overlap(z(1, 4, 4), z(1, 4, 4), z(1, 4, 4), z(1, 4, 4), 4, 3)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


def test_exported_limits_and_thing_mask():
    lib = _lib.get()
    assert lib.cerberus_center_peaks_max_kernel() == ops.CENTER_PEAKS_MAX_KERNEL == cases.PEAK_MAX_KERNEL >= 7
    assert lib.cerberus_group_pixels_max_centers() == ops.GROUP_PIXELS_MAX_CENTERS == cases.GROUP_MAX_CENTERS >= 1024
    assert lib.cerberus_instance_overlap_max_bins() == ops.INSTANCE_OVERLAP_MAX_BINS == cases.OVERLAP_MAX_BINS
    assert 101 * (101 + 2 * 20) <= ops.INSTANCE_OVERLAP_MAX_BINS and 4 * ops.INSTANCE_OVERLAP_MAX_BINS <= 64 * 1024
    assert ops.thing_mask_of(cases.THINGS) == 0x7F800 and ops.thing_mask_of([0, 63]) == (1 << 63) | 1
    assert ops.thing_mask_of([64]) is None and ops.thing_mask_of([-1]) is None and ops.thing_mask_of([]) == 0
    with open(os.path.join(REPO, "cerberusnet_amd", "csrc", "panoptic.hip")) as f:
        src = f.read()
    assert "#pragma clang fp contract(off)" in src
    for line in ("constexpr int kPeakTileH = %d, kPeakTileW = %d;" % (cases.PEAK_TILE_H, cases.PEAK_TILE_W),
                 "constexpr int kPeakMaxKernel = %d;" % cases.PEAK_MAX_KERNEL, "constexpr int kChunk = kThreads * kQuad;",
                 "constexpr int kCenterChunk = %d;" % cases.CENTER_CHUNK, "constexpr int kGroupMaxCenters = %d;" % cases.GROUP_MAX_CENTERS,
                 "constexpr int kOverlapGroupsPerImage = %d;" % cases.OVERLAP_GROUPS_PER_IMAGE,
                 "constexpr int kOverlapMaxBins = %d;" % cases.OVERLAP_MAX_BINS):
        assert line in src, line


def test_argument_rejection_without_gpu():
    lib = _lib.get()
    one = 4096                                                         # never dereferenced: every call below returns before a launch
    peaks = lambda ptrs, B, H, W, k=7, dtype=0: lib.cerberus_center_peaks(*ptrs, B, H, W, 0.1, k, dtype, None)
    group = lambda ptrs, B, H, W, kmax=100, dtype=0: lib.cerberus_group_pixels(*ptrs, B, H, W, kmax, 0x7F800, dtype, None)
    over = lambda ptrs, B, H, W, M=101, C=20: lib.cerberus_instance_overlap(*ptrs, B, H, W, M, C, None)
    for k in range(2):
        assert peaks([one] * k + [None] + [one] * (1 - k), 2, 8, 8) == -1, k
    for k in (0, 1, 2, 4):
        assert group([one] * k + [None] + [one] * (4 - k), 2, 8, 8) == -1, k
    assert group([None] * 5, 2, 8, 8, 4097) == -5 and group([None, None, None, None, None], 2, 8, 8, 0) == -1
    for k in range(7):
        assert over([one] * k + [None] + [one] * (6 - k), 2, 8, 8) == -1, k
    for bad in (0, 2, 4, 17, -3):                                      # even or out of range: CERB_EINVAL
        assert peaks([one] * 2, 2, 8, 8, bad) == -1, bad
    assert peaks([None] * 2, 2, 8, 8, 15) == -1 and peaks([None] * 2, 0, 8, 8, 15) == 0
    assert peaks([one] * 2, 2, 8, 8, 7, 9) == group([one] * 5, 2, 8, 8, 100, 9) == -2
    for dtype in (1, 2, 3):
        assert peaks([one] * 2, 2, 8, 8, 7, dtype) == group([one] * 5, 2, 8, 8, 100, dtype) == -5
    assert group([None] * 5, 0, 8, 8) == over([None] * 7, 0, 8, 8) == 0
    for bad in ((-1, 8, 8), (2, 0, 8), (2, 8, -3)):
        assert peaks([one] * 2, *bad) == group([one] * 5, *bad) == over([one] * 7, *bad) == -1, bad
    for shape in ((1, 65536, 32768), (65536, 8, 8)):
        assert peaks([one] * 2, *shape) == group([one] * 5, *shape) == over([one] * 7, *shape) == -6
    assert peaks([one] * 2, 1, 16 * 65535 + 1, 1) == -6
    assert over([one] * 7, 2, 8, 8, 0, 3) == over([one] * 7, 2, 8, 8, 4, 0) == -1
    assert over([None] * 7, 2, 8, 8, 101, 20) == -1 and over([None] * 7, 2, 8, 8, 127, 1) == -5 and over([None] * 7, 2, 8, 8, 101, 30) == -5


def test_header_and_binding_declare_the_symbols():
    with open(os.path.join(REPO, "include", "cerberus_hip.h")) as f:
        header = f.read()
    for name, nargs in (("cerberus_center_peaks", 9), ("cerberus_group_pixels", 12), ("cerberus_instance_overlap", 13)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    for name in ("cerberus_center_peaks_max_kernel", "cerberus_group_pixels_max_centers", "cerberus_instance_overlap_max_bins"):
        assert re.search(r"\bint\s+%s\s*\(void\)\s*;" % name, header) and _lib.PROTOTYPES[name][1] == []
    assert "#define CERBERUS_HIP_ABI_VERSION 7 " in header            # additions only


# ---- what the GPU tests' shapes and seeds cross ------------------------------------------------------------------------------------
def test_the_gpu_shapes_cross_every_tile_chunk_and_stride():
    assert cases.crossings() == {"center_peaks: two tiles in both directions", "center_peaks: partial tiles",
                                 "group_pixels: more than one workgroup per image",
                                 "group_pixels: a lane's 4 pixels cross the image's end", "group_pixels: a second centre chunk",
                                 "instance_overlap: the stride past 256 workgroups per image", "instance_overlap: scalar route",
                                 "instance_overlap: vector route", "instance_overlap: more than half the LDS bins"}
    assert {c[0] for c in cases.GROUP_GPU_CASES} == set(cases.GROUP_SHAPES)
    assert {k for c in cases.GROUP_GPU_CASES for k in c[1]} >= set(cases.GROUP_COUNTS)
    assert any(c[1] == [0, 99] for c in cases.GROUP_GPU_CASES)
    assert all(W <= 256 for _, _, W in cases.GROUP_SHAPES)
    assert {(1, 1, 1, 1), (2, 1, 5, 7), (1, 1, 1, 9), (1, 1, 3, 66), (2, 1, 37, 53), (3, 1, 16, 33)} <= set(cases.PEAK_SHAPES)
    assert set(cases.OVERLAP_SHAPES) == {(1, 5, 7), (2, 37, 53), (2, 8, 64), (2, 257, 1024)} and set(cases.OVERLAP_SIZES) == {(2, 2), (101, 19)}


def test_the_gpu_inputs_meet_their_conditions():
    tied = 0
    for shape, counts, kind in cases.GROUP_GPU_CASES:
        ctr, cnt, off = cases.group_gpu_inputs(shape, counts, kind)
        assert ctr.shape == (shape[0], max(max(counts), 1), 2) and off.shape == (shape[0], 2) + shape[1:]
        for b, k in enumerate(counts):
            if k < 2:
                continue
            if kind in ("int", "quarter"):
                assert np.array_equal(off * 4, np.round(off * 4)) and np.abs(off).max() <= 8     # 21 bits at most: exact in fp32
                tied += cases.ties32(ctr[b, :k], off[b])
            if kind == "float":
                inside, _ = cases.band(ctr[b, :k], off[b])
                print(shape, k, "pixels in the band:", int(inside.sum()))
                assert inside.mean() <= cases.FLOAT_BAND_MAX_SHARE
        if kind == "nan":
            assert np.isnan(off).any() and np.isinf(off).any()
    assert tied > 0
    x = cases.heatmap_special((2, 1, 35, 130), 700)
    assert np.isnan(x).any() and np.isinf(x).any() and (x == np.float32(0.1)).any() and (x == 0).any()
    assert (x[0, 0, 8, cases.PEAK_TILE_W - 2:cases.PEAK_TILE_W + 2] == 2.0).all()
    maps = cases.id_maps((2, 37, 53), 800, 101, 19)
    assert maps[0].max() >= 101 and maps[0].min() < 0 and maps[2].max() >= 19 and maps[2].min() < 0 and (maps[0] == 0).mean() > 0.5
