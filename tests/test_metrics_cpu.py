"""CPU tests of the training metrics (cerberusnet_amd/statistics/, csrc/metrics.hip): the classes with ``backend='torch'`` on CPU
tensors against results of the reference's own DepthMetric (tests/golden/metrics.npz, written by tools/gen_golden_metrics.py)
and against the numpy restatements of tests/metrics_cases.py, the ``backend='hip'`` fall-back on CPU tensors, the recorded
``metric_data`` and its summaries, and the op / C-ABI layer as far as it goes without a GPU.

Bounds.  Depth against the reference's own numbers: the same stock ops in the same order on the same machine, so 1e-6 relative in
float32 (a few ulp for a different summation blocking) and 1e-12 in float64.  Flow and SAD in float32 against the float64
restatement: 1e-5 relative, the value bound of test_depth_loss_cpu.py's neighbours for sums of a few hundred fp32 terms."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import metrics_cases as cases
from cerberusnet_amd import _lib
from cerberusnet_amd import build as cbuild
from cerberusnet_amd import ops
from cerberusnet_amd import statistics as S
from cerberusnet_amd.statistics import base as SB
from cerberusnet_amd.statistics.depth import KEYS as DEPTH_KEYS
from conftest import REPO

F32_TOL, F64_TOL, RESTATED_TOL = 1e-6, 1e-12, 1e-5


def second_batch(p):
    """The prediction of a golden case's second batch (tools/gen_golden_metrics.py): its rows rolled by half the height."""
    return np.ascontiguousarray(np.roll(p, p.shape[-2] // 2, axis=-2))


def rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(a - ref) / np.abs(ref)))


# ---- depth against the reference's own results ---------------------------------------------------------------------------
def test_the_golden_file_holds_the_inputs_of_the_cases(golden):
    g = golden("metrics")
    for i, (shape, _kwargs) in enumerate(cases.GOLDEN_DEPTH_CASES):
        p, t = cases.golden_depth_inputs(i)
        assert np.array_equal(g["d%d_pred" % i], p) and np.array_equal(g["d%d_gt" % i], t)
        assert p.shape == shape and p.dtype == np.float32 and t.dtype == np.float32 and p.size <= 3 * 12 * 20
        assert (p == 0).any() and (t == 0).any() and (t >= 80).any() and ((t > 0) & (t < 80)).any()
        for tag in ("f32", "f64"):
            for key in ("Batch_Loss",) + DEPTH_KEYS:
                assert g["d%d_%s_%s" % (i, tag, key)].shape == ((2,) if key == "Batch_Loss" else (2, shape[0])), key


@pytest.mark.parametrize("backend", ["torch", "hip"])       # on CPU tensors 'hip' falls back to the stock ops
@pytest.mark.parametrize("i", range(len(cases.GOLDEN_DEPTH_CASES)))
def test_depth_metric_reproduces_the_reference(golden, i, backend):
    g = golden("metrics")
    _, kwargs = cases.GOLDEN_DEPTH_CASES[i]
    for tag, dtype, tol in (("f32", torch.float32, F32_TOL), ("f64", torch.float64, F64_TOL)):
        metric = ca.DepthMetric(backend=backend, **kwargs)
        gt = torch.from_numpy(g["d%d_gt" % i]).to(dtype)
        for k, p in enumerate((g["d%d_pred" % i], second_batch(g["d%d_pred" % i]))):
            pred = torch.from_numpy(p).to(dtype)
            before = pred.clone()
            metric.add_sample({"depth": pred}, {"disparity": gt}, loss=0.5 + k)
            assert torch.equal(pred, before)                       # the reference writes 1e-7 into the zeros
        assert list(metric.metric_data) == ["Batch_Loss"] + list(DEPTH_KEYS)
        for key in DEPTH_KEYS:
            want, got = g["d%d_%s_%s" % (i, tag, key)], np.stack(metric.metric_data[key])
            print("%d %s %s %s: rel %.3e" % (i, backend, tag, key, rel(got, want)))
            assert got.shape == want.shape and got.dtype == want.dtype, (key, got.dtype, want.dtype)
            assert rel(got, want) <= tol, key
        assert metric.metric_data["Batch_Loss"] == [0.5, 1.5]
        # the summaries, by the reference's formulas on the recorded data
        mean, var = metric.get_current_statistics(main_only=False)
        summary = g["d%d_%s_summary" % (i, tag)]
        assert len(mean) == len(var) == 9 and rel(mean, summary[0]) <= 10 * tol and rel(var, summary[1]) <= 1e-4
        assert abs(metric.get_last_batch() - float(g["d%d_%s_last" % (i, tag)])) <= 10 * tol * abs(float(g["d%d_%s_last" % (i, tag)]))
        main, loss = metric.get_current_statistics()[0]
        data = np.concatenate(metric.metric_data[metric.main_metric])
        assert main == data.mean() and loss == 1.0
        assert metric.get_current_statistics(return_loss=False)[1] == (data.var(ddof=1),)
        last = metric.get_last_batch(main_metric=False)
        assert len(last) == 8 and all(a.shape == (g["d%d_pred" % i].shape[0],) for a in last)


def test_depth_metric_layouts_lists_and_images_without_a_valid_pixel():
    p, g = cases.depth_inputs((2, 9, 20))
    g = g.copy()
    g[1] = 0.0                                                      # image 1 has no valid pixel
    want = cases.depth_ref64(p, g)[2]
    for pred in (torch.from_numpy(p), torch.from_numpy(p[:, 0]), [torch.from_numpy(p), torch.zeros(1)]):
        metric = ca.DepthMetric(main_metric="a1")
        metric.add_sample({"depth": pred}, {"disparity": torch.from_numpy(g)})
        for key, ref in zip(DEPTH_KEYS, want):
            got = metric.metric_data[key][0]
            assert got.shape == (2,) and np.isnan(got[1]) and np.isfinite(got[0]) and rel(got[0], ref[0]) <= RESTATED_TOL, key
    assert metric.main_metric == "Batch_a1"


# ---- segmentation against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["torch", "hip"])
@pytest.mark.parametrize("shape,ignore", [((2, 5, 9, 20), 255), ((3, 19, 6, 10), -1), ((1, 70, 5, 8), 255)])
def test_segmentation_metric_against_the_restatement(backend, shape, ignore):
    B, C = shape[:2]
    metric = ca.SegmentationMetric(C, main_metric="IoU", ignore_index=ignore, backend=backend)
    total = np.zeros((C, C), dtype=np.int64)
    for k in range(2):
        x, t = cases.logits(shape, 5000 + 10 * k), cases.labels(shape, 5005 + 10 * k, ignore)
        t.reshape(-1)[3], t.reshape(-1)[7] = C + 2, -7              # out of range and not the ignore label: skipped
        x[0, :, 0, 0] = 1.0                                         # an all-way tie: class 0
        x[0, 2, 0, 1] = np.nan                                      # a NaN logit: class 2
        conf = cases.confusion_ref(x, t, ignore)
        assert conf[0].sum() < t[0].size and conf.sum() > 0
        total += conf.sum(axis=0)
        metric.add_sample({"seg": torch.from_numpy(x)}, {"seg": torch.from_numpy(t)}, loss=float(k))
        acc, iou = cases.seg_metrics_ref(conf)
        assert metric.metric_data["Batch_PixelAcc"][k].shape == (B, 1) and metric.metric_data["Batch_IoU"][k].shape == (B, C)
        assert np.array_equal(metric.metric_data["Batch_PixelAcc"][k], acc)
        assert np.array_equal(metric.metric_data["Batch_IoU"][k], iou, equal_nan=True)
    mat = metric.metric_data["Confusion_Mat"]
    assert isinstance(mat, torch.Tensor) and mat.dtype == torch.int64 and np.array_equal(mat.numpy(), total)
    assert list(metric.metric_data) == ["Batch_Loss", "Batch_PixelAcc", "Batch_IoU", "Confusion_Mat"]
    # the summaries, by the reference's formulas (semantic.py:71-104, :196-211)
    with np.errstate(divide="ignore", invalid="ignore"):
        epoch_iou = np.diag(total) / (total.sum(axis=1) + total.sum(axis=0) - np.diag(total))
    per_image = np.concatenate(metric.metric_data["Batch_IoU"])
    mean, var = metric.get_current_statistics()
    assert mean == (np.nanmean(epoch_iou), 0.5) and var == (np.nanvar(per_image, axis=1).mean(), 0.5)
    mean, var = metric.get_current_statistics(main_only=False, return_loss=False)
    acc_all = np.concatenate(metric.metric_data["Batch_PixelAcc"]).ravel()
    assert mean == (np.nanmean(epoch_iou), acc_all.mean()) and var[1] == acc_all.var(ddof=1)
    assert metric.get_last_batch() == np.nanmean(metric.metric_data["Batch_IoU"][-1])
    assert np.array_equal(metric._confmat_cls_iou(mat), epoch_iou, equal_nan=True)
    assert np.array_equal(metric._confmat_cls_iou(total), epoch_iou, equal_nan=True)
    pr, rc = metric._confmat_cls_pr_rc(total.astype(np.float64) + 1)
    assert np.allclose(pr, np.diag(total + 1) / (total + 1).sum(axis=0)) and np.allclose(rc, np.diag(total + 1) / (total + 1).sum(axis=1))
    metric.print_epoch_statistics()
    metric._reset_metric()
    assert metric.metric_data["Batch_IoU"] == [] and int(metric.metric_data["Confusion_Mat"].sum()) == 0


def test_an_image_with_every_pixel_ignored_gets_nan():
    shape = (2, 5, 4, 6)
    x, t = cases.logits(shape, 5100), cases.labels(shape, 5105)
    t[1] = 255
    metric = ca.SegmentationMetric(5, main_metric="PixelAcc")
    metric.add_sample({"seg": torch.from_numpy(x)}, {"seg": torch.from_numpy(t)})
    acc, iou = metric.metric_data["Batch_PixelAcc"][0], metric.metric_data["Batch_IoU"][0]
    assert np.isnan(acc[1, 0]) and np.isnan(iou[1]).all() and np.isfinite(acc[0, 0])
    assert np.array_equal(metric.get_last_batch(), acc, equal_nan=True)


# ---- flow against the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["torch", "hip"])
@pytest.mark.parametrize("four_d_mask", [False, True])
def test_flow_metric_against_the_restatement(backend, four_d_mask):
    shape = (2, 9, 20)
    fp, fg, mask = cases.flow_inputs(shape)
    img, seq, _ = cases.warp_inputs((2, 3, 9, 20), 5200)
    _, counts, epe, fl = cases.flow_ref64(fp, fg, mask)
    assert counts.min() > 0 and np.array_equal(counts, cases.flow_counts32(fp, fg, mask))
    sad = cases.warp_sad_ref64(img, seq, fp) / (3 * 9 * 20)
    metric = ca.OpticFlowMetric(main_metric="EPE", backend=backend)
    m = torch.from_numpy(mask)[:, None] if four_d_mask else torch.from_numpy(mask)
    targets = {"flow": torch.from_numpy(fg), "flow_mask": m, "l_img": torch.from_numpy(img), "l_seq": torch.from_numpy(seq)}
    metric.add_sample({"flow": [torch.from_numpy(fp), torch.zeros(1)]}, targets, loss=None)
    assert targets["flow_mask"] is m and m.shape == ((2, 1, 9, 20) if four_d_mask else (2, 9, 20))     # not squeezed in place
    assert metric.metric_data["Batch_Loss"] == [0] and list(metric.metric_data) == ["Batch_Loss", "Batch_SAD", "Batch_Fl_all", "Batch_EPE"]
    for key, want in (("Batch_EPE", epe), ("Batch_Fl_all", fl), ("Batch_SAD", sad)):
        got = metric.metric_data[key][0]
        print("%s %s: rel %.3e" % (backend, key, rel(got, want)))
        assert got.shape == (2,) and got.dtype == np.float32 and rel(got, want) <= RESTATED_TOL, key
    # without flow / flow_mask: zeros of the reference's shape, and the SAD
    del targets["flow"]
    metric.add_sample({"flow": torch.from_numpy(fp)}, targets)
    assert all(np.array_equal(metric.metric_data[k][1], np.zeros((2, 1))) for k in ("Batch_EPE", "Batch_Fl_all"))
    assert np.array_equal(metric.metric_data["Batch_SAD"][1], metric.metric_data["Batch_SAD"][0])
    assert metric.get_last_batch() == 0.0 and len(metric.get_last_batch(main_metric=False)) == 3


def test_a_mask_of_zeros_gives_nan_for_that_image_only():
    fp, fg, mask = cases.flow_inputs((2, 9, 20))
    mask = mask.copy()
    mask[0] = 0.0
    img, seq, _ = cases.warp_inputs((2, 3, 9, 20), 5200)
    metric = ca.OpticFlowMetric()
    metric.add_sample({"flow": torch.from_numpy(fp)}, {"flow": torch.from_numpy(fg), "flow_mask": torch.from_numpy(mask),
                                                        "l_img": torch.from_numpy(img), "l_seq": torch.from_numpy(seq)})
    epe, fl = metric.metric_data["Batch_EPE"][0], metric.metric_data["Batch_Fl_all"][0]
    assert np.isnan(epe[0]) and np.isnan(fl[0]) and np.isfinite(epe[1]) and np.isfinite(fl[1])


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_constructors_keep_the_reference_surface():
    for cls, args, main in ((ca.SegmentationMetric, (19,), "IoU"), (ca.DepthMetric, (), "RMSE_Log"), (ca.OpticFlowMetric, (), "SAD")):
        metric = cls(*args, main_metric=main, base_dir="/nonexistent/dir", mode="validation")          # no file is touched
        assert metric.main_metric == "Batch_" + main and metric.mode == "validation" and metric.backend == "hip"
        assert cls(*args, main_metric="Batch_" + main).main_metric == "Batch_" + main and isinstance(metric, ca.MetricBase)
        params = inspect.signature(cls.add_sample).parameters
        assert list(params)[:4] == ["self", "predictions", "targets", "loss"] and params["loss"].default == 0
        with pytest.raises(AssertionError):
            cls(*args, main_metric="NoSuchMetric")
        with pytest.raises(AssertionError):
            cls(*args, main_metric=main, mode="testing")
        with pytest.raises(ValueError):
            cls(*args, main_metric=main, backend="cuda")
        for name in ("get_current_statistics", "get_last_batch", "print_epoch_statistics", "_reset_metric", "_confmat_cls_pr_rc"):
            assert callable(getattr(metric, name))
        assert "h5py" in ca.MetricBase.__doc__ and "ignored" in cls.__doc__ and "differences" in cls.__doc__
    assert not os.path.exists("/nonexistent/dir")


def test_names_are_exported_and_the_source_is_built():
    names = ["MetricBase", "SegmentationMetric", "DepthMetric", "OpticFlowMetric"]
    assert set(names) <= set(S.__all__) and set(names) <= set(ca.__all__)
    for n in names:
        assert getattr(ca, n) is getattr(S, n)
    assert "metrics.hip" in cbuild.SOURCES and "metrics.hip" in cbuild.EXPERIMENT_SOURCES


def test_one_host_copy_per_add_sample(monkeypatch):
    copies = []
    real = SB.host_copy
    for mod in (S.semantic, S.depth, S.optical_flow):
        monkeypatch.setattr(mod, "host_copy", lambda t: (copies.append(tuple(t.shape)), real(t))[1])
    p, g = cases.depth_inputs((2, 9, 20))
    fp, fg, mask = cases.flow_inputs((2, 9, 20))
    img, seq, _ = cases.warp_inputs((2, 3, 9, 20), 5200)
    x, t = cases.logits((2, 5, 9, 20), 5300), cases.labels((2, 5, 9, 20), 5305)
    tt = torch.from_numpy
    ca.DepthMetric().add_sample({"depth": tt(p)}, {"disparity": tt(g)})
    ca.OpticFlowMetric().add_sample({"flow": tt(fp)}, {"flow": tt(fg), "flow_mask": tt(mask), "l_img": tt(img), "l_seq": tt(seq)})
    ca.SegmentationMetric(5).add_sample({"seg": tt(x)}, {"seg": tt(t)})
    assert copies == [(8, 2), (3, 2), (2, 5, 5)]


# ---- the op / C-ABI layer -------------------------------------------------------------------------------------------------------
def test_op_schemas():
    s = lambda n: str(getattr(torch.ops.cerberus, n).default._schema)
    assert s("seg_confusion") == "cerberus::seg_confusion(Tensor logits, Tensor target, int ignore_index) -> Tensor"
    assert s("depth_metric_sums") == ("cerberus::depth_metric_sums(Tensor pred, Tensor gt, float min_depth, float max_depth) -> "
                                      "(Tensor sums, Tensor counts)")
    assert s("flow_metric_sums") == "cerberus::flow_metric_sums(Tensor flow_pred, Tensor flow_gt, Tensor mask) -> (Tensor sums, Tensor counts)"
    assert s("warp_sad") == "cerberus::warp_sad(Tensor image, Tensor source, Tensor flow) -> Tensor"


def test_meta_implementations_give_the_shapes_and_dtypes():
    m = lambda *shape, dtype=torch.float32: torch.empty(*shape, device="meta", dtype=dtype)
    conf = torch.ops.cerberus.seg_confusion(m(2, 19, 5, 7), m(2, 5, 7, dtype=torch.int64), 255)
    assert conf.shape == (2, 19, 19) and conf.dtype == torch.int64 and conf.device.type == "meta"
    for p in (m(3, 1, 5, 7), m(3, 5, 7)):
        sums, counts = torch.ops.cerberus.depth_metric_sums(p, m(3, 5, 7), 0.0, 80.0)
        assert sums.shape == (3, 5) and sums.dtype == torch.float64 and counts.shape == (3, 4) and counts.dtype == torch.int64
    sums, counts = torch.ops.cerberus.flow_metric_sums(m(2, 2, 5, 7), m(2, 2, 5, 7), m(2, 5, 7))
    assert sums.shape == (2, 2) and sums.dtype == torch.float64 and counts.shape == (2, 1) and counts.dtype == torch.int64
    sad = torch.ops.cerberus.warp_sad(m(4, 3, 5, 7), m(4, 3, 5, 7), m(4, 2, 5, 7))
    assert sad.shape == (4,) and sad.dtype == torch.float64 and sad.device.type == "meta"


def test_cpu_tensors_through_the_raw_ops_raise():
    f = lambda *shape: torch.ones(*shape)
    calls = [lambda: torch.ops.cerberus.seg_confusion(f(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), 255),
             lambda: torch.ops.cerberus.depth_metric_sums(f(1, 1, 4, 4), f(1, 4, 4), 0.0, 80.0),
             lambda: torch.ops.cerberus.depth_metric_sums(f(1, 1, 4, 4).requires_grad_(True), f(1, 4, 4), 0.0, 80.0),
             lambda: torch.ops.cerberus.flow_metric_sums(f(1, 2, 4, 4), f(1, 2, 4, 4), f(1, 4, 4)),
             lambda: torch.ops.cerberus.warp_sad(f(1, 3, 4, 4), f(1, 3, 4, 4), f(1, 2, 4, 4))]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


def test_workspace_bytes_in_python_equal_the_library():
    lib = _lib.get()
    pairs = ((ops._depth_metric_workspace_bytes, lib.cerberus_depth_metric_workspace_bytes),
             (ops._flow_metric_workspace_bytes, lib.cerberus_flow_metric_workspace_bytes),
             (ops._warp_sad_workspace_bytes, lib.cerberus_warp_sad_workspace_bytes))
    for shape in ((1, 1, 1), (1, 1, 4), (2, 37, 53), (1, 32, 32), (1, 32, 33), (2, 128, 256), (4, 512, 1024), (2, 1024, 2048),
                  (7, 1025, 31), (0, 8, 8), (-1, 8, 8), (1, 0, 8), (65535, 8, 8), (65536, 8, 8), (1, 46340, 46340), (1, 65536, 32768)):
        for mirror, real in pairs:
            assert mirror(*shape) == real(*shape), (shape, mirror.__name__)
    assert ops._depth_metric_workspace_bytes(2, 32, 33) == 2 * 2 * 56 and ops._flow_metric_workspace_bytes(1, 32, 32) == 20
    assert ops._warp_sad_workspace_bytes(3, 128, 256) == 3 * 32 * 8 and ops._warp_sad_workspace_bytes(1, 65536, 32768) == 0
    assert ops._depth_metric_workspace_bytes(65536, 8, 8) == 0 and ops.SEG_CONFUSION_MAX_CLASSES == 64


def test_argument_rejection_without_gpu():
    lib = _lib.get()
    one = 4096                                                         # never dereferenced: every call below returns before a launch
    big = 1 << 30
    seg = lambda ptrs, B, C, H, W, dtype=0: lib.cerberus_seg_confusion(*ptrs, B, C, H, W, 255, dtype, None)
    dep = lambda ptrs, ws, B, h, w, lo=0.0, hi=80.0, dtype=0: lib.cerberus_depth_metric_sums(*ptrs, ws, B, h, w, lo, hi, dtype, None)
    flo = lambda ptrs, ws, B, H, W, dtype=0: lib.cerberus_flow_metric_sums(*ptrs, ws, B, H, W, dtype, None)
    sad = lambda ptrs, ws, B, C, H, W, dtype=0: lib.cerberus_warp_sad(*ptrs, ws, B, C, H, W, dtype, None)
    # null pointers: CERB_EINVAL, each pointer in turn
    for k in range(3):
        assert seg([one] * k + [None] + [one] * (2 - k), 2, 5, 8, 8) == -1, k
    for k in range(5):
        assert dep([one] * k + [None] + [one] * (4 - k), big, 2, 8, 8) == -1, k
        assert sad([one] * k + [None] + [one] * (4 - k), big, 2, 3, 8, 8) == -1, k
    for k in range(6):
        assert flo([one] * k + [None] + [one] * (5 - k), big, 2, 8, 8) == -1, k
    # dtypes: unknown CERB_EDTYPE, fp16 / bf16 / fp64 CERB_EUNSUPPORTED
    assert seg([None] * 3, 2, 5, 8, 8, 9) == dep([None] * 5, big, 2, 8, 8, dtype=9) == flo([None] * 6, big, 2, 8, 8, 9) == -2
    assert sad([None] * 5, big, 2, 3, 8, 8, 9) == -2
    for dtype in (1, 2, 3):
        assert seg([one] * 3, 2, 5, 8, 8, dtype) == dep([one] * 5, big, 2, 8, 8, dtype=dtype) == -5
        assert flo([one] * 6, big, 2, 8, 8, dtype) == sad([one] * 5, big, 2, 3, 8, 8, dtype) == -5
    # an empty batch: 0, no launch
    assert seg([None] * 3, 0, 5, 8, 8) == dep([None] * 5, 0, 0, 8, 8) == flo([None] * 6, 0, 0, 8, 8) == sad([None] * 5, 0, 0, 3, 8, 8) == 0
    # sizes
    for bad in ((-1, 8, 8), (2, 0, 8), (2, 8, -3)):
        assert seg([one] * 3, bad[0], 5, *bad[1:]) == dep([one] * 5, big, *bad) == flo([one] * 6, big, *bad) == -1, bad
        assert sad([one] * 5, big, bad[0], 3, *bad[1:]) == -1, bad
    assert seg([one] * 3, 2, 1, 8, 8) == -1 and sad([one] * 5, big, 2, 0, 8, 8) == -1                  # too few channels
    assert seg([None] * 3, 2, 64, 8, 8) == -1                     # 64 classes pass the class check: the null pointers are next
    assert seg([None] * 3, 2, 65, 8, 8) == -5                     # CERB_EUNSUPPORTED: the bins do not fit LDS
    assert dep([one] * 5, big, 2, 8, 8, 80.0, 80.0) == -1 and dep([one] * 5, big, 2, 8, 8, float("nan"), 80.0) == -1
    # CERB_ETOOLARGE: the pixel count of an image does not fit an int, the batch does not fit the grid
    for shape in ((1, 65536, 32768), (65536, 8, 8)):
        assert seg([one] * 3, shape[0], 5, *shape[1:]) == dep([one] * 5, 1 << 40, *shape) == flo([one] * 6, 1 << 40, *shape) == -6
        assert sad([one] * 5, 1 << 40, shape[0], 3, *shape[1:]) == -6
    # the workspace: one byte short, misaligned
    for fn, ptrs, need, shape in ((dep, 5, lib.cerberus_depth_metric_workspace_bytes(2, 8, 8), (2, 8, 8)),
                                  (flo, 6, lib.cerberus_flow_metric_workspace_bytes(2, 8, 8), (2, 8, 8)),
                                  (sad, 5, lib.cerberus_warp_sad_workspace_bytes(2, 8, 8), (2, 3, 8, 8))):
        assert need > 0
        assert fn([one] * ptrs, need - 1, *shape) == -1
        assert fn([one] * (ptrs - 1) + [one + 4], need, *shape) == -1


def test_header_and_binding_declare_the_symbols():
    with open(os.path.join(REPO, "include", "cerberus_hip.h")) as f:
        header = f.read()
    for name, nargs in (("cerberus_seg_confusion", 10), ("cerberus_depth_metric_workspace_bytes", 3), ("cerberus_depth_metric_sums", 13),
                        ("cerberus_flow_metric_workspace_bytes", 3), ("cerberus_flow_metric_sums", 12),
                        ("cerberus_warp_sad_workspace_bytes", 3), ("cerberus_warp_sad", 12)):
        m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert "#define CERBERUS_HIP_ABI_VERSION 7 " in header            # additions only
