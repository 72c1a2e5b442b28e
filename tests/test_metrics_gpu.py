"""GPU tests of the training metrics (csrc/metrics.hip, cerberusnet_amd/statistics/): the ops ``cerberus::seg_confusion``,
``depth_metric_sums``, ``flow_metric_sums``, ``warp_sad`` and the classes ``SegmentationMetric`` / ``DepthMetric`` /
``OpticFlowMetric`` with ``backend='hip'``.

Yardsticks (tests/metrics_cases.py): integer results -- the confusion matrix, n_valid, the a1 / a2 / a3 counts, the Fl outlier
count -- must EQUAL the numpy restatement (the fp32-comparison counts that of the kernels' fp32 arithmetic; the generators
assert that fp32 and float64 agree on them).  Floating-point results -- the five depth sums, the EPE sum, the SAD and the
finished metrics -- are compared with float64: the relative error of each is at most 4 x max(e_stock, 2^-23), e_stock being the
error of the ``backend='torch'`` fp32 chain run on the GPU in the same test (the bound and floor of tests/test_seg_loss_gpu.py
and test_depth_loss_gpu.py).  For the sums, e_stock is the error of the same sum taken with the chain's own stock ops.
ONE exception: ``Batch_Invariant`` = mean(l^2) - (sum |l| / n)^2 of an image with a SINGLE valid pixel is exactly 0 in float64
and in the fp32 chain, while the float64 finish of the fp32 term l^2 leaves about 1e-8 l^2; there, and only there, its error is
measured against its minuend mean(l^2).  Everywhere else it is held to its own float64 value like every other metric.

Shapes (B,H,W): the smallest at which each route can go wrong.  Scalar route (H*W odd or 2 mod 4, idle lanes): (1,1,1), (1,5,7),
(2,37,53) (2 workgroups per image, a ragged last one), (1,3,66).  Vector route: (1,1,4), (2,8,64), (3,16,33) (odd W: a lane's 4
pixels cross a row).  (2,128,256): 32 workgroups per image, so the per-image partial folds matter; every thread of
``metric_finish_kernel`` still reads at most ONE partial there, and no workgroup of ``seg_confusion_kernel`` takes a second chunk.

Past one round (tests/reduction_cases.py, checked on the CPU by tests/test_reduction_tiers_cpu.py; the last section): (2,257,1024),
vector, and (2,601,1023), scalar: 257 and 601 partials PER IMAGE, two images so that ``first = blockIdx.x * n`` matters, more than
the 256 workgroups per image of ``seg_confusion`` (C = 3 there, C = 2 for ``warp_sad``).  At these sizes no seed keeps every ratio
clear of the thresholds; the generator moves the few predictions that lie near one.  A sum over a whole map could hide one
mis-addressed partial, so image 1 is also given ONE valid depth pixel, and ONE unmasked flow pixel, in the first chunk, in 255,
256, 511, 512 and the last, and labels of one class only in the chunks that ``seg_confusion`` reaches by its stride.  The sums of
image 1 then EQUAL that pixel's fp32 terms (as float64) where a term is made of correctly rounded operations only: |d|/g, d^2/g,
d^2, the EPE and the mask.  The two depth sums that go through ``logf``, l^2 and |l|, are not held to equality, because the
device's ``logf`` need not return numpy's last bit: they are held to float64 by ``check_bound`` at its floor (4 x 2^-23)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cerberusnet_amd as ca
import metrics_cases as cases
import reduction_cases as rc
from cerberusnet_amd.loss_functions.UnFlowLoss import mesh_grid, norm_grid
from cerberusnet_amd.synth import hash_uniform
from cerberusnet_amd.statistics import base as SB
from cerberusnet_amd.statistics.depth import KEYS as DEPTH_KEYS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0
FLOOR = 2.0 ** -23
ROUTE_SHAPES = [(2, 37, 53), (2, 8, 64)]                # one per route, for the tests of a property
ops = torch.ops.cerberus


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def shifted(t):
    """A contiguous copy of ``t`` at a storage offset of one element: 4 bytes (8 for labels) past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 1, device=t.device, dtype=t.dtype)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def check_bound(name, got, stock, ref, scale=None):
    """Every element of ``got`` within FACTOR x max(e_stock, FLOOR) of float64, relative to ``scale`` (default: the reference
    itself).  A NaN reference wants a NaN; a reference of exactly 0 wants exactly 0."""
    got, stock, ref = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, stock, ref))
    scale = np.abs(ref) if scale is None else np.abs(np.asarray(scale, dtype=np.float64).reshape(-1))
    assert got.shape == stock.shape == ref.shape == scale.shape, (name, got.shape, stock.shape, ref.shape)
    for i, (g, s, r, d) in enumerate(zip(got, stock, ref, scale)):
        if np.isnan(r):
            assert np.isnan(g), (name, i, g)
        elif d == 0:
            assert g == 0, (name, i, g)
        else:
            ef, es = abs(g - r) / d, abs(s - r) / d
            print("%s[%d]: float64 %.9e fused rel %.3e stock fp32 rel %.3e ratio %.2f" % (name, i, r, ef, es, ef / max(es, FLOOR)))
            assert ef <= FACTOR * max(es, FLOOR), (name, i, g, s, r)


# ---- segmentation -------------------------------------------------------------------------------------------------------------
def seg_inputs(shape3, C, seed=6000, ignore=255):
    shape = (shape3[0], C) + tuple(shape3[1:])
    return cases.logits(shape, seed), cases.labels(shape, seed + 5, ignore)


def seg_class_results(x, t, ignore=255, backend="hip"):
    metric = ca.SegmentationMetric(x.shape[1], ignore_index=ignore, backend=backend)
    metric.add_sample({"seg": dev(x)}, {"seg": dev(t)})
    return metric.metric_data["Batch_PixelAcc"][0], metric.metric_data["Batch_IoU"][0], metric.metric_data["Confusion_Mat"].numpy()


@pytest.mark.parametrize("C", [2, 5, 19])
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_confusion_matrix_equals_the_restatement(shape, C):
    x, t = seg_inputs(shape, C)
    want = cases.confusion_ref(x, t)
    got = ops.seg_confusion(dev(x), dev(t), 255)
    assert got.shape == (shape[0], C, C) and got.dtype == torch.int64 and np.array_equal(host(got), want)
    acc, iou = cases.seg_metrics_ref(want)
    for backend in ("hip", "torch"):
        a, i, total = seg_class_results(x, t, backend=backend)
        assert np.array_equal(a, acc, equal_nan=True) and np.array_equal(i, iou, equal_nan=True), backend
        assert np.array_equal(total, want.sum(axis=0)), backend
    if x[0, 0].size > 16:
        assert want.sum() > 0 and (t == 255).any()


@pytest.mark.parametrize("shape", ROUTE_SHAPES)
def test_confusion_matrix_corner_decisions(shape):
    C = 5
    x, t = seg_inputs(shape, C)
    n = t[0].size
    # argmax ties at the first, a middle and the last class: the first maximal class wins; a NaN logit is the maximum
    x[0, :, 0, 0] = 7.0
    x[0, [1, 3], 0, 1] = 9.0
    x[0, [2, 4], 0, 2] = 9.0
    x[1, 3, 0, 0], x[1, 4, 0, 0] = np.nan, np.nan
    x[1, 0, 0, 1], x[1, 2, 0, 1] = np.inf, np.nan
    t[0, 0, :3], t[1, 0, :2] = [0, 1, 2], [4, 4]
    pred = np.argmax(x, axis=1)
    assert pred[0, 0, :3].tolist() == [0, 1, 2] and pred[1, 0, :2].tolist() == [3, 2]
    # labels outside [0, C) other than the ignore label: skipped
    t[0].reshape(-1)[[n // 2, n // 2 + 1, n - 1]] = [C, -1, 1 << 40]
    want = cases.confusion_ref(x, t)
    assert np.array_equal(host(ops.seg_confusion(dev(x), dev(t), 255)), want)
    assert want[0, 0, 0] >= 1 and want[0, 1, 1] >= 1 and want[0, 2, 2] >= 1 and want[1, 4, 3] >= 1 and want[1, 4, 2] >= 1
    # an ignore label other than 255: 255 is then out of range, and skipped as well
    t3 = np.where(t == 255, 3, t)
    got = host(ops.seg_confusion(dev(x), dev(t3), 3))
    assert np.array_equal(got, cases.confusion_ref(x, t3, 3)) and got[:, 3].sum() == 0 and got.sum() > 0
    assert np.array_equal(host(ops.seg_confusion(dev(x), dev(t), -100)), want)       # 255 is out of range for 5 classes anyway
    # every pixel of image 1 ignored: a zero matrix, NaN accuracy and IoU for that image only
    t[1] = 255
    a, i, total = seg_class_results(x, t)
    assert np.isnan(a[1, 0]) and np.isnan(i[1]).all() and np.isfinite(a[0, 0]) and np.array_equal(total, want[0])
    assert int(host(ops.seg_confusion(dev(x), dev(t), 255))[1].sum()) == 0


def test_64_classes_run_fused_and_65_take_the_stock_path(monkeypatch):
    shape = (2, 8, 64)
    for C in (64, 65):
        x, t = seg_inputs(shape, C, seed=6100)
        xd, td = dev(x), dev(t)
        want = torch.stack([torch.bincount((C * td[b] + torch.argmax(xd[b], dim=0))[td[b] != 255], minlength=C * C).reshape(C, C)
                            for b in range(shape[0])])                           # the reference's chain, per image
        assert np.array_equal(host(want), cases.confusion_ref(x, t)) and len(np.unique(t)) > 60
        calls = []
        real = torch.ops.cerberus.seg_confusion
        metric = ca.SegmentationMetric(C)
        monkeypatch.setattr(metric, "_fused", lambda *a, _f=metric._fused: (calls.append(_f(*a)), calls[-1])[1])
        metric.add_sample({"seg": xd}, {"seg": td})
        assert calls == [C == 64]
        assert np.array_equal(metric.metric_data["Confusion_Mat"].numpy(), host(want).sum(axis=0))
        if C == 64:
            assert torch.equal(real(xd, td, 255), want)
        else:
            with pytest.raises(RuntimeError, match=r"2\.\.64"):
                real(xd, td, 255)


def test_confusion_matrix_repeats_and_replays_in_a_graph():
    shape, C = (2, 128, 256), 19
    s_x = torch.zeros((shape[0], C) + shape[1:], device=DEV)
    s_t = torch.zeros(shape, device=DEV, dtype=torch.int64)
    x0, t0 = seg_inputs(shape, C, seed=6200)
    s_x.copy_(dev(x0))
    s_t.copy_(dev(t0))
    first = ops.seg_confusion(s_x, s_t, 255)
    assert torch.equal(first, ops.seg_confusion(s_x, s_t, 255)) and np.array_equal(host(first), cases.confusion_ref(x0, t0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            ops.seg_confusion(s_x, s_t, 255)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.seg_confusion(s_x, s_t, 255)
    for k in range(2):
        x, t = seg_inputs(shape, C, seed=6210 + 10 * k)
        s_x.copy_(dev(x))
        s_t.copy_(dev(t))
        graph.replay()                                   # the matrix is zeroed by a kernel node of the call: no accumulation
        torch.cuda.synchronize()
        assert np.array_equal(host(out), cases.confusion_ref(x, t)), k


# ---- depth ------------------------------------------------------------------------------------------------------------------
def depth_class_results(p, g, backend):
    metric = ca.DepthMetric(backend=backend)
    metric.add_sample({"depth": p}, {"disparity": g})
    return [metric.metric_data[k][0] for k in DEPTH_KEYS]


def depth_stock_sums(pd, gd):
    """(B,5) float64: the five sums by the stock chain's own fp32 ops on the GPU, in its operation order (depth.py:35-68)."""
    valid = (gd < cases.MAX_DEPTH) & (gd > cases.MIN_DEPTH)
    pz = torch.where(pd[:, 0] == 0, pd[:, 0] + 1e-7, pd[:, 0])
    difference = (pz - gd).masked_fill(~valid, 0.)
    squared_diff = difference.pow(2)
    log_diff = (torch.log(pz) - torch.log(gd)).masked_fill(~valid, 0.)
    terms = [(difference.abs() / gd).masked_fill(~valid, 0.), (squared_diff / gd).masked_fill(~valid, 0.), squared_diff,
             log_diff.pow(2), log_diff.abs()]
    return np.stack([host(t.sum(dim=(1, 2))).astype(np.float64) for t in terms], axis=1)


def check_depth(name, p, g):
    """Op and class on (p, g) against float64 and the restated counts; returns the op's (sums, counts)."""
    ref_sums, ref_counts, ref_metrics = cases.depth_ref64(p, g)
    assert np.array_equal(ref_counts, cases.depth_counts32(p, g))
    pd, gd = dev(p), dev(g)
    before = pd.clone()
    sums, counts = ops.depth_metric_sums(pd, gd, cases.MIN_DEPTH, cases.MAX_DEPTH)
    assert sums.shape == (p.shape[0], 5) and sums.dtype == torch.float64 and counts.shape == (p.shape[0], 4) and counts.dtype == torch.int64
    assert np.array_equal(host(counts), ref_counts), name
    fused, stock = depth_class_results(pd, gd, "hip"), depth_class_results(pd, gd, "torch")
    assert torch.equal(pd, before)                                   # nothing is written into the prediction
    stock_sums = depth_stock_sums(pd, gd)
    for k, what in enumerate(("sum |d|/g", "sum d^2/g", "sum d^2", "sum l^2", "sum |l|")):
        check_bound("%s %s" % (name, what), host(sums)[:, k], stock_sums[:, k], ref_sums[:, k])
    n = ref_counts[:, 0]
    for key, f, s, r in zip(DEPTH_KEYS, fused, stock, ref_metrics):
        assert f.shape == (p.shape[0],) and f.dtype == np.float64
        scale = None
        if key == "Batch_Invariant":       # its own float64 value, except for an image with one valid pixel (module docstring)
            assert all(r[n == 1] == 0)
            scale = np.where(n == 1, ref_sums[:, 3], np.abs(r))
        check_bound("%s %s" % (name, key), f, s, r, scale=scale)
    return sums, counts


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_depth_statistics_against_float64(shape):
    p, g = cases.depth_inputs(shape)
    if p.size > 16:
        assert (g == 0).any() and (g >= 80).any() and ((g > 0) & (g < 80)).any()
    sums, counts = check_depth("depth %s" % (shape,), p, g)
    # the (B,h,w) layout and a list-valued prediction: the same call
    s3, c3 = ops.depth_metric_sums(dev(p[:, 0]), dev(g), cases.MIN_DEPTH, cases.MAX_DEPTH)
    assert torch.equal(s3, sums) and torch.equal(c3, counts)
    a = depth_class_results([dev(p), torch.zeros(1, device=DEV)], dev(g), "hip")
    b = depth_class_results(dev(p[:, 0]), dev(g), "hip")
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", ROUTE_SHAPES)
def test_depth_corner_decisions(shape):
    # exact zeros in the prediction become 1e-7, out of place
    p, g = cases.depth_inputs(shape, zero_share=0.05)
    assert ((p[:, 0] == 0) & (g > 0) & (g < 80)).sum() > 3
    clean_sums, clean_counts = check_depth("depth %s with zeros" % (shape,), p, g)
    # what gt == 0 and gt >= 80 pixels hold changes no bit
    invalid = np.flatnonzero((g.reshape(-1) == 0) | (g.reshape(-1) >= 80))
    assert (g.reshape(-1)[invalid] == 0).any() and (g.reshape(-1)[invalid] >= 80).any()
    pn = p.copy()
    pn.reshape(-1)[invalid[0::3]], pn.reshape(-1)[invalid[1::3]], pn.reshape(-1)[invalid[2::3]] = np.nan, np.inf, -1e30
    sums, counts = ops.depth_metric_sums(dev(pn), dev(g), cases.MIN_DEPTH, cases.MAX_DEPTH)
    assert torch.equal(sums, clean_sums) and torch.equal(counts, clean_counts) and bool(torch.isfinite(sums).all())
    # a NaN ground truth is an invalid pixel
    valid = np.flatnonzero((g.reshape(-1) > 0) & (g.reshape(-1) < 80))
    gn, gz = g.copy(), g.copy()
    gn.reshape(-1)[valid[3]], gz.reshape(-1)[valid[3]] = np.nan, 0.0
    for a, b in zip(ops.depth_metric_sums(dev(p), dev(gn), 0.0, 80.0), ops.depth_metric_sums(dev(p), dev(gz), 0.0, 80.0)):
        assert torch.equal(a, b)
    # a negative prediction at a valid pixel: NaN log sums for that image, as the reference; the other sums stay finite
    pneg = p.copy()
    pneg.reshape(-1)[valid[0]] = -2.0
    sums = host(ops.depth_metric_sums(dev(pneg), dev(g), 0.0, 80.0)[0])
    assert np.isnan(sums[0, 3:]).all() and np.isfinite(sums[0, :3]).all() and np.isfinite(sums[1]).all()
    # an image without a valid pixel: NaN metrics for it, finite ones for the other
    g0 = g.copy()
    g0[0] = 0.0
    fused = depth_class_results(dev(p), dev(g0), "hip")
    ref = cases.depth_ref64(p, g0)[2]
    for key, f, r in zip(DEPTH_KEYS, fused, ref):
        assert np.isnan(f[0]) and np.isnan(r[0]) and np.isfinite(f[1]), key


# ---- flow ---------------------------------------------------------------------------------------------------------------------
def flow_targets(fg, mask, img, seq):
    return {"flow": dev(fg), "flow_mask": dev(mask), "l_img": dev(img), "l_seq": dev(seq)}


def flow_class_results(fp, targets, backend):
    metric = ca.OpticFlowMetric(backend=backend)
    metric.add_sample({"flow": fp}, targets)
    return [metric.metric_data[k][0] for k in ("Batch_EPE", "Batch_Fl_all", "Batch_SAD")]


def flow_stock_sums(fp, fg, mask, img, seq):
    """The EPE sum and the SAD, (B,) float64 each, by the stock chain's own fp32 ops on the GPU (optical_flow.py:55-57, :68-70
    before the mean)."""
    diff = fp - fg
    epe_sum = torch.sum((diff[:, 0] ** 2 + diff[:, 1] ** 2) ** 0.5 * mask, dim=(1, 2))
    b, _, h, w = seq.shape
    grid = norm_grid(mesh_grid(b, h, w, device=seq.device).type_as(seq) + fp)
    warped = F.grid_sample(seq, grid, mode="bilinear", padding_mode="border", align_corners=False)
    return host(epe_sum).astype(np.float64), host((img - warped).abs().sum(dim=(1, 2, 3))).astype(np.float64)


def check_flow(name, fp, fg, mask, img, seq):
    """Ops and class on these inputs against float64 and the restated count; returns the ops' (sums, counts, sad)."""
    ref_sums, ref_counts, ref_epe, ref_fl = cases.flow_ref64(fp, fg, mask)
    assert np.array_equal(ref_counts, cases.flow_counts32(fp, fg, mask))
    ref_sad = cases.warp_sad_ref64(img, seq, fp)
    per_image = img[0].size
    targets = flow_targets(fg, mask, img, seq)
    sums, counts = ops.flow_metric_sums(dev(fp), dev(fg), dev(mask))
    sad = ops.warp_sad(dev(img), dev(seq), dev(fp))
    B = fp.shape[0]
    assert sums.shape == (B, 2) and sums.dtype == torch.float64 and counts.shape == (B, 1) and counts.dtype == torch.int64
    assert sad.shape == (B,) and sad.dtype == torch.float64
    assert np.array_equal(host(counts), ref_counts), name
    assert np.array_equal(host(sums)[:, 1], ref_sums[:, 1])                  # a sum of zeros and ones: exact
    fused, stock = flow_class_results(dev(fp), targets, "hip"), flow_class_results(dev(fp), targets, "torch")
    stock = [np.asarray(s, dtype=np.float64) for s in stock]
    stock_epe_sum, stock_sad = flow_stock_sums(dev(fp), dev(fg), dev(mask), dev(img), dev(seq))
    check_bound(name + " sum epe", host(sums)[:, 0], stock_epe_sum, ref_sums[:, 0])
    check_bound(name + " sad", host(sad), stock_sad, ref_sad)
    for key, f, s, r in zip(("Batch_EPE", "Batch_Fl_all", "Batch_SAD"), fused, stock, (ref_epe, ref_fl, ref_sad / per_image)):
        assert f.shape == (B,) and f.dtype == np.float64
        check_bound("%s %s" % (name, key), f, s, r)
    # what flow_warp would have written, summed in float64: the same elements, so only the order of a float64 sum differs
    warped = ca.flow_warp(dev(seq), dev(fp))
    direct = host((dev(img) - warped).abs().double().sum(dim=(1, 2, 3)))
    assert np.all(np.abs(host(sad) - direct) <= 1e-12 * np.abs(direct)), (name, host(sad), direct)
    return sums, counts, sad


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_flow_statistics_and_sad_against_float64(shape, C):
    fp, fg, mask = cases.flow_inputs(shape)
    img, seq, _ = cases.warp_inputs((shape[0], C) + tuple(shape[1:]), 7000)
    check_flow("flow %s C=%d" % (shape, C), fp, fg, mask, img, seq)


@pytest.mark.parametrize("shape", ROUTE_SHAPES)
def test_flow_corner_decisions(shape):
    B, H, W = shape
    # flows that sample far outside the image (border padding clamps them): the generator's flows, eight times as long
    # (a power of two: every difference and every error scales exactly, so they keep clear of 3; the ratio does by the assertion)
    fp, fg, mask = (a.copy() for a in cases.flow_inputs(shape))
    img, seq, _ = cases.warp_inputs((B, 3, H, W), 7100)
    far_p, far_g = 8.0 * fp, 8.0 * fg
    e, ratio = cases._flow_terms(far_p, far_g, mask, np.float64)
    assert cases.clear_of(e, (3.0,)) and cases.clear_of(ratio, (0.05,)) and (np.abs(far_p) > W).any()
    check_flow("flow %s far outside" % (shape,), far_p, far_g, mask, img, seq)
    # a mask of all zeros for one image: NaN for it (0 / 0), finite for the other
    mask[0] = 0.0
    targets = flow_targets(fg, mask, img, seq)
    epe, fl, sad = flow_class_results(dev(fp), targets, "hip")
    assert np.isnan(epe[0]) and np.isnan(fl[0]) and np.isfinite(epe[1]) and np.isfinite(fl[1]) and np.isfinite(sad).all()
    sums = host(ops.flow_metric_sums(dev(fp), dev(fg), dev(mask))[0])
    assert sums[0, 0] == 0 and sums[0, 1] == 0
    # a (B,1,H,W) mask keeps its shape, and gives the numbers of the (B,H,W) one; a list-valued prediction takes element 0
    m4 = dev(mask)[:, None]
    targets4 = dict(targets, flow_mask=m4)
    again = flow_class_results([dev(fp), torch.zeros(1, device=DEV)], targets4, "hip")
    assert targets4["flow_mask"] is m4 and m4.shape == (B, 1, H, W)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(again, (epe, fl, sad)))
    # without flow / flow_mask: zeros, as the reference, and the same SAD
    bare = {"l_img": targets["l_img"], "l_seq": targets["l_seq"], "flow_mask": targets["flow_mask"]}
    epe0, fl0, sad0 = flow_class_results(dev(fp), bare, "hip")
    assert np.array_equal(epe0, np.zeros((B, 1))) and np.array_equal(fl0, np.zeros((B, 1))) and np.array_equal(sad0, sad)


# ---- every op: per-image separation, misaligned views, reproducibility, no gradient ----------------------------------------------
def all_ops(x, t, p, g, fp, fg, mask, img, seq):
    """The results of the four ops as one flat list of tensors."""
    return [ops.seg_confusion(x, t, 255), *ops.depth_metric_sums(p, g, 0.0, 80.0), *ops.flow_metric_sums(fp, fg, mask),
            ops.warp_sad(img, seq, fp)]


@functools.lru_cache(maxsize=None)
def op_inputs(shape):
    """Computed once per shape and shared; the arrays are not written to."""
    x, t = seg_inputs(shape, 5, seed=7200)
    p, g = cases.depth_inputs(shape)
    fp, fg, mask = cases.flow_inputs(shape)
    img, seq, _ = cases.warp_inputs((shape[0], 3) + tuple(shape[1:]), 7210)
    return x, t, p, g, fp, fg, mask, img, seq


@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 16, 33), (3, 37, 53)])      # scalar, vector, scalar with two workgroups per image
def test_each_row_equals_the_result_of_that_image_alone(shape):
    arrays = op_inputs(shape)
    full = all_ops(*(dev(a) for a in arrays))
    assert all(not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2]) for a in arrays)     # distinct images
    for b in range(3):
        alone = all_ops(*(dev(a[b:b + 1]) for a in arrays))
        for whole, one in zip(full, alone):
            assert torch.equal(whole[b:b + 1], one), b
    assert float(full[1].abs().sum()) > 0 and int(full[0].sum()) > 0


@pytest.mark.parametrize("shape", [(2, 8, 64), (2, 128, 256)])
def test_a_view_at_an_offset_of_one_element_gives_the_same_results(shape):
    arrays = [dev(a) for a in op_inputs(shape)]
    assert all(a.data_ptr() % 16 == 0 for a in arrays)
    want = all_ops(*arrays)
    moved = [shifted(a) for a in arrays]
    got = all_ops(*moved)
    for k, (a, b) in enumerate(zip(want, got)):
        if a.dtype == torch.int64:
            assert torch.equal(a, b), k                     # the integers are equal
        else:                                               # the bound of the module docstring, with no stock error: the floor
            assert bool(((a - b).abs() <= FACTOR * FLOOR * a.abs()).all()), k
            assert torch.equal(a, b), k                     # and in fact the same bits: only the loads differ between the routes
    # one operand moved at a time
    for k in range(len(arrays)):
        mixed = list(arrays)
        mixed[k] = moved[k]
        for a, b in zip(want, all_ops(*mixed)):
            assert torch.equal(a, b), k


@pytest.mark.parametrize("shape", [(2, 37, 53), (2, 128, 256)])
def test_two_runs_give_the_same_bits(shape):
    arrays = [dev(a) for a in op_inputs(shape)]
    for a, b in zip(all_ops(*arrays), all_ops(*arrays)):
        assert torch.equal(a, b)


def test_the_ops_are_not_differentiable_and_refuse_what_they_do_not_cover():
    x, t, p, g, fp, fg, mask, img, seq = (dev(a) for a in op_inputs((2, 8, 64)))
    for call in (lambda: ops.warp_sad(img, seq, fp.clone().requires_grad_(True)).sum(),
                 lambda: ops.depth_metric_sums(p.clone().requires_grad_(True), g, 0.0, 80.0)[0].sum(),
                 lambda: ops.flow_metric_sums(fp.clone().requires_grad_(True), fg, mask)[0].sum()):
        with pytest.raises(RuntimeError, match="not differentiable"):
            call().backward()
    with pytest.raises(RuntimeError, match="float32"):
        ops.depth_metric_sums(p.half(), g, 0.0, 80.0)
    with pytest.raises(RuntimeError, match="float32"):
        ops.warp_sad(img.double(), seq.double(), fp.double())
    with pytest.raises(RuntimeError, match="int64"):
        ops.seg_confusion(x, t.int(), 255)
    with pytest.raises(RuntimeError, match="mask must be"):
        ops.flow_metric_sums(fp, fg, mask[:, None])
    with pytest.raises(RuntimeError, match=r"pred must be \(B,1,h,w\) or \(B,h,w\)"):
        ops.depth_metric_sums(p.expand(2, 3, 8, 64), g, 0.0, 80.0)
    with pytest.raises(RuntimeError, match="must lie below"):
        ops.depth_metric_sums(p, g, 80.0, 0.0)
    with pytest.raises(RuntimeError):
        ops.warp_sad(img.cpu(), seq, fp)
    # 16-bit and 64-bit tensors take the stock path from the classes: float32 / float64 arrays
    half = depth_class_results(p.half(), g.half(), "hip")
    dbl = depth_class_results(p.double(), g.double(), "hip")
    assert all(a.dtype == np.float32 for a in half) and all(a.dtype == np.float64 for a in dbl[:5])
    ref = cases.depth_ref64(host(p), host(g))[2]
    assert all(np.allclose(a, r, rtol=1e-11) for a, r in zip(dbl[:5], ref[:5]))


# ---- one synchronising copy per add_sample: the device part is capturable ----------------------------------------------------
def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_the_device_part_of_add_sample_replays_in_a_graph(backend, monkeypatch):
    """Everything before the host copy is captured in a graph (a synchronisation would fail the capture) and replayed on other
    inputs; the replayed tensor, copied once and recorded, gives what an eager ``add_sample`` records."""
    shape = (2, 8, 64)
    statics = [torch.zeros_like(dev(a)) for a in op_inputs(shape)]
    x, t, p, g, fp, fg, mask, img, seq = statics
    seg, depth, flow = ca.SegmentationMetric(5, backend=backend), ca.DepthMetric(backend=backend), ca.OpticFlowMetric(backend=backend)
    targets = {"flow": fg, "flow_mask": mask, "l_img": img, "l_seq": seq}
    for s, a in zip(statics, op_inputs(shape)):
        s.copy_(dev(a))
    graphs = [capture(lambda: seg._device_part({"seg": x}, {"seg": t})),
              capture(lambda: depth._device_part({"depth": p}, {"disparity": g})),
              capture(lambda: flow._device_part({"flow": fp}, targets))]
    # other inputs: the same arrays with the two images swapped
    for s, a in zip(statics, op_inputs(shape)):
        s.copy_(dev(a[::-1].copy()))
    for graph, _ in graphs:
        graph.replay()
    torch.cuda.synchronize()
    copies = []
    real = SB.host_copy
    for mod in (ca.statistics.semantic, ca.statistics.depth, ca.statistics.optical_flow):
        monkeypatch.setattr(mod, "host_copy", lambda tensor: (copies.append(1), real(tensor))[1])
    seg._record(real(graphs[0][1]))
    depth._record(real(graphs[1][1][0]), graphs[1][1][1])
    flow._record(real(graphs[2][1][0]), graphs[2][1][1])
    seg.add_sample({"seg": x}, {"seg": t})
    depth.add_sample({"depth": p}, {"disparity": g})
    flow.add_sample({"flow": fp}, targets)
    assert copies == [1, 1, 1]                               # one copy per eager add_sample
    for metric in (seg, depth, flow):
        for key, data in metric.metric_data.items():
            if key.startswith("Batch_") and key != "Batch_Loss":
                assert len(data) == 2 and np.array_equal(data[0], data[1], equal_nan=True), key
                assert np.isfinite(data[0]).any(), key


# ---- past one round of the finish kernels: 257 and 601 partials per image, seg_confusion's stride ---------------------------------
@functools.lru_cache(maxsize=None)
def table_results(shape):
    """The four ops on the whole maps of a table shape, computed once and shared; not written to."""
    return all_ops(*(dev(a) for a in rc.metric_inputs(shape)))


MARKERS = [(shape, k) for shape in rc.METRIC_CASES for k in rc.metric_marker_chunks(shape)]
MARKER_IDS = ["%s-%d" % ("x".join(map(str, s)), k) for s, k in MARKERS]


@pytest.mark.parametrize("shape", rc.METRIC_CASES)
def test_table_shapes_confusion_matrix(shape):
    x, t = rc.metric_inputs(shape)[:2]
    want = cases.confusion_ref(x, t)
    assert np.array_equal(host(table_results(shape)[0]), want) and (want > 0).all()
    for backend in ("hip", "torch"):
        assert np.array_equal(seg_class_results(x, t, backend=backend)[2], want.sum(axis=0)), backend


@pytest.mark.parametrize("shape", rc.METRIC_CASES)
def test_table_shapes_depth_statistics(shape):
    p, g = rc.metric_inputs(shape)[2:4]
    sums, counts = check_depth("depth %s" % (shape,), p, g)
    assert torch.equal(sums, table_results(shape)[1]) and torch.equal(counts, table_results(shape)[2])


@pytest.mark.parametrize("shape", rc.METRIC_CASES)
def test_table_shapes_flow_statistics_and_sad(shape):
    fp, fg, mask, img, seq = rc.metric_inputs(shape)[4:]
    sums, counts, sad = check_flow("flow %s C=%d" % (shape, rc.METRIC_WARP_CHANNELS), fp, fg, mask, img, seq)
    for a, b in zip((sums, counts, sad), table_results(shape)[3:]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape,k", MARKERS, ids=MARKER_IDS)
def test_one_valid_depth_pixel_in_chunk_k_of_image_1(shape, k):
    """Image 1 (so that ``first = blockIdx.x * n`` is not 0) holds ONE valid pixel, inside chunk k: its counts are [1, ...] and
    its sums are that pixel's terms, whichever thread of the finish kernel the chunk's partial falls to."""
    p, g, pixel = rc.depth_metric_marker(shape, k)
    sums, counts = ops.depth_metric_sums(dev(p), dev(g), cases.MIN_DEPTH, cases.MAX_DEPTH)
    want_counts = cases.depth_counts32(p, g)
    assert np.array_equal(host(counts), want_counts) and want_counts[1, 0] == 1
    _, *terms32, _ = cases._depth_terms(p, g, np.float32)
    _, *terms64, _ = cases._depth_terms(p, g, np.float64)
    at = lambda term: float(term[1].reshape(-1)[pixel])
    got = host(sums)[1]
    # |d|/g, d^2/g and d^2 are a subtraction, a product and a division, each correctly rounded: the fp32 term, as float64
    assert got[:3].tolist() == [at(t) for t in terms32[:3]], (got, [at(t) for t in terms32])
    # l^2 and |l| go through logf: the bound of the module docstring with no stock error, i.e. its floor
    ref = [at(t) for t in terms64[3:]]
    check_bound("depth %s chunk %d log terms" % (shape, k), got[3:], ref, ref)
    # image 0 keeps the bits of its full-map result
    assert torch.equal(sums[0], table_results(shape)[1][0]) and torch.equal(counts[0], table_results(shape)[2][0])


@pytest.mark.parametrize("shape,k", MARKERS, ids=MARKER_IDS)
def test_one_unmasked_flow_pixel_in_chunk_k_of_image_1(shape, k):
    fp, fg, mask, pixel = rc.flow_metric_marker(shape, k)
    sums, counts = ops.flow_metric_sums(dev(fp), dev(fg), dev(mask))
    assert host(counts)[1].tolist() == [1] and np.array_equal(host(counts), cases.flow_counts32(fp, fg, mask))
    e32, _ = cases._flow_terms(fp, fg, mask, np.float32)
    # two products, a sum and a square root, each correctly rounded: the fp32 term, as float64
    assert host(sums)[1].tolist() == [float(e32[1].reshape(-1)[pixel]), 1.0], (host(sums)[1], e32[1].reshape(-1)[pixel])
    assert torch.equal(sums[0], table_results(shape)[3][0]) and torch.equal(counts[0], table_results(shape)[4][0])


@pytest.mark.parametrize("shape", rc.METRIC_CASES)
def test_a_class_that_only_strided_chunks_of_image_1_hold(shape):
    x, t, count = rc.confusion_marker(shape)
    want = cases.confusion_ref(x, t)
    got = host(ops.seg_confusion(dev(x), dev(t), 255))
    assert np.array_equal(got[1, 2], want[1, 2]) and int(got[1, 2].sum()) == count > 0
    assert int(got[0, 2].sum()) == 0 and np.array_equal(got, want)


def test_a_table_shape_twice_and_misaligned_gives_the_same_bits():
    shape = rc.case_of("metric", (2, 257, 1024))
    arrays = [dev(a) for a in rc.metric_inputs(shape)]
    assert all(a.data_ptr() % 16 == 0 for a in arrays)
    want = table_results(shape)
    for other in (all_ops(*arrays), all_ops(*(shifted(a) for a in arrays))):
        for k, (a, b) in enumerate(zip(want, other)):
            assert torch.equal(a, b), k


def test_confusion_matrix_with_classes_switched_off():
    """Logits of -inf: leading planes, a middle one, and every plane of a pixel (``torch.argmax`` then gives class 0)."""
    shape, C = (2, 8, 64), 5
    x, t = seg_inputs(shape, C, seed=6300)
    pick = lambda seed: hash_uniform((2, 8, 64), seed, 0.0, 1.0) < 0.3
    x[:, 0][pick(6301)] = -np.inf
    x[:, 1][pick(6302)] = -np.inf
    x[:, 3][pick(6303)] = -np.inf
    x[:, :, 0, :4] = -np.inf
    x[:, 1:, 1, :4] = -np.inf                        # only class 0 finite
    x[:, :-1, 2, :4] = -np.inf                       # only the last class finite
    t[:, :3, :4] = 2
    pred = np.argmax(x, axis=1)
    assert (pred[:, 0, :4] == 0).all() and (pred[:, 1, :4] == 0).all() and (pred[:, 2, :4] == C - 1).all()
    assert torch.equal(torch.argmax(torch.from_numpy(x), dim=1), torch.from_numpy(pred))
    assert (np.isneginf(x[:, 0]) & np.isneginf(x[:, 1])).sum() > 50
    want = cases.confusion_ref(x, t)
    for xin in (dev(x), shifted(dev(x))):            # both routes
        assert np.array_equal(host(ops.seg_confusion(xin, dev(t), 255)), want)
    assert want[0, 2, 0] >= 8 and want[0, 2, C - 1] >= 4
