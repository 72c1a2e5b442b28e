"""GPU tests of the panoptic metric (csrc/panoptic.hip, cerberusnet_amd/utilities/panoptic_post_processing.py,
statistics/panoptic.py): the ops ``cerberus::center_peaks``, ``group_pixels`` and ``instance_overlap`` and the class
``PanopticMetric``.  The yardstick is always the stock restatement run ON THE CPU (``peaks_stock``, ``group_stock`` and the thing
map, ``np.add.at``), never an op's own output.

Bounds.  ``center_peaks`` only compares and ``instance_overlap`` only counts: exact.  ``group_pixels`` with integer and
quarter-pixel offsets on images no wider than 256: every product and sum has at most 21 bits and is exact in fp32, so the ids
are equal including the tied pixels (test_panoptic_cpu.py asserts that ties exist).  With arbitrary fp32 offsets equality is
required outside the band of pixels whose two smallest float64 distances differ by at most 1e-6 relative -- an order of
magnitude above the few fp32 roundings of a distance -- and inside it either of the two ids passes.

The shapes are those of tests/panoptic_cases.py; test_panoptic_cpu.py holds the table of what they cross."""
import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import panoptic_cases as cases
from cerberusnet_amd import ops as cops
from cerberusnet_amd.statistics import panoptic as SP
from cerberusnet_amd.utilities import panoptic_post_processing as pp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ops = torch.ops.cerberus
tt = torch.from_numpy
MASK_ALL = -1


def dev(a):
    return tt(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- center_peaks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.PEAK_SHAPES)
def test_center_peaks_equal_the_stock_chain(shape):
    x = cases.heatmap_special(shape, 700 + shape[-1])
    xd = dev(x)
    for kernel in cases.PEAK_KERNELS:
        for threshold in cases.PEAK_THRESHOLDS:
            want = pp.peaks_stock(tt(x), threshold, kernel).numpy()
            got = ops.center_peaks(xd, threshold, kernel)
            assert got.shape == xd.shape and got.dtype == torch.float32 and same(host(got), want), (kernel, threshold)
            assert same(host(ops.center_peaks(xd[:, 0], threshold, kernel)), want[:, 0])
    assert same(host(xd), x)                                        # the input is never written
    want = pp.peaks_stock(tt(x), 0.1, 3).numpy()
    assert not np.isnan(want).any() and (want == -1).any()
    if x.size > 100:
        assert (want > 0).any() and (x == np.float32(0.1)).any() and not (want == np.float32(0.1)).any()


def test_center_peaks_on_views_kernel_limits_and_backends():
    shape = (2, 1, 35, 130)
    x = cases.heatmap_special(shape, 710)
    want = pp.peaks_stock(tt(x), 0.1, 7).numpy()
    buf = torch.zeros(x.size + 1, device=DEV)
    view = buf[1:].view(shape)                                      # 4 bytes into a larger buffer
    view.copy_(dev(x))
    assert view.data_ptr() % 16 == 4 and same(host(ops.center_peaks(view, 0.1, 7)), want)
    wide = torch.zeros((2, 1, 35, 260), device=DEV)
    wide[..., ::2] = dev(x)
    sliced = wide[..., ::2]                                         # a non-contiguous slice
    assert not sliced.is_contiguous() and same(host(ops.center_peaks(sliced, 0.1, 7)), want)
    assert same(host(wide[..., ::2]), x)
    for kernel in (9, 15):
        assert same(host(ops.center_peaks(dev(x), 0.1, kernel)), pp.peaks_stock(tt(x), 0.1, kernel).numpy()), kernel
    for kernel in (0, 2, 17):
        with pytest.raises(RuntimeError, match="nms_kernel"):
            ops.center_peaks(dev(x), 0.1, kernel)
    assert same(host(pp.center_peaks(dev(x), 0.1, 17)), pp.peaks_stock(tt(x), 0.1, 17).numpy())       # the stock path above the limit
    for backend in ("hip", "torch"):
        got = pp.find_instance_center(dev(x[:1]), nms_kernel=7, top_k=100, backend=backend)
        assert torch.equal(got.cpu(), pp.find_instance_center(tt(x[:1]), nms_kernel=7, top_k=100, backend="torch")), backend
    with pytest.raises(RuntimeError, match="float32"):
        ops.center_peaks(dev(x).double(), 0.1, 7)


# ---- group_pixels -----------------------------------------------------------------------------------------------------------------
def group_want(ctr, cnt, off, sem=None, things=None):
    want = pp.group_stock(tt(off), tt(ctr), tt(cnt))
    if sem is not None:
        want = pp.thing_map(tt(sem), things) * want
    return want.numpy()


@pytest.mark.parametrize("case", cases.GROUP_GPU_CASES, ids=lambda c: "%s-%s-%s" % (c[0], c[1], c[2]))
def test_group_pixels_equal_the_stock_chain(case):
    shape, counts, kind = case
    ctr, cnt, off = cases.group_gpu_inputs(shape, counts, kind)
    want = group_want(ctr, cnt, off)
    got = host(ops.group_pixels(dev(off), dev(ctr), dev(cnt), None, MASK_ALL))
    assert got.shape == shape and got.dtype == np.int64
    if kind == "float":
        for b, k in enumerate(counts):
            inside, two = cases.band(ctr[b, :k], off[b])
            g, w = got[b].reshape(-1), want[b].reshape(-1)
            print("image %d: %d pixels in the band, %d of them differ" % (b, inside.sum(), (g != w)[inside].sum()))
            assert np.array_equal(g[~inside], w[~inside])
            assert np.all((g[inside] == two[0][inside]) | (g[inside] == two[1][inside]))
    else:
        assert np.array_equal(got, want)
    for b, k in enumerate(counts):
        assert got[b].max() <= k and (k == 0 or got[b].min() >= 1)
    # the thing mask: bits 0 and 63, labels 255, -1 and 64
    sem = cases.labels(shape, 900 + shape[1])
    sem[:, 0, :3] = [0, 63, 62]
    for things in ([0, 63], cases.THINGS):
        mask = cops.thing_mask_of(things)
        masked = host(cops.group_pixels(dev(off), dev(ctr), dev(cnt), dev(sem), mask))
        assert np.array_equal(masked, np.where(np.isin(sem, things), got, 0))
        assert (masked[np.isin(sem, [255, -1, 64, 62])] == 0).all()
    if kind != "float":
        assert np.array_equal(host(pp.group_things(dev(off), dev(ctr), dev(cnt), dev(sem), cases.THINGS, "hip")),
                              group_want(ctr, cnt, off, sem, cases.THINGS))


def test_group_pixels_through_the_reference_functions_and_limits():
    shape, counts, kind = cases.GROUP_GPU_CASES[3]                  # (2,37,53), [0, 99], quarter
    ctr, cnt, off = cases.group_gpu_inputs(shape, counts, kind)
    one = tt(ctr[1, :99])
    want = pp.group_pixels(one, tt(off[1:2]), backend="torch")
    for backend in ("hip", "torch"):
        assert torch.equal(pp.group_pixels(one.to(DEV), dev(off[1:2]), backend=backend).cpu(), want), backend
    with pytest.raises(RuntimeError, match="at most 4096"):
        ops.group_pixels(dev(off), torch.zeros((2, 4097, 2), dtype=torch.int64, device=DEV), dev(cnt), None, MASK_ALL)
    with pytest.raises(RuntimeError, match="int64"):
        ops.group_pixels(dev(off), dev(ctr).int(), dev(cnt), None, MASK_ALL)
    empty = ops.group_pixels(dev(off), torch.zeros((2, 0, 2), dtype=torch.int64, device=DEV), dev(cnt), None, MASK_ALL)
    assert empty.shape == shape and int(empty.abs().sum()) == 0


# ---- instance_overlap -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.OVERLAP_SIZES)
@pytest.mark.parametrize("shape", cases.OVERLAP_SHAPES)
def test_instance_overlap_equals_np_add_at(shape, size):
    M, C = size
    maps = cases.id_maps(shape, 800 + shape[2], M, C)
    want = cases.overlap_ref(*maps, M, C)
    got = ops.instance_overlap(*[dev(m) for m in maps], M, C)
    assert [tuple(g.shape) for g in got] == [(shape[0], M, M), (shape[0], M, C), (shape[0], M, C)]
    assert all(g.dtype == torch.int64 and np.array_equal(host(g), w) for g, w in zip(got, want))
    assert 0 < want[0].sum() < maps[0].size and want[1].sum() < want[0].sum()
    # every pixel in one bin; every pixel out of range
    ones = [np.full(shape, M - 1, np.int64), np.full(shape, 1, np.int64), np.full(shape, C - 1, np.int64), np.full(shape, 0, np.int64)]
    inter, pc, tc = (host(g) for g in ops.instance_overlap(*[dev(m) for m in ones], M, C))
    n = shape[1] * shape[2]
    assert (inter[:, M - 1, 1] == n).all() and inter.sum() == shape[0] * n and (pc[:, M - 1, C - 1] == n).all() and (tc[:, 1, 0] == n).all()
    ones[0][:] = M
    assert all(int(g.sum()) == 0 for g in ops.instance_overlap(*[dev(m) for m in ones], M, C))


def test_instance_overlap_on_a_misaligned_view_and_limits():
    shape, (M, C) = (2, 8, 64), (101, 19)
    maps = cases.id_maps(shape, 810, M, C)
    want = cases.overlap_ref(*maps, M, C)
    shifted = []
    for m in maps:
        buf = torch.zeros(m.size + 1, dtype=torch.int64, device=DEV)
        buf[1:].view(shape).copy_(dev(m))
        shifted.append(buf[1:].view(shape))
    assert shifted[0].data_ptr() % 16 == 8
    assert all(np.array_equal(host(g), w) for g, w in zip(ops.instance_overlap(*shifted, M, C), want))
    with pytest.raises(RuntimeError, match="16128"):
        ops.instance_overlap(*shifted, 127, 1)
    with pytest.raises(RuntimeError, match="int64"):
        ops.instance_overlap(shifted[0].int(), *shifted[1:], M, C)


# ---- run to run, graph replay -------------------------------------------------------------------------------------------------------
def test_ops_and_the_device_part_repeat_and_replay_in_one_graph():
    shape = (2, 37, 53)
    B, H, W = shape
    M, C = 101, 19
    metric = ca.PanopticMetric(C)

    def inputs(seed):
        ctr, cnt, off = cases.group_gpu_inputs(shape, [99, 5], "quarter", seed)
        pred = {"seg": np.random.default_rng(seed).random((B, C, H, W)).astype(np.float32), "center": cases.heatmap((B, 1, H, W), seed),
                "offset": off}
        tgt = {"seg": cases.labels(shape, seed + 1), "center": cases.heatmap((B, 1, H, W), seed + 2),
               "offset": cases.offsets(shape, seed + 3, "quarter")}
        return [cases.heatmap_special((B, 1, H, W), seed), off, ctr, cnt, *cases.id_maps(shape, seed, M, C)], pred, tgt

    def run(s, p, t):
        packed, peaks = metric._device_part(p, t)
        return [ops.center_peaks(s[0], 0.1, 7), ops.group_pixels(s[1], s[2], s[3], s[6], 0x7F800),
                *ops.instance_overlap(s[4], s[5], s[6], s[7], M, C), packed, peaks]

    def expected(arrays, pred, tgt):
        x, off, ctr, cnt, pi, ti, ps, ts = arrays
        cpu = ca.PanopticMetric(C, backend="torch")
        packed, peaks = cpu._device_part({k: tt(v) for k, v in pred.items()}, {k: tt(v) for k, v in tgt.items()})
        return [pp.peaks_stock(tt(x), 0.1, 7).numpy(), group_want(ctr, cnt, off, ps, cases.THINGS), *cases.overlap_ref(pi, ti, ps, ts, M, C),
                packed.numpy(), peaks.numpy()]

    def check(outs, want, tag):
        for i, (o, w) in enumerate(zip(outs, want)):
            o = host(o)
            if i == 5:                                              # the packed rows: the last column holds float64 bits
                assert np.array_equal(o[:, :-1], w[:, :-1]), (tag, i)
                a, b = o[:, -1].copy().view(np.float64), w[:, -1].copy().view(np.float64)
                assert np.all(np.abs(a - b) <= 1e-6 * np.abs(b)), (tag, a, b)
            else:
                assert same(o, w), (tag, i)

    arrays, pred, tgt = inputs(1000)
    static = [dev(a) for a in arrays]
    s_pred, s_tgt = {k: dev(v) for k, v in pred.items()}, {k: dev(v) for k, v in tgt.items()}
    first, second = run(static, s_pred, s_tgt), run(static, s_pred, s_tgt)
    assert all(torch.equal(a, b) or same(host(a), host(b)) for a, b in zip(first, second))       # bit-equal run to run
    check(first, expected(arrays, pred, tgt), "eager")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run(static, s_pred, s_tgt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # a synchronisation in here would fail the capture
        outs = run(static, s_pred, s_tgt)
    for k in range(2):
        arrays, pred, tgt = inputs(1010 + 10 * k)
        for s, a in zip(static, arrays):
            s.copy_(dev(a))
        for d, src in ((s_pred, pred), (s_tgt, tgt)):
            for key, v in src.items():
                d[key].copy_(dev(v))
        graph.replay()                                              # the matrices are zeroed by a kernel node: no accumulation
        torch.cuda.synchronize()
        check(outs, expected(arrays, pred, tgt), "replay %d" % k)


# ---- PanopticMetric end to end ------------------------------------------------------------------------------------------------------
def test_panoptic_metric_end_to_end(monkeypatch):
    pred, tgt = cases.scene()
    points = tgt.pop("center_points")
    cpu = ca.PanopticMetric(19, backend="torch")
    cpu.add_sample({k: tt(v) for k, v in pred.items()}, dict({k: tt(v) for k, v in tgt.items()}, center_points=points))
    assert cpu.metric_data["Batch_PQ"][0].shape == (2,) and cpu.metric_data["Batch_Center_MSE"][0].shape == (2,)
    copies, finds = [], []
    real_copy, real_nonzero = SP.host_copy, torch.nonzero
    monkeypatch.setattr(SP, "host_copy", lambda t: (copies.append(tuple(t.shape)), real_copy(t))[1])
    monkeypatch.setattr(SP.torch, "nonzero", lambda *a, **k: (finds.append(1), real_nonzero(*a, **k))[1])
    for backend in ("hip", "torch"):
        d_pred, d_tgt = {k: dev(v) for k, v in pred.items()}, {k: dev(v) for k, v in tgt.items()}
        keep = {k: v.clone() for k, v in list(d_pred.items()) + [("t_" + k, v) for k, v in d_tgt.items()]}
        metric = ca.PanopticMetric(19, backend=backend)
        del copies[:], finds[:]
        metric.add_sample(d_pred, dict(d_tgt, center_points=points), loss=0.5)
        assert len(copies) == 1 and finds == [1], backend
        metric.add_sample(d_pred, dict(d_tgt, center_points=[[], []]))
        assert len(copies) == 2 and finds == [1], backend                                         # no center_points: no nonzero
        for key in ("Batch_PQ", "Batch_SQ", "Batch_RQ", "Batch_Center_MSE"):
            print(backend, key, metric.metric_data[key][0], cpu.metric_data[key][0])
            assert np.array_equal(metric.metric_data[key][0], cpu.metric_data[key][0]), (backend, key)
            assert np.array_equal(metric.metric_data[key][1], cpu.metric_data[key][0]) or key == "Batch_Center_MSE"
        assert metric.metric_data["Batch_Center_MSE"][1].shape == (0,)
        got, want = metric.metric_data["Batch_Offset_MSE"][0].astype(np.float64), cpu.metric_data["Batch_Offset_MSE"][0].astype(np.float64)
        print(backend, "offset error", got, want)
        assert got.shape == (2,) and np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), backend
        for k, v in keep.items():
            assert torch.equal(v, d_tgt[k[2:]] if k.startswith("t_") else d_pred[k]), (backend, k)
    assert np.all(cpu.metric_data["Batch_PQ"][0] > 0)
