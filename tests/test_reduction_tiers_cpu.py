"""CPU tests of tests/reduction_cases.py: the shape table reaches every tier of the reductions in csrc/seg_loss.hip,
depth_loss.hip and metrics.hip (the second and third step of the one-workgroup finish kernels, both load routes; the grid
strides of ``inv_huber_max_kernel`` and ``seg_confusion_kernel``; both branches of ``fold_parts``), the inputs of the GPU tests
meet the conditions those tests rely on, and a float32 restatement of ``lse_step`` shows what the ``x == m`` select changes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_cases
import reduction_cases as rc
from cerberusnet_amd import ops
from cerberusnet_amd.loss_functions import depth_losses as D
from cerberusnet_amd.synth import hash_uniform

# what each case is in the table for, keyed by the case itself: a row that leaves the table leaves its key here, and the
# first test names what went with it
PURPOSE = {
    "seg": {((1, 2, 257, 1024), 0.0, "ones", 255): ["seg_ce_final second step, vector"],
            ((1, 3, 601, 1023), 2.0, "dynamic", -1): ["seg_ce_final second step, scalar", "seg_ce_final third step"],
            ((2, 2, 129, 1028), 0.5, "given", 255): ["seg_ce_final second step, vector",
                                                     "seg_ce image boundary inside a chunk, past 256 partials"]},
    "depth": {((1, 1, 257, 1024), (1, 257, 1024)): ["inv_huber_final second step, vector"],
              ((1, 1, 601, 1023), (1, 601, 1023)): ["inv_huber_final second step, scalar", "inv_huber_final third step"],
              ((1, 1, 1025, 1024), (1, 1025, 1024)): ["inv_huber_max grid stride, vector", "fold_parts full: every lane one uint4"],
              ((1, 1, 1537, 1023), (1, 1537, 1023)): ["inv_huber_max grid stride, scalar",
                                                      "inv_huber_max grid stride taken by some workgroups only"],
              ((1, 1, 6, 1000), (1, 6, 1000)): ["fold_parts tail loop in a lane other than 0"],
              ((1, 1, 513, 512), (1, 1026, 1024)): ["inv_huber_final second step, gather"]},
    "metric": {(2, 257, 1024): ["metric_finish second step in image 1, vector", "seg_confusion stride, vector"],
               (2, 601, 1023): ["metric_finish second step in image 1, scalar", "metric_finish third step",
                                "seg_confusion stride, scalar"]},
}


# ---- the table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", sorted(rc.TIERS))
def test_the_table_reaches_every_tier(op):
    fn, tiers = rc.TIERS[op]
    for case, must in PURPOSE[op].items():
        assert case in rc.TABLES[op], "case %s, in the table for the tier(s) %s, is gone" % (case, "; ".join(must))
        assert set(must) <= fn(case) and set(must) <= set(tiers), (case, sorted(fn(case)))
    missing = rc.uncovered(op, rc.TABLES[op])
    assert not missing, "no case of reduction_cases.%s_CASES reaches the tier(s): %s" % (op.upper(), "; ".join(missing))
    assert set(rc.TABLES[op]) == set(PURPOSE[op]), "a case without a stated purpose"


@pytest.mark.parametrize("op", sorted(rc.TIERS))
def test_a_table_without_one_of_its_cases_names_what_it_lost(op):
    """What ``uncovered`` reports for a table short of one case is what PURPOSE says the case is there for; a case that shares
    its tiers with a larger one (the smallest of its kind) is held by the ``is gone`` assertion above."""
    sole = 0
    for case in rc.TABLES[op]:
        missing = rc.uncovered(op, [c for c in rc.TABLES[op] if c != case])
        assert set(missing) <= set(PURPOSE[op][case]), (case, missing)
        sole += bool(missing)
    assert sole >= 2, op
    assert rc.uncovered("seg", [c for c in rc.SEG_CASES if c[0] != (1, 3, 601, 1023)]) == [
        "seg_ce_final second step, scalar", "seg_ce_final third step"]


def test_the_counts_of_the_table_are_those_of_the_issue():
    n = lambda s: rc.chunks(s[0] * s[2] * s[3], ops.SEG_CHUNK_PIXELS)
    want = {(1, 2, 257, 1024): 257, (1, 3, 601, 1023): 601, (2, 2, 129, 1028): 260}
    for c in rc.SEG_CASES:
        assert c[0] not in want or n(c[0]) == want[c[0]], c
    want = {(1, 1, 257, 1024): (257, "vector"), (1, 1, 601, 1023): (601, "scalar"), (1, 1, 1025, 1024): (1025, "vector"),
            (1, 1, 1537, 1023): (1536, "scalar"), (1, 1, 6, 1000): (6, "vector"), (1, 1, 513, 512): (257, "gather")}
    for c in rc.DEPTH_CASES:
        assert c[0] not in want or (n(c[0]), rc.depth_route(c)) == want[c[0]], c
    want = {(2, 257, 1024): 257, (2, 601, 1023): 601}
    for s in rc.METRIC_CASES:
        assert s not in want or rc.chunks(s[1] * s[2], ops.METRIC_CHUNK_PIXELS) == want[s], s
    assert ops.SEG_CHUNK_PIXELS == ops.INV_HUBER_CHUNK_PIXELS == ops.METRIC_CHUNK_PIXELS == 1024 and ops.INV_HUBER_MAX_PARTS == 1024
    assert (129 * 1028) // 1024 == 129 and (129 * 1028) % 1024            # image 1 of (2,2,129,1028) begins inside chunk 129
    assert rc.marker_chunks(601) == [0, 255, 256, 511, 512, 600] and rc.marker_chunks(257) == [0, 255, 256]
    chunks_of = lambda pshape, gshape: rc.depth_marker_chunks((pshape, gshape))
    assert chunks_of((1, 1, 1025, 1024), (1, 1025, 1024)) == [0, 255, 256, 511, 512, 1024]
    assert chunks_of((1, 1, 1537, 1023), (1, 1537, 1023)) == [0, 255, 256, 511, 512, 1024, 1535]
    assert chunks_of((1, 1, 6, 1000), (1, 6, 1000)) == [0, 5]


# ---- seg_cross_entropy: whole maps and markers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.SEG_CASES)
def test_seg_cases_have_a_finite_float64_reference(case):
    shape, gamma, kind, ignore = case
    x, t = rc.seg_inputs(shape, ignore)
    counted = t[t != ignore]
    assert counted.size > 0.7 * t.size and (t == ignore).any() and (counted != 1).any()      # class 1 has weight 0 under `given`
    ce = F.cross_entropy(torch.from_numpy(x).double(), torch.from_numpy(t), ignore_index=ignore)
    assert bool(torch.isfinite(ce)) and float(ce) > 0
    for k in rc.marker_chunks(rc.chunks(t.size, ops.SEG_CHUNK_PIXELS)):
        tm, p, cls = rc.seg_marker(shape, k)
        assert p // ops.SEG_CHUNK_PIXELS == k and (tm != 255).sum() == 1 and tm.reshape(-1)[p] == cls and 0 <= cls < shape[1]
        v = rc.seg_marker_ce64(x, p, cls)
        want = F.cross_entropy(torch.from_numpy(x).double(), torch.from_numpy(tm), ignore_index=255).item()
        assert np.isfinite(v) and v > 0 and abs(v - want) <= 1e-12 * want
    assert float(rc.seg_marker_weights(shape[1]).min()) >= 0.5


# ---- seg_cross_entropy: -inf and far-apart logits --------------------------------------------------------------------------------
def _ce64(x, t, w):
    return F.cross_entropy(torch.from_numpy(x).double(), torch.from_numpy(t), weight=torch.from_numpy(w).double(),
                           ignore_index=rc.INF_IGNORE)


@pytest.mark.parametrize("shape", rc.INF_SHAPES)
@pytest.mark.parametrize("pattern", sorted(rc.INF_PATTERNS))
def test_inf_patterns_never_switch_off_the_target_of_a_counted_pixel(shape, pattern):
    x, t, mask, planes = rc.inf_case(shape, pattern)
    counted = mask & (t != rc.INF_IGNORE)
    assert counted.sum() >= 1 and (mask & (t == rc.INF_IGNORE)).sum() >= 1, (pattern, int(counted.sum()))
    assert not np.isin(t[counted], planes).any()
    assert np.isneginf(np.moveaxis(x, 1, 0)[planes][:, mask]).all()
    assert np.isinf(x).sum() == mask.sum() * len(planes) and not np.isnan(x).any()
    assert np.isfinite(x.max(axis=1)).all()                              # at least one finite logit in every pixel
    ce = _ce64(x, t, rc.inf_weights(shape[1]))
    assert bool(torch.isfinite(ce)) and float(ce) > 0
    if pattern != "leading C-1":                                        # about a quarter of the pixels
        assert 0.15 < mask.mean() < 0.35, mask.mean()
    xi, ti, mi, _ = rc.inf_case(shape, pattern, ignored_only=True)
    clean = rc.seg_inputs(shape, rc.INF_IGNORE)[0]
    assert mi.sum() >= 1 and (ti[mi] == rc.INF_IGNORE).all() and np.array_equal(np.moveaxis(xi, 1, 0)[:, ~mi], np.moveaxis(clean, 1, 0)[:, ~mi])


@pytest.mark.parametrize("shape", rc.INF_SHAPES)
@pytest.mark.parametrize("pattern", sorted(rc.FAR_PATTERNS))
def test_far_patterns_have_a_float64_loss_that_fp32_can_hold(shape, pattern):
    x, t, mask, planes = rc.far_case(shape, pattern)
    counted = mask & (t != rc.INF_IGNORE)
    assert counted.sum() >= 1 and np.isfinite(x).all()
    x64 = torch.from_numpy(x).double()
    per_pixel = F.cross_entropy(x64, torch.from_numpy(t), ignore_index=rc.INF_IGNORE, reduction="none")
    assert float(per_pixel.max()) < 3e4 and float(per_pixel.sum()) < 1e8      # far inside fp32, the sum of a workgroup too
    assert bool(torch.isfinite(_ce64(x, t, rc.inf_weights(shape[1]))))
    values = rc.FAR_PATTERNS[pattern][0]
    assert all((np.moveaxis(x, 1, 0)[c][mask] == np.float32(v)).all() for c, v in values.items())
    if pattern == "spread 104 and 88":
        px = np.moveaxis(x, 1, 0)[:, mask]
        assert (px[6] - px[1] == 104).all() and (px[6] - px[12] == 88).all()
        assert np.exp(np.float32(-104)) == 0 and 0 < np.exp(np.float32(-88)) < np.finfo(np.float32).tiny   # zero; subnormal


def test_lse_step_restated_in_float32_before_and_after_the_select():
    inf = np.inf
    table = [([-inf, -inf, 2, 1], True), ([-inf, 2, -inf, 1], False), ([2, -inf, -inf, 1], False)]
    for v, poisoned in table:
        want = np.float32(2.3132617)
        old, new = rc.lse_streamed(v, rc.lse_step_parent), rc.lse_streamed(v, rc.lse_step_fixed)
        assert np.isnan(old) == poisoned and (poisoned or old == want), (v, old)
        assert new == want, (v, new)
    assert abs(float(np.float32(2.3132617)) - 2.0 - 0.31326166) < 1e-7              # the stock cross-entropy with target 2
    # -inf planes anywhere, at least one finite logit: within the GPU test's bound of float64
    for C in (2, 5, 19):
        u = hash_uniform((200, C), 4242 + C, -4.0, 4.0)
        off = hash_uniform((200, C), 4250 + C, 0.0, 1.0) < 0.4
        off[np.arange(200), np.argmin(hash_uniform((200, C), 4260 + C, 0.0, 1.0), axis=1)] = False
        v = np.where(off, -np.inf, u).astype(np.float32)
        ref = torch.logsumexp(torch.from_numpy(v).double(), 1).numpy()
        new = np.array([rc.lse_streamed(row, rc.lse_step_fixed) for row in v])
        old = np.array([rc.lse_streamed(row, rc.lse_step_parent) for row in v])
        assert np.isfinite(new).all() and np.abs(new - ref).max() <= (C + 8) * 2.0 ** -24 * np.abs(ref).max()
        lead2 = off[:, 0] & off[:, 1]
        assert (lead2.any() or C == 2) and np.array_equal(np.isnan(old), lead2)            # the parent: NaN exactly at two leading -inf
        assert np.array_equal(old[~lead2], new[~lead2])
    # all-finite logits: not a bit changes -- equal neighbours, zeros of both signs, the extremes
    rows = [hash_uniform((19,), 77 + i, -4.0, 4.0) for i in range(300)]
    rows += [np.round(hash_uniform((19,), 900 + i, -4.0, 4.0)) for i in range(100)]        # many equal values
    rows += [np.array(r, dtype=np.float32) for r in ([0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [3e38, 3e38, -3e38], [-3e38, -3e38, 3e38],
                                                       [1e-45, 1e-45, 0.0], [50.0, -54.0, -38.0, 50.0], [1e4, -1e4, 1e4])]
    for v in rows:
        old, new = rc.lse_streamed(v, rc.lse_step_parent), rc.lse_streamed(v, rc.lse_step_fixed)
        assert old.tobytes() == new.tobytes(), (v, old, new)
    # every plane -inf: -inf, and +inf planes: +inf (the loss of such a pixel is then NaN or +inf, never finite)
    assert rc.lse_streamed([-inf] * 4, rc.lse_step_fixed) == -inf
    assert rc.lse_streamed([1, inf, 2], rc.lse_step_fixed) == inf and rc.lse_streamed([inf, inf, 2], rc.lse_step_fixed) == inf


# ---- inv_huber ----------------------------------------------------------------------------------------------------------------
def _err32(case, p, g):
    gp = rc.depth_gt_at_prediction(case, g)
    d = np.maximum(p.reshape(gp.shape), np.float32(0)) - gp
    return np.where(gp > 0, np.abs(d), np.float32(0)).reshape(-1)


@pytest.mark.parametrize("case", rc.DEPTH_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_depth_cases_and_their_markers(case):
    p, g = rc.depth_inputs(case)
    assert p.shape == case[0] and g.shape == case[1] and p.dtype == g.dtype == np.float32
    gp = rc.depth_gt_at_prediction(case, g)
    assert gp.shape == (case[0][0],) + case[0][2:]
    v = D._inv_huber_stock(torch.from_numpy(p).double().reshape(gp.shape), torch.from_numpy(np.ascontiguousarray(gp)).double())
    assert bool(torch.isfinite(v)) and float(v) > 0
    assert float(_err32(case, p, g).max()) < 6.0 and (gp > 0).any() and (gp == 0).any()
    n = rc.chunks(p.size, ops.INV_HUBER_CHUNK_PIXELS)
    for k in rc.depth_marker_chunks(case):
        pm, gm, pixel, err = rc.depth_marker(case, k)
        e = _err32(case, pm, gm)
        assert pixel // ops.INV_HUBER_CHUNK_PIXELS == k and e[pixel] == err == np.float32(20.0 + 5.0 * k / 64.0)
        assert float(np.float32(0.2) * err) == (256 + k) / 64.0             # the cutoff 0.2 m is exact in fp32
        assert np.flatnonzero(e == e.max()).tolist() == [pixel] and np.sort(e)[-2] < 6.0          # the strict global maximum
    if n > ops.INV_HUBER_MAX_PARTS:
        pt, gt, pixels = rc.depth_tie(case)
        e = _err32(case, pt, gt)
        assert np.flatnonzero(e == e.max()).tolist() == list(pixels) and e.max() == 19.0
        assert pixels[0] // 1024 == 0 and pixels[1] // 1024 >= ops.INV_HUBER_MAX_PARTS
        gpt = rc.depth_gt_at_prediction(case, gt).reshape(-1)
        assert pt.reshape(-1)[pixels[0]] > gpt[pixels[0]] and pt.reshape(-1)[pixels[1]] < gpt[pixels[1]]    # opposite signs of d


# ---- the metric ops -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rc.METRIC_CASES)
def test_metric_cases_and_their_markers(shape):
    x, t, p, g, fp, fg, mask, img, seq = rc.metric_inputs(shape)
    B, H, W = shape
    assert x.shape == (B, rc.METRIC_SEG_CLASSES, H, W) and img.shape == (B, rc.METRIC_WARP_CHANNELS, H, W) and B == 2
    sums, counts, metrics = metrics_cases.depth_ref64(p, g)
    assert np.isfinite(sums).all() and all(np.isfinite(m).all() for m in metrics) and (counts[:, 0] > 0.5 * H * W).all()
    assert np.array_equal(counts, metrics_cases.depth_counts32(p, g))
    fsums, fcounts, epe, fl = metrics_cases.flow_ref64(fp, fg, mask)
    assert np.isfinite(fsums).all() and np.isfinite(epe).all() and (fcounts > 0).all()
    assert np.array_equal(fcounts, metrics_cases.flow_counts32(fp, fg, mask))
    assert not np.array_equal(p[0], p[1]) and not np.array_equal(fp[0], fp[1])                # distinct images
    conf = metrics_cases.confusion_ref(x, t)
    assert (conf > 0).all() and (t == 255).any()
    for k in rc.metric_marker_chunks(shape):
        pm, gm, pixel = rc.depth_metric_marker(shape, k)
        valid = (gm > 0) & (gm < 80)
        assert valid[1].sum() == 1 and valid[1].reshape(-1)[pixel] and pixel // 1024 == k
        assert np.array_equal(pm[0], p[0]) and np.array_equal(gm[0], g[0])
        c64, c32 = metrics_cases.depth_ref64(pm, gm)[1], metrics_cases.depth_counts32(pm, gm)
        want = [1] + [int(rc.DEPTH_MARKER_PREDICTIONS[k % 4] < th) for th in metrics_cases.DEPTH_THRESHOLDS]
        assert np.array_equal(c64, c32) and c32[1].tolist() == want
        fm, fgm, mm, pixel = rc.flow_metric_marker(shape, k)
        assert mm[1].sum() == 1 and mm[1].reshape(-1)[pixel] == 1 and np.array_equal(mm[0], mask[0])
        s64, n64, _, _ = metrics_cases.flow_ref64(fm, fgm, mm)
        assert np.array_equal(n64, metrics_cases.flow_counts32(fm, fgm, mm)) and n64[1, 0] == 1
        assert abs(s64[1, 0] - 5.0) < 1e-4 and s64[1, 1] == 1
    xc, tc, count = rc.confusion_marker(shape)
    two = tc == 2
    assert count > 200 and two[1].sum() == count and not two[0].any()
    assert np.flatnonzero(two[1].reshape(-1)).min() >= rc.CONF_GROUPS_PER_IMAGE * ops.METRIC_CHUNK_PIXELS
    assert set(np.unique(tc)) == {0, 1, 2, 255}
    assert metrics_cases.confusion_ref(xc, tc)[1, 2].sum() == count
