"""The shapes at which the reductions of csrc/seg_loss.hip, depth_loss.hip and metrics.hip go past one round, and the inputs
that single out one partial, shared by tests/test_reduction_tiers_cpu.py (which checks that the table reaches every tier) and
the GPU tests of the three ops.  Also the non-finite and far-apart logit patterns of the segmentation loss.

All three files reduce alike: a workgroup folds ``*_CHUNK_PIXELS`` pixels into one partial, and a second launch of ONE
workgroup of ``FINISH_THREADS`` threads adds the partials by ``for (i = threadIdx.x; i < n; i += 256)`` and the LDS tree of loss_reduce.h (``tree_sum``).  Up to
256 partials every thread of a finish kernel reads at most one.  The constants the kernels do not export are restated here
with the line they mirror."""
import functools

import numpy as np

import depth_loss_cases
import metrics_cases
import seg_loss_cases
from cerberusnet_amd import ops
from cerberusnet_amd.synth import hash_uniform

FINISH_THREADS = 256          # loss_reduce.h `constexpr int kReduceThreads = 256`: `i += kThreads` of seg_ce_final_kernel,
#                               inv_huber_final_kernel and metric_finish_kernel
CONF_GROUPS_PER_IMAGE = 256   # metrics.hip `constexpr int kConfGroupsPerImage = 256`: seg_confusion_kernel's `ch += gridDim.x`
FOLD_QUAD = 4                 # depth_loss.hip fold_parts: `i0 = threadIdx.x * kQuad`, one uint4 per lane or the tail loop


def chunks(pixels, chunk):
    return (pixels + chunk - 1) // chunk


# ---- the table ------------------------------------------------------------------------------------------------------------
# seg_cross_entropy: (shape (B,C,H,W), gamma, kind of weights, ignore value) -- the rows join COMBOS of test_seg_loss_gpu.py
SEG_CASES = [((1, 2, 257, 1024), 0.0, "ones", 255),
             ((1, 3, 601, 1023), 2.0, "dynamic", -1),
             ((2, 2, 129, 1028), 0.5, "given", 255)]
# inv_huber: (prediction shape (B,1,h,w), ground-truth shape (B,H,W))
DEPTH_CASES = [((1, 1, 257, 1024), (1, 257, 1024)),
               ((1, 1, 601, 1023), (1, 601, 1023)),
               ((1, 1, 1025, 1024), (1, 1025, 1024)),
               ((1, 1, 1537, 1023), (1, 1537, 1023)),
               ((1, 1, 6, 1000), (1, 6, 1000)),
               ((1, 1, 513, 512), (1, 1026, 1024))]
# the metric ops: (B,H,W); seg_confusion with METRIC_SEG_CLASSES classes, warp_sad with METRIC_WARP_CHANNELS channels
METRIC_CASES = [(2, 257, 1024), (2, 601, 1023)]
METRIC_SEG_CLASSES = 3
METRIC_WARP_CHANNELS = 2


def case_of(op, shape):
    """The row of a table by its (prediction) shape; the tests that want one particular row ask for it by shape, never by position."""
    rows = [c for c in TABLES[op] if (c if op == "metric" else c[0]) == shape]
    assert len(rows) == 1, "reduction_cases.%s_CASES has %d rows of shape %s" % (op.upper(), len(rows), shape)
    return rows[0]


def seg_tiers(case):
    (B, C, H, W), *_ = case
    route = "vector" if H * W % 4 == 0 else "scalar"
    n = chunks(B * H * W, ops.SEG_CHUNK_PIXELS)
    out = set()
    if n > FINISH_THREADS:
        out.add("seg_ce_final second step, %s" % route)
    if n > 2 * FINISH_THREADS:
        out.add("seg_ce_final third step")
    if n > FINISH_THREADS and B > 1 and (H * W) % ops.SEG_CHUNK_PIXELS:
        out.add("seg_ce image boundary inside a chunk, past 256 partials")
    return out


def depth_route(case):
    pshape, gshape = case
    if tuple(pshape[2:]) != tuple(gshape[1:]):
        return "gather"
    return "vector" if pshape[2] * pshape[3] % 4 == 0 else "scalar"


def depth_tiers(case):
    pshape, _ = case
    route = depth_route(case)
    n = chunks(pshape[0] * pshape[2] * pshape[3], ops.INV_HUBER_CHUNK_PIXELS)
    nparts = min(n, ops.INV_HUBER_MAX_PARTS)
    out = set()
    if n > FINISH_THREADS:
        out.add("inv_huber_final second step, %s" % route)
    if n > 2 * FINISH_THREADS:
        out.add("inv_huber_final third step")
    if n > ops.INV_HUBER_MAX_PARTS:
        out.add("inv_huber_max grid stride, %s" % route)
        if n < 2 * ops.INV_HUBER_MAX_PARTS:
            out.add("inv_huber_max grid stride taken by some workgroups only")
    if nparts == ops.INV_HUBER_MAX_PARTS:
        out.add("fold_parts full: every lane one uint4")
    if nparts > FOLD_QUAD and nparts % FOLD_QUAD:
        out.add("fold_parts tail loop in a lane other than 0")
    return out


def metric_tiers(shape):
    B, H, W = shape
    route = "vector" if H * W % 4 == 0 else "scalar"
    n = chunks(H * W, ops.METRIC_CHUNK_PIXELS)
    out = set()
    if n > FINISH_THREADS and B > 1:
        out.add("metric_finish second step in image 1, %s" % route)
    if n > 2 * FINISH_THREADS and B > 1:
        out.add("metric_finish third step")
    if n > CONF_GROUPS_PER_IMAGE and B > 1:
        out.add("seg_confusion stride, %s" % route)
    return out


TIERS = {
    "seg": (seg_tiers, ["seg_ce_final second step, vector", "seg_ce_final second step, scalar", "seg_ce_final third step",
                        "seg_ce image boundary inside a chunk, past 256 partials"]),
    "depth": (depth_tiers, ["inv_huber_final second step, vector", "inv_huber_final second step, scalar",
                            "inv_huber_final second step, gather", "inv_huber_final third step",
                            "inv_huber_max grid stride, vector", "inv_huber_max grid stride, scalar",
                            "inv_huber_max grid stride taken by some workgroups only", "fold_parts full: every lane one uint4",
                            "fold_parts tail loop in a lane other than 0"]),
    "metric": (metric_tiers, ["metric_finish second step in image 1, vector", "metric_finish second step in image 1, scalar",
                              "metric_finish third step", "seg_confusion stride, vector", "seg_confusion stride, scalar"]),
}
TABLES = {"seg": SEG_CASES, "depth": DEPTH_CASES, "metric": METRIC_CASES}


def uncovered(op, table):
    """The tiers of ``op`` that no case of ``table`` reaches."""
    fn, tiers = TIERS[op]
    reached = set().union(*[fn(c) for c in table]) if table else set()
    return [t for t in tiers if t not in reached]


def marker_chunks(nchunks, extra=()):
    """The chunks a marker is placed in: the first, both sides of the finish kernels' first and second wrap, the last."""
    return sorted({k for k in (0, 255, 256, 511, 512, nchunks - 1) + tuple(extra) if 0 <= k < nchunks})


def marker_pixel(k, pixels, chunk=1024):
    """A pixel inside chunk ``k`` of a map of ``pixels``, at an offset that differs from chunk to chunk."""
    return min(k * chunk + (37 * k + 5) % chunk, pixels - 1)


# ---- seg_cross_entropy ------------------------------------------------------------------------------------------------------
def seg_inputs(shape, ignore_index, seed=900):
    """Logits and labels of a whole-map case: those of ``_inputs`` in test_seg_loss_gpu.py."""
    t = seg_loss_cases.labels(shape, seed + 5, ignore_index)
    if t.reshape(-1)[0] == ignore_index:
        t.reshape(-1)[0] = 0
    return seg_loss_cases.logits(shape, seed), t


def seg_marker_weights(C):
    """Class weights in [0.5, 2), none of them 0: the one pixel that counts must count."""
    return hash_uniform((C,), 78, 0.5, 2.0)


def seg_marker(shape, k, ignore_index=255):
    """(labels, pixel, class): every label the ignore value except the one at a pixel inside chunk ``k``."""
    B, C, H, W = shape
    p = marker_pixel(k, B * H * W, ops.SEG_CHUNK_PIXELS)
    t = np.full((B, H, W), ignore_index, dtype=np.int64)
    t.reshape(-1)[p] = p % C
    return t, p, p % C


def seg_marker_ce64(x, p, cls):
    """lse - x_t of pixel ``p`` (an index into the flattened (B,H,W) map) in float64: the weighted mean over one pixel."""
    hw = x.shape[2] * x.shape[3]
    v = x[p // hw].reshape(x.shape[1], -1)[:, p % hw].astype(np.float64)
    return float(v.max() + np.log(np.exp(v - v.max()).sum()) - v[cls])


# ---- non-finite and far-apart logits of seg_cross_entropy ----------------------------------------------------------------------
INF_SHAPES = [(2, 19, 37, 53), (2, 19, 8, 64)]        # scalar and vector route
# the class planes set to -inf on the chosen pixels, for C classes
INF_PATTERNS = {"leading 1": lambda C: [0], "leading 2": lambda C: [0, 1], "leading C-1": lambda C: list(range(C - 1)),
                "middle": lambda C: [C // 2], "last": lambda C: [C - 1], "0 and 2": lambda C: [0, 2]}
# far-apart finite logits: {plane: value}; `only` = the label a counted pixel must have (None: any but a plane at -3e38),
# because the loss of a pixel with a logit 3e38 above its target's is beyond fp32
FAR_PATTERNS = {"+1e4": ({3: 1e4}, None), "-1e4": ({3: -1e4}, None), "+-1e4": ({0: 1e4, 5: -1e4}, None),
                "+3e38": ({2: 3e38}, 2), "-3e38": ({4: -3e38}, None), "+-3e38": ({4: -3e38, 2: 3e38}, 2),
                "spread 104 and 88": ({1: -54.0, 6: 50.0, 12: -38.0}, None)}
INF_IGNORE = 255


def _chosen(shape, t, planes, seed, only=None):
    """About a quarter of the pixels, by a hash field; of the pixels that count, only those whose label is none of ``planes``
    (and is ``only``, if given)."""
    B, C, H, W = shape
    pick = hash_uniform((B, H, W), seed, 0.0, 1.0) < 0.25
    ok = (t == INF_IGNORE) | ~np.isin(t, planes)
    if only is not None:
        ok &= (t == INF_IGNORE) | (t == only)
    return pick & ok


def inf_case(shape, pattern, ignored_only=False):
    """(logits, labels, mask (B,H,W) of the pixels changed, planes): the -inf pattern on the inputs of the route shapes."""
    x, t = seg_inputs(shape, INF_IGNORE)
    planes = INF_PATTERNS[pattern](shape[1])
    mask = _chosen(shape, t, planes, 911)
    if ignored_only:
        mask &= t == INF_IGNORE
    x = x.copy()
    for c in planes:
        x[:, c][mask] = -np.inf
    return x, t, mask, planes


def far_case(shape, pattern):
    x, t = seg_inputs(shape, INF_IGNORE)
    values, only = FAR_PATTERNS[pattern]
    low = [c for c, v in values.items() if v < -1e30]
    mask = _chosen(shape, t, low, 913, only)
    x = x.copy()
    for c, v in values.items():
        x[:, c][mask] = v
    return x, t, mask, sorted(values)


def inf_weights(C):
    """The `given` weights of test_seg_loss_gpu.py: [0.5, 2) with class 1 at weight 0."""
    w = hash_uniform((C,), 77, 0.5, 2.0)
    w[1] = 0.0
    return w


def lse_step_parent(x, m, s):
    """seg_loss.hip's lse_step before the x == m select, in float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float32(x) - np.float32(m)
        e = np.exp(-np.abs(d), dtype=np.float32)
        s = np.float32(s * e + np.float32(1)) if d > 0 else np.float32(s + e)
    return np.float32(max(m, x)) if not np.isnan(x) else m, s


def lse_step_fixed(x, m, s):
    """seg_loss.hip's lse_step, in float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float32(0) if x == m else np.float32(x) - np.float32(m)
        e = np.exp(-np.abs(d), dtype=np.float32)
        s = np.float32(s * e + np.float32(1)) if d > 0 else np.float32(s + e)
    return np.float32(max(m, x)) if not np.isnan(x) else m, s


def lse_streamed(v, step):
    """The kernels' streamed logsumexp of one pixel's logits with ``step`` as lse_step; float32 throughout."""
    v = np.asarray(v, dtype=np.float32)
    m, s = v[0], np.float32(1)
    for x in v[1:]:
        m, s = step(x, m, s)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(m + np.log(s, dtype=np.float32))


# ---- inv_huber ------------------------------------------------------------------------------------------------------------
def depth_inputs(case, seed=2000):
    """Prediction (B,1,h,w) and ground truth (B,H,W) of a table case: the generators of test_depth_loss_gpu.py."""
    pshape, gshape = case
    return depth_loss_cases.prediction(pshape, seed), depth_loss_cases.ground_truth(gshape, seed + 5)


def depth_gt_at_prediction(case, g):
    """The ground truth a prediction pixel reads: itself, or every (H/h, W/w)-th pixel under the gather."""
    pshape, gshape = case
    return g[:, ::gshape[1] // pshape[2], ::gshape[2] // pshape[3]]


def depth_marker_chunks(case):
    pshape, _ = case
    n = chunks(pshape[0] * pshape[2] * pshape[3], ops.INV_HUBER_CHUNK_PIXELS)
    return marker_chunks(n, extra=(ops.INV_HUBER_MAX_PARTS,))


def _plant_depth(case, p, g, pixel, pv, gv):
    """Writes prediction ``pv`` and ground truth ``gv`` at prediction pixel ``pixel`` (through the gather, if any)."""
    pshape, gshape = case
    ry, rx = gshape[1] // pshape[2], gshape[2] // pshape[3]
    b, r = divmod(pixel, pshape[2] * pshape[3])
    y, x = divmod(r, pshape[3])
    p.reshape(-1)[pixel] = pv
    g[b, y * ry, x * rx] = gv


def depth_marker(case, k):
    """(p, g, pixel, err): the strict global maximum of err planted inside chunk ``k``: m = 20 + 5 k / 64, a prediction of m + 1
    against a ground truth of 1, all exact in fp32, different from chunk to chunk and far above the 6 that the generators'
    errors stay below.  m is a multiple of 5/64 so that the cutoff c = 0.2f * m is EXACT in fp32 (0.2 m = (256 + k) / 64, and
    0.2f is off by 1.5e-8, less than half a unit): the float64 reference then uses the cutoff that every fp32 evaluation uses.
    With an inexact cutoff the gradient at the maximum measures how S = sum(1/2 - d^2 / 2c^2) responds to the rounding of c, not
    the reduction: with m = 19 + k / 64 = 27 at (1,1,1537,1023), 4756 pixels lie just above c = 5.4, and float64 arithmetic on
    the fp32 cutoff alone is 5.5e-7 off the float64 gradient there, above the 4 * 2^-23 that the GPU test allows."""
    p, g = (a.copy() for a in depth_inputs(case))
    pixel = marker_pixel(k, p.size, ops.INV_HUBER_CHUNK_PIXELS)
    m = np.float32(20.0 + 5.0 * k / 64.0)
    _plant_depth(case, p, g, pixel, m + np.float32(1.0), 1.0)
    return p, g, pixel, m


def depth_tie(case):
    """(p, g, pixels): two equal maxima of opposite sign of d, one in chunk 0 and one in the last chunk."""
    p, g = (a.copy() for a in depth_inputs(case))
    n = chunks(p.size, ops.INV_HUBER_CHUNK_PIXELS)
    pixels = (marker_pixel(0, p.size), marker_pixel(n - 1, p.size))
    _plant_depth(case, p, g, pixels[0], 20.5, 1.5)
    _plant_depth(case, p, g, pixels[1], 0.5, 19.5)
    return p, g, pixels


# ---- the metric ops ---------------------------------------------------------------------------------------------------------
def _clear_depth(shape, seed):
    """``metrics_cases.depth_inputs`` at a size where no seed keeps every ratio clear of the thresholds (about 1e-4 of the pixels
    lie within the clearance): the predictions of those pixels are moved by a factor 1 + 2^-8, then the clearance holds."""
    p, g = metrics_cases.depth_inputs(shape, seed=seed, check=False)
    for _ in range(4):
        valid, *_, r = metrics_cases._depth_terms(p, g, np.float64)
        near = np.zeros(g.shape, dtype=bool)
        for t in metrics_cases.DEPTH_THRESHOLDS:
            near |= valid & (np.abs(r - t) <= 2 * metrics_cases.CLEARANCE * t)
        if not near.any():
            break
        p[:, 0][near] *= np.float32(1.0 + 2.0 ** -8)
    valid, *_, r = metrics_cases._depth_terms(p, g, np.float64)
    assert metrics_cases.clear_of(r[valid], metrics_cases.DEPTH_THRESHOLDS), shape
    return p, g


def _clear_flow(shape, seed):
    """``metrics_cases.flow_inputs`` likewise: the x component of a prediction whose error or ratio lies near a threshold moves
    by 1/64."""
    fp, fg, mask = metrics_cases.flow_inputs(shape, seed=seed, check=False)
    for _ in range(4):
        e, ratio = metrics_cases._flow_terms(fp, fg, mask, np.float64)
        near = (np.abs(e - 3.0) <= 2 * metrics_cases.CLEARANCE * 3.0) | (np.abs(ratio - 0.05) <= 2 * metrics_cases.CLEARANCE * 0.05)
        if not near.any():
            break
        fp[:, 0][near] += np.float32(1.0 / 64)
    e, ratio = metrics_cases._flow_terms(fp, fg, mask, np.float64)
    assert metrics_cases.clear_of(e, (3.0,)) and metrics_cases.clear_of(ratio, (0.05,)), shape
    return fp, fg, mask


@functools.lru_cache(maxsize=None)
def metric_inputs(shape):
    """(x, t, p, g, fp, fg, mask, img, seq) of a table shape, the order of ``op_inputs`` in test_metrics_gpu.py.  Computed once per
    shape and shared; the arrays are not written to."""
    B, H, W = shape
    sshape = (B, METRIC_SEG_CLASSES, H, W)
    x, t = metrics_cases.logits(sshape, 7300), metrics_cases.labels(sshape, 7305)
    p, g = _clear_depth(shape, 3300)
    fp, fg, mask = _clear_flow(shape, 4300)
    img, seq, _ = metrics_cases.warp_inputs((B, METRIC_WARP_CHANNELS, H, W), 7310)
    return x, t, p, g, fp, fg, mask, img, seq


def metric_marker_chunks(shape):
    return marker_chunks(chunks(shape[1] * shape[2], ops.METRIC_CHUNK_PIXELS))


DEPTH_MARKER_PREDICTIONS = (1.125, 1.5, 1.75, 6.0)     # against a ground truth of 1: inside a1, a2, a3, none


def depth_metric_marker(shape, k):
    """(p, g, pixel): image 0 as in ``metric_inputs``; image 1 with exactly ONE valid pixel, inside chunk ``k``."""
    _, _, p, g, *_ = metric_inputs(shape)
    p, g = p.copy(), g.copy()
    pixel = marker_pixel(k, shape[1] * shape[2], ops.METRIC_CHUNK_PIXELS)
    g[1] = 0.0
    g[1].reshape(-1)[pixel] = 1.0
    p[1, 0].reshape(-1)[pixel] = DEPTH_MARKER_PREDICTIONS[k % 4]
    return p, g, pixel


def flow_metric_marker(shape, k):
    """(fp, fg, mask, pixel): image 1 with exactly ONE unmasked pixel, inside chunk ``k``, 3 and 4 px off: an outlier."""
    _, _, _, _, fp, fg, mask, _, _ = metric_inputs(shape)
    fp, mask = fp.copy(), mask.copy()
    pixel = marker_pixel(k, shape[1] * shape[2], ops.METRIC_CHUNK_PIXELS)
    mask[1] = 0.0
    mask[1].reshape(-1)[pixel] = 1.0
    for c, off in ((0, 3.0), (1, 4.0)):
        fp[1, c].reshape(-1)[pixel] = fg[1, c].reshape(-1)[pixel] + np.float32(off)
    return fp, fg, mask, pixel


def confusion_marker(shape):
    """(x, t, count): labels of class 2 ONLY inside the chunks of image 1 that a workgroup reaches by its stride (chunk >=
    CONF_GROUPS_PER_IMAGE), class 0 or 1 (or the ignore value) everywhere else; count = the pixels of class 2."""
    B, H, W = shape
    x = metric_inputs(shape)[0]
    t = (hash_uniform(shape, 7320, 0.0, 1.0) < 0.5).astype(np.int64)
    t[hash_uniform(shape, 7321, 0.0, 1.0) < 0.1] = 255
    strided = np.arange(H * W) >= CONF_GROUPS_PER_IMAGE * ops.METRIC_CHUNK_PIXELS
    two = strided & (hash_uniform((H * W,), 7322, 0.0, 1.0) < 0.3)
    t[1].reshape(-1)[two] = 2
    return x, t, int(two.sum())
