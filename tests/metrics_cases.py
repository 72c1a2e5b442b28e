"""Inputs and yardsticks of the training-metric tests, shared by tests/test_metrics_cpu.py, tests/test_metrics_gpu.py and the
generator of tests/golden/metrics.npz (tools/gen_golden_metrics.py): everything comes from ``hash_uniform`` seeds.

Yardsticks.  The reference's ``SegmentationMetric`` and ``OpticFlowMetric`` cannot run without a GPU (``.cuda()``,
``.get_device()``), so theirs are the numpy restatements below, integer or float64, each citing the reference lines it restates
(nnet_training/statistics/).  ``DepthMetric`` has the reference's own results in the golden file and a restatement here for the
shapes of the GPU tests.

Counts that come from fp32 comparisons (a1 / a2 / a3, the Fl outliers) are restated in numpy float32 with the kernels'
per-pixel arithmetic.  The generators ASSERT that no ratio or error they produce lies within relative 1e-5 of a threshold
(1.25, 1.25^2, 1.25^3, 3, 0.05): fp32 rounding moves a ratio by about 1e-7, so fp32 and float64 then agree on every count.  The
seeds below were chosen so that this holds; no pixel is excluded."""
import numpy as np

from cerberusnet_amd.synth import hash_uniform

CLEARANCE = 1e-5
DEPTH_THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
MIN_DEPTH, MAX_DEPTH = 0.0, 80.0

# (B, H, W) of the GPU tests: the scalar route, the vector route, and one with 64 workgroups (see test_metrics_gpu.py)
SCALAR_SHAPES = [(1, 1, 1), (1, 5, 7), (2, 37, 53), (1, 3, 66)]
VECTOR_SHAPES = [(1, 1, 4), (2, 8, 64), (3, 16, 33)]
SHAPES = SCALAR_SHAPES + VECTOR_SHAPES + [(2, 128, 256)]

# seeds for which the generated ratios and errors keep clear of the thresholds, per shape (found by tools/gen_golden_metrics.py
# --seeds, which tries seeds upward from a start value)
DEPTH_SEEDS = {(1, 1, 1): 3000, (1, 5, 7): 3000, (2, 37, 53): 3000, (1, 3, 66): 3000, (1, 1, 4): 3000, (2, 8, 64): 3000,
               (3, 16, 33): 3000, (2, 128, 256): 3270, (2, 9, 20): 3000, (3, 12, 20): 3000, (3, 5, 7): 3000, (3, 37, 53): 3000}
FLOW_SEEDS = {(1, 1, 1): 4000, (1, 5, 7): 4000, (2, 37, 53): 4000, (1, 3, 66): 4000, (1, 1, 4): 4000, (2, 8, 64): 4000,
              (3, 16, 33): 4000, (2, 128, 256): 4010, (2, 9, 20): 4000, (3, 12, 20): 4000, (3, 5, 7): 4000, (3, 37, 53): 4000}

# the golden cases of DepthMetric: prediction shape and constructor keywords
GOLDEN_DEPTH_CASES = [((2, 1, 9, 20), dict(main_metric="RMSE_Log")), ((3, 12, 20), dict(main_metric="Batch_a1"))]


def clear_of(values, thresholds, clearance=CLEARANCE):
    """True if no finite value lies within relative ``clearance`` of a threshold."""
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    return all(bool((np.abs(v - t) > clearance * t).all()) for t in thresholds)


# ---- segmentation ---------------------------------------------------------------------------------------------------------
def logits(shape, seed):
    return hash_uniform(shape, seed, -4.0, 4.0)


def labels(shape, seed, ignore_index=255, ignore_share=0.15):
    """(B,H,W) int64 labels for logits of ``shape`` = (B,C,H,W), in runs along a row (neighbouring pixels of a label map mostly
    agree); about ``ignore_share`` of them are the ignore label."""
    B, C, H, W = shape
    u = hash_uniform((B, H, (W + 3) // 4), seed, 0.0, 1.0, dtype=np.float64)
    t = np.repeat(np.minimum(np.floor(u * C), C - 1).astype(np.int64), 4, axis=2)[:, :, :W].copy()
    t[hash_uniform((B, H, W), seed + 1, 0.0, 1.0) < ignore_share] = ignore_index
    return t


def confusion_ref(x, t, ignore_index=255):
    """(B,C,C) int64 [image, label, prediction]: semantic.py:41-48 and ``_gen_confusion_mat`` (:190-194) per image, with every
    label outside [0, C) skipped as the ignore label is.  ``np.argmax`` has ``torch.argmax``'s rule: the first maximum, and a
    NaN counts as the maximum."""
    B, C = x.shape[:2]
    out = np.zeros((B, C, C), dtype=np.int64)
    for b in range(B):
        pred = np.argmax(x[b], axis=0).reshape(-1).astype(np.int64)
        lab = t[b].reshape(-1)
        keep = (lab != ignore_index) & (lab >= 0) & (lab < C)
        out[b] = np.bincount(C * lab[keep] + pred[keep], minlength=C * C).reshape(C, C)
    return out


def seg_metrics_ref(conf):
    """Pixel accuracy (B,1) and IoU (B,C) of (B,C,C) matrices in float64: semantic.py:50-52 and ``_confmat_cls_iou`` (:135-143)."""
    conf = conf.astype(np.float64)
    hits = np.diagonal(conf, axis1=1, axis2=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (hits.sum(axis=1) / conf.sum(axis=(1, 2)))[:, None], hits / (conf.sum(axis=2) + conf.sum(axis=1) - hits)


# ---- depth ----------------------------------------------------------------------------------------------------------------
def _depth_terms(pred, gt, dtype):
    """The per-pixel terms of depth.py:35-72 in ``dtype``: (valid, |d|/g, d^2/g, d^2, l^2, |l|, r)."""
    p, g = pred.reshape(gt.shape).astype(dtype), gt.astype(dtype)
    valid = (g > dtype(MIN_DEPTH)) & (g < dtype(MAX_DEPTH))
    p = np.where(p == 0, dtype(1e-7), p)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = p - g
        l = np.log(p) - np.log(g)
        r = np.maximum(p / g, g / p)
        return valid, np.abs(d) / g, d * d / g, d * d, l * l, np.abs(l), r


def depth_inputs(shape, seed=None, zero_share=0.0, check=True):
    """Prediction (B,1,h,w) and ground truth (B,h,w), float32, for ``shape`` = (B,h,w).  The ground truth is uniform in
    [0.5, 100) -- a fifth of it at or beyond ``MAX_DEPTH`` -- with a tenth set to 0 (no measurement); the prediction is the
    ground truth times a factor that is log-uniform in [1/4, 4), so all three accuracy thresholds split the pixels; a share
    ``zero_share`` of the prediction is exactly 0.  ``check=False`` (timing runs on large maps, where no count is compared) skips the
    assertion that the ratios keep clear of the thresholds."""
    seed = DEPTH_SEEDS[tuple(shape)] if seed is None else seed
    g = hash_uniform(shape, seed, 0.5, 100.0)
    factor = np.exp(hash_uniform(shape, seed + 2, -np.log(4.0), np.log(4.0), dtype=np.float64))
    p = (g.astype(np.float64) * factor).astype(np.float32)
    g[hash_uniform(shape, seed + 1, 0.0, 1.0) < 0.1] = 0.0
    if zero_share:
        p[hash_uniform(shape, seed + 3, 0.0, 1.0) < zero_share] = 0.0
    if p.size <= 4:
        p.reshape(-1)[0], g.reshape(-1)[0] = 2.5, 1.0                        # a few pixels: one that counts
    valid, *_, r = _depth_terms(p, g, np.float64)
    assert not check or clear_of(r[valid], DEPTH_THRESHOLDS), ("a depth ratio within %g of a threshold" % CLEARANCE, shape, seed)
    return p[:, None], g


def depth_ref64(pred, gt):
    """(sums (B,5), counts (B,4), the eight metrics in the order of ``statistics.depth.KEYS``) in float64 / int64."""
    valid, *terms, r = _depth_terms(pred, gt, np.float64)
    sums = np.stack([np.where(valid, t, 0.0).sum(axis=(1, 2)) for t in terms], axis=1)
    counts = np.stack([valid.sum(axis=(1, 2))] + [(valid & (r < t)).sum(axis=(1, 2)) for t in DEPTH_THRESHOLDS], axis=1).astype(np.int64)
    n = counts[:, 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        sq_log = sums[:, 3] / n
        metrics = [sums[:, 0] / n, sums[:, 1] / n, np.sqrt(sums[:, 2] / n), np.sqrt(sq_log), sq_log - sums[:, 4] ** 2 / n ** 2,
                   counts[:, 1] / n, counts[:, 2] / n, counts[:, 3] / n]
    return sums, counts, metrics


def depth_counts32(pred, gt):
    """(B,4) int64: the counts from the kernels' fp32 arithmetic (thresholds rounded to fp32, as torch's comparison with a
    Python scalar)."""
    valid, *_, r = _depth_terms(pred, gt, np.float32)
    rows = [valid.sum(axis=(1, 2))] + [(valid & (r < np.float32(t))).sum(axis=(1, 2)) for t in DEPTH_THRESHOLDS]
    return np.stack(rows, axis=1).astype(np.int64)


# ---- flow -----------------------------------------------------------------------------------------------------------------
def _flow_terms(fp, fg, mask, dtype):
    """optical_flow.py:28-37, :53-63 per pixel in ``dtype``: (epe * mask, the outlier ratio)."""
    d = fp.astype(dtype) - fg.astype(dtype)
    e = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) * mask.astype(dtype)
    g = fg.astype(dtype)
    mag = np.maximum(np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]), dtype(np.float32(1e-10)))
    return e, e / mag


def flow_inputs(shape, seed=None, check=True):
    """flow_pred, flow_gt (B,2,H,W) and mask (B,H,W), float32, for ``shape`` = (B,H,W).  The ground truth is uniform in
    [-20, 20); the prediction is off by 8 u^3 per component, u uniform in [-1, 1) (mostly small errors, some beyond 3 px); the
    mask is 1 on four fifths of the pixels.  ``check=False``: as for ``depth_inputs``."""
    seed = FLOW_SEEDS[tuple(shape)] if seed is None else seed
    B, H, W = shape
    fg = hash_uniform((B, 2, H, W), seed, -20.0, 20.0)
    fp = (fg + 8.0 * hash_uniform((B, 2, H, W), seed + 1, -1.0, 1.0) ** 3).astype(np.float32)
    mask = (hash_uniform(shape, seed + 2, 0.0, 1.0) < 0.8).astype(np.float32)
    if mask.size <= 4:
        mask.reshape(-1)[0] = 1.0
    e, ratio = _flow_terms(fp, fg, mask, np.float64)
    assert not check or (clear_of(e, (3.0,)) and clear_of(ratio, (0.05,))), ("a flow error within %g of a threshold" % CLEARANCE, shape, seed)
    return fp, fg, mask


def flow_ref64(fp, fg, mask):
    """(sums (B,2), counts (B,1), EPE (B,), Fl (B,)) in float64 / int64."""
    e, ratio = _flow_terms(fp, fg, mask, np.float64)
    sums = np.stack([e.sum(axis=(1, 2)), mask.astype(np.float64).sum(axis=(1, 2))], axis=1)
    counts = ((e > 3) & (ratio > 0.05)).sum(axis=(1, 2)).astype(np.int64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return sums, counts, sums[:, 0] / sums[:, 1], counts[:, 0] / sums[:, 1]


def flow_counts32(fp, fg, mask):
    e, ratio = _flow_terms(fp, fg, mask, np.float32)
    return ((e > np.float32(3)) & (ratio > np.float32(0.05))).sum(axis=(1, 2)).astype(np.int64)[:, None]


def warp_inputs(shape, seed, reach=3.0):
    """image, source (B,C,H,W) in [0, 1) and a flow (B,2,H,W) uniform in [-reach, reach), for ``shape`` = (B,C,H,W)."""
    B, C, H, W = shape
    return (hash_uniform(shape, seed, 0.0, 1.0), hash_uniform(shape, seed + 1, 0.0, 1.0),
            hash_uniform((B, 2, H, W), seed + 2, -reach, reach))


def warp_sad_ref64(image, source, flow):
    """(B,) float64: sum |image - flow_warp(source, flow)| (optical_flow.py:68-70 before the mean) with the stock grid_sample
    restatement of flow_warp in float64 on the CPU."""
    import torch
    from cerberusnet_amd.loss_functions.UnFlowLoss import _torch_flow_warp
    im, src, fl = (torch.from_numpy(np.ascontiguousarray(a)).double() for a in (image, source, flow))
    return (im - _torch_flow_warp(src, fl)).abs().sum(dim=(1, 2, 3)).numpy()


def golden_depth_inputs(i):
    shape, _ = GOLDEN_DEPTH_CASES[i]
    p, g = depth_inputs((shape[0],) + tuple(shape[-2:]), zero_share=0.02)
    return (p if len(shape) == 4 else p[:, 0]), g
