"""Inputs and yardsticks of the panoptic tests (test_panoptic_cpu.py, test_panoptic_gpu.py, tools/gen_golden_panoptic.py): seeded
numpy inputs, the kernels' tile / chunk / stride constants restated with the line they mirror, the shapes of the GPU tests, and
numpy restatements where a test needs one (``np.add.at`` for the overlap matrices)."""
import numpy as np

# ---- csrc/panoptic.hip, restated -------------------------------------------------------------------------------------------------
PEAK_TILE_H = 16              # `constexpr int kPeakTileH = 16, kPeakTileW = 64;`: outputs of a center_peaks workgroup
PEAK_TILE_W = 64
PEAK_MAX_KERNEL = 15          # `constexpr int kPeakMaxKernel = 15;`
PIXEL_CHUNK = 1024            # `constexpr int kChunk = kThreads * kQuad;`: pixels of a group_pixels / instance_overlap workgroup
CENTER_CHUNK = 256            # `constexpr int kCenterChunk = 256;`: centres per LDS fill of group_pixels
GROUP_MAX_CENTERS = 4096      # `constexpr int kGroupMaxCenters = 4096;`
OVERLAP_GROUPS_PER_IMAGE = 256  # `constexpr int kOverlapGroupsPerImage = 256;`: instance_overlap_kernel's `ch += gridDim.x`
OVERLAP_MAX_BINS = 16128      # `constexpr int kOverlapMaxBins = 16128;`

# ---- the shapes of the GPU tests ---------------------------------------------------------------------------------------------------
PEAK_SHAPES = [(1, 1, 1, 1), (2, 1, 5, 7), (1, 1, 1, 9), (1, 1, 3, 66), (2, 1, 37, 53), (3, 1, 16, 33), (2, 1, 35, 130)]
PEAK_KERNELS = [1, 3, 5, 7]
PEAK_THRESHOLDS = [0.1, 0.0, -0.5]
GROUP_SHAPES = [(1, 5, 7), (2, 37, 53), (2, 8, 64), (1, 128, 256)]
GROUP_COUNTS = [0, 1, 2, 99, 100, 300]          # 300: past one LDS chunk of centres
OVERLAP_SHAPES = [(1, 5, 7), (2, 37, 53), (2, 8, 64), (2, 257, 1024)]
OVERLAP_SIZES = [(2, 2), (101, 19)]             # (M, C)
FLOAT_BAND = 1e-6                               # relative gap of the two smallest float64 distances inside which either id passes
FLOAT_BAND_MAX_SHARE = 1e-3                     # at most 0.1 % of the pixels may lie in the band
THINGS = [11, 12, 13, 14, 15, 16, 17, 18]


def crossings():
    """What the GPU shapes cross, by name; test_panoptic_cpu.py asserts that every name is there."""
    out = set()
    for _, _, H, W in PEAK_SHAPES:
        if H > PEAK_TILE_H and W > PEAK_TILE_W:
            out.add("center_peaks: two tiles in both directions")
        if H % PEAK_TILE_H and W % PEAK_TILE_W:
            out.add("center_peaks: partial tiles")
    for B, H, W in GROUP_SHAPES:
        if H * W > PIXEL_CHUNK:
            out.add("group_pixels: more than one workgroup per image")
        if (H * W) % 4:
            out.add("group_pixels: a lane's 4 pixels cross the image's end")
    if any(CENTER_CHUNK < k < 2 * CENTER_CHUNK for k in GROUP_COUNTS):
        out.add("group_pixels: a second centre chunk")
    for B, H, W in OVERLAP_SHAPES:
        if -(-H * W // PIXEL_CHUNK) > OVERLAP_GROUPS_PER_IMAGE:
            out.add("instance_overlap: the stride past 256 workgroups per image")
        if (H * W) % 4:
            out.add("instance_overlap: scalar route")
        else:
            out.add("instance_overlap: vector route")
    for M, C in OVERLAP_SIZES:
        if M * (M + 2 * C) > OVERLAP_MAX_BINS // 2:
            out.add("instance_overlap: more than half the LDS bins")
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def heatmap(shape, seed, step=1.0 / 32):
    """A heat map in [0, 1) quantised to ``step``: many exact ties and plateaus, and values equal to the threshold 0; none
    equals float32(0.1) -- ``heatmap_special`` plants those."""
    rng = np.random.default_rng(seed)
    return (np.floor(rng.random(shape) / step) * step).astype(np.float32)


def heatmap_special(shape, seed):
    """``heatmap`` with the corner values planted where the shape has room: float32(0.1) (equal to the threshold: no peak), a
    plateau of 2.0 across the seam of the first two tiles in x and in y, NaN, +inf and -inf."""
    x = heatmap(shape, seed)
    B, _, H, W = shape
    flat = x.reshape(B, -1)
    n = flat.shape[1]
    flat[:, :: 7] = np.float32(0.1)
    if W > PEAK_TILE_W + 1:
        x[0, 0, H // 4, PEAK_TILE_W - 2:PEAK_TILE_W + 2] = 2.0
    if H > PEAK_TILE_H + 1:
        x[-1, 0, PEAK_TILE_H - 2:PEAK_TILE_H + 2, W // 3] = 2.0
    if n >= 35:
        flat[0, n // 2] = np.nan
        flat[-1, n // 3] = np.inf
        flat[-1, n // 5] = -np.inf
        flat[0, n - 1] = np.nan
    return x


def centers(count, H, W, seed):
    """``count`` distinct centres (y, x) in row-major order, int64 (count, 2); positions repeat when the image is smaller."""
    rng = np.random.default_rng(seed)
    n = H * W
    idx = np.sort(rng.choice(n, size=count, replace=count > n))
    return np.stack([idx // W, idx % W], axis=1).astype(np.int64)


def offsets(shape, seed, kind):
    """(B,2,H,W) float32 offsets: 'int' (integers in [-8, 8]), 'half' / 'quarter' (multiples of 0.5 / 0.25), 'float'
    (arbitrary), 'nan' ('quarter' with a few NaNs and infinities)."""
    rng = np.random.default_rng(seed)
    B, H, W = shape
    if kind == "float":
        return (rng.standard_normal((B, 2, H, W)) * 6).astype(np.float32)
    step = {"int": 1.0, "half": 0.5, "quarter": 0.25, "nan": 0.25}[kind]
    out = (np.round(rng.uniform(-8, 8, (B, 2, H, W)) / step) * step).astype(np.float32)
    if kind == "nan":
        flat = out.reshape(B, 2, -1)
        n = flat.shape[2]
        flat[0, 0, n // 3] = np.nan
        flat[0, 1, n // 2] = np.nan
        flat[-1, 0, n // 4] = np.inf
        flat[-1, 1, n - 1] = -np.inf
    return out


# group_pixels on the GPU: (shape, per-image counts, kind of offsets)
GROUP_GPU_CASES = [((1, 5, 7), [0], "int"), ((1, 5, 7), [1], "int"), ((1, 5, 7), [2], "quarter"),
                   ((2, 37, 53), [0, 99], "quarter"), ((2, 37, 53), [100, 2], "int"), ((2, 37, 53), [99, 100], "float"),
                   ((2, 8, 64), [300, 1], "quarter"), ((2, 8, 64), [99, 99], "float"),
                   ((1, 128, 256), [99], "quarter"), ((1, 128, 256), [300], "int"), ((1, 128, 256), [100], "float"),
                   ((2, 37, 53), [99, 5], "nan")]


def group_gpu_inputs(shape, counts, kind, seed=400):
    """centres (B,Kmax,2) int64 (rows past an image's count hold (H, 0), as ``select_centers`` leaves them), counts (B,) int64
    and offsets (B,2,H,W) of a GROUP_GPU_CASES entry."""
    B, H, W = shape
    kmax = max(max(counts), 1)
    ctr = np.zeros((B, kmax, 2), dtype=np.int64)
    ctr[:, :, 0] = H
    for b, k in enumerate(counts):
        ctr[b, :k] = centers(k, H, W, seed + 11 * b + k)
    return ctr, np.asarray(counts, dtype=np.int64), offsets(shape, seed + 7 + sum(counts), kind)


def labels(shape, seed, classes=19):
    """(B,H,W) int64 labels in runs of a few pixels, with the out-of-range labels 255, -1 and 64 in a few places."""
    rng = np.random.default_rng(seed)
    B, H, W = shape
    runs = rng.integers(0, classes, size=(B, H * W // 3 + 1))
    out = np.repeat(runs, 3, axis=1)[:, :H * W].astype(np.int64)
    out[:, 1::11] = 255
    out[:, 2::13] = -1
    out[:, 3::17] = 64
    return out.reshape(B, H, W)


def distances64(ctr, off):
    """(K, H*W) float64 distances of one image: the yardstick of the band test."""
    _, H, W = off.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    py, px = (y + off[0].astype(np.float64)).reshape(-1), (x + off[1].astype(np.float64)).reshape(-1)
    return np.sqrt((ctr[:, 0:1] - py[None]) ** 2 + (ctr[:, 1:2] - px[None]) ** 2)


def band(ctr, off):
    """Pixels (H*W,) bool whose two smallest float64 distances differ by at most FLOAT_BAND relative, and the two ids."""
    d = distances64(ctr, off)
    order = np.argsort(d, axis=0, kind="stable")[:2]
    d0, d1 = np.take_along_axis(d, order[:1], 0)[0], np.take_along_axis(d, order[1:2], 0)[0]
    return (d1 - d0) <= FLOAT_BAND * d1, order + 1


def ties32(ctr, off):
    """The number of pixels of one image whose minimal fp32 distance is reached by more than one centre."""
    _, H, W = off.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    py, px = (y + off[0]).reshape(-1), (x + off[1]).reshape(-1)
    dy, dx = ctr[:, 0:1].astype(np.float32) - py[None], ctr[:, 1:2].astype(np.float32) - px[None]
    d = np.sqrt(dy * dy + dx * dx)
    return int(((d == d.min(axis=0, keepdims=True)).sum(axis=0) > 1).sum())


def id_maps(shape, seed, M, C, spread=3):
    """Four (B,H,W) int64 maps for instance_overlap: ids mostly 0 with blocks of instances, classes in runs; ids and classes
    outside [0, M) / [0, C) in a few places (``spread`` more ids and classes than fit, and negatives)."""
    rng = np.random.default_rng(seed)
    B, H, W = shape
    n = H * W
    def ids():
        out = np.zeros((B, n), dtype=np.int64)
        blocks = rng.integers(0, M + spread, size=(B, n // 16 + 1))
        keep = rng.random((B, n // 16 + 1)) < 0.3
        out[:] = np.repeat(np.where(keep, blocks, 0), 16, axis=1)[:, :n]
        out[:, 5::97] = -1
        return out.reshape(B, H, W)
    def cls():
        out = np.repeat(rng.integers(0, C + spread, size=(B, n // 5 + 1)), 5, axis=1)[:, :n].astype(np.int64)
        out[:, 7::89] = 255
        out[:, 9::83] = -3
        return out.reshape(B, H, W)
    return ids(), ids(), cls(), cls()


def overlap_ref(pred_inst, tgt_inst, pred_seg, tgt_seg, M, C):
    """cerberus::instance_overlap with ``np.add.at``."""
    B = pred_inst.shape[0]
    inter, pc, tc = np.zeros((B, M, M), np.int64), np.zeros((B, M, C), np.int64), np.zeros((B, M, C), np.int64)
    for b in range(B):
        pi, ti, ps, ts = (a[b].reshape(-1) for a in (pred_inst, tgt_inst, pred_seg, tgt_seg))
        ok = (pi >= 0) & (pi < M) & (ti >= 0) & (ti < M)
        np.add.at(inter[b], (pi[ok], ti[ok]), 1)
        okp, okt = ok & (ps >= 0) & (ps < C), ok & (ts >= 0) & (ts < C)
        np.add.at(pc[b], (pi[okp], ps[okp]), 1)
        np.add.at(tc[b], (ti[okt], ts[okt]), 1)
    return inter, pc, tc


# ---- the golden cases (tools/gen_golden_panoptic.py runs the reference on them) ------------------------------------------------------
# find_instance_center: (name, shape, seed, kwargs); 'tied': every peak has the value 1.0; 'plateau': a 3 x 3 block of equal maxima
CENTER_CASES = [("k3", (1, 1, 12, 20), 100, dict(nms_kernel=3)),
                ("k7", (1, 1, 12, 20), 101, dict(nms_kernel=7)),
                ("k7_3d", (1, 12, 20), 101, dict(nms_kernel=7, threshold=0.3)),
                ("top_below", (1, 1, 12, 20), 102, dict(nms_kernel=3, top_k=4)),
                ("top_equal", (1, 1, 12, 20), 102, dict(nms_kernel=3, top_k=None)),      # top_k is set to the peak count
                ("top_above", (1, 1, 12, 20), 102, dict(nms_kernel=3, top_k=200)),
                ("tied", (1, 1, 16, 24), 103, dict(nms_kernel=3, top_k=10)),
                ("plateau", (1, 1, 12, 20), 104, dict(nms_kernel=3))]


def center_case_input(name, shape, seed):
    x = heatmap(shape, seed, step=1.0 / 1024)
    if name == "tied":
        x = np.zeros(shape, dtype=np.float32)
        x.reshape(-1)[:: 9] = 1.0                     # 43 isolated-or-not peaks of value 1.0
    if name == "plateau":
        x[..., 4:7, 8:11] = 1.5
    return x


# group_pixels: (name, (H, W), K, kind, seed)
GROUP_CASES = [("int", (9, 14), 5, "int", 200), ("half", (9, 14), 7, "half", 201), ("float", (11, 13), 6, "float", 202),
               ("nan", (9, 14), 5, "nan", 203), ("k1", (5, 7), 1, "quarter", 204)]


def group_case_input(H, W, K, kind, seed):
    return centers(K, H, W, seed + 50), offsets((1, H, W), seed, kind)


def pq_case_maps(name):
    """Crafted (1,H,W) id and class maps for calculate_pq: pred_inst, pred_seg, target_inst, target_seg."""
    H, W = 8, 12
    pi, ti = np.zeros((1, H, W), np.int64), np.zeros((1, H, W), np.int64)
    ps, ts = np.full((1, H, W), 3, np.int64), np.full((1, H, W), 3, np.int64)
    if name == "nan":
        return pi, ps, ti, ts
    if name == "plain":                                # one good match, one miss on each side
        pi[0, 1:4, 1:5], ti[0, 1:4, 1:6] = 1, 1
        pi[0, 5:7, 8:11], ti[0, 5:8, 0:3] = 2, 2
        ps[pi > 0], ts[ti > 0] = 13, 13
    if name == "background":                           # the prediction covers almost everything, the target has no instance there
        pi[0, :, :] = 1
        pi[0, 0, 0:2] = 0
        ti[0, 7, 10:12] = 1
        ps[pi > 0], ts[ti > 0] = 11, 11
    if name == "demotion":                             # a match whose majority classes differ, a match that agrees, label 255
        pi[0, 1:4, 1:5], ti[0, 1:4, 1:5] = 1, 1
        pi[0, 5:8, 6:10], ti[0, 5:8, 6:11] = 2, 3
        ps[0, 1:4, 1:5], ts[0, 1:4, 1:5] = 13, 13
        ps[0, 1, 1] = 14
        ps[0, 5:8, 6:10], ts[0, 5:8, 6:11] = 12, 15
        ts[0, 0, :] = 255
    if name == "no_zero":                              # no background pixel on the prediction's side
        pi[0, :, :6], pi[0, :, 6:] = 1, 2
        ti[0, :, :6], ti[0, :, 6:] = 4, 0
        ps[:], ts[:] = 11, 11
    return pi, ps, ti, ts


PQ_CASES = ["nan", "plain", "background", "demotion", "no_zero"]


def scene(seed=300, H=40, W=72, classes=19):
    """A two-image scene for PanopticMetric: ``predictions`` and ``targets`` as dicts of numpy arrays (``center_points`` a list
    of lists).  Offsets are multiples of 0.25, so that every distance is exact in fp32.  Image 0: four target instances, of which
    the prediction finds one well, one shifted, one with the wrong class and misses one; image 1: two instances, one found."""
    rng = np.random.default_rng(seed)
    B = 2
    boxes = [[(4, 14, 5, 20, 13), (6, 16, 30, 44, 11), (22, 34, 8, 24, 15), (24, 36, 50, 66, 17)],
             [(5, 17, 10, 26, 12), (20, 32, 40, 60, 18)]]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tgt_seg = np.repeat(rng.integers(0, 11, size=(B, H, W // 8)), 8, axis=2).astype(np.int64)
    tgt_seg[:, :2, :] = 255
    pred_lab = tgt_seg.copy()
    pred_lab[pred_lab == 255] = 0
    tgt_ctr, pred_ctr = np.zeros((B, 1, H, W), np.float32), np.zeros((B, 1, H, W), np.float32)
    tgt_off, points = np.zeros((B, 2, H, W), np.float32), [[], []]
    pred_off = np.zeros((B, 2, H, W), np.float32)
    for b in range(B):
        for k, (y0, y1, x0, x1, cls) in enumerate(boxes[b]):
            cy, cx = (y0 + y1) // 2, (x0 + x1) // 2
            inside = (yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)
            tgt_seg[b][inside] = cls
            blob = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 8.0).astype(np.float32)
            tgt_ctr[b, 0] = np.maximum(tgt_ctr[b, 0], blob)
            tgt_off[b, 0][inside], tgt_off[b, 1][inside] = (cy - yy)[inside], (cx - xx)[inside]
            points[b].append([int(cy), int(cx)])
            if (b, k) in ((0, 3), (1, 1)):             # missed by the prediction
                continue
            dy, dx = (3, 2) if (b, k) == (0, 1) else (0, 0)       # a shifted instance
            moved = (yy >= y0 + dy) & (yy < y1 + dy) & (xx >= x0 + dx) & (xx < x1 + dx)
            pred_lab[b][moved] = 16 if (b, k) == (0, 2) else cls  # a wrong class
            pred_ctr[b, 0] = np.maximum(pred_ctr[b, 0], np.float32(0.9) * np.roll(blob, (dy, dx), axis=(0, 1)))
            pred_off[b, 0][moved], pred_off[b, 1][moved] = (cy + dy - yy)[moved], (cx + dx - xx)[moved]
    pred_ctr += (rng.random((B, 1, H, W)) * 0.05).astype(np.float32)
    pred_off += (np.round(rng.uniform(-1, 1, (B, 2, H, W)) * 4) / 4).astype(np.float32)
    logits = (rng.random((B, classes, H, W)) * 0.5).astype(np.float32)
    np.put_along_axis(logits, pred_lab[:, None], 2.0, axis=1)
    predictions = {"seg": logits, "center": pred_ctr, "offset": pred_off}
    targets = {"seg": tgt_seg, "center": tgt_ctr, "offset": tgt_off, "center_points": points}
    return predictions, targets
