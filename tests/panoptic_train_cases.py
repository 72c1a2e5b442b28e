"""Inputs of the panoptic training tests (tests/test_panoptic_train_cpu.py, test_panoptic_train_gpu.py) and of
tools/gen_golden_panoptic_train.py, which runs the reference's PanopticTargetGenerator and DeeplabPanopticLoss on them and
writes tests/golden/panoptic_train.npz.  Everything here is deterministic numpy; the float64 evaluations of the loss and the
closed-form integer model of the 2048 x 2048 target case are written out here, not taken from the code under test."""
import functools

import numpy as np

from cerberusnet_amd.synth import hash_uniform

THINGS = [11, 12, 13, 14, 15, 16, 17, 18]
IGNORE = 255
BIG_ID = (1 << 24) + 5          # an id that float32 cannot hold
ITEMS = ["semantic", "foreground", "center", "offset", "semantic_mask", "center_mask", "offset_mask"]


def _rect(ids, y0, y1, x0, x1, value):
    ids[y0:y1, x0:x1] = value


def _seg(id_, cat, crowd=0):
    return {"id": int(id_), "category_id": int(cat), "iscrowd": int(crowd)}


def _tiny():
    ids = np.zeros((5, 7), dtype=np.int64)
    _rect(ids, 1, 4, 2, 6, 11000)
    ids[1, 2] = 0                               # an L-shaped corner: the centre is no integer
    return [ids], [[_seg(11000, 11)]]


def _scalar():
    """(2,37,53): image 0 has three live rows and a padded row whose id occurs in the map; image 1 has no live row at all."""
    a = np.full((37, 53), 7000, dtype=np.int64)                 # stuff
    _rect(a, 3, 20, 4, 30, BIG_ID)                              # a thing with an id above 2^24
    _rect(a, 5, 9, 6, 11, 7000)                                 # ... with a hole
    _rect(a, 22, 35, 30, 50, 13001)                             # a crowd thing
    _rect(a, 30, 37, 0, 9, 12002)                               # a thing that only the padded row names
    b = np.full((37, 53), 7000, dtype=np.int64)
    _rect(b, 10, 20, 10, 20, 13001)
    segs0 = [_seg(BIG_ID, 11), _seg(7000, 7), _seg(13001, 13, 1)]
    return [a, b], [segs0, []], [[_seg(12002, 12)], [_seg(7000, 7), _seg(13001, 13), _seg(12002, 12), _seg(BIG_ID, 11)]]


def _vector():
    a = np.zeros((8, 64), dtype=np.int64)
    _rect(a, 0, 8, 0, 20, 8000)                                 # stuff
    _rect(a, 1, 6, 22, 41, 14001)                               # a thing whose quads straddle its border
    a[5, 40] = 0
    _rect(a, 2, 8, 45, 63, 15001)                               # a crowd thing
    b = np.zeros((8, 64), dtype=np.int64)
    _rect(b, 0, 3, 1, 7, 14001)
    _rect(b, 4, 8, 30, 64, 8000)
    b[7, 63] = 16001                                            # a one-pixel thing in the last pixel
    segs0 = [_seg(8000, 8), _seg(14001, 14), _seg(15001, 15, 1)]
    segs1 = [_seg(16001, 16), _seg(14001, 14), _seg(8000, 8)]
    return [a, b], [segs0, segs1]


SMALL_AREA = 12


def _big():
    """(1,67,131): windows clipped on all four borders, two overlapping windows, a crowd thing, a stuff segment, a live row whose
    id is absent, a map id without a row, an instance of exactly SMALL_AREA pixels and one of a pixel less."""
    a = np.full((67, 131), 9000, dtype=np.int64)                # stuff
    _rect(a, 0, 9, 0, 12, 11001)                                # top left: clipped above and on the left
    a[0, 0:5] = 9000
    _rect(a, 58, 67, 118, 131, 11002)                           # bottom right: clipped below and on the right
    a[66, 128:131] = 9000
    _rect(a, 24, 37, 40, 61, 12001)                             # two things whose windows overlap
    _rect(a, 28, 41, 62, 80, 12002)
    a[40, 62:70] = 9000
    _rect(a, 45, 60, 20, 50, 13001)                             # a crowd thing
    _rect(a, 10, 20, 90, 120, 5)                                # an id that no row names
    _rect(a, 50, 53, 70, 74, 14001)                             # exactly SMALL_AREA pixels: not small
    _rect(a, 50, 53, 80, 84, 14002)                             # one pixel less: small
    a[52, 83] = 9000
    segs = [_seg(9000, 9), _seg(11001, 11), _seg(11002, 11), _seg(12001, 12), _seg(99999, 12), _seg(12002, 12), _seg(13001, 13, 1),
            _seg(14001, 14), _seg(14002, 14)]
    return [a], [segs]


def _kw(sigma=8, stuff=False, crowd=False, area=0, weight=1):
    return dict(ignore_label=IGNORE, thing_list=THINGS, sigma=sigma, ignore_stuff_in_offset=stuff, small_instance_area=area,
                small_instance_weight=weight, ignore_crowd_in_semantic=crowd)


# name -> (builder, keyword arguments); a builder returns (maps, live segments per image[, what the padded rows hold])
TARGET_CASES = {
    "tiny": (_tiny, _kw()),
    "scalar": (_scalar, _kw(sigma=3)),
    "vector": (_vector, _kw(sigma=2)),
    "vector_flags": (_vector, _kw(sigma=2, stuff=True, crowd=True)),
    "big": (_big, _kw(area=SMALL_AREA, weight=3)),
    "big_s2": (_big, _kw(sigma=2, stuff=True, crowd=True, area=SMALL_AREA, weight=3)),
}


@functools.lru_cache(maxsize=None)
def target_case(name):
    """(ids (B,H,W) int64, seg_ids, seg_category, seg_iscrowd (B,S) int64, seg_count (B,) int64, segments per image, kwargs)."""
    builder, kwargs = TARGET_CASES[name]
    built = builder()
    maps, segs = built[0], built[1]
    pads = built[2] if len(built) > 2 else [[] for _ in maps]
    S = max(1, max(len(s) + len(p) for s, p in zip(segs, pads)))
    table = np.zeros((3, len(maps), S), dtype=np.int64)
    for b, (live, pad) in enumerate(zip(segs, pads)):
        for i, seg in enumerate(list(live) + list(pad)):
            table[:, b, i] = seg["id"], seg["category_id"], seg["iscrowd"]
    count = np.asarray([len(s) for s in segs], dtype=np.int64)
    return np.stack(maps), table[0], table[1], table[2], count, segs, kwargs


def colour(ids):
    """The (H,W,3) int32 array the reference's rgb2id decodes to ``ids`` (its last channel exceeds 255 for an id above 2^24)."""
    ids = np.asarray(ids, dtype=np.int32)
    return np.stack([ids % 256, ids // 256 % 256, ids // 65536], -1).astype(np.int32)


def widened(name, S):
    """The tables of a case padded to S rows with the real rows LAST: S - n live filler rows of stuff whose ids occur nowhere."""
    ids, sid, cat, crowd, count, _, kwargs = target_case(name)
    B, n = sid.shape
    assert all(int(c) == n for c in count), "widened() needs a case whose rows are all live"
    fill = S - n
    wide = np.zeros((3, B, S), dtype=np.int64)
    wide[0, :, :fill] = 500000 + np.arange(fill)
    wide[1, :, :fill] = 9
    wide[0, :, fill:], wide[1, :, fill:], wide[2, :, fill:] = sid, cat, crowd
    return ids, wide[0], wide[1], wide[2], np.full((B,), S, dtype=np.int64), kwargs


# ---- the 2048 x 2048 case: a closed-form integer model ------------------------------------------------------------------------
# one instance over the whole image: sum y = W H (H - 1) / 2 is 2^32 - 2^21 at 2048 x 2048 (past any signed 32-bit sum, a hair
# below an unsigned one) and passes 2^32 at 2112 x 2048
HUGE_SHAPES = [(2048, 2048), (2112, 2048)]
HUGE_SMALL = (100, 103, 200, 205)           # rows 100..102, columns 200..204 of a second thing


def huge_case(shape):
    H, W = shape
    ids = np.full((1, H, W), 11007, dtype=np.int64)
    y0, y1, x0, x1 = HUGE_SMALL
    ids[0, y0:y1, x0:x1] = 12009
    table = np.asarray([[[11007, 12009]], [[11, 12]], [[0, 0]]], dtype=np.int64)
    return ids, table[0], table[1], table[2], np.asarray([2], dtype=np.int64), _kw(sigma=8, area=16, weight=3)


def huge_expected(shape, gauss):
    """center_points, offset, center and semantic_mask of ``huge_case`` from integer arithmetic: the sums of an arithmetic
    series, one float64 division per centre, one float64 subtraction rounded to float32 per pixel."""
    H, W = shape
    y0, y1, x0, x1 = HUGE_SMALL
    n_small = (y1 - y0) * (x1 - x0)
    sy_small = sum(range(y0, y1)) * (x1 - x0)
    sx_small = sum(range(x0, x1)) * (y1 - y0)
    sy_all, sx_all = H * (H - 1) // 2 * W, W * (W - 1) // 2 * H
    n_big = H * W - n_small
    assert sy_all - sy_small > (1 << 32 if H > 2048 else 1 << 31)
    centres = np.asarray([[float(sy_all - sy_small) / float(n_big), float(sx_all - sx_small) / float(n_big)],
                          [float(sy_small) / float(n_small), float(sx_small) / float(n_small)]], dtype=np.float64)
    small = np.zeros((H, W), dtype=bool)
    small[y0:y1, x0:x1] = True
    ys = np.arange(H, dtype=np.float64)[:, None]
    xs = np.arange(W, dtype=np.float64)[None, :]
    offset = np.empty((1, 2, H, W), dtype=np.float32)
    offset[0, 0] = np.where(small, centres[1, 0] - ys, centres[0, 0] - ys).astype(np.float32)
    offset[0, 1] = np.where(small, centres[1, 1] - xs, centres[0, 1] - xs).astype(np.float32)
    center = np.zeros((H, W), dtype=np.float32)
    size = gauss.shape[0]
    reach = size // 2
    for cy, cx in centres:
        top, left = int(cy) - reach, int(cx) - reach
        a, b, c, d = max(top, 0), min(top + size, H), max(left, 0), min(left + size, W)
        center[a:b, c:d] = np.maximum(center[a:b, c:d], gauss[a - top:b - top, c - left:d - left])
    semantic_mask = np.where(small, np.float32(3), np.float32(1)).astype(np.float32)          # 15 pixels < 16: small
    return centres, offset, center[None, None], semantic_mask[None]


# ---- the loss -------------------------------------------------------------------------------------------------------------------
CENTER_WEIGHT, OFFSET_WEIGHT = 200.0, 0.1
MASK_COMBOS = [(False, False), (True, False), (False, True), (True, True)]
GOLDEN_LOSS_SHAPE = (2, 5, 7)
# (B,H,W): scalar route, vector route, and the two shapes at which the finish reads more than one partial per thread
LOSS_SHAPES_SCALAR = [(1, 1, 1), (1, 5, 7), (2, 37, 53), (1, 3, 66)]
LOSS_SHAPES_VECTOR = [(1, 1, 4), (2, 8, 64), (3, 16, 33)]
LOSS_TIER_SHAPES = [(1, 257, 1024), (1, 601, 1023)]
LOSS_CHUNK = 1024             # panoptic_train.hip `kChunk`; ops.PANOPTIC_CHUNK_PIXELS restates it
FINISH_THREADS = 256          # loss_reduce.h `kReduceThreads`: `i += kThreads` of ploss_final_kernel
LOSS_TIERS = ["ploss_final second step, vector", "ploss_final second step, scalar", "ploss_final third step, vector",
              "ploss_final third step, scalar"]


def loss_tiers(shape):
    B, H, W = shape
    route = "vector" if H * W % 4 == 0 else "scalar"
    out = set()
    for n in ((B * H * W + LOSS_CHUNK - 1) // LOSS_CHUNK, (2 * B * H * W + LOSS_CHUNK - 1) // LOSS_CHUNK):
        if n > FINISH_THREADS:
            out.add("ploss_final second step, %s" % route)
        if n > 2 * FINISH_THREADS:
            out.add("ploss_final third step, %s" % route)
    return out


@functools.lru_cache(maxsize=None)
def loss_inputs(shape, seed=5100):
    """(center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask) float32; the masks hold 0 on about a third
    of the pixels and the weights 0.5, 1 and 3 elsewhere; every fifth offset prediction equals its target exactly (a tie of the
    L1 term).  Shared and never written to."""
    B, H, W = shape
    cp = hash_uniform((B, 1, H, W), seed, 0.0, 1.0)
    ct = hash_uniform((B, 1, H, W), seed + 1, 0.0, 1.0)
    op = hash_uniform((B, 2, H, W), seed + 2, -40.0, 40.0)
    ot = hash_uniform((B, 2, H, W), seed + 3, -40.0, 40.0)
    tie = (np.arange(op.size) % 5 == 0).reshape(op.shape)
    op = np.where(tie, ot, op).astype(np.float32)

    def mask(s):
        u = hash_uniform((B, H, W), s, 0.0, 1.0)
        return np.select([u < 0.35, u < 0.6, u < 0.8], [0.0, 0.5, 1.0], 3.0).astype(np.float32)
    return cp, ct, mask(seed + 4), op, ot, mask(seed + 5)


def loss64(cp, ct, cm, op, ot, om, cw, ow, mode):
    """(loss, grad_center, grad_offset) in float64; ``mode`` 'reference' or 'pixel'; a mask may be None."""
    def term(p, t, m, weight, absolute):
        d = p.astype(np.float64) - t.astype(np.float64)
        f = np.abs(d) if absolute else d * d
        slope = np.sign(d) if absolute else 2.0 * d
        if m is None:
            return weight * f.mean(), weight * slope / d.size
        m = np.broadcast_to(m.astype(np.float64)[:, None], d.shape)
        total = m.sum()
        if not total > 0:
            return 0.0, np.zeros_like(d)
        if mode == "reference":
            return weight * f.mean(), weight * slope / d.size
        keep = m != 0
        return weight * np.where(keep, m * np.where(keep, f, 0.0), 0.0).sum() / total, np.where(keep, weight * m * np.where(keep, slope, 0.0) / total, 0.0)
    lc, gc = term(cp, ct, cm, cw, False)
    lo, go = term(op, ot, om, ow, True)
    return lc + lo, gc, go
