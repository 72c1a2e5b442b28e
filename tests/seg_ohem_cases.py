"""Inputs of the OHEM cross-entropy tests, shared by tests/test_seg_ohem_cpu.py, tests/test_seg_ohem_gpu.py and the generator
of tests/golden/seg_ohem.npz (tools/gen_golden_seg_ohem.py): everything comes from ``hash_uniform`` seeds.

Confident logits: those of ``seg_loss_cases`` plus ``BOOST`` on the target's plane at the valid pixels where a third hash
field is below ``CONFIDENT_SHARE``.  Most target probabilities then sit above 0.99, so a large ``min_kept`` puts the
``min_kept``-th smallest probability inside a dense cluster of keys that share their leading digits: the radix select has to
go down to its last digit.

The constants of csrc/seg_ohem.hip that decide which path a case takes are exported by ``cerberusnet_amd.ops``
(``OHEM_DIGIT_BITS``, ``OHEM_BINS``, ``SEG_CHUNK_PIXELS``); ``tiers`` below names the paths from them."""
import functools

import numpy as np

import seg_loss_cases
from cerberusnet_amd import ops
from cerberusnet_amd.synth import hash_uniform

IGNORE = 255
BOOST = 8.0
CONFIDENT_SHARE = 0.7
LOGIT_SEED, LABEL_SEED = 1300, 1310
CONFIDENT_SEED = 1313      # the third hash field (the labels take 1310 and 1311); with it the small rows' kept sets are at least
#                            1.7e-4 (relative, in float64) from changing, 100 times the fp32 softmax's own error
FINISH_THREADS = 256          # loss_reduce.h `constexpr int kReduceThreads = 256`: `i += kThreads` of ohem_final_kernel

# (shape (B,C,H,W), thresh, min_kept, small): the small rows are pinned to the reference's kept sets (the golden file)
ROWS = [((2, 19, 37, 53), 0.7, 256, True),
        ((2, 19, 37, 53), 0.7, 2000, True),
        ((2, 19, 8, 64), 0.7, 600, True),
        ((2, 2, 129, 1028), 0.7, 150000, False),
        ((1, 3, 601, 1023), 0.7, 400000, False),
        ((1, 3, 601, 1023), 0.9, 100, False)]
SMALL_SHAPES = [(2, 19, 37, 53), (2, 19, 8, 64)]      # scalar and vector route

# the golden cases: (class name, shape, constructor keywords, number of heads).  `min_kept` 10 ** 6 is min_kept >= num_valid;
# a use_weight=True case runs with the reference's own 19 weights, which the golden file holds as data
GOLDEN_CASES = [("SoftmaxCrossEntropyOHEMLoss", (2, 19, 37, 53), dict(ignore_label=255, thresh=0.7, min_kept=256, use_weight=True), 1),
                ("SoftmaxCrossEntropyOHEMLoss", (2, 19, 37, 53), dict(ignore_label=255, thresh=0.7, min_kept=2000, use_weight=False), 1),
                ("SoftmaxCrossEntropyOHEMLoss", (2, 19, 8, 64), dict(ignore_label=255, thresh=0.7, min_kept=600, use_weight=True), 1),
                ("SoftmaxCrossEntropyOHEMLoss", (2, 19, 8, 64), dict(ignore_label=255, thresh=0.7, min_kept=10 ** 6, use_weight=True), 1),
                ("SoftmaxCrossEntropyOHEMLoss", (2, 19, 8, 64), dict(ignore_label=255, thresh=0.7, min_kept=0, use_weight=False), 1),
                ("MixSoftmaxCrossEntropyOHEMLoss", (2, 19, 8, 64), dict(ignore_index=255, thresh=0.7, min_kept=600, use_weight=True), 1),
                ("MixSoftmaxCrossEntropyOHEMLoss", (2, 19, 37, 53),
                 dict(aux=True, aux_weight=0.4, ignore_index=255, thresh=0.7, min_kept=2000, use_weight=False), 2)]


@functools.lru_cache(maxsize=None)
def _inputs(shape, head):
    B, C, H, W = shape
    t = seg_loss_cases.labels(shape, LABEL_SEED, IGNORE)
    if t.reshape(-1)[0] == IGNORE:
        t.reshape(-1)[0] = 0
    x = seg_loss_cases.logits(shape, LOGIT_SEED + 100 * head)
    sure = (t != IGNORE) & (hash_uniform((B, H, W), CONFIDENT_SEED + 100 * head, 0.0, 1.0) < CONFIDENT_SHARE)
    b, h, w = np.nonzero(sure)
    x[b, t[b, h, w], h, w] += np.float32(BOOST)
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t


def inputs(shape, head=0):
    """(logits (B,C,H,W) float32, labels (B,H,W) int64) of a shape; ``head`` > 0 gives other logits for the same labels (the
    aux heads).  Computed once and shared: the arrays are read-only, copy before writing."""
    return _inputs(tuple(shape), head)


def class_weights(C):
    """Class weights in [0.5, 2), none of them 0."""
    return hash_uniform((C,), 1320, 0.5, 2.0)


def prob64(x, t):
    """(prob (B,H,W) float64, valid): the target probability in float64, -1 where the pixel is not valid."""
    B, C, H, W = x.shape
    v = x.astype(np.float64)
    m = v.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(v - m)
        p = e / e.sum(axis=1, keepdims=True)
    valid = (t != IGNORE) & (t >= 0) & (t < C)
    safe = np.where(valid, t, 0)
    return np.where(valid, np.take_along_axis(p, safe[:, None], 1)[:, 0], -1.0), valid


def prob32_numpy(x):
    """The reference's own fp32 softmax (seg_losses.py:66-68 in its operation order), (B,C,H,W)."""
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def keys(prob):
    """The select's sort keys of valid probabilities: the bit pattern, all ones for a NaN."""
    p = np.asarray(prob, dtype=np.float32)
    return np.where(np.isnan(p), np.uint32(0xffffffff), p.view(np.uint32))


def radix_select(key, k, bits=None):
    """The digit-wise select of csrc/seg_ohem.hip as a numpy model: (the k-th smallest key (k 1-based), the rank left among the
    keys equal to it, the number of keys that shared the prefix when each digit was counted)."""
    bits = ops.OHEM_DIGIT_BITS if bits is None else bits
    assert sum(bits) == 32 and all(1 << b <= ops.OHEM_BINS for b in bits)
    key = np.asarray(key, dtype=np.uint32)
    assert 1 <= k <= key.size
    prefix, low, rank, live, counted = 0, 32, int(k), np.ones(key.size, dtype=bool), []
    for b in bits:
        low -= b
        counted.append(int(live.sum()))
        digit = (key[live] >> np.uint32(low)) & np.uint32((1 << b) - 1)
        cum = np.cumsum(np.bincount(digit, minlength=1 << b))
        d = int(np.searchsorted(cum, rank))               # the first bin whose running count reaches the rank
        rank -= int(cum[d - 1]) if d else 0
        prefix |= d << low
        live &= (key >> np.uint32(low)) == np.uint32(prefix >> low)
    return np.uint32(prefix), rank, counted


def expected_threshold(prob, thresh, min_kept, dtype=np.float32):
    """(threshold, keep_all) of the selection from the valid probabilities (NaN allowed), compared in ``dtype``."""
    p = np.asarray(prob, dtype=dtype).reshape(-1)
    th = dtype(np.float32(thresh))
    if min_kept >= p.size:
        return dtype(np.inf), True
    if min_kept > 0:
        kth = np.sort(p)[min_kept - 1]                    # NaN sorts last
        return (kth if kth > th else th), False
    return th, False


def tiers(row):
    """The paths of csrc/seg_ohem.hip that a row reaches, from the exported constants and the row's own float64 probabilities."""
    shape, thresh, min_kept, _small = row
    B, C, H, W = shape
    x, t = inputs(shape)
    p, valid = prob64(x, t)
    pv = p[valid].astype(np.float32)
    n = (B * H * W + ops.SEG_CHUNK_PIXELS - 1) // ops.SEG_CHUNK_PIXELS
    out = {"vector" if H * W % 4 == 0 else "scalar"}
    if min_kept >= pv.size:
        out.add("branch: keep all")
    elif min_kept > 0:
        kth, rank, counted = radix_select(keys(pv), min_kept)
        out.add("branch: kth" if kth.view(np.float32) > np.float32(thresh) else "branch: thresh")
        if counted[-1] > 1 and len(np.unique(keys(pv)[(keys(pv) >> np.uint32(ops.OHEM_DIGIT_BITS[-1])) ==
                                                      (kth >> np.uint32(ops.OHEM_DIGIT_BITS[-1]))])) > 1:
            out.add("last digit decides")
    else:
        out.add("branch: thresh")
    if n > FINISH_THREADS:
        out.add("more than 256 chunks")
    if n > 2 * FINISH_THREADS:
        out.add("more than 512 chunks")
    if B > 1 and (H * W) % ops.SEG_CHUNK_PIXELS:
        out.add("image boundary inside a chunk")
    return out


TIERS = ["vector", "scalar", "branch: keep all", "branch: kth", "branch: thresh", "last digit decides", "more than 256 chunks",
         "more than 512 chunks", "image boundary inside a chunk"]
# rows beyond ROWS that the GPU tests add on the small shapes, by (shape, thresh, min_kept)
EXTRA_ROWS = [((2, 19, 8, 64), 0.7, 10 ** 6, True), ((2, 19, 8, 64), 0.7, 0, True)]


def nearest_gap(prob, valid, threshold):
    """The smallest relative distance of a valid probability to the threshold, the pixels AT the threshold excepted: with
    float64 probabilities and the threshold selected from them, how far the kept set is from changing."""
    p = prob[valid]
    d = np.abs(p - threshold) / threshold
    d = d[p != threshold]
    return float(d.min()) if d.size else np.inf


def marker_inputs(shape, chunks_planted):
    """(logits, labels, planted pixels): every pixel easy (its target 12 above the rest) except one hard pixel inside each of
    ``chunks_planted`` (its target 6 below the rest); labels ``p % C`` everywhere, none ignored."""
    B, C, H, W = shape
    n = B * H * W
    t = (np.arange(n) % C).astype(np.int64).reshape(B, H, W)
    x = np.zeros(shape, dtype=np.float32)
    b, h, w = np.indices((B, H, W)).reshape(3, -1)
    x[b, t.reshape(-1), h, w] = 12.0
    planted = []
    for k in chunks_planted:
        p = min(k * ops.SEG_CHUNK_PIXELS + (37 * k + 5) % ops.SEG_CHUNK_PIXELS, n - 1)
        x[b[p], t.reshape(-1)[p], h[p], w[p]] = -6.0
        planted.append(p)
    return x, t, planted
