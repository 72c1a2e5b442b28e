"""GPU tests of the OHEM cross-entropy (csrc/seg_ohem.hip): ``cerberus::seg_ohem_cross_entropy``, ``seg_ohem_cross_entropy``
and the classes ``SoftmaxCrossEntropyOHEMLoss`` / ``MixSoftmaxCrossEntropyOHEMLoss``.

The selection is checked EXACTLY, with no band, against the op's own ``prob`` output: the threshold is
``max(thresh, sort(prob[valid])[min_kept - 1])`` bit for bit and the counts are those recomputed from ``prob``.  ``prob`` itself
is checked against float64 with a bound of four times numpy-fp32's own worst error on the same inputs (the reference computes
its softmax in numpy fp32; about 2e-6).  Only the small rows of tests/seg_ohem_cases.py compare kept sets with the reference
(tests/golden/seg_ohem.npz), after asserting that every probability is at least 25 bounds from the threshold; on the large rows
fp32 numpy itself disagrees with float64 about the set, so loss and gradient are compared with a float64 evaluation over the
op's own kept mask.  Tolerances of tests/test_seg_loss_gpu.py: value 1e-5 relative; gradient ``l2_err`` and ``rel_err`` each at
most 4 x max(e_stock, 2^-23) with e_stock the error of the stock fp32 chain (or of the golden fp32 gradient) on the same mask.

Measured on an MI355X: see the docstring of ``test_prob_against_float64``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cerberusnet_amd as ca
import reduction_cases as rc
import seg_ohem_cases as oc
from cerberusnet_amd import ops
from conftest import l2_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_TOL = 1e-5
GRAD_FACTOR = 4.0
GRAD_FLOOR = 2.0 ** -23
IGNORE = oc.IGNORE


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)           # a copy: the shared inputs are read-only


def run_op(x, t, w, thresh, min_kept, grad=True, ignore=IGNORE):
    """The raw op on numpy inputs: a dict of numpy outputs, ``kept`` re-derived from prob as the backward does."""
    xd = dev(x).requires_grad_(grad)
    wd = dev(np.ones(x.shape[1], dtype=np.float32) if w is None else w)
    loss, prob, lse, state, counts = torch.ops.cerberus.seg_ohem_cross_entropy(xd, dev(t), wd, ignore, thresh, min_kept)
    out = dict(loss=loss.detach().cpu().numpy(), prob=prob.cpu().numpy(), lse=lse.cpu().numpy(), state=state.cpu().numpy(),
               counts=counts.cpu().numpy())
    if grad:
        out["grad"] = torch.autograd.grad(loss, xd)[0].cpu().numpy()
    p = out["prob"]
    out["valid"] = ~(p < 0)
    with np.errstate(invalid="ignore"):
        out["kept"] = out["valid"] if out["state"][4] != 0 else (p >= 0) & (p <= out["state"][3])
    return out


def check_selection(name, out, t, C, thresh, min_kept):
    """Threshold bit for bit and both counts, from the op's own prob."""
    valid = (t != IGNORE) & (t >= 0) & (t < C)
    assert np.array_equal(out["valid"], valid), name
    assert np.all(out["prob"][~valid] == -1.0), name
    pv = out["prob"][valid]
    want, keep_all = oc.expected_threshold(pv, thresh, min_kept)
    got = out["state"][3]
    print("%s: threshold %.9g (want %.9g), num_valid %d, num_kept %d, rank among ties %g" %
          (name, got, want, out["counts"][0], out["counts"][1], out["state"][5]))
    assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32), (name, got, want)
    assert (out["state"][4] != 0) == keep_all, name
    assert out["counts"][0] == valid.sum(), name
    with np.errstate(invalid="ignore"):
        assert out["counts"][1] == (valid.sum() if keep_all else (pv <= want).sum()), name
    assert out["counts"][1] == out["kept"].sum(), name
    if not keep_all and 0 < min_kept <= (~np.isnan(pv)).sum():      # a NaN kth gives thresh: fewer than min_kept may be kept
        assert out["counts"][1] >= min_kept, name
        if want > np.float32(thresh):                  # the kth branch: the rank left counts min_kept among the ties at kth
            assert out["state"][5] == min_kept - (pv < want).sum(), name
    return want


# ---- 1. the selection, exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", oc.ROWS + oc.EXTRA_ROWS, ids=lambda r: "%s-%g-%d" % (r[0], r[1], r[2]))
def test_selection_is_exact_on_every_row(row):
    shape, thresh, min_kept, _small = row
    x, t = oc.inputs(shape)
    out = run_op(x, t, None, thresh, min_kept, grad=False)
    check_selection(str(row), out, t, shape[1], thresh, min_kept)
    reached = oc.tiers(row)
    if "branch: kth" in reached:
        assert out["state"][3] > np.float32(thresh)
    if "branch: thresh" in reached:
        assert out["state"][3] == np.float32(thresh)


@pytest.mark.parametrize("shape", oc.SMALL_SHAPES)
def test_selection_at_the_ends_of_the_rank(shape):
    x, t = oc.inputs(shape)
    num_valid = int((t != IGNORE).sum())
    for thresh in (0.7, 1e-6):
        for min_kept in (1, 2, num_valid - 1, num_valid, num_valid + 1, -3):
            out = run_op(x, t, None, thresh, min_kept, grad=False)
            check_selection("%s thresh %g min_kept %d" % (shape, thresh, min_kept), out, t, shape[1], thresh, min_kept)


@pytest.mark.parametrize("shape", oc.SMALL_SHAPES)
def test_ties_at_kth_are_all_kept(shape):
    x, t = oc.inputs(shape)
    min_kept, thresh = 500, 1e-3
    first = run_op(x, t, None, thresh, min_kept, grad=False)
    hw = shape[2] * shape[3]
    order = np.argsort(np.where(first["valid"], first["prob"], np.inf).reshape(-1), kind="stable")
    kth_pixel = int(order[min_kept - 1])
    assert first["prob"].reshape(-1)[kth_pixel] == first["state"][3] > np.float32(thresh)
    others = [int(p) for p in order[min_kept + 40:min_kept + 45]]          # five pixels that were NOT kept
    assert not first["kept"].reshape(-1)[others].any()
    x, t = x.copy(), t.copy()
    for p in others:
        x[p // hw].reshape(shape[1], -1)[:, p % hw] = x[kth_pixel // hw].reshape(shape[1], -1)[:, kth_pixel % hw]
        t.reshape(-1)[p] = t.reshape(-1)[kth_pixel]
    out = run_op(x, t, None, thresh, min_kept)
    want = check_selection("ties %s" % (shape,), out, t, shape[1], thresh, min_kept)
    assert want == first["state"][3] and out["counts"][1] == first["counts"][1] + 5 and out["state"][5] == 1
    six = [kth_pixel] + others
    assert out["kept"].reshape(-1)[six].all() and len({out["prob"].reshape(-1)[p] for p in six}) == 1
    g = np.abs(out["grad"]).sum(axis=1).reshape(-1)
    assert (g[six] > 0).all() and np.array_equal(g > 0, out["kept"].reshape(-1))


@pytest.mark.parametrize("shape", oc.SMALL_SHAPES)
def test_nan_logits_order_above_every_number(shape):
    x, t = oc.inputs(shape)
    x = x.copy()
    hw = shape[2] * shape[3]
    flat = t.reshape(-1)
    sick = [int(p) for p in np.flatnonzero(flat != IGNORE)[[3, 50, 51, 400, -1]]]
    for i, p in enumerate(sick):
        x[p // hw, (i * 7) % shape[1]].reshape(-1)[p % hw] = np.nan
    num_valid = int((flat != IGNORE).sum())
    for min_kept in (0, 300, num_valid - 6, num_valid - 5, num_valid - 2, num_valid - 1):
        # dropped: never kept by a threshold, whatever the rank; a NaN kth gives thresh
        out = run_op(x, t, None, 0.7, min_kept)
        want = check_selection("nan %s min_kept %d" % (shape, min_kept), out, t, shape[1], 0.7, min_kept)
        assert np.isnan(out["prob"].reshape(-1)[sick]).all() and not out["kept"].reshape(-1)[sick].any()
        if min_kept > num_valid - 5:
            assert want == np.float32(0.7)
        assert np.isfinite(out["loss"]) and np.isfinite(out["grad"]).all()
        assert (np.abs(out["grad"]).sum(axis=1).reshape(-1)[sick] == 0).all()
    for min_kept in (num_valid, num_valid + 7):
        out = run_op(x, t, None, 0.7, min_kept)                            # kept, NaN ones included: not a silently dropped pixel
        check_selection("nan %s min_kept %d" % (shape, min_kept), out, t, shape[1], 0.7, min_kept)
        assert out["kept"].reshape(-1)[sick].all() and np.isnan(out["loss"]) and out["counts"][1] == num_valid


@pytest.mark.parametrize("pattern", sorted(rc.INF_PATTERNS))
@pytest.mark.parametrize("shape", rc.INF_SHAPES)
def test_minus_inf_logits(shape, pattern):
    x, t, mask, planes = rc.inf_case(shape, pattern)
    w = rc.inf_weights(shape[1])
    for min_kept in (0, 700):
        out = run_op(x, t, w, 0.7, min_kept)
        check_selection("-inf %s %s %d" % (shape, pattern, min_kept), out, t, shape[1], 0.7, min_kept)
        assert np.isfinite(out["loss"]) and np.isfinite(out["grad"]).all() and np.isfinite(out["prob"]).all()
        ref_v, ref_g = _reference64(x, t, w, out["kept"])
        assert abs(out["loss"] - ref_v) <= VALUE_TOL * abs(ref_v)
        assert l2_err(out["grad"], ref_g) <= 1e-5
        for c in planes:                                                   # a class switched off gets exactly 0.0f
            assert (out["grad"][:, c][mask] == 0).all()


# ---- 2. prob against float64 -----------------------------------------------------------------------------------------------
def _numpy_fp32_error(x, t):
    """The worst relative error of the reference's numpy-fp32 softmax at the target, against float64."""
    p64, valid = oc.prob64(x, t)
    p32 = np.take_along_axis(oc.prob32_numpy(x), np.where(valid, t, 0)[:, None], 1)[:, 0]
    return float((np.abs(p32[valid] - p64[valid]) / p64[valid]).max())


@pytest.mark.parametrize("shape", sorted({r[0] for r in oc.ROWS}))
def test_prob_against_float64(shape):
    """Measured on an MI355X, worst relative error of prob / the bound (4 x numpy-fp32's own worst error): (1,3,601,1023)
    7.53e-07 / 1.10e-06; (2,2,129,1028) 5.48e-07 / 1.03e-06; (2,19,8,64) 7.86e-07 / 1.52e-06; (2,19,37,53) 8.59e-07 / 1.77e-06.
    prob = expf(x_t - lse) carries the absolute error of lse (about (C + 8) 2^-24 |lse|, with |lse| up to 12 here) as a relative
    error."""
    x, t = oc.inputs(shape)
    bound = 4 * _numpy_fp32_error(x, t)
    out = run_op(x, t, None, 0.7, 100, grad=False)
    p64, valid = oc.prob64(x, t)
    err = float((np.abs(out["prob"][valid] - p64[valid]) / p64[valid]).max())
    print("prob %s: worst relative error %.3e, bound %.3e" % (shape, err, bound))
    assert 1e-6 < bound < 4e-6 and err <= bound
    lse64 = torch.logsumexp(torch.from_numpy(x.astype(np.float64)), 1).numpy()
    assert rel_err(out["lse"], lse64) <= (shape[1] + 8) * 2.0 ** -24


# ---- 3. the small rows against the reference's own run -------------------------------------------------------------------------
def _reference64(x, t, w, kept):
    """(loss, gradient) in float64 on the CPU over a given kept mask: the rewritten target through F.cross_entropy."""
    x64 = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    tt = torch.from_numpy(np.where(kept, t, IGNORE))
    w64 = None if w is None else torch.from_numpy(w).double()
    v = F.cross_entropy(x64, tt, weight=w64, ignore_index=IGNORE)
    g, = torch.autograd.grad(v, x64)
    return v.item(), g.numpy()


def _check_grad(name, fused, stock, ref):
    for metric in (l2_err, rel_err):
        ef, es = metric(fused, ref), metric(stock, ref)
        print("%s %s: fused %.3e stock fp32 %.3e (bound %.3e)" % (name, metric.__name__, ef, es, GRAD_FACTOR * max(es, GRAD_FLOOR)))
        assert ef <= GRAD_FACTOR * max(es, GRAD_FLOOR), (name, metric.__name__, ef, es)


@pytest.mark.parametrize("i", range(len(oc.GOLDEN_CASES)))
def test_small_rows_equal_the_reference(golden, i):
    g = golden("seg_ohem")
    name, shape, kwargs, nheads = oc.GOLDEN_CASES[i]
    weight = g["c%d_weight" % i]
    t = oc.inputs(shape)[1]
    total, scale = 0.0, 1.0
    for h in range(nheads):
        x = oc.inputs(shape, h)[0]
        bound = 4 * _numpy_fp32_error(x, t)
        p64, valid = oc.prob64(x, t)
        th64, keep_all = oc.expected_threshold(p64[valid], kwargs["thresh"], kwargs["min_kept"], np.float64)
        if not keep_all:                       # the gap condition: no probability within 25 bounds of the threshold
            gap = oc.nearest_gap(p64, valid, float(th64))
            print("case %d head %d: gap %.3e, 25 x bound %.3e" % (i, h, gap, 25 * bound))
            assert gap >= 25 * bound
        out = run_op(x, t, weight, kwargs["thresh"], kwargs["min_kept"])
        check_selection("golden %d head %d" % (i, h), out, t, shape[1], kwargs["thresh"], kwargs["min_kept"])
        assert np.array_equal(out["kept"], g["c%d_kept" % i][h].astype(bool))
        ref_v, ref_g = _reference64(x, t, weight, out["kept"])
        assert abs(out["loss"] - ref_v) <= VALUE_TOL * abs(ref_v)
        _check_grad("golden %d head %d" % (i, h), scale * out["grad"], g["c%d_grad" % i][h], scale * ref_g)
        total += scale * float(out["loss"])
        scale = kwargs.get("aux_weight", 0.2)
    assert abs(total - float(g["c%d_value" % i])) <= VALUE_TOL * abs(float(g["c%d_value" % i]))


# ---- 4. the large rows against float64 over the op's own kept mask -----------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in oc.ROWS if not r[3]], ids=lambda r: "%s-%g-%d" % (r[0], r[1], r[2]))
def test_large_rows_against_float64_over_the_own_mask(row):
    shape, thresh, min_kept, _ = row
    x, t = oc.inputs(shape)
    x = x.copy()
    hw = shape[2] * shape[3]
    ignored = np.flatnonzero(t.reshape(-1) == IGNORE)[[0, 5, 1000, -1]]
    for p in ignored:                                                      # NaN logits at ignored pixels change nothing
        x[p // hw, p % shape[1]].reshape(-1)[p % hw] = np.nan
    w = oc.class_weights(shape[1])
    out = run_op(x, t, w, thresh, min_kept)
    check_selection(str(row), out, t, shape[1], thresh, min_kept)
    clean = np.nan_to_num(x, nan=0.0)
    ref_v, ref_g = _reference64(clean, t, w, out["kept"])
    print("%s: loss %.9g, float64 over the same mask %.9g" % (row, out["loss"], ref_v))
    assert abs(out["loss"] - ref_v) <= VALUE_TOL * abs(ref_v)
    xs = dev(clean).requires_grad_(True)
    vs = F.cross_entropy(xs, dev(np.where(out["kept"], t, IGNORE)), weight=dev(w), ignore_index=IGNORE)
    gs, = torch.autograd.grad(vs, xs)
    _check_grad(str(row), out["grad"], gs.cpu().numpy(), ref_g)
    dead = np.broadcast_to(~out["kept"][:, None], out["grad"].shape)
    assert (out["grad"][dead] == 0).all() and np.isfinite(out["grad"]).all()      # exact zeros, at the NaN pixels too
    assert (np.abs(out["grad"]).sum(axis=1)[out["kept"]] > 0).all()


# ---- 5. one hard pixel per chunk ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 601, 1023), (2, 2, 129, 1028)])
def test_one_hard_pixel_per_chunk_is_exactly_the_kept_set(shape):
    """A lost flush of any workgroup's bins or partials shows up: the kept set must be exactly the planted pixels."""
    n = shape[0] * shape[2] * shape[3]
    nchunks = (n + ops.SEG_CHUNK_PIXELS - 1) // ops.SEG_CHUNK_PIXELS
    planted_in = rc.marker_chunks(nchunks)
    x, t, planted = oc.marker_inputs(shape, planted_in)
    assert len(planted) == len(set(planted)) >= 4 and nchunks > 256
    out = run_op(x, t, None, 1e-6, len(planted))
    check_selection("markers %s" % (shape,), out, t, shape[1], 1e-6, len(planted))
    assert out["counts"][1] == len(planted) and sorted(np.flatnonzero(out["kept"].reshape(-1))) == sorted(planted)
    assert sorted(np.flatnonzero(np.abs(out["grad"]).sum(axis=1).reshape(-1))) == sorted(planted)
    ref_v, ref_g = _reference64(x, t, None, out["kept"])
    assert abs(out["loss"] - ref_v) <= VALUE_TOL * abs(ref_v) and l2_err(out["grad"], ref_g) <= 1e-5
    # one fewer than planted: every planted pixel ties at kth, all are kept
    out = run_op(x, t, None, 1e-6, len(planted) - 1, grad=False)
    assert out["counts"][1] == len(planted) and out["state"][5] == len(planted) - 1


# ---- 6. the same bits ------------------------------------------------------------------------------------------------------------------
def _step(x, t, w, thresh, min_kept):
    loss, prob, lse, state, counts = torch.ops.cerberus.seg_ohem_cross_entropy(x, t, w, IGNORE, thresh, min_kept)
    g, = torch.autograd.grad(loss, x)
    return loss.detach(), prob, lse, state, counts, g


@pytest.mark.parametrize("row", [oc.ROWS[1], oc.ROWS[3]], ids=lambda r: "%s-%g-%d" % (r[0], r[1], r[2]))
def test_two_runs_give_the_same_bits(row):
    shape, thresh, min_kept, _ = row
    x, t = oc.inputs(shape)
    w = dev(oc.class_weights(shape[1]))
    runs = [_step(dev(x).requires_grad_(True), dev(t), w, thresh, min_kept) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("row", [oc.ROWS[2], oc.ROWS[3]], ids=lambda r: "%s-%g-%d" % (r[0], r[1], r[2]))
def test_misaligned_views_give_the_bits_of_the_aligned_call(row):
    shape, thresh, min_kept, _ = row
    x, t = oc.inputs(shape)
    w = dev(oc.class_weights(shape[1]))
    aligned, td = dev(x), dev(t)
    buf = torch.zeros(aligned.numel() + 1, device=DEV)
    shifted = buf[1:].view(shape)
    shifted.copy_(aligned)
    tbuf = torch.zeros(td.numel() + 1, dtype=torch.int64, device=DEV)
    tshift = tbuf[1:].view(td.shape)
    tshift.copy_(td)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and tshift.data_ptr() % 16 == 8
    want = _step(aligned.detach().requires_grad_(True), td, w, thresh, min_kept)
    for xin, tin in ((shifted, td), (aligned, tshift)):
        xx = xin.detach().requires_grad_(True)
        assert xx.data_ptr() == xin.data_ptr()
        for a, b in zip(want, _step(xx, tin, w, thresh, min_kept)):
            assert torch.equal(a, b)


def test_graphed_replay_is_bit_equal_to_eager():
    """Forward and backward captured in ONE graph on a single stream, replayed twice per input with an eager call in between:
    the bins are zeroed by a kernel node of the call, the counts are integer adds, the sums run in a fixed order."""
    shape, thresh, min_kept = (2, 19, 37, 53), 0.7, 2000
    s_x = torch.zeros(shape, device=DEV, requires_grad=True)
    s_t = torch.zeros((shape[0],) + shape[2:], dtype=torch.int64, device=DEV)
    w = dev(oc.class_weights(shape[1]))

    def step(x, t):
        out = ca.seg_ohem_cross_entropy(x, t, w, IGNORE, thresh, min_kept, return_stats=True)
        g, = torch.autograd.grad(out[0], x)
        return tuple(o.detach() for o in out) + (g,)

    with torch.no_grad():
        s_x.copy_(dev(oc.inputs(shape)[0]))
        s_t.copy_(dev(oc.inputs(shape)[1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(s_x, s_t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(s_x, s_t)
    for head in (1, 0):
        x, t = oc.inputs(shape, head)
        with torch.no_grad():
            s_x.copy_(dev(x))
            s_t.copy_(dev(t))
        eager = step(dev(x).requires_grad_(True), dev(t))
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(captured, eager):
                assert torch.equal(a, b), head
        assert bool(torch.isfinite(captured[0])) and int(captured[3]) >= min_kept and float(captured[4].abs().max()) > 0


# ---- 7. the classes and the wrapper ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(oc.GOLDEN_CASES)))
def test_classes_hip_against_torch(golden, i):
    g = golden("seg_ohem")
    name, shape, kwargs, nheads = oc.GOLDEN_CASES[i]
    t = dev(oc.inputs(shape)[1])
    res = {}
    for backend in ("hip", "torch"):
        fn = getattr(ca, name)(backend=backend, class_weights=g["c%d_weight" % i] if kwargs["use_weight"] else None, **kwargs).to(DEV)
        heads = [dev(oc.inputs(shape, h)[0]).requires_grad_(True) for h in range(nheads)]
        loss = fn(heads if nheads > 1 else heads[0], t)
        assert loss.shape == () and loss.dtype == torch.float32 and loss.device.type == "cuda"
        res[backend] = (loss.item(), [a.cpu().numpy() for a in torch.autograd.grad(loss, heads)])
    want_v = float(g["c%d_value" % i])
    print("case %d: hip %.9g torch %.9g reference %.9g" % (i, res["hip"][0], res["torch"][0], want_v))
    for backend in res:
        assert abs(res[backend][0] - want_v) <= VALUE_TOL * abs(want_v)
        for h in range(nheads):
            assert l2_err(res[backend][1][h], g["c%d_grad" % i][h]) <= 1e-5
            assert np.array_equal(np.abs(res[backend][1][h]).sum(axis=1) > 0, g["c%d_kept" % i][h].astype(bool))


def test_wrapper_routes_and_stats():
    shape, thresh, min_kept = (2, 19, 8, 64), 0.7, 600
    x, t = oc.inputs(shape)
    xd, td, w = dev(x), dev(t), dev(oc.class_weights(shape[1]))
    loss, threshold, num_valid, num_kept = ca.seg_ohem_cross_entropy(xd, td, w, IGNORE, thresh, min_kept, return_stats=True)
    assert all(o.device.type == "cuda" and o.shape == () for o in (loss, threshold, num_valid, num_kept))
    assert num_valid.dtype == torch.int64 and int(num_valid) == int((t != IGNORE).sum()) and int(num_kept) == min_kept
    # what the op cannot take goes to the stock restatement on the logits' device: the same selection, the loss within tolerance
    stock = ca.loss_functions.ohem_losses._ohem_stock(xd, td, w, IGNORE, thresh, min_kept, ca.seg_cross_entropy)
    # (the stock softmax rounds otherwise: the thresholds agree to a few fp32 units, the counts exactly -- the gap is wide)
    assert abs(float(stock[1]) - float(threshold)) <= 2e-6 * float(threshold)
    assert int(stock[2]) == int(num_valid) and int(stock[3]) == int(num_kept)
    assert abs(float(stock[0]) - float(loss)) <= VALUE_TOL * float(loss)
    v16 = ca.seg_ohem_cross_entropy(xd.half(), td, w, IGNORE, thresh, min_kept)
    assert v16.dtype == torch.float16 and abs(float(v16) - float(loss)) <= 2e-2 * float(loss)
    wg = w.clone().requires_grad_(True)
    xg = xd.clone().requires_grad_(True)
    v = ca.seg_ohem_cross_entropy(xg, td, wg, IGNORE, thresh, min_kept)
    gx, gw = torch.autograd.grad(v, (xg, wg))
    assert abs(float(v.detach()) - float(loss)) <= VALUE_TOL * float(loss) and float(gw.abs().max()) > 0 and float(gx.abs().max()) > 0
    with pytest.raises(RuntimeError, match="no gradient for its class weights"):
        torch.autograd.grad(torch.ops.cerberus.seg_ohem_cross_entropy(xg, td, wg, IGNORE, thresh, min_kept)[0], (xg, wg))
    one = ca.seg_ohem_cross_entropy(xd[:, :1], td.clamp(max=0), None, IGNORE, thresh, min_kept)
    assert float(one) == 0.0
    cpu = ca.seg_ohem_cross_entropy(xd.cpu(), td.cpu(), w.cpu(), IGNORE, thresh, min_kept)
    assert cpu.device.type == "cpu" and abs(float(cpu) - float(loss)) <= VALUE_TOL * float(loss)
    with pytest.raises(RuntimeError, match="no double backward"):
        xx = xd.clone().requires_grad_(True)
        g, = torch.autograd.grad(ca.seg_ohem_cross_entropy(xx, td, w, IGNORE, thresh, min_kept), xx, create_graph=True)
        g.sum().backward()
    with pytest.raises(RuntimeError, match="float32"):
        torch.ops.cerberus.seg_ohem_cross_entropy(xd.half(), td, w, IGNORE, thresh, min_kept)
    with pytest.raises(RuntimeError, match="at least 2 classes"):
        torch.ops.cerberus.seg_ohem_cross_entropy(xd[:, :1].contiguous(), td, w[:1], IGNORE, thresh, min_kept)
    # an out-of-range label that is not the ignore value: NaN in the numerator, no part in the selection, a zero gradient
    tb = t.copy()
    tb.reshape(-1)[11] = shape[1]
    out = run_op(x, tb, None, thresh, min_kept)
    torch.cuda.synchronize()
    assert np.isnan(out["loss"]) and out["prob"].reshape(-1)[11] == -1 and out["counts"][0] == int(((tb != IGNORE) & (tb < shape[1])).sum())
    assert (out["grad"].reshape(shape[0], shape[1], -1)[0, :, 11] == 0).all()
    # every pixel ignored: 0 / 0 as stock, nothing but zeros in the gradient
    out = run_op(x, np.full_like(t, IGNORE), None, thresh, min_kept)
    assert np.isnan(out["loss"]) and (out["grad"] == 0).all() and out["counts"].tolist() == [0, 0]
