"""GPU tests of the supervised depth loss (csrc/depth_loss.hip): ``inv_huber_loss`` / ``cerberus::inv_huber`` and the classes
``InvHuberLoss`` / ``InvHuberLossPyr``.

Yardstick: the reference's formula (``InvHuberLoss.forward``, restated as ``depth_losses._inv_huber_stock``) evaluated in
float64 on the CPU, value and autograd gradient; the stock fp32 chain runs on the GPU in the same test.  Values: relative error
<= 1e-5.  Gradients are checked IN TWO PARTS, because the gradient through the cutoff ``c = 0.2 * err.max()`` lands on the
pixel(s) that hold the maximum and is 100 to 10^5 times larger than any other element, so every norm of the whole gradient
sees that pixel only:
  * with the elements where ``err == m`` zeroed in fused, stock and reference alike, ``l2_err`` and ``rel_err`` against float64
    are each at most 4 x max(e_stock, 2^-23) (the bound and the floor of tests/test_seg_loss_gpu.py);
  * at the ``err == m`` elements, the relative error of each element meets the same bound against the stock chain's error at
    that element; where the reference gradient there is 0 (a maximum at a pixel with pred <= 0), the fused one is exactly 0.

Shapes: the smallest at which each route can go wrong.  Scalar route (h*w odd or 2 mod 4, idle lanes): (1,1,1,1), (1,1,5,7),
(2,1,37,53) (4 workgroups, a ragged last one), (1,1,3,66).  Vector route: (1,1,1,4), (2,1,8,64) (exactly one full workgroup),
(3,1,16,33) (odd w: a lane's 4 pixels cross a row).  (2,1,128,256): 64 workgroups, so the partial folds matter; every thread of
``inv_huber_final_kernel`` still reads at most ONE partial there, and the max pass takes no grid stride.

Past one round (tests/reduction_cases.py, checked on the CPU by tests/test_reduction_tiers_cpu.py; section 11): (1,1,257,1024)
vector and (1,1,601,1023) scalar, 257 and 601 partials for the finish; (1,1,1025,1024) vector, 1025 chunks on the max pass's 1024
workgroups (workgroup 0 walks a second chunk; ``fold_parts`` loads its full 1024 partial maxima); (1,1,1537,1023) scalar, 1536
chunks (half the workgroups walk two); (1,1,6,1000), 6 partial maxima (lane 1 of ``fold_parts`` takes the tail loop); a (1,1,513,512)
prediction against a (1,1026,1024) ground truth, the gather with 257 partials.  A sum or a maximum over a whole map could hide one
mis-addressed partial, so the strict maximum is also planted in the first chunk, in 255, 256, 511, 512, 1024 and the last."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cerberusnet_amd as ca
import depth_loss_cases as cases
import reduction_cases as rc
from cerberusnet_amd.loss_functions import depth_losses as D
from conftest import l2_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_TOL = 1e-5
GRAD_FACTOR = 4.0
GRAD_FLOOR = 2.0 ** -23

SCALAR_SHAPES = [(1, 1, 1, 1), (1, 1, 5, 7), (2, 1, 37, 53), (1, 1, 3, 66)]
VECTOR_SHAPES = [(1, 1, 1, 4), (2, 1, 8, 64), (3, 1, 16, 33)]
SHAPES = SCALAR_SHAPES + VECTOR_SHAPES + [(2, 1, 128, 256)]
ROUTE_SHAPES = [(2, 1, 37, 53), (2, 1, 8, 64)]         # one per route, for the tests of a property


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inputs(shape, seed=2000):
    """Prediction (B,1,h,w) and ground truth (B,h,w).  The shapes of a few pixels get a pixel that counts: valid, pred > 0."""
    p, g = cases.prediction(shape, seed), cases.ground_truth(shape, seed + 5)
    if p.size <= 16:
        p.reshape(-1)[0], g.reshape(-1)[0] = 2.5, 1.0
    return p, g


def _reference(p, g):
    """Value and gradient of the reference's formula in float64 on the CPU."""
    p64 = torch.from_numpy(p).double().requires_grad_(True)
    v = D._inv_huber_stock(p64.reshape(g.shape), torch.from_numpy(g).double())
    gr, = torch.autograd.grad(v, p64)
    return v.item(), gr.numpy()


@functools.lru_cache(maxsize=None)
def _reference_of_shape(shape):
    """Computed once per shape and shared; the arrays are not written to."""
    return _reference(*_inputs(shape))


def _max_mask(p, g):
    """The elements where err == m, from the fp32 arithmetic of the kernels (relu, one subtraction, abs: all exact in float64
    too, so the float64 reference agrees on the set unless two different errors round to the same fp32 value)."""
    d = np.maximum(p.reshape(g.shape), np.float32(0)) - g
    err = np.where(g > 0, np.abs(d), np.float32(0))
    return (err == err.max()).reshape(p.shape)


def _fused(p, g):
    """(value, gradient) of the wrapper on device tensors."""
    pp = p.detach().clone().requires_grad_(True)
    v = ca.inv_huber_loss(pp, g)
    gr, = torch.autograd.grad(v, pp)
    return v.detach(), gr


def _stock(p, g):
    """(value, gradient) of the stock fp32 chain on device tensors of equal size."""
    pp = p.detach().clone().requires_grad_(True)
    v = D._inv_huber_stock(pp.reshape(g.shape), g)
    gr, = torch.autograd.grad(v, pp)
    return v.detach(), gr


def _check_value(name, v, vs, ref_v):
    print("%s value: fused rel %.3e stock fp32 rel %.3e" % (name, abs(v - ref_v) / abs(ref_v), abs(vs - ref_v) / abs(ref_v)))
    assert abs(v - ref_v) <= VALUE_TOL * abs(ref_v), (name, v, ref_v)


def _check_grad(name, fused, stock, ref, at_max):
    """The two parts of the module docstring."""
    away = ~at_max
    for metric in (l2_err, rel_err):
        ef, es = metric(fused * away, ref * away), metric(stock * away, ref * away)
        print("%s away from the maximum %s: fused %.3e stock fp32 %.3e ratio %.2f (bound %.3e)" % (
            name, metric.__name__, ef, es, ef / max(es, GRAD_FLOOR), GRAD_FACTOR * max(es, GRAD_FLOOR)))
        assert ef <= GRAD_FACTOR * max(es, GRAD_FLOOR), (name, metric.__name__, ef, es)
    assert at_max.any()
    for f, s, r in zip(fused[at_max], stock[at_max], ref[at_max]):
        if r == 0:
            assert f == 0, (name, f)
            continue
        ef, es = abs(float(f) - r) / abs(r), abs(float(s) - r) / abs(r)
        print("%s at the maximum: reference %.6e fused rel %.3e stock fp32 rel %.3e ratio %.2f" % (
            name, r, ef, es, ef / max(es, GRAD_FLOOR)))
        assert ef <= GRAD_FACTOR * max(es, GRAD_FLOOR), (name, f, s, r)


def _check_case(name, p, g, ref=None, gt_for_op=None):
    """Fused and stock on the GPU against float64, value and gradient; returns the fused (value, gradient).  ``gt_for_op``: the
    finer ground truth that the fused op gathers ``g`` from."""
    ref_v, ref_g = ref if ref is not None else _reference(p, g)
    pd, gd = dev(p), dev(g)
    v, gr = _fused(pd, gd if gt_for_op is None else dev(gt_for_op))
    vs, gs = _stock(pd, gd)
    assert v.shape == () and v.dtype == torch.float32 and gr.shape == pd.shape and gr.dtype == torch.float32
    _check_value(name, v.item(), vs.item(), ref_v)
    at_max = _max_mask(p, g)
    d64 = np.maximum(p.reshape(g.shape).astype(np.float64), 0) - g
    err64 = np.where(g > 0, np.abs(d64), 0)
    assert np.array_equal(at_max.reshape(g.shape), err64 == err64.max())
    _check_grad(name, gr.cpu().numpy(), gs.cpu().numpy(), ref_g, at_max)
    return v, gr


# ---- 1. value and gradient against float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_value_and_gradient_against_float64(shape):
    p, g = _inputs(shape)
    if p.size > 16:
        assert (g > 0).any() and (g == 0).any() and (p <= 0).any()
        assert ((g > 0).reshape(p.shape) & (p <= 0)).any() and ((g > 0).reshape(p.shape) & (p > 0)).any()
    else:
        assert g.reshape(-1)[0] > 0 and p.reshape(-1)[0] > 0
    v, gr = _check_case("inv_huber %s" % (shape,), p, g, _reference_of_shape(shape))
    # the raw op: the same bits, and the state the backward reads; a (B,h,w) prediction is the same call
    loss, state = torch.ops.cerberus.inv_huber(dev(p), dev(g))
    assert torch.equal(loss, v) and state.shape == (4,) and state.dtype == torch.float32
    d = np.maximum(p.reshape(g.shape), np.float32(0)) - g
    m = np.where(g > 0, np.abs(d), np.float32(0)).max()
    assert float(state[3]) == float(m) and float(state[0]) == float(np.float32(0.2) * m)       # the maximum is exact
    assert float(state[2]) == float(np.float32(1) / np.float32(p.size))
    v3, g3 = _fused(dev(p[:, 0]), dev(g))
    assert torch.equal(v3, v) and torch.equal(g3, gr[:, 0])
    dead = (dev(g) <= 0)[:, None] | (dev(p) <= 0)
    assert bool((gr[dead] == 0).all()) and bool(torch.isfinite(gr).all())


# ---- 2. where the maximum lies ------------------------------------------------------------------------------------------
def _plant(p, g, where):
    p, g = p.copy(), g.copy()
    fp, fg, n = p.reshape(-1), g.reshape(-1), p.size
    if where == "first":
        fp[0], fg[0] = 20.0, 1.0
    elif where == "last":
        fp[n - 1], fg[n - 1] = 20.0, 1.0
    elif where == "tie":                        # different workgroups, equal errors, opposite signs of d
        fp[5], fg[5] = 20.5, 1.5
        fp[n - 7], fg[n - 7] = 0.5, 19.5
    elif where == "relu":                       # the pixel sets c; its own gradient is 0
        fp[n // 2], fg[n // 2] = -3.0, 25.0
    elif where == "invalid":                    # the largest |d| of all, at a pixel that does not count
        fp[n // 3], fg[n // 3] = 1000.0, 0.0
    return p, g


@pytest.mark.parametrize("shape", [(2, 1, 37, 53), (2, 1, 128, 256)])
@pytest.mark.parametrize("where", ["first", "last", "tie", "relu", "invalid"])
def test_where_the_maximum_lies(shape, where):
    p, g = _plant(*_inputs(shape), where)
    at_max = _max_mask(p, g)
    flat = np.flatnonzero(at_max.reshape(-1))
    n = p.size
    want = {"first": [0], "last": [n - 1], "tie": [5, n - 7], "relu": [n // 2]}.get(where)
    if want is not None:
        assert flat.tolist() == want
    else:
        assert n // 3 not in flat and len(flat) == 1
    if where == "tie":
        assert flat[0] // 1024 != flat[1] // 1024
    v, gr = _check_case("inv_huber %s maximum %s" % (shape, where), p, g)
    _, state = torch.ops.cerberus.inv_huber(dev(p), dev(g))
    if where in ("first", "last", "tie"):
        assert float(state[0]) == float(np.float32(0.2) * np.float32(19.0))
    if where == "relu":
        assert float(state[0]) == 5.0 and float(gr.reshape(-1)[n // 2]) == 0.0
    if where == "invalid":
        assert float(state[3]) < 6.0 and float(gr.reshape(-1)[n // 3]) == 0.0
    if where == "tie":
        a, b = gr.reshape(-1)[flat[0]].item(), gr.reshape(-1)[flat[1]].item()
        assert a == -b and a != 0                 # the same magnitude, the sign of d


# ---- 3. the pyramid gather ----------------------------------------------------------------------------------------------
def _bits_of_op(p, g):
    pp = p.detach().clone().requires_grad_(True)
    loss, state = torch.ops.cerberus.inv_huber(pp, g)
    gr, = torch.autograd.grad(loss, pp)
    return loss.detach(), state, gr


@pytest.mark.parametrize("pshape,gshape", [((2, 1, 16, 32), (2, 64, 128)), ((1, 1, 9, 10), (1, 27, 20))])
def test_gather_gives_the_bits_of_the_resized_ground_truth(pshape, gshape):
    p, g = dev(cases.prediction(pshape, 2100)), dev(cases.ground_truth(gshape, 2105))
    resized = F.interpolate(g[:, None], pshape[2:], mode="nearest")[:, 0].contiguous()
    ry, rx = gshape[1] // pshape[2], gshape[2] // pshape[3]
    assert torch.equal(resized, g[:, ::ry, ::rx]) and bool((resized > 0).any()) and bool((resized == 0).any())
    for a, b in zip(_bits_of_op(p, g), _bits_of_op(p, resized)):
        assert torch.equal(a, b)
    assert torch.equal(ca.inv_huber_loss(p, g), _bits_of_op(p, resized)[0])
    assert float(_bits_of_op(p, g)[2].abs().max()) > 0


def test_a_non_integer_ratio_is_resized_by_the_wrapper():
    p, g = dev(cases.prediction((1, 1, 9, 10), 2110)), dev(cases.ground_truth((1, 25, 31), 2115))
    resized = F.interpolate(g[:, None], (9, 10), mode="nearest")[:, 0]
    v, gr = _fused(p, g)
    v2, gr2 = _fused(p, resized)
    assert torch.equal(v, v2) and torch.equal(gr, gr2) and float(v) > 0
    with pytest.raises(RuntimeError, match="integer multiple"):
        torch.ops.cerberus.inv_huber(p, g)


def test_pyramid_class_against_float64():
    gshape, sizes, lvl_weights = (2, 32, 64), ((32, 64), (16, 32), (8, 16)), [1.0, 0.5, 0.25]
    g = cases.ground_truth(gshape, 2125)
    levels = [cases.prediction((2, 1) + s, 2120 + k) for k, s in enumerate(sizes)]
    resized = [F.interpolate(torch.from_numpy(g)[:, None], s, mode="nearest")[:, 0].numpy() for s in sizes]
    refs = [_reference(p, r) for p, r in zip(levels, resized)]
    want = 0.5 * sum(lw * v for lw, (v, _) in zip(lvl_weights, refs))
    outs = {}
    for backend in ("hip", "torch"):
        lv = [dev(p).requires_grad_(True) for p in levels]
        v = ca.InvHuberLossPyr(lvl_weights, weight=0.5, backend=backend)({"depth": lv}, {"disparity": dev(g)})
        outs[backend] = (v.item(), [x.cpu().numpy() for x in torch.autograd.grad(v, lv)])
    _check_value("pyramid", outs["hip"][0], outs["torch"][0], want)
    for k, (p, r, lw) in enumerate(zip(levels, resized, lvl_weights)):
        _check_grad("pyramid level %d" % k, outs["hip"][1][k], outs["torch"][1][k], 0.5 * lw * refs[k][1], _max_mask(p, r))


# ---- 4. the corner decisions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ROUTE_SHAPES)
def test_nan_at_a_valid_pixel_makes_the_value_nan(shape):
    p, g = _inputs(shape)
    for i in (0, p.size - 1):
        pn, gn = p.copy(), g.copy()
        pn.reshape(-1)[i], gn.reshape(-1)[i] = np.nan, 1.0
        assert bool(torch.isnan(ca.inv_huber_loss(dev(pn), dev(gn)))), i
    assert bool(torch.isfinite(ca.inv_huber_loss(dev(p), dev(g))))


@pytest.mark.parametrize("shape", ROUTE_SHAPES)
def test_what_an_invalid_pixel_holds_changes_no_bit(shape):
    p, g = _inputs(shape)
    clean_v, clean_g = _fused(dev(p), dev(g))
    invalid = np.flatnonzero(g.reshape(-1) == 0)
    for i in (int(invalid[0]), int(invalid[-1])):
        for junk in (np.nan, 1e30, -np.inf):
            pn = p.copy()
            pn.reshape(-1)[i] = junk
            v, gr = _fused(dev(pn), dev(g))
            assert torch.equal(v, clean_v) and torch.equal(gr, clean_g) and float(gr.reshape(-1)[i]) == 0.0, (i, junk)
    # a NaN ground truth is an invalid pixel
    valid = np.flatnonzero(g.reshape(-1) > 0)
    gn, gz = g.copy(), g.copy()
    gn.reshape(-1)[valid[3]], gz.reshape(-1)[valid[3]] = np.nan, 0.0
    v, gr = _fused(dev(p), dev(gn))
    vz, gz_ = _fused(dev(p), dev(gz))
    assert torch.equal(v, vz) and torch.equal(gr, gz_) and bool(torch.isfinite(v)) and not torch.equal(v, clean_v)


@pytest.mark.parametrize("shape", ROUTE_SHAPES)
def test_a_zero_cutoff_gives_zero_and_a_zero_gradient(shape):
    p, g = _inputs(shape)
    v, gr = _fused(dev(p), dev(np.zeros_like(g)))                      # no valid pixel
    assert float(v) == 0.0 and bool((gr == 0).all())
    exact = np.where((g > 0).reshape(p.shape), g.reshape(p.shape), p)  # every valid pixel exact, the invalid ones off
    assert (exact[(g == 0).reshape(p.shape)] != 0).any()
    v, gr = _fused(dev(exact), dev(g))
    assert float(v) == 0.0 and bool((gr == 0).all())
    vs, _ = _stock(dev(exact), dev(g))
    assert bool(torch.isnan(vs))                                       # the reference's 0 / 0


@pytest.mark.parametrize("shape", ROUTE_SHAPES)
def test_dead_pixels_get_exactly_zero(shape):
    p, g = _inputs(shape)
    pd, gd = dev(p).requires_grad_(True), dev(g)
    dead = (gd <= 0)[:, None] | (pd.detach() <= 0)
    assert int(dead.sum()) > 0 and int((~dead).sum()) > 0
    for upstream in (3.0, float("nan")):
        gr, = torch.autograd.grad(ca.inv_huber_loss(pd, gd), pd, grad_outputs=torch.tensor(upstream, device=DEV))
        assert bool((gr[dead] == 0).all()), upstream
        assert bool(torch.isnan(gr[~dead]).all() if upstream != upstream else (gr[~dead] != 0).all())


# ---- 5. misaligned and non-contiguous views -------------------------------------------------------------------------------
def test_misaligned_views_give_the_bits_of_the_aligned_call():
    shape = (2, 1, 8, 64)
    p, g = _inputs(shape)
    pa, ga = dev(p), dev(g)

    def shifted(t):
        buf = torch.zeros(t.numel() + 1, device=DEV)
        out = buf[1:].view(t.shape)
        out.copy_(t)
        return out
    ps, gs = shifted(pa), shifted(ga)
    assert pa.data_ptr() % 16 == 0 and ga.data_ptr() % 16 == 0
    assert ps.data_ptr() % 16 == 4 and gs.data_ptr() % 16 == 4 and ps.is_contiguous() and gs.is_contiguous()
    want = _bits_of_op(pa, ga)
    for pin, gin in ((ps, gs), (ps, ga), (pa, gs)):
        pp = pin.detach().requires_grad_(True)
        assert pp.data_ptr() == pin.data_ptr()
        loss, state = torch.ops.cerberus.inv_huber(pp, gin)
        gr, = torch.autograd.grad(loss, pp)
        for a, b in zip(want, (loss.detach(), state, gr)):
            assert torch.equal(a, b)
    # a non-contiguous view of the prediction gives the bits of its contiguous copy
    wide = torch.zeros(shape[:3] + (shape[3] + 8,), device=DEV)
    wide[..., :shape[3]] = pa
    view = wide[..., :shape[3]]
    assert not view.is_contiguous()
    for a, b in zip(want, _bits_of_op(view, ga)):
        assert torch.equal(a, b)


# ---- 6. linearity in the upstream gradient ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ROUTE_SHAPES)
def test_gradient_is_exactly_linear_in_the_upstream_gradient(shape):
    p, g = _inputs(shape)
    gd = dev(g)
    grads = []
    for factor in (1.0, 4.0, 0.125):
        pp = dev(p).requires_grad_(True)
        gr, = torch.autograd.grad(ca.inv_huber_loss(pp, gd) * factor, pp)
        grads.append(gr)
    assert torch.equal(grads[1], grads[0] * 4.0) and torch.equal(grads[2], grads[0] * 0.125)
    assert float(grads[0].abs().max()) > 0


# ---- 7. reproducibility -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 37, 53), (2, 1, 128, 256)])
def test_two_runs_give_the_same_bits(shape):
    p, g = _inputs(shape)
    pd, gd = dev(p), dev(g)
    runs = [_bits_of_op(pd, gd) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 8. graph replay ----------------------------------------------------------------------------------------------------
def test_inv_huber_graphed_replay_is_bit_equal_to_eager():
    """Value + backward captured in ONE graph on a single stream (linear: no parallel branches), replayed on three different
    inputs with an eager call in between: nothing is zeroed, nothing synchronises, and the fixed-order reductions give the
    eager bits every time."""
    shape = (2, 1, 128, 256)
    s_p = torch.zeros(shape, device=DEV, requires_grad=True)
    s_g = torch.zeros((shape[0],) + shape[2:], device=DEV)

    def step(p, g):
        v = ca.inv_huber_loss(p, g)
        gr, = torch.autograd.grad(v, p)
        return v, gr

    p0, g0 = _inputs(shape, 2200)
    with torch.no_grad():
        s_p.copy_(dev(p0))
        s_g.copy_(dev(g0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(s_p, s_g)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_v, g_g = step(s_p, s_g)
    for i in range(3):
        p, g = _inputs(shape, 2210 + 20 * i)
        with torch.no_grad():
            s_p.copy_(dev(p))
            s_g.copy_(dev(g))
        graph.replay()
        torch.cuda.synchronize()
        v, gr = step(dev(p).requires_grad_(True), dev(g))                 # the eager call in between
        assert torch.equal(g_v, v.detach()), (i, float(g_v), float(v))
        assert torch.equal(g_g, gr), i
        assert bool(torch.isfinite(g_v)) and float(g_g.abs().max()) > 0


# ---- 9. the class, on the reference's golden cases ----------------------------------------------------------------------
@pytest.mark.parametrize("i", [i for i, c in enumerate(cases.GOLDEN_CASES) if c[0] == "InvHuberLoss"])
def test_class_against_the_reference_golden(golden, monkeypatch, i):
    gold = golden("depth_loss")
    _, shape, kwargs, _ = cases.GOLDEN_CASES[i]
    p, g = gold["c%d_pred" % i], gold["c%d_gt" % i]
    want_v, want_g = float(gold["c%d_f64_value" % i]), gold["c%d_f64_grad" % i]
    ps = dev(p).requires_grad_(True)
    vs = ca.InvHuberLoss(backend="torch", **kwargs)({"depth": ps}, {"disparity": dev(g)})
    gs, = torch.autograd.grad(vs, ps)

    def boom(*_a, **_k):
        raise AssertionError("a stock formulation was taken with backend='hip'")
    monkeypatch.setattr(torch, "relu", boom)
    monkeypatch.setattr(F, "relu", boom)
    monkeypatch.setattr(torch.Tensor, "max", boom)
    pp = dev(p).requires_grad_(True)
    v = ca.InvHuberLoss(backend="hip", **kwargs)({"depth": pp}, {"disparity": dev(g)})
    gr, = torch.autograd.grad(v, pp)
    monkeypatch.undo()
    label = "reference %d %s %s" % (i, shape, kwargs)
    assert v.shape == () and v.dtype == torch.float32
    _check_value(label, v.item(), vs.item(), want_v)
    _check_grad(label, gr.cpu().numpy(), gs.cpu().numpy(), want_g, _max_mask(p, g))


# ---- 10. the stock path, and what the raw op refuses --------------------------------------------------------------------
def test_wrapper_takes_the_stock_path_for_what_the_op_does_not_cover():
    shape = (2, 1, 8, 64)
    p, g = _inputs(shape)
    pd, gd = dev(p), dev(g)
    fused = ca.inv_huber_loss(pd, gd)
    # A 16-bit prediction: stock ops (in fp32 from the subtraction on: the fp32 ground truth promotes).  Rounding a prediction
    # below 8 to fp16 moves d by at most 2^-9.  The loss moves by at most 5 times that through the terms (|dterm/dd| is 1 on
    # the linear side and d / c <= m / c = 5 on the quadratic one) plus 0.2 * 12 times that through the cutoff (m moves by at
    # most 2^-9, c by 0.2 of it, and |dterm/dc| = |1/2 - d^2 / (2 c^2)| <= 12): 7.4 * 2^-9 in all, an absolute bound.
    v16 = ca.inv_huber_loss(pd.half(), gd)
    assert float(p.max()) < 8.0 and abs(float(v16) - float(fused)) <= 7.4 * 2.0 ** -9
    # CPU tensors: stock ops; two fp32 evaluations, each within VALUE_TOL of the float64 value
    cpu = ca.inv_huber_loss(pd.cpu(), gd.cpu())
    assert cpu.device.type == "cpu" and abs(float(cpu) - float(fused)) <= 2 * VALUE_TOL * float(fused)
    # a ground truth that asks for a gradient: stock ops, and it gets one
    gg = gd.clone().requires_grad_(True)
    v = ca.inv_huber_loss(pd, gg)
    assert float(torch.autograd.grad(v, gg)[0].abs().sum()) > 0
    assert abs(float(v.detach()) - float(fused)) <= 2 * VALUE_TOL * float(fused)
    with pytest.raises(RuntimeError, match="no gradient for the ground truth"):
        torch.autograd.grad(torch.ops.cerberus.inv_huber(pd.clone().requires_grad_(True), gg)[0], gg)
    # what the raw op refuses
    op = torch.ops.cerberus.inv_huber
    with pytest.raises(RuntimeError, match="float32"):
        op(pd.half(), gd)
    with pytest.raises(RuntimeError, match="float32"):
        op(pd, gd.double())
    with pytest.raises(RuntimeError, match=r"gt must be \(B,H,W\)"):
        op(pd, gd[:1])
    with pytest.raises(RuntimeError, match=r"gt must be \(B,H,W\)"):
        op(pd, gd[:, None])
    with pytest.raises(RuntimeError, match="integer multiple"):
        op(pd, gd[:, :, :-1])
    with pytest.raises(RuntimeError, match=r"pred must be \(B,1,h,w\) or \(B,h,w\)"):
        op(pd.expand(2, 3, 8, 64), gd)
    with pytest.raises(RuntimeError):
        op(pd.cpu(), gd)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        op(pd.cpu(), gd.cpu())
    # no double backward
    pp = pd.clone().requires_grad_(True)
    gr, = torch.autograd.grad(ca.inv_huber_loss(pp, gd), pp, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(gr.sum(), pp)


# ---- 11. past one round: 257 to 1536 partials, the max pass's grid stride, both branches of fold_parts ----------------------------
CASE_IDS = ["x".join(map(str, c[0])) for c in rc.DEPTH_CASES]


def _at_prediction(case, g):
    """(the ground truth a prediction pixel reads, the finer one for the op or None)"""
    return np.ascontiguousarray(rc.depth_gt_at_prediction(case, g)), (g if rc.depth_route(case) == "gather" else None)


@functools.lru_cache(maxsize=None)
def _reference_of_case(case):
    p, g = rc.depth_inputs(case)
    return _reference(p, _at_prediction(case, g)[0])


def _state(p, g):
    return torch.ops.cerberus.inv_huber(dev(p), dev(g))[1]


@pytest.mark.parametrize("case", rc.DEPTH_CASES, ids=CASE_IDS)
def test_table_shapes_against_float64(case):
    p, g = rc.depth_inputs(case)
    gp, fine = _at_prediction(case, g)
    _check_case("inv_huber %s" % (case,), p, gp, _reference_of_case(case), gt_for_op=fine)
    d = np.maximum(p.reshape(gp.shape), np.float32(0)) - gp
    m = np.where(gp > 0, np.abs(d), np.float32(0)).max()
    state = _state(p, g)
    assert float(state[3]) == float(m) and float(state[0]) == float(np.float32(0.2) * m)
    assert float(state[2]) == float(np.float32(1) / np.float32(p.size))


@pytest.mark.parametrize("case,k", [(c, k) for c in rc.DEPTH_CASES for k in rc.depth_marker_chunks(c)],
                         ids=["%s-%d" % (i, k) for c, i in zip(rc.DEPTH_CASES, CASE_IDS) for k in rc.depth_marker_chunks(c)])
def test_the_strict_maximum_in_chunk_k(case, k):
    """The maximum of err is 20 + 5 k / 64 (its cutoff is exact in fp32: reduction_cases.depth_marker), at one pixel inside chunk k: a chunk that the max pass's stride skips, or a partial
    maximum that ``fold_parts`` does not read, leaves a maximum below 6."""
    p, g, pixel, err = rc.depth_marker(case, k)
    gp, fine = _at_prediction(case, g)
    _check_case("inv_huber %s maximum in chunk %d" % (case, k), p, gp, gt_for_op=fine)
    state = _state(p, g)
    assert float(state[3]) == float(err) and float(state[0]) == float(np.float32(0.2) * err), (float(state[3]), float(err))


@pytest.mark.parametrize("case", [c for c in rc.DEPTH_CASES if "inv_huber_max grid stride, %s" % rc.depth_route(c) in rc.depth_tiers(c)],
                         ids=lambda c: "x".join(map(str, c[0])))
def test_a_tie_between_chunk_0_and_a_chunk_past_1024(case):
    p, g, pixels = rc.depth_tie(case)
    assert pixels[0] < 1024 and pixels[1] // 1024 >= ca.ops.INV_HUBER_MAX_PARTS
    v, gr = _check_case("inv_huber %s tie" % (case,), p, g)
    state = _state(p, g)
    assert float(state[3]) == 19.0 and float(state[0]) == float(np.float32(0.2) * np.float32(19.0))
    # ties = 2: state[1] = 0.2 S / ties against float64 (every term of S is <= 0: no cancellation)
    d = np.maximum(p.reshape(g.shape).astype(np.float64), 0) - g
    err = np.where(g > 0, np.abs(d), 0)
    c = 0.2 * err.max()
    share = 0.2 * (0.5 - d[err > c] ** 2 / (2 * c * c)).sum() / 2
    assert abs(float(state[1]) - share) <= VALUE_TOL * abs(share), (float(state[1]), share)
    a, b = gr.reshape(-1)[pixels[0]].item(), gr.reshape(-1)[pixels[1]].item()
    assert a == -b and a != 0                     # split evenly: the same magnitude, the sign of d


def test_a_table_shape_twice_and_misaligned_gives_the_same_bits():
    case = rc.case_of("depth", (1, 1, 1025, 1024))
    p, g = rc.depth_inputs(case)
    pa, ga = dev(p), dev(g)

    def shifted(t):
        buf = torch.zeros(t.numel() + 1, device=DEV)
        out = buf[1:].view(t.shape)
        out.copy_(t)
        return out
    ps, gs = shifted(pa), shifted(ga)
    assert pa.data_ptr() % 16 == 0 and ga.data_ptr() % 16 == 0 and ps.data_ptr() % 16 == 4 and gs.data_ptr() % 16 == 4
    want = _bits_of_op(pa, ga)
    for a, b in zip(want, _bits_of_op(pa, ga)):
        assert torch.equal(a, b)
    pp = ps.detach().requires_grad_(True)
    assert pp.data_ptr() == ps.data_ptr()
    loss, state = torch.ops.cerberus.inv_huber(pp, gs)
    gr, = torch.autograd.grad(loss, pp)
    for a, b in zip(want, (loss.detach(), state, gr)):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(want[0])) and float(want[2].abs().max()) > 0
