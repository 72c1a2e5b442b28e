"""GPU tests of the segmentation loss (csrc/seg_loss.hip): ``seg_cross_entropy`` / ``cerberus::seg_cross_entropy``,
``class_balance_weights`` / ``cerberus::class_histogram`` and the classes ``FocalLoss2D`` / ``SegCrossEntropy``.

Yardstick: ``F.cross_entropy(logits, target, weight=w, ignore_index=i)`` and the focal factor of its mean, evaluated in float64
on the CPU.  Tolerances are those of tests/test_photometric_gpu.py.  Values: relative error <= 1e-5.  Gradients: ``l2_err`` and
``rel_err`` against float64, each at most 4 x max(e_stock, 2^-23), where e_stock is the same error of the stock fp32 chain run
on the GPU in the same test; the floor of one fp32 rounding unit is there because at a 35-pixel case the stock error is a
matter of luck (a CPU emulation of the fused order gave ratios up to 2.7 against stock at (1,2,5,7)).

Shapes: the smallest at which each route can go wrong.  Scalar route (H*W odd or 2 mod 4, one workgroup with idle lanes):
(1,19,1,1), (1,2,5,7), (2,19,37,53), (1,19,3,66).  Vector route: (1,19,1,4), (2,19,8,64), (3,5,16,33) (odd W: a lane's 4
pixels cross a row).  (2,150,9,20): many classes.  (2,19,128,256): 64 workgroups, so the partial fold matters; every thread of
``seg_ce_final_kernel`` still reads at most ONE partial there.  Its strided loop runs at the shapes of
tests/reduction_cases.py (checked on the CPU by tests/test_reduction_tiers_cpu.py): (1,2,257,1024), vector, 257 partials -- thread
0 adds two; (1,3,601,1023), scalar, 601 -- threads add three or two; (2,2,129,1028), vector, 260, the image boundary inside a
chunk.  At those shapes a sum could hide one mis-addressed partial, so section 11 also counts ONE pixel, placed in the first
chunk, in 255, 256, 511, 512 and in the last.  (2,19,8,64) as a view 4 bytes into a larger buffer: misaligned pointers, bit-equal
to the aligned call; (2,2,129,1028) likewise.

Section 12: logits of -inf (classes switched off), +inf, and finite logits up to 6e38 apart, on one shape per route."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cerberusnet_amd as ca
import reduction_cases as rc
import seg_loss_cases as cases
from cerberusnet_amd.synth import hash_uniform
from conftest import l2_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_TOL = 1e-5
GRAD_FACTOR = 4.0
GRAD_FLOOR = 2.0 ** -23

SCALAR_SHAPES = [(1, 19, 1, 1), (1, 2, 5, 7), (2, 19, 37, 53), (1, 19, 3, 66)]
VECTOR_SHAPES = [(1, 19, 1, 4), (2, 19, 8, 64), (3, 5, 16, 33)]
SHAPES = SCALAR_SHAPES + VECTOR_SHAPES + [(2, 150, 9, 20), (2, 19, 128, 256)]
GAMMAS = [0.0, 2.0, 0.5]
WEIGHTS = ["ones", "dynamic", "given"]
IGNORES = [255, -1]
# every shape with every gamma, every kind of weights and both ignore values once; one shape per route with the whole product
COMBOS = [(shape, g, w, i) for shape in SHAPES for g, w, i in ((0.0, "ones", 255), (2.0, "dynamic", -1), (0.5, "given", 255))]
COMBOS += [(shape, g, w, i) for shape in ((2, 19, 37, 53), (2, 19, 8, 64)) for g in GAMMAS for w in WEIGHTS for i in IGNORES
           if (shape, g, w, i) not in COMBOS]
COMBOS += rc.SEG_CASES                    # past 256 partials: the strided loop of seg_ce_final_kernel (reduction_cases.py)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _labels(shape, ignore_index, seed=905):
    t = cases.labels(shape, seed, ignore_index)
    if t.reshape(-1)[0] == ignore_index:         # the one-pixel shapes need a pixel that counts
        t.reshape(-1)[0] = 0
    return t


def _inputs(shape, ignore_index, seed=900):
    return cases.logits(shape, seed), _labels(shape, ignore_index, seed + 5)


def _weights(kind, shape, t, ignore_index):
    """(C,) float32 class weights: ones; the reference's dynamic weights (its ``unique`` formula, on the CPU); a given vector in
    [0.5, 2) with class 1 at weight 0."""
    C = shape[1]
    if kind == "ones":
        return np.ones(C, dtype=np.float32)
    if kind == "dynamic":
        tt = torch.from_numpy(t)
        w = torch.ones(C)
        ids, counts = tt[tt != ignore_index].unique(return_counts=True)
        w[ids] = 0.125 / (0.125 + counts / float(tt.nelement()))
        return w.numpy()
    w = hash_uniform((C,), 77, 0.5, 2.0)
    w[1] = 0.0
    return w


def _check_weights(got, want):
    """Dynamic weights formed on the GPU against the same formula on the CPU: the counts are integers and equal; two divisions
    and a sum follow, each within one fp32 rounding unit of the CPU's."""
    assert got.dtype == torch.float32 and got.device.type == "cuda"
    want = torch.from_numpy(want)
    assert torch.equal(got.cpu() == 1.0, want == 1.0)                      # the absent classes
    assert float(((got.cpu() - want).abs() / want).max()) <= 3 * 2.0 ** -23


def _stock(x, t, w, ignore_index, gamma):
    ce = F.cross_entropy(x, t, weight=w, ignore_index=ignore_index)
    return ce if gamma == 0 else torch.pow(1 - torch.exp(-ce), gamma) * ce


@functools.lru_cache(maxsize=None)
def _reference(shape, gamma, kind, ignore_index):
    """Value and logit gradient in float64 on the CPU, computed once per case and shared."""
    x, t = _inputs(shape, ignore_index)
    w = _weights(kind, shape, t, ignore_index)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    v = _stock(x64, torch.from_numpy(t), torch.from_numpy(w).double(), ignore_index, gamma)
    g, = torch.autograd.grad(v, x64)
    return v.item(), g.numpy()


def _check_grad(name, fused, stock, ref):
    for metric in (l2_err, rel_err):
        ef, es = metric(fused, ref), metric(stock, ref)
        print("%s %s: fused %.3e stock fp32 %.3e (bound %.3e)" % (name, metric.__name__, ef, es, GRAD_FACTOR * max(es, GRAD_FLOOR)))
        assert ef <= GRAD_FACTOR * max(es, GRAD_FLOOR), (name, metric.__name__, ef, es)


def _check_value(name, v, vs, ref_v):
    print("%s value: fused rel %.3e stock fp32 rel %.3e" % (name, abs(v - ref_v) / abs(ref_v), abs(vs - ref_v) / abs(ref_v)))
    assert abs(v - ref_v) <= VALUE_TOL * abs(ref_v), (name, v, ref_v)


def _fused(x, t, w, ignore_index, gamma):
    """(value, gradient) of the wrapper on device tensors."""
    xx = x.detach().clone().requires_grad_(True)
    v = ca.seg_cross_entropy(xx, t, w, ignore_index, gamma)
    g, = torch.autograd.grad(v, xx)
    return v.detach(), g


# ---- 1. value and gradient against float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,gamma,kind,ignore_index", COMBOS)
def test_value_and_gradient_against_float64(shape, gamma, kind, ignore_index):
    x, t = _inputs(shape, ignore_index)
    w = _weights(kind, shape, t, ignore_index)
    ref_v, ref_g = _reference(shape, gamma, kind, ignore_index)
    xd, td = dev(x), dev(t)
    wd = None if kind == "ones" else dev(w)
    if kind == "dynamic":
        _check_weights(ca.class_balance_weights(td, shape[1], ignore_index, 0.125), w)      # the histogram op
    v, g = _fused(xd, td, wd, ignore_index, gamma)
    assert v.shape == () and v.dtype == torch.float32 and g.shape == xd.shape
    xs = xd.clone().requires_grad_(True)
    vs = _stock(xs, td, dev(w), ignore_index, gamma)
    gs, = torch.autograd.grad(vs, xs)
    name = "seg %s gamma %g %s ignore %d" % (shape, gamma, kind, ignore_index)
    _check_value(name, v.item(), vs.item(), ref_v)
    _check_grad(name, g.cpu().numpy(), gs.cpu().numpy(), ref_g)
    # the raw op: the same bits, lse per pixel, and the state the backward reads
    loss, lse, state = torch.ops.cerberus.seg_cross_entropy(xd, td, dev(w), ignore_index, gamma)
    assert torch.equal(loss, v) and lse.shape == td.shape and state.shape == (4,)
    lse64 = torch.logsumexp(torch.from_numpy(x).double(), 1)
    # each of the C - 1 additions into the running sum rounds by at most 2^-24 of it, which is that much in its logarithm;
    # expf, logf and the last addition are a few units more
    assert rel_err(lse.cpu().numpy(), lse64.numpy()) <= (shape[1] + 8) * 2.0 ** -24
    assert float(state[3]) == 0.0 and float(state[1]) > 0
    if gamma == 0:
        assert torch.equal(loss, state[0])                                      # exactly ce: a branch, not pow(., 0)


def test_misaligned_logits_give_the_bits_of_the_aligned_call():
    shape, ignore_index = (2, 19, 8, 64), 255
    x, t = _inputs(shape, ignore_index)
    w = dev(_weights("given", shape, t, ignore_index))
    td = dev(t)
    aligned = dev(x)
    buf = torch.zeros(aligned.numel() + 1, device=DEV)
    shifted = buf[1:].view(shape)
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    res = []
    for xin in (aligned, shifted):
        xx = xin.detach().requires_grad_(True)
        assert xx.data_ptr() == xin.data_ptr()
        loss, lse, state = torch.ops.cerberus.seg_cross_entropy(xx, td, w, ignore_index, 2.0)
        g, = torch.autograd.grad(loss, xx)
        res.append((loss.detach(), lse, state, g))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # misaligned labels too (a view 8 bytes into a larger buffer)
    tbuf = torch.zeros(td.numel() + 1, dtype=torch.int64, device=DEV)
    tshift = tbuf[1:].view(td.shape)
    tshift.copy_(td)
    assert tshift.data_ptr() % 16 == 8
    xx = aligned.detach().requires_grad_(True)
    loss, lse, state = torch.ops.cerberus.seg_cross_entropy(xx, tshift, w, ignore_index, 2.0)
    g, = torch.autograd.grad(loss, xx)
    for a, b in zip(res[0], (loss.detach(), lse, state, g)):
        assert torch.equal(a, b)


# ---- 2. ignored pixels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 19, 37, 53), (2, 19, 8, 64)])
@pytest.mark.parametrize("ignore_index", IGNORES)
def test_ignored_pixels_get_an_exactly_zero_gradient(shape, ignore_index):
    x, t = _inputs(shape, ignore_index)
    td = dev(t)
    v, g = _fused(dev(x), td, None, ignore_index, 2.0)
    dead = (td == ignore_index)[:, None].expand_as(g)
    assert int(dead.sum()) > 0 and bool(torch.isfinite(v))
    assert bool((g[dead] == 0).all()) and bool(torch.isfinite(g).all())
    assert bool((g[~dead] != 0).any())
    # every pixel ignored: 0 / 0 as stock, and nothing but zeros in the gradient (a select, not NaN * 0)
    v, g = _fused(dev(x), torch.full_like(td, ignore_index), None, ignore_index, 2.0)
    assert bool(torch.isnan(v)) and bool((g == 0).all())
    # den == 0 with valid pixels: every class at weight 0
    v, g = _fused(dev(x), td, torch.zeros(shape[1], device=DEV), ignore_index, 0.0)
    assert bool(torch.isnan(v)) and bool((g == 0).all())


# ---- 3. NaN handling ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 19, 37, 53), (2, 19, 8, 64)])
def test_nan_logits(shape):
    ignore_index = 255
    x, t = _inputs(shape, ignore_index)
    td = dev(t)
    w = dev(_weights("given", shape, t, ignore_index))
    clean = ca.seg_cross_entropy(dev(x), td, w, ignore_index, 2.0)
    flat = t.reshape(-1)
    valid_p, ignored_p = int(np.flatnonzero(flat != ignore_index)[7]), int(np.flatnonzero(flat == ignore_index)[3])
    hw = shape[2] * shape[3]
    for p, channel in ((valid_p, 0), (valid_p, shape[1] - 1), (ignored_p, 0), (ignored_p, 5)):
        xn = x.copy()
        xn[p // hw, channel].reshape(-1)[p % hw] = np.nan
        v = ca.seg_cross_entropy(dev(xn), td, w, ignore_index, 2.0)
        if p == valid_p:
            assert bool(torch.isnan(v)), (p, channel)                      # not a silently dropped pixel
        else:
            assert torch.equal(v, clean), (p, channel)                     # skipped by selection, not multiplied by 0


# ---- 4. out-of-range labels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 19, 37, 53), (2, 19, 8, 64)])
@pytest.mark.parametrize("bad", ["C", "-5", "2^40"])
def test_out_of_range_label(shape, bad):
    ignore_index = 255
    x, t = _inputs(shape, ignore_index)
    t = t.copy()
    p = 11
    t.reshape(-1)[p] = {"C": shape[1], "-5": -5, "2^40": 1 << 40}[bad]
    v, g = _fused(dev(x), dev(t), None, ignore_index, 0.0)
    torch.cuda.synchronize()                                               # the call returns normally: no fault, no assertion
    assert bool(torch.isnan(v))                                            # neither dropped nor counted
    hw = shape[2] * shape[3]
    assert bool((g[p // hw, :, (p % hw) // shape[3], (p % hw) % shape[3]] == 0).all())
    hist = torch.ops.cerberus.class_histogram(dev(t), shape[1], ignore_index)
    keep = (t != ignore_index) & (t >= 0) & (t < shape[1])
    assert torch.equal(hist.cpu(), torch.from_numpy(np.bincount(t[keep], minlength=shape[1])))


# ---- 5. linearity in the upstream gradient ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 19, 37, 53), (2, 19, 8, 64)])
def test_gradient_is_exactly_linear_in_the_upstream_gradient(shape):
    ignore_index = -1
    x, t = _inputs(shape, ignore_index)
    td = dev(t)
    w = ca.class_balance_weights(td, shape[1], ignore_index)
    grads = []
    for factor in (1.0, 4.0, 0.125):
        xx = dev(x).requires_grad_(True)
        g, = torch.autograd.grad(ca.seg_cross_entropy(xx, td, w, ignore_index, 2.0) * factor, xx)
        grads.append(g)
    assert torch.equal(grads[1], grads[0] * 4.0) and torch.equal(grads[2], grads[0] * 0.125)
    assert float(grads[0].abs().max()) > 0


# ---- 6. reproducibility -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 19, 37, 53), (2, 19, 128, 256)])
def test_two_runs_give_the_same_bits(shape):
    ignore_index = 255
    x, t = _inputs(shape, ignore_index)
    xd, td = dev(x), dev(t)
    runs = []
    for _ in range(2):
        w = ca.class_balance_weights(td, shape[1], ignore_index)
        v, g = _fused(xd, td, w, ignore_index, 2.0)
        runs.append((w, v, g))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 7. graph replay ----------------------------------------------------------------------------------------------------
def test_seg_loss_graphed_replay_is_bit_equal_to_eager():
    """Dynamic weights + value + backward captured in ONE graph on a single stream (linear: no parallel branches), replayed
    on three different inputs with an eager call in between: no unique(), no synchronisation, and the fixed-order reductions
    give the eager bits every time."""
    shape, ignore_index = (2, 19, 128, 256), 255
    s_x = torch.zeros(shape, device=DEV, requires_grad=True)
    s_t = torch.zeros((shape[0],) + shape[2:], dtype=torch.int64, device=DEV)

    def step(x, t):
        w = ca.class_balance_weights(t, shape[1], ignore_index, 0.125)
        v = ca.seg_cross_entropy(x, t, w, ignore_index, 2.0)
        g, = torch.autograd.grad(v, x)
        return v, g

    x0, t0 = _inputs(shape, ignore_index, 950)
    with torch.no_grad():
        s_x.copy_(dev(x0))
        s_t.copy_(dev(t0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(s_x, s_t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_v, g_g = step(s_x, s_t)
    for i in range(3):
        x, t = _inputs(shape, ignore_index, 960 + 20 * i)
        with torch.no_grad():
            s_x.copy_(dev(x))
            s_t.copy_(dev(t))
        graph.replay()
        torch.cuda.synchronize()
        v, g = step(dev(x).requires_grad_(True), dev(t))                  # the eager call in between
        assert torch.equal(g_v, v.detach()), (i, float(g_v), float(v))
        assert torch.equal(g_g, g), i
        assert bool(torch.isfinite(g_v)) and float(g_g.abs().max()) > 0


# ---- 8. class histogram -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignore_index", IGNORES)
@pytest.mark.parametrize("num_classes", [2, 19, 150, 1024])
def test_class_histogram_equals_bincount(num_classes, ignore_index):
    for shape, seed in (((2, 50, 51), 30), ((2, 512, 512), 31)):           # one workgroup with a ragged end; 256 with a grid stride
        u = hash_uniform(shape, seed, 0.0, 1.0, dtype=np.float64)
        t = np.floor(u * u * (num_classes + 6)).astype(np.int64) - 3      # skewed, with labels below 0 and at C and above
        t[hash_uniform(shape, seed + 1, 0.0, 1.0) < 0.15] = ignore_index
        t[hash_uniform(shape, seed + 2, 0.0, 1.0) < 0.01] = 1 << 35
        keep = (t != ignore_index) & (t >= 0) & (t < num_classes)
        assert (~keep).sum() > 0 and (t < 0).any() and (t >= num_classes).any()
        want = torch.bincount(torch.from_numpy(t[keep]), minlength=num_classes)
        got = torch.ops.cerberus.class_histogram(dev(t), num_classes, ignore_index)
        assert got.dtype == torch.int64 and got.shape == (num_classes,)
        assert torch.equal(got.cpu(), want), (shape, num_classes)
        assert torch.equal(torch.ops.cerberus.class_histogram(dev(t), num_classes, ignore_index), got)
    assert int(torch.ops.cerberus.class_histogram(torch.zeros(0, dtype=torch.int64, device=DEV), num_classes, ignore_index).sum()) == 0


def test_class_balance_weights_above_the_compiled_limit_and_raw_op_errors():
    C, ignore_index = ca.ops.HISTOGRAM_MAX_CLASSES + 5, 255
    t = _labels((2, C, 9, 20), ignore_index)
    w = ca.class_balance_weights(dev(t), C, ignore_index)                  # torch.bincount
    _check_weights(w, _weights("dynamic", (2, C, 9, 20), t, ignore_index))
    with pytest.raises(RuntimeError, match="num_classes"):
        torch.ops.cerberus.class_histogram(dev(t), C, ignore_index)
    with pytest.raises(RuntimeError, match="int64"):
        torch.ops.cerberus.class_histogram(dev(t).int(), 19, ignore_index)


# ---- 9. the classes, on the reference's golden cases --------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(cases.GOLDEN_CASES)))
def test_classes_against_the_reference_golden(golden, monkeypatch, i):
    g = golden("seg_loss")
    name, shape, kwargs, _ = cases.GOLDEN_CASES[i]
    x, t = dev(g["c%d_logits" % i]), dev(g["c%d_target" % i])
    want_v, want_g = float(g["c%d_f64_value" % i]), g["c%d_f64_grad" % i]
    xs = x.clone().requires_grad_(True)
    vs = getattr(ca, name)(backend="torch", **kwargs)({"seg": xs}, {"seg": t})
    gs, = torch.autograd.grad(vs, xs)

    def boom(*_a, **_k):
        raise AssertionError("a stock formulation was taken with backend='hip'")
    monkeypatch.setattr(F, "cross_entropy", boom)
    monkeypatch.setattr(torch, "unique", boom)
    monkeypatch.setattr(torch.Tensor, "unique", boom)
    xx = x.clone().requires_grad_(True)
    v = getattr(ca, name)(**kwargs)({"seg": xx}, {"seg": t})
    gx, = torch.autograd.grad(v, xx)
    monkeypatch.undo()
    label = "reference %d %s %s %s" % (i, name, shape, kwargs)
    assert v.shape == () and v.dtype == torch.float32
    _check_value(label, v.item(), vs.item(), want_v)
    _check_grad(label, gx.cpu().numpy(), gs.cpu().numpy(), want_g)


# ---- 10. the stock path, and what the raw op refuses --------------------------------------------------------------------
def test_wrapper_takes_the_stock_path_for_what_the_op_does_not_cover():
    shape, ignore_index = (2, 19, 8, 64), 255
    x, t = _inputs(shape, ignore_index)
    xd, td = dev(x), dev(t)
    w = dev(_weights("given", shape, t, ignore_index))
    fused = ca.seg_cross_entropy(xd, td, w, ignore_index)
    # 16-bit logits: stock ops, a 16-bit result.  Rounding a logit to fp16 moves it by at most 2^-11 * 4; lse and x_t are
    # 1-Lipschitz in that, so ce (> 1 here) moves by less than 2^-8, and the fp16 result adds 2^-11 relative: 1e-2 in all
    v16 = ca.seg_cross_entropy(xd.half(), td, w, ignore_index)
    assert v16.dtype == torch.float16 and float(fused) > 1.0
    assert abs(float(v16) - float(fused)) <= 1e-2 * float(fused)
    # a weight that asks for a gradient: stock ops, and it gets one
    wg = w.clone().requires_grad_(True)
    xg = xd.clone().requires_grad_(True)
    v = ca.seg_cross_entropy(xg, td, wg, ignore_index, 2.0)
    gx, gw = torch.autograd.grad(v, (xg, wg))
    assert float(gw.abs().sum()) > 0 and float(gx.abs().sum()) > 0
    assert abs(float(v) - float(ca.seg_cross_entropy(xd, td, w, ignore_index, 2.0))) <= VALUE_TOL * float(v)
    with pytest.raises(RuntimeError, match="no gradient for its class weights"):
        torch.autograd.grad(torch.ops.cerberus.seg_cross_entropy(xg, td, wg, ignore_index, 2.0)[0], (xg, wg))
    # one class: stock ops (the value is 0)
    one = ca.seg_cross_entropy(xd[:, :1], td.clamp(max=0), None, ignore_index)
    assert torch.equal(one, F.cross_entropy(xd[:, :1], td.clamp(max=0), ignore_index=ignore_index)) and float(one) == 0.0
    # CPU tensors: stock ops
    cpu = ca.seg_cross_entropy(xd.cpu(), td.cpu(), w.cpu(), ignore_index)
    assert cpu.device.type == "cpu" and abs(float(cpu) - float(fused)) <= VALUE_TOL * float(fused)
    # what the raw op refuses
    op = torch.ops.cerberus.seg_cross_entropy
    with pytest.raises(RuntimeError, match="float32"):
        op(xd.half(), td, w, ignore_index, 0.0)
    with pytest.raises(RuntimeError, match="int64"):
        op(xd, td.int(), w, ignore_index, 0.0)
    with pytest.raises(RuntimeError, match="one value per class"):
        op(xd, td, w[:-1], ignore_index, 0.0)
    with pytest.raises(RuntimeError, match=r"target must be \(B,H,W\)"):
        op(xd, td[:, None], w, ignore_index, 0.0)
    with pytest.raises(RuntimeError, match=r"target must be \(B,H,W\)"):
        op(xd, td[:, :, :-1], w, ignore_index, 0.0)
    with pytest.raises(RuntimeError):
        op(xd, td, w, ignore_index, -1.0)                                   # gamma < 0
    # no double backward
    xx = xd.clone().requires_grad_(True)
    g, = torch.autograd.grad(ca.seg_cross_entropy(xx, td, w, ignore_index, 2.0), xx, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(g.sum(), xx)
    # a non-contiguous view of the logits gives the bits of its contiguous copy
    wide = torch.zeros(shape[:3] + (shape[3] + 8,), device=DEV)
    wide[..., :shape[3]] = xd
    assert torch.equal(ca.seg_cross_entropy(wide[..., :shape[3]], td, w, ignore_index), fused)


# ---- 11. past 256 partials: one counted pixel, placed where the finish kernel's loop wraps -------------------------------------
@functools.lru_cache(maxsize=None)
def _device_logits(shape):
    """The logits of a table shape, host and device, shared by the marker cases; neither is written to."""
    x = _inputs(shape, 255)[0]
    return x, dev(x)


def _bits(x, t, w, ignore_index, gamma):
    xx = x.detach().requires_grad_(True)
    assert xx.data_ptr() == x.data_ptr()
    loss, lse, state = torch.ops.cerberus.seg_cross_entropy(xx, t, w, ignore_index, gamma)
    g, = torch.autograd.grad(loss, xx)
    return loss.detach(), lse, state, g


MARKERS = [(c[0], k) for c in rc.SEG_CASES for k in rc.marker_chunks(rc.chunks(c[0][0] * c[0][2] * c[0][3], ca.ops.SEG_CHUNK_PIXELS))]


@pytest.mark.parametrize("shape,k", MARKERS, ids=["%s-%d" % ("x".join(map(str, s)), k) for s, k in MARKERS])
def test_one_counted_pixel_in_chunk_k(shape, k):
    """Every label is the ignore value except one inside chunk k: the value is that pixel's cross-entropy (its weight cancels in
    num / den), and the gradient is non-zero in that pixel's C entries and 0.0 everywhere else.  A partial that the finish
    kernel skips or reads twice changes the value by all or twice of it."""
    B, C, H, W = shape
    x, xd = _device_logits(shape)
    t, p, cls = rc.seg_marker(shape, k)
    td, wd = dev(t), dev(rc.seg_marker_weights(C))
    v, _, state, g = _bits(xd, td, wd, 255, 0.0)                              # one call: value, state and gradient
    with torch.no_grad():
        vs = _stock(xd, td, wd, 255, 0.0)
    _check_value("seg %s one pixel in chunk %d" % (shape, k), v.item(), vs.item(), rc.seg_marker_ce64(x, p, cls))
    b, r = divmod(p, H * W)
    assert bool((g[b, :, r // W, r % W] != 0).all()) and int((g != 0).sum()) == C
    assert float(state[1]) == float(rc.seg_marker_weights(C)[cls])               # den: the one weight, exactly


def test_a_table_shape_twice_and_misaligned_gives_the_same_bits():
    shape, gamma, kind, ignore_index = rc.case_of("seg", (2, 2, 129, 1028))
    x, t = _inputs(shape, ignore_index)
    xd, td, wd = dev(x), dev(t), dev(_weights(kind, shape, t, ignore_index))
    buf = torch.zeros(xd.numel() + 1, device=DEV)
    shifted = buf[1:].view(shape)
    shifted.copy_(xd)
    assert xd.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    want = _bits(xd, td, wd, ignore_index, gamma)
    for other in (_bits(xd, td, wd, ignore_index, gamma), _bits(shifted, td, wd, ignore_index, gamma)):
        for a, b in zip(want, other):
            assert torch.equal(a, b)
    assert bool(torch.isfinite(want[0])) and float(want[3].abs().max()) > 0


# ---- 12. -inf, +inf and far-apart logits -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pattern_case(kind, shape, pattern):
    return rc.inf_case(shape, pattern) if kind == "inf" else rc.far_case(shape, pattern)


@functools.lru_cache(maxsize=None)
def _pattern_reference(kind, shape, pattern, gamma):
    """Value and logit gradient in float64 on the CPU, computed once per case."""
    x, t, _, _ = _pattern_case(kind, shape, pattern)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    v = _stock(x64, torch.from_numpy(t), torch.from_numpy(rc.inf_weights(shape[1])).double(), rc.INF_IGNORE, gamma)
    g, = torch.autograd.grad(v, x64)
    return v.item(), g.numpy()


def _check_pattern(kind, shape, pattern, gamma):
    """Fused and stock fp32 on the GPU against float64 with the bounds of section 1; returns the fused gradient."""
    x, t, mask, planes = _pattern_case(kind, shape, pattern)
    ref_v, ref_g = _pattern_reference(kind, shape, pattern, gamma)
    assert np.isfinite(ref_v) and np.isfinite(ref_g).all()
    xd, td, wd = dev(x), dev(t), dev(rc.inf_weights(shape[1]))
    v, g = _fused(xd, td, wd, rc.INF_IGNORE, gamma)
    xs = xd.clone().requires_grad_(True)
    vs = _stock(xs, td, wd, rc.INF_IGNORE, gamma)
    gs, = torch.autograd.grad(vs, xs)
    name = "seg %s %s gamma %g" % (shape, pattern, gamma)
    _check_value(name, v.item(), vs.item(), ref_v)
    _check_grad(name, g.cpu().numpy(), gs.cpu().numpy(), ref_g)
    _, lse, _ = torch.ops.cerberus.seg_cross_entropy(xd, td, wd, rc.INF_IGNORE, gamma)
    lse, lse64 = lse.cpu().numpy(), torch.logsumexp(torch.from_numpy(x).double(), 1).numpy()
    for part in (mask, ~mask):                       # the changed pixels on their own: a plane at 3e38 would hide the others
        assert rel_err(lse[part], lse64[part]) <= (shape[1] + 8) * 2.0 ** -24, (name, rel_err(lse[part], lse64[part]))
    assert bool(torch.isfinite(g).all())
    return g, mask, planes


@pytest.mark.parametrize("shape", rc.INF_SHAPES)
@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("pattern", sorted(rc.INF_PATTERNS))
def test_minus_inf_logits_against_float64(shape, gamma, pattern):
    """Classes switched off by -inf on about a quarter of the pixels (never the target of a counted pixel): value, gradient and
    lse as for finite logits, and a gradient of exactly 0.0 at every -inf logit."""
    g, mask, planes = _check_pattern("inf", shape, pattern, gamma)
    at_inf = g.movedim(1, 0)[planes][:, dev(mask)]
    assert at_inf.numel() == len(planes) * int(mask.sum()) and bool((at_inf == 0).all())
    if len(planes) < shape[1] - 1:                  # with one finite logit left, the target's, the softmax is exactly one-hot
        assert float(g.movedim(1, 0)[:, dev(mask)].abs().max()) > 0


@pytest.mark.parametrize("shape", rc.INF_SHAPES)
@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("pattern", sorted(rc.FAR_PATTERNS))
def test_far_apart_finite_logits_against_float64(shape, gamma, pattern):
    """Planes at +-1e4, at +-3e38 (x - m overflows to +-inf) and 104 and 88 below the maximum (exp underflows to 0 and to a
    subnormal)."""
    _check_pattern("far", shape, pattern, gamma)


@pytest.mark.parametrize("shape", rc.INF_SHAPES)
@pytest.mark.parametrize("pattern", sorted(rc.INF_PATTERNS))
def test_minus_inf_logits_at_ignored_pixels_change_no_bit(shape, pattern):
    x, t = _inputs(shape, rc.INF_IGNORE)
    xi, ti, mask, _ = rc.inf_case(shape, pattern, ignored_only=True)
    assert np.array_equal(t, ti) and mask.any() and np.isneginf(xi).any()
    td, wd = dev(t), dev(rc.inf_weights(shape[1]))
    clean, masked = _bits(dev(x), td, wd, rc.INF_IGNORE, 2.0), _bits(dev(xi), td, wd, rc.INF_IGNORE, 2.0)
    for k in (0, 2, 3):                              # loss, state, gradient; lse is what it is at an ignored pixel
        assert torch.equal(clean[k], masked[k]), k
    assert torch.equal(clean[1][dev(~mask)], masked[1][dev(~mask)])


@pytest.mark.parametrize("shape", rc.INF_SHAPES)
@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_a_counted_pixel_with_a_non_finite_loss_is_never_dropped(shape, gamma):
    """DESIGN.md 3.18.  A target logit of -inf: +inf, as stock.  Every plane -inf: NaN, as stock.  A +inf plane: +inf if it is not
    the target's and NaN if it is, where stock returns NaN both times."""
    x, t = _inputs(shape, rc.INF_IGNORE)
    C, hw = shape[1], shape[2] * shape[3]
    wd, td = dev(rc.inf_weights(C)), dev(t)
    flat = t.reshape(-1)
    p = int(np.flatnonzero((flat != rc.INF_IGNORE) & (flat != 1) & (flat != 0))[7])        # counted, weight not 0
    cls = int(flat[p])
    other = 0 if cls != 0 else 2

    def run(planes, value):
        xn = x.copy()
        for c in planes:
            xn[p // hw, c].reshape(-1)[p % hw] = value
        xd = dev(xn)
        return ca.seg_cross_entropy(xd, td, wd, rc.INF_IGNORE, gamma), _stock(xd, td, wd, rc.INF_IGNORE, gamma)

    def kind(v):
        return "nan" if bool(torch.isnan(v)) else "+inf" if bool(torch.isposinf(v)) else "-inf" if bool(torch.isneginf(v)) else "finite"

    v, vs = run([cls], -np.inf)                      # the target switched off: against the stock result of this very call
    assert kind(v) == kind(vs) != "finite", (kind(v), kind(vs))
    v, vs = run(range(C), -np.inf)
    assert kind(v) == kind(vs) == "nan"
    v, vs = run([other], np.inf)
    assert kind(v) == "+inf" and kind(vs) == "nan"
    v, vs = run([other, C - 1 if cls != C - 1 else C - 2], np.inf)
    assert kind(v) == "+inf" and kind(vs) == "nan"
    v, vs = run([cls], np.inf)
    assert kind(v) == "nan" and kind(vs) == "nan"
    clean, clean_s = run([], 0.0)
    assert kind(clean) == kind(clean_s) == "finite"
