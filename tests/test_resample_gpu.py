"""GPU tests of the resampling kernels (csrc/upsample.hip: ``cerberus::flow_upsample`` and its backward, ``area_resize``,
``area_pyramid``) on every kernel route, in fp32, fp16 and bf16.  The cases, the float64 references and the model that says
which route a case takes are in tests/resample_cases.py; tests/test_resample_cpu.py holds the case table to that model.

Yardsticks, and nothing else: (1) bit equality; (2) the bracket of test_depth_recon_gpu.py -- the error of the HIP op against
the float64 CPU reference is at most GRAD_FACTOR x the error of the stock fp32 chain (``F.interpolate(x * k, ...)`` and its
autograd backward, run on the GPU in the same test) against the same reference, with a floor of one fp32 unit roundoff for
the cases in which the stock chain is exact.  There is no fixed tolerance: at W >= 256 the fp32 source coordinate alone
carries ~6e-5 of weight error against float64, in both chains alike."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cerberusnet_amd as ca
from conftest import l2_err, rel_err
import resample_cases as rc
from resample_cases import AREA_CASES, CASES, MISALIGNED_CASES, case_id

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FACTOR = 4.0
FLOOR = 2.0 ** -24
HALVES = [torch.float16, torch.bfloat16]
STAGED_CASE, DIRECT_CASE = CASES[0], CASES[1]           # (2,2,9,256,4): oW == kUpMaxW; (1,2,5,257,4): one column wider

up = lambda x, k: torch.ops.cerberus.flow_upsample(x, k)
up_bwd = lambda g, k: torch.ops.cerberus.flow_upsample_backward(g, k)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _routes(case, aligned=True):
    B, C, H, W, k = case
    return "+".join(sorted(rc.bwd_routes(H, W, k, aligned, planes=B * C).routes))


def _bracket(name, hip, stock, ref):
    for metric in (rel_err, l2_err):
        eh, es = metric(hip, ref), metric(stock, ref)
        print("%s %s: hip %.3e stock fp32 %.3e" % (name, metric.__name__, eh, es))
        assert eh <= GRAD_FACTOR * max(es, FLOOR), (name, metric.__name__, eh, es)


def _offset_by_one_element(t):
    """The same values, contiguous, at an address one element past an allocation's start: not a multiple of 16 bytes, nor
    (16-bit) of 8 -- the alignment upsample_bwd_kernel and area_pyramid branch on.  ``.contiguous()`` in the bindings
    returns such a view itself."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + t.element_size()
    assert view.data_ptr() % (4 * t.element_size()) != 0 and t.data_ptr() % 16 == 0
    assert view.contiguous().data_ptr() == view.data_ptr()
    return view


# ---- a. fp32 against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fp32_forward_and_backward_against_float64(case, monkeypatch):
    k = case[4]
    x, go, ref_out, ref_gin = rc.reference(case)
    xs = dev(x).requires_grad_(True)
    s_out = rc.stock(xs, k)
    s_gin, = torch.autograd.grad(s_out, xs, dev(go))
    s_out, s_gin = s_out.detach().cpu().numpy(), s_gin.cpu().numpy()
    monkeypatch.setattr(F, "interpolate", lambda *_a, **_k: pytest.fail("the stock path was taken"))
    xd = dev(x).requires_grad_(True)
    out = up(xd, k)
    gin, = torch.autograd.grad(out, xd, dev(go))
    gin2 = up_bwd(dev(go), k)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == rc.out_shape(case) and tuple(gin.shape) == case[:4]
    assert _same_bits(gin, gin2)                        # deterministic: two backward runs, through autograd and direct
    name = "%s [%s]" % (case_id(case), _routes(case))
    _bracket(name + " forward", out.detach().cpu().numpy(), s_out, ref_out)
    _bracket(name + " backward", gin.cpu().numpy(), s_gin, ref_gin)


# ---- b. 16-bit: the same template, only ld / st differ ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALVES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_16_bit_forward_and_backward_are_the_fp32_kernels_rounded_once(case, dtype):
    """No tolerance: the 16-bit kernels convert their loads to the floats the fp32 kernels load (the staged copy too), do
    the same fp32 arithmetic in the same order and round to nearest even on the store, as ``.to()`` does.  The fp32 side is
    pinned to float64 by the test above."""
    k = case[4]
    x, go = (dev(a).to(dtype) for a in rc.inputs(case))
    out, gin = up(x, k), up_bwd(go, k)
    assert out.dtype == dtype and gin.dtype == dtype
    assert _same_bits(out, up(x.float(), k).to(dtype)), "forward " + _routes(case)
    assert _same_bits(gin, up_bwd(go.float(), k).to(dtype)), "backward " + _routes(case)


# ---- c. a gradient / source that is not aligned takes the scalar route and gives the same bits ---------------------------
@pytest.mark.parametrize("dtype", [torch.float32] + HALVES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("case", MISALIGNED_CASES, ids=case_id)
def test_a_misaligned_gradient_takes_the_direct_route_with_equal_bits(case, dtype):
    """Every load of the direct route and of the forward is a scalar ``ld`` (upsample.hip:57-58, :201, :214); the 16- and
    8-byte loads of the staged copy are behind the alignment test of upsample.hip:109."""
    k = case[4]
    x, go = (dev(a).to(dtype) for a in rc.inputs(case))
    assert _same_bits(up_bwd(_offset_by_one_element(go), k), up_bwd(go, k)), (_routes(case), _routes(case, False))
    assert _same_bits(up(_offset_by_one_element(x), k), up(x, k))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("shape,sizes", [((1, 2, 32, 64), [(16, 32), (8, 16)]), ((2, 1, 16, 40), [(8, 20), (4, 10)])])
def test_area_pyramid_of_a_misaligned_source_falls_back_scale_by_scale(shape, sizes, dtype):
    x = dev(rc.area_input(shape)).to(dtype)
    want = ca.area_pyramid(x, sizes)
    got = ca.area_pyramid(_offset_by_one_element(x), sizes)
    for g, w, size in zip(got, want, sizes):
        assert _same_bits(g, w), size
        assert _same_bits(g, ca.area_resize(x, size)), size


# ---- d. non-finite gradients stay where their taps are -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", [STAGED_CASE, DIRECT_CASE], ids=case_id)
def test_non_finite_gradient_reaches_its_support_only(case, dtype):
    B, C, H, W, k = case
    go = dev(rc.inputs(case)[1]).to(dtype)
    clean = up_bwd(go, k)
    assert bool(torch.isfinite(clean).all())
    spots = [(0, 1, 2 * k + 1, W * k - 3, float("nan")), (B - 1, 0, H * k - 1, 5 * k + 2, float("inf"))]
    bad = go.clone()
    keep = np.ones(case[:4], bool)
    of = rc.support(H, W, k)
    for b, c, oy, ox, v in spots:
        bad[b, c, oy, ox] = v
        for y, xx in of(oy, ox):
            keep[b, c, y, xx] = False
    assert 2 <= (~keep).sum() <= 8
    poisoned = up_bwd(bad, k)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(poisoned)[keep], _bits(clean)[keep]), _routes(case)
    assert not np.isfinite(poisoned.float().cpu().numpy()[~keep]).all()      # the poison did arrive somewhere
    assert _same_bits(up_bwd(go, k), clean)               # and a fresh clean run gives the clean bits


# ---- e. autograd wiring ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(1, 2, 7, 33, 3), (1, 2, 12, 20, 6), STAGED_CASE, (2, 3, 1, 9, 8)], ids=case_id)
def test_the_gradient_of_the_backward_is_the_forward(case):
    """The op is linear: the adjoint of its adjoint is the op (ops._upsample_bwd_backward)."""
    k = case[4]
    x, go = rc.inputs(case)
    g = dev(go).requires_grad_(True)
    v = dev(x)                                            # a cotangent of the backward's output has the input's shape
    gg, = torch.autograd.grad(up_bwd(g, k), g, v)
    assert _same_bits(gg, up(v, k))
    # and once more through both registrations: d/dx <up(x), go> = up_bwd(go), whose gradient w.r.t. go is up(v)
    xd = dev(x).requires_grad_(True)
    gin, = torch.autograd.grad(up(xd, k), xd, g, create_graph=True)
    gg2, = torch.autograd.grad(gin, g, v)
    assert _same_bits(gg2, gg)


def test_meta_implementations_give_the_shapes_and_dtypes_of_the_kernels():
    for case in CASES:
        k = case[4]
        for dtype in [torch.float32] + HALVES:
            x = torch.zeros(case[:4], dtype=dtype, device=DEV)
            out = up(x, k)
            m_out = up(x.to("meta"), k)
            assert (m_out.shape, m_out.dtype, m_out.device.type) == (out.shape, dtype, "meta"), case
            gin = up_bwd(out, k)
            m_gin = up_bwd(m_out, k)
            assert (m_gin.shape, m_gin.dtype) == (gin.shape, dtype) and gin.shape == x.shape, case


@pytest.mark.parametrize("case", [(3, 2, 17, 5, 5), STAGED_CASE], ids=case_id)
def test_a_broadcast_gradient_equals_its_materialised_copy(case):
    """``out.sum(0)``-style gradients arrive expanded, with batch stride 0."""
    B, C, H, W, k = case
    one = dev(rc.inputs(case)[1][:1])
    go = one.expand(B, C, H * k, W * k)
    assert go.stride(0) == 0 and not go.is_contiguous()
    assert _same_bits(up_bwd(go, k), up_bwd(go.clone(memory_format=torch.contiguous_format), k))
    x = dev(rc.inputs(case)[0]).requires_grad_(True)
    gin, = torch.autograd.grad(up(x, k).sum(0).mul(one[0]).sum(), x)
    assert _same_bits(gin, up_bwd(go, k))


# ---- g. area resizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,sizes", AREA_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_area_resize_from_more_sources_bit_for_bit(shape, sizes):
    """fp32: the bits of torch's CPU kernel (a fractional down-size, an integer down-size, an up-size; windows of fewer than
    a hundred elements, which ATen sums serially: test_resample_cpu.py).  16-bit: the fp32 kernel on the upcast input,
    rounded once."""
    x = rc.area_input(shape)
    for size in sizes:
        ref = F.interpolate(torch.from_numpy(x), size, mode="area")
        out = ca.area_resize(dev(x), size)
        assert _same_bits(out, ref), size
        for dtype in HALVES:
            x16 = dev(x).to(dtype)
            assert _same_bits(ca.area_resize(x16, size), ca.area_resize(x16.float(), size).to(dtype)), (size, dtype)


@pytest.mark.parametrize("dtype", HALVES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape,sizes", [((1, 2, 32, 64), [(16, 32), (8, 16)]),      # W / 2 a multiple of 4: four outputs per thread
                                         ((1, 2, 32, 40), [(16, 20), (8, 10)]),      # 20-wide rows, but 10-wide ones beside them
                                         ((1, 2, 32, 36), [(16, 18), (8, 9)])])      # W / 2 = 18: one output per thread
def test_area_pyramid_16_bit_half_scale_equals_area_resize(shape, sizes, dtype):
    x = dev(rc.area_input(shape)).to(dtype)
    outs = ca.area_pyramid(x, sizes)
    for o, size in zip(outs, sizes):
        assert o.dtype == dtype and _same_bits(o, ca.area_resize(x, size)), size
        assert _same_bits(o, ca.area_resize(x.float(), size).to(dtype)), size


# ---- f. graph capture (the name sorts these last: conftest._LAST) -----------------------------------------------------------
@pytest.mark.parametrize("case", [STAGED_CASE, DIRECT_CASE], ids=case_id)
def test_graphed_forward_and_backward_replay_the_eager_bits(case):
    k = case[4]
    s_x = torch.zeros(case[:4], device=DEV, requires_grad=True)
    s_go = torch.zeros(rc.out_shape(case), device=DEV)

    def step(x, go):
        out = up(x, k)
        g, = torch.autograd.grad(out, x, go)
        return out.detach(), g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(s_x, s_go)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_gin = step(s_x, s_go)
    x0, go0 = rc.inputs(case)
    for scale in (1.0, -0.5):
        x, go = dev(x0) * scale, dev(go0) * scale
        with torch.no_grad():
            s_x.copy_(x)
            s_go.copy_(go)
        graph.replay()
        torch.cuda.synchronize()
        runs = [step(x.clone().requires_grad_(True), go) for _ in range(2)]
        assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])
        assert _same_bits(g_out, runs[0][0]) and _same_bits(g_gin, runs[0][1]), scale
        assert float(runs[0][1].abs().sum()) > 0
