"""GPU tests of the census (ternary) term (csrc/census.hip): ``census_loss`` / ``cerberus::census_loss``.

Yardstick, as in test_photometric_gpu: the package's own stock-op formulation (``TernaryLoss(...).mean()``) evaluated in
float64 on the CPU.  Values: relative error <= 1e-5.  Gradients: ``l2_err`` and ``rel_err`` against float64, each at most
4 x the same error of the stock fp32 chain run on the GPU in the same test (the factor allows for another, equally valid
operation order and nothing more).  Every case asserts that its float64 gradient is not all zero."""
import functools

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import census_cases as cases
from cerberusnet_amd.loss_functions import UnFlowLoss as U
from cerberusnet_amd.loss_functions.UnFlowLoss import unFlowLoss
from cerberusnet_amd.synth import hash_uniform
from conftest import l2_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_TOL = 1e-5
GRAD_FACTOR = 4.0

SHAPES = [(2, 3, 32, 128),                        # whole 16 x 64 tiles
          (2, 3, 37, 53), (1, 3, 70, 40),         # ragged; one column of tiles
          (1, 3, 16, 200), (1, 3, 9, 64),         # one row of tiles
          (2, 3, 17, 65),                         # one row and one column beyond a tile
          (4, 3, 512, 1024), (4, 3, 256, 512), (4, 3, 128, 256), (4, 3, 64, 128)]   # the loss scales of the model step
DISTANCES = [1, 2, 3]
FAMILIES = cases.FAMILIES
_images = cases.images


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stock(im, im_warp, d):
    return ca.TernaryLoss(im, im_warp, d).mean()


@functools.lru_cache(maxsize=4)
def _f64(shape, family, d, both=False):
    """value and gradient(s) of the stock formulation in float64 on the CPU, one batch item at a time (the mean over the
    batch is the mean of the items' means; the K-plane intermediates of the full-size cases stay small)"""
    im, im_warp = _images(shape, family)
    B = shape[0]
    value, grads = 0.0, [[], []]
    for i in range(B):
        a = torch.from_numpy(im[i:i + 1]).double().requires_grad_(both)
        b = torch.from_numpy(im_warp[i:i + 1]).double().requires_grad_(True)
        v = _stock(a, b, d) / B
        for k, g in enumerate(torch.autograd.grad(v, (a, b) if both else (b,))):
            grads[k].append(g.numpy())
        value += v.item()
    return value, [np.concatenate(g) for g in grads if g]


def _check_grad(name, fused, stock, ref):
    assert float(np.abs(ref).max()) > 0, name            # a zero reference gradient would check nothing
    for metric in (l2_err, rel_err):
        ef, es = metric(fused, ref), metric(stock, ref)
        print("%s %s: fused %.3e stock fp32 %.3e" % (name, metric.__name__, ef, es))
        assert ef <= GRAD_FACTOR * es, (name, metric.__name__, ef, es)


def _value_and_gradient(shape, family, d):
    im, im_warp = _images(shape, family)
    ref_v, (ref_g,) = _f64(shape, family, d)
    a = dev(im)
    b = dev(im_warp).requires_grad_(True)
    v = ca.census_loss(a, b, d)
    assert v.shape == () and v.dtype == torch.float32
    g, = torch.autograd.grad(v, b)
    bs = dev(im_warp).requires_grad_(True)
    vs = _stock(a, bs, d)
    gs, = torch.autograd.grad(vs, bs)
    name = "census %s %s d=%d" % (shape, family, d)
    print("%s value: fused rel %.3e stock fp32 rel %.3e" % (name, abs(v.item() - ref_v) / abs(ref_v), abs(vs.item() - ref_v) / abs(ref_v)))
    assert ref_v > 0
    assert abs(v.item() - ref_v) <= VALUE_TOL * abs(ref_v)
    _check_grad(name, g.cpu().numpy(), gs.cpu().numpy(), ref_g)


@pytest.mark.parametrize("d", DISTANCES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_census_value_and_gradient_against_float64(shape, family, d):
    _value_and_gradient(shape, family, d)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d", DISTANCES)
def test_census_smallest_legal_map(d, family):
    """H = W = 2 d + 1: every pixel is masked except the centre one; and one such extent beside a larger one."""
    p = 2 * d + 1
    for shape in ((1, 3, p, p), (2, 3, p, 70), (2, 3, 21, p)):
        _value_and_gradient(shape, family, d)


@pytest.mark.parametrize("d", DISTANCES)
@pytest.mark.parametrize("family", FAMILIES)
def test_census_gradient_of_im(family, d):
    """An ``im`` that asks for a gradient gets one (the same kernel with the images' roles exchanged); the single-sided
    results are the bits of the two-sided ones."""
    shape = (2, 3, 37, 53)
    im, im_warp = _images(shape, family)
    _, ref = _f64(shape, family, d, True)
    a, b = dev(im).requires_grad_(True), dev(im_warp).requires_grad_(True)
    got = torch.autograd.grad(ca.census_loss(a, b, d), (a, b))
    as_, bs = dev(im).requires_grad_(True), dev(im_warp).requires_grad_(True)
    stock = torch.autograd.grad(_stock(as_, bs, d), (as_, bs))
    for name, x, y, z in zip(("d/d im", "d/d im_warp"), got, stock, ref):
        _check_grad("%s %s d=%d" % (name, family, d), x.cpu().numpy(), y.cpu().numpy(), z)
    a2 = dev(im).requires_grad_(True)                      # only im asks
    g2, = torch.autograd.grad(ca.census_loss(a2, dev(im_warp), d), a2)
    assert torch.equal(g2, got[0])
    b2 = dev(im_warp).requires_grad_(True)                 # only im_warp asks
    g3, = torch.autograd.grad(ca.census_loss(dev(im), b2, d), b2)
    assert torch.equal(g3, got[1])


@pytest.mark.parametrize("d", DISTANCES)
def test_census_edge_behaviour(d):
    shape = (2, 3, 37, 53)
    im, im_warp = _images(shape, "unit")
    # identical images: value exactly 0, gradient exactly 0
    a = dev(im)
    b = dev(im).requires_grad_(True)
    v = ca.census_loss(a, b, d)
    g, = torch.autograd.grad(v, b)
    assert float(v.detach()) == 0.0
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) == 0.0
    # a NaN in an interior pixel of either input: a NaN value, not a silently dropped pixel
    for which in (0, 1):
        pair = [dev(im), dev(im_warp)]
        pair[which][1, 2, 20, 30] = float("nan")
        assert bool(torch.isnan(ca.census_loss(pair[0], pair[1], d))), which
        assert bool(torch.isnan(_stock(pair[0], pair[1], d))), which
    # a NaN in a border or a corner pixel: every such pixel lies in the window of an interior one, so the stock
    # formulation gives NaN, and so does the op
    for y, x in ((0, 17), (36, 5), (9, 0), (0, 0), (36, 52)):
        for which in (0, 1):
            pair = [dev(im), dev(im_warp)]
            pair[which][0, 1, y, x] = float("nan")
            assert bool(torch.isnan(_stock(pair[0], pair[1], d))), (y, x, which)
            assert bool(torch.isnan(ca.census_loss(pair[0], pair[1], d))), (y, x, which)
    # exactly linear in the upstream gradient for powers of two
    grads = []
    for factor in (1.0, 4.0, 0.125):
        b = dev(im_warp).requires_grad_(True)
        g, = torch.autograd.grad(ca.census_loss(dev(im), b, d) * factor, b)
        grads.append(g)
    assert float(grads[0].abs().max()) > 0
    assert torch.equal(grads[1], grads[0] * 4.0) and torch.equal(grads[2], grads[0] * 0.125)


def test_two_runs_give_the_same_bits():
    for shape in ((2, 3, 37, 53), (4, 3, 512, 1024)):
        for d in DISTANCES:
            im, im_warp = (dev(a) for a in _images(shape, "smooth"))
            runs = []
            for _ in range(2):
                b = im_warp.clone().requires_grad_(True)
                v = ca.census_loss(im, b, d)
                runs.append((v.detach(), torch.autograd.grad(v, b)[0]))
            for x, y in zip(*runs):
                assert torch.equal(x, y)


def test_wrappers_take_the_stock_path_for_what_the_op_does_not_cover():
    shape = (1, 3, 16, 24)
    im, im_warp = (dev(a) for a in _images(shape, "unit"))
    op = torch.ops.cerberus.census_loss
    fused = ca.census_loss(im, im_warp, 1)
    assert torch.equal(fused, op(im, im_warp, 1))
    assert torch.equal(ca.census_loss(im, im_warp), fused)                     # max_distance defaults to 1
    v16 = ca.census_loss(im.half(), im_warp.half(), 1)                         # 16-bit: stock ops
    assert v16.dtype == torch.float16
    with pytest.raises(RuntimeError, match="float32"):
        op(im.half(), im_warp.half(), 1)
    im4, w4 = torch.cat([im, im[:, :1]], 1), torch.cat([im_warp, im_warp[:, :1]], 1)
    assert torch.equal(ca.census_loss(im4, w4, 1), ca.TernaryLoss(im4, w4, 1).mean())   # 4 channels: the first three, stock ops
    assert abs(float(ca.census_loss(im4, w4, 1)) - float(fused)) <= 1e-5 * float(fused)
    with pytest.raises(RuntimeError, match="3 channels"):
        op(im4, w4, 1)
    v4 = ca.census_loss(im, im_warp, 4)                                        # a 9 x 9 window: stock ops
    assert torch.equal(v4, ca.TernaryLoss(im, im_warp, 4).mean())
    with pytest.raises(RuntimeError, match="max_distance"):
        op(im, im_warp, 4)
    with pytest.raises(RuntimeError, match="max_distance"):
        op(im, im_warp, 0)
    cpu = ca.census_loss(im.cpu(), im_warp.cpu(), 1)                           # CPU tensors: stock ops
    assert cpu.device.type == "cpu" and abs(float(cpu) - float(fused)) <= 1e-5 * float(fused)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        op(im.cpu(), im_warp.cpu(), 1)
    small = ca.census_loss(im[..., :4, :], im_warp[..., :4, :], 2)             # H < 2 d + 1: the stock path (an all-zero map)
    assert float(small) == 0.0
    with pytest.raises(RuntimeError, match="at least 5 x 5"):
        op(im[..., :4, :], im_warp[..., :4, :], 2)
    with pytest.raises(RuntimeError, match="shapes differ"):
        op(im, im_warp[..., :-1], 1)
    # a non-contiguous view is made contiguous, not misread
    wide = torch.cat([im_warp, im_warp], 3)
    assert torch.equal(ca.census_loss(im, wide[..., :24], 1), fused)
    # no double backward
    b = im_warp.clone().requires_grad_(True)
    g, = torch.autograd.grad(ca.census_loss(im, b, 1), b, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        g.sum().backward()


def _flows(B, H, W, seed):
    coarse = torch.from_numpy(hash_uniform((B, 2, max(2, H // 8), max(2, W // 8)), seed, -6.0, 6.0))
    up = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    return (up + torch.from_numpy(hash_uniform((B, 2, H, W), seed + 1, -0.25, 0.25))).numpy()


@pytest.mark.parametrize("w", [0.5, 2.0])
def test_unflow_loss_fused_with_ternary_matches_float64(monkeypatch, w):
    """unFlowLoss(fused=True, weights with ternary) against the same loss with backend='torch' evaluated in float64 on the
    CPU, on the setup of test_unflow_loss_fused_matches_unfused with its bounds; and the fused route calls none of the stock
    formulations."""
    B, H, W = 2, 128, 256
    img1, img2 = hash_uniform((B, 3, H, W), 71, -2.0, 2.0), hash_uniform((B, 3, H, W), 72, -2.0, 2.0)
    sizes = [(H, W), (H // 4, W // 4), (H // 8, W // 8), (H // 16, W // 16), (H // 32, W // 32)]
    weights = {"l1": .15, "ssim": .85, "ternary": w}
    mk64 = lambda s: [torch.from_numpy(_flows(B, h, w_, s + i)).double().requires_grad_(True) for i, (h, w_) in enumerate(sizes)]
    fw, bw = mk64(80), mk64(90)
    ref = unFlowLoss(weights=weights, backend="torch")(
        {"flow": fw, "flow_b": bw}, {"l_img": torch.from_numpy(img1).double(), "l_seq": torch.from_numpy(img2).double()})
    ref_grads = [g.numpy() for g in torch.autograd.grad(ref, fw[:4] + bw[:4])]
    plain = unFlowLoss(backend="torch")(
        {"flow": fw, "flow_b": bw}, {"l_img": torch.from_numpy(img1).double(), "l_seq": torch.from_numpy(img2).double()})
    assert abs(ref.item() - plain.item()) > 1e-3 * abs(ref.item())            # the ternary term carries weight here

    def boom(*_a, **_k):
        raise AssertionError("the stock path was taken with fused=True")
    monkeypatch.setattr(U, "TernaryLoss", boom)
    monkeypatch.setattr(U, "_ssim_distance", boom)
    monkeypatch.setattr(U, "_edge_aware_smoothness", boom)
    mk = lambda s: [dev(_flows(B, h, w_, s + i)).requires_grad_(True) for i, (h, w_) in enumerate(sizes)]
    gfw, gbw = mk(80), mk(90)
    loss = unFlowLoss(fused=True, weights=weights)({"flow": gfw, "flow_b": gbw}, {"l_img": dev(img1), "l_seq": dev(img2)})
    grads = torch.autograd.grad(loss, gfw[:4] + gbw[:4])
    print("unFlowLoss ternary %g: fused %.9g float64 %.9g" % (w, float(loss.detach()), ref.item()))
    assert abs(float(loss.detach()) - ref.item()) <= 1e-5 * abs(ref.item())
    for a, b in zip(grads, ref_grads):
        print("flow gradient l2_err fused vs float64: %.3e" % l2_err(a.cpu().numpy(), b))
        assert l2_err(a.cpu().numpy(), b) < 5e-3


def test_unflow_loss_ternary_only_fused(monkeypatch):
    """weights={'ternary': w} alone: the fused route is the census op and nothing else of the photometric term."""
    im, im_warp = (dev(a) for a in _images((2, 3, 37, 53), "unit"))
    def boom(*_a, **_k):
        raise AssertionError("the stock path was taken with fused=True")
    monkeypatch.setattr(U, "TernaryLoss", boom)
    got = unFlowLoss(fused=True, weights={"ternary": 0.25}).loss_photometric(im, im_warp)
    assert torch.equal(got, 0.25 * torch.ops.cerberus.census_loss(im_warp, im, 1))


def test_census_loss_graphed_replay_is_bit_equal_to_eager():
    """Value + backward captured in ONE graph on a single stream (linear: no parallel branches), replayed on three
    different inputs with an eager call in between: the fixed-order reduction gives the eager bits every time."""
    shape = (2, 3, 128, 256)
    for d in (1, 3):
        s_im = torch.zeros(shape, device=DEV)
        s_warp = torch.zeros(shape, device=DEV, requires_grad=True)

        def step():
            v = ca.census_loss(s_im, s_warp, d)
            g, = torch.autograd.grad(v, s_warp)
            return v, g

        im0, warp0 = _images(shape, "unit", 300)
        with torch.no_grad():
            s_im.copy_(dev(im0))
            s_warp.copy_(dev(warp0))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g_v, g_g = step()
        for i, family in enumerate(("unit", "smooth", "noise")):
            im, im_warp = _images(shape, family, 310 + 10 * i)
            with torch.no_grad():
                s_im.copy_(dev(im))
                s_warp.copy_(dev(im_warp))
            graph.replay()
            torch.cuda.synchronize()
            b = dev(im_warp).requires_grad_(True)
            v = ca.census_loss(dev(im), b, d)          # the eager call in between
            g, = torch.autograd.grad(v, b)
            assert float(v) > 0
            assert torch.equal(g_v, v.detach()), (d, i, float(g_v), float(v))
            assert torch.equal(g_g, g), (d, i)
