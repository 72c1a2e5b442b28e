"""GPU tests of the fused loss terms (csrc/photometric.hip): ``photometric_loss`` (L1 + SSIM) and ``edge_smoothness``.

Yardstick for values and gradients: the package's own stock-op formulation (``unFlowLoss(backend='torch')``'s
``loss_photometric`` / ``_edge_aware_smoothness``) evaluated in float64 on the CPU.  Values: relative error <= 1e-5 (the
figure of the hip-vs-torch loss agreement in test_loss_side_gpu).  Gradients: ``l2_err`` and ``rel_err`` against float64,
each at most 4 x the same error of the stock fp32 chain run on the GPU in the same test (the factor allows for another,
equally valid operation order and nothing more).

The tests at the end of the file hold the same ops, and unFlowLoss away from its default keywords, to results of the
reference's own code (tests/golden/photometric.npz)."""
import functools

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import photometric_cases as pc
from cerberusnet_amd.loss_functions import UnFlowLoss as U
from cerberusnet_amd.loss_functions.UnFlowLoss import unFlowLoss
from cerberusnet_amd.synth import hash_uniform
from conftest import l2_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_TOL = 1e-5
GRAD_FACTOR = 4.0

SHAPES = [(2, 3, 32, 128),                        # whole 16 x 64 tiles
          (2, 3, 37, 53), (1, 2, 70, 40),         # ragged; one column of tiles
          (1, 1, 2, 2), (1, 1, 3, 3),             # the smallest ReflectionPad2d(1) accepts
          (1, 3, 16, 200), (1, 1, 5, 64),         # one row of tiles
          (2, 1, 64, 128),
          (4, 3, 512, 1024), (4, 3, 256, 512), (4, 3, 128, 256), (4, 3, 64, 128)]   # the loss scales of the model step
WEIGHTS = [(0.15, 0.85), (1.0, 0.0), (0.0, 1.0)]
FAMILIES = ["noise", "smooth"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _smooth_field(shape, seed, lo=-2.0, hi=2.0):
    B, C, H, W = shape
    coarse = torch.from_numpy(hash_uniform((B, C, max(2, H // 8), max(2, W // 8)), seed, lo, hi))
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).numpy()


def _images(shape, family, seed=100):
    """noise: two independent uniform fields in [-2, 2); smooth: a smooth field + small noise against a copy shifted by
    one column with noise of its own (what a warped image is to its target)."""
    B, C, H, W = shape
    if family == "noise":
        return hash_uniform(shape, seed, -2.0, 2.0), hash_uniform(shape, seed + 1, -2.0, 2.0)
    field = _smooth_field((B, C, H, W + 1), seed)
    orig = field[..., :-1] + hash_uniform(shape, seed + 2, -0.02, 0.02)
    recons = field[..., 1:] + hash_uniform(shape, seed + 3, -0.02, 0.02)
    return orig.astype(np.float32), recons.astype(np.float32)


def _stock_photometric(orig, recons, weights):
    l1, ssim = weights
    fn = unFlowLoss(backend="torch", weights={"l1": l1 or None, "ssim": ssim or None})
    return fn.loss_photometric(orig, recons)


@functools.lru_cache(maxsize=2)
def _photometric_f64(shape, family):
    """The two terms' means and gradients (w.r.t. im_recons) in float64 on the CPU; the loss is linear in them."""
    orig, recons = _images(shape, family)
    o = torch.from_numpy(orig).double()
    out = []
    for weights in ((1.0, 0.0), (0.0, 1.0)):
        r = torch.from_numpy(recons).double().requires_grad_(True)
        v = _stock_photometric(o, r, weights)
        g, = torch.autograd.grad(v, r)
        out.append((v.item(), g.numpy()))
    return out


def _photometric_ref(shape, family, weights):
    (v1, g1), (v2, g2) = _photometric_f64(shape, family)
    return weights[0] * v1 + weights[1] * v2, weights[0] * g1 + weights[1] * g2


def _check_grad(name, fused, stock, ref):
    for metric in (l2_err, rel_err):
        ef, es = metric(fused, ref), metric(stock, ref)
        print("%s %s: fused %.3e stock fp32 %.3e" % (name, metric.__name__, ef, es))
        assert ef <= GRAD_FACTOR * es, (name, metric.__name__, ef, es)


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_photometric_value_and_gradient_against_float64(shape, family, weights):
    orig, recons = _images(shape, family)
    ref_v, ref_g = _photometric_ref(shape, family, weights)
    o = dev(orig)
    r = dev(recons).requires_grad_(True)
    v = ca.photometric_loss(o, r, *weights)
    assert v.shape == () and v.dtype == torch.float32
    g, = torch.autograd.grad(v, r)
    rs = dev(recons).requires_grad_(True)
    vs = _stock_photometric(o, rs, weights)
    gs, = torch.autograd.grad(vs, rs)
    name = "photometric %s %s %s" % (shape, family, weights)
    print("%s value: fused rel %.3e stock fp32 rel %.3e" % (name, abs(v.item() - ref_v) / abs(ref_v), abs(vs.item() - ref_v) / abs(ref_v)))
    assert abs(v.item() - ref_v) <= VALUE_TOL * abs(ref_v)
    _check_grad(name, g.cpu().numpy(), gs.cpu().numpy(), ref_g)


@pytest.mark.parametrize("family", FAMILIES)
def test_photometric_gradient_of_im_orig(family):
    """An im_orig that asks for a gradient gets one (the same kernel with the images' roles exchanged), never None / zeros."""
    shape = (2, 3, 37, 53)
    orig, recons = _images(shape, family)
    o64, r64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (orig, recons))
    ref = torch.autograd.grad(_stock_photometric(o64, r64, (0.15, 0.85)), (o64, r64))
    o, r = dev(orig).requires_grad_(True), dev(recons).requires_grad_(True)
    got = torch.autograd.grad(ca.photometric_loss(o, r, 0.15, 0.85), (o, r))
    os_, rs = dev(orig).requires_grad_(True), dev(recons).requires_grad_(True)
    stock = torch.autograd.grad(_stock_photometric(os_, rs, (0.15, 0.85)), (os_, rs))
    for name, a, b, c in zip(("d/d im_orig", "d/d im_recons"), got, stock, ref):
        _check_grad("%s %s" % (name, family), a.cpu().numpy(), b.cpu().numpy(), c.numpy())
    # only im_orig asks
    o2 = dev(orig).requires_grad_(True)
    g2, = torch.autograd.grad(ca.photometric_loss(o2, dev(recons), 0.15, 0.85), o2)
    assert torch.equal(g2, got[0])


def _flow(shape, family, seed):
    B, C, H, W = shape
    if family == "noise":
        return hash_uniform(shape, seed, -6.0, 6.0)
    return (_smooth_field(shape, seed, -6.0, 6.0) + hash_uniform(shape, seed + 1, -0.25, 0.25)).astype(np.float32)


@pytest.mark.parametrize("alpha", [0.2, 10.0])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("degree,hw", [(1, (2, 2)), (1, (2, 9)), (1, (37, 53)), (1, (64, 128)), (1, (512, 1024)),
                                       (2, (3, 3)), (2, (3, 40)), (2, (21, 3)), (2, (37, 53)), (2, (64, 128)), (2, (130, 70)),
                                       (2, (512, 1024))])
def test_smoothness_value_and_gradient_against_float64(degree, hw, family, alpha):
    B = 4 if hw == (512, 1024) else 2
    flow = _flow((B, 2) + hw, family, 200)
    image = hash_uniform((B, 3) + hw, 210, -2.0, 2.0) if family == "noise" else \
        (_smooth_field((B, 3) + hw, 211) + hash_uniform((B, 3) + hw, 212, -0.02, 0.02)).astype(np.float32)
    f64 = torch.from_numpy(flow).double().requires_grad_(True)
    ref_v = U._edge_aware_smoothness(f64, torch.from_numpy(image).double(), alpha, degree)
    ref_g, = torch.autograd.grad(ref_v, f64)
    ref_v = ref_v.item()
    img = dev(image)
    f = dev(flow).requires_grad_(True)
    v = ca.edge_smoothness(f, img, alpha, degree)
    assert v.shape == () and v.dtype == torch.float32
    g, = torch.autograd.grad(v, f)
    fs = dev(flow).requires_grad_(True)
    vs = U._edge_aware_smoothness(fs, img, alpha, degree)
    gs, = torch.autograd.grad(vs, fs)
    name = "smoothness degree %d %s %s alpha %g" % (degree, hw, family, alpha)
    print("%s value: fused rel %.3e stock fp32 rel %.3e" % (name, abs(v.item() - ref_v) / abs(ref_v), abs(vs.item() - ref_v) / abs(ref_v)))
    assert abs(v.item() - ref_v) <= VALUE_TOL * abs(ref_v)
    _check_grad(name, g.cpu().numpy(), gs.cpu().numpy(), ref_g.numpy())


def test_smoothness_of_more_flow_and_image_channels():
    flow, image = _flow((2, 3, 19, 70), "noise", 220), hash_uniform((2, 1, 19, 70), 221, -2.0, 2.0)
    f64 = torch.from_numpy(flow).double().requires_grad_(True)
    ref_v = U._edge_aware_smoothness(f64, torch.from_numpy(image).double(), 0.2, 2)
    ref_g, = torch.autograd.grad(ref_v, f64)
    f = dev(flow).requires_grad_(True)
    v = ca.edge_smoothness(f, dev(image), 0.2, 2)
    g, = torch.autograd.grad(v, f)
    assert abs(v.item() - ref_v.item()) <= VALUE_TOL * abs(ref_v.item())
    assert l2_err(g.cpu().numpy(), ref_g.numpy()) < 1e-5


def test_wrappers_take_the_stock_path_for_what_the_ops_do_not_cover():
    shape = (1, 3, 16, 24)
    orig, recons = (dev(a) for a in _images(shape, "noise"))
    v16 = ca.photometric_loss(orig.half(), recons.half(), 0.15, 0.85)          # 16-bit: stock ops
    assert v16.dtype == torch.float16
    assert abs(float(v16) - float(ca.photometric_loss(orig, recons, 0.15, 0.85))) < 5e-3
    with pytest.raises(RuntimeError, match="float32"):
        torch.ops.cerberus.photometric_loss(orig.half(), recons.half(), 0.15, 0.85)
    flow = dev(_flow((1, 2, 16, 24), "noise", 230)).requires_grad_(True)
    img = orig.clone().requires_grad_(True)                                    # an image that asks for a gradient: stock ops
    gf, gi = torch.autograd.grad(ca.edge_smoothness(flow, img, 0.2, 2), (flow, img))
    assert gi is not None and float(gi.abs().sum()) > 0
    with pytest.raises(RuntimeError, match="no gradient for its image"):
        torch.autograd.grad(torch.ops.cerberus.edge_smoothness(flow, img, 0.2, 2), (flow, img))
    with pytest.raises(RuntimeError):
        torch.ops.cerberus.edge_smoothness(flow, orig, 0.2, 3)
    with pytest.raises(RuntimeError):
        torch.ops.cerberus.photometric_loss(orig[..., :1], recons[..., :1], 0.15, 0.85)   # W < 2


def test_photometric_edge_behaviour():
    shape = (2, 3, 37, 53)
    orig, _ = _images(shape, "smooth")
    # identical images: value 0 (or rounding of SSIM = 1), finite gradient
    o = dev(orig)
    r = dev(orig).requires_grad_(True)
    v = ca.photometric_loss(o, r, 0.15, 0.85)
    g, = torch.autograd.grad(v, r)
    assert 0.0 <= float(v) < 1e-6
    assert bool(torch.isfinite(g).all())
    # a NaN in one pixel of either input: a NaN value, not a silently dropped pixel
    for which in (0, 1):
        pair = [dev(orig), dev(_images(shape, "smooth")[1])]
        pair[which][1, 2, 20, 30] = float("nan")
        for weights in WEIGHTS:
            assert bool(torch.isnan(ca.photometric_loss(pair[0], pair[1], *weights))), (which, weights)
    # exactly linear in the upstream gradient for powers of two
    orig, recons = _images(shape, "noise")
    grads = []
    for factor in (1.0, 4.0, 0.125):
        r = dev(recons).requires_grad_(True)
        g, = torch.autograd.grad(ca.photometric_loss(dev(orig), r, 0.15, 0.85) * factor, r)
        grads.append(g)
    assert torch.equal(grads[1], grads[0] * 4.0) and torch.equal(grads[2], grads[0] * 0.125)
    f = dev(_flow((2, 2, 37, 53), "noise", 240))
    sg = []
    for factor in (1.0, 4.0):
        ff = f.clone().requires_grad_(True)
        g, = torch.autograd.grad(ca.edge_smoothness(ff, dev(orig), 0.2, 2) * factor, ff)
        sg.append(g)
    assert torch.equal(sg[1], sg[0] * 4.0)


def test_two_runs_give_the_same_bits():
    for shape in ((2, 3, 37, 53), (4, 3, 512, 1024)):
        orig, recons = (dev(a) for a in _images(shape, "noise"))
        flow = dev(_flow((shape[0], 2) + shape[2:], "smooth", 250))
        runs = []
        for _ in range(2):
            r = recons.clone().requires_grad_(True)
            f = flow.clone().requires_grad_(True)
            v = ca.photometric_loss(orig, r, 0.15, 0.85)
            s = ca.edge_smoothness(f, orig, 0.2, 2)
            runs.append((v.detach(), torch.autograd.grad(v, r)[0], s.detach(), torch.autograd.grad(s, f)[0]))
        for a, b in zip(*runs):
            assert torch.equal(a, b)


def _flows(B, H, W, seed):
    coarse = torch.from_numpy(hash_uniform((B, 2, max(2, H // 8), max(2, W // 8)), seed, -6.0, 6.0))
    up = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    return (up + torch.from_numpy(hash_uniform((B, 2, H, W), seed + 1, -0.25, 0.25))).numpy()


def test_unflow_loss_fused_matches_unfused(monkeypatch):
    """unFlowLoss(fused=True) against unFlowLoss(fused=False) on the setup of
    test_unflow_loss_uses_the_pyramid_and_matches_the_torch_backend (test_loss_side_gpu), same bounds; and with fused=True
    the stock formulations are not called at all."""
    B, H, W = 2, 128, 256
    img1, img2 = dev(hash_uniform((B, 3, H, W), 71, -2.0, 2.0)), dev(hash_uniform((B, 3, H, W), 72, -2.0, 2.0))
    sizes = [(H, W), (H // 4, W // 4), (H // 8, W // 8), (H // 16, W // 16), (H // 32, W // 32)]
    mk = lambda s: [dev(_flows(B, h, w, s + i)).requires_grad_(True) for i, (h, w) in enumerate(sizes)]
    res = []
    for fused in (True, False):
        if fused:
            def boom(*_a, **_k):
                raise AssertionError("the stock path was taken with fused=True")
            monkeypatch.setattr(U, "_ssim_distance", boom)
            monkeypatch.setattr(U, "_edge_aware_smoothness", boom)
        else:
            monkeypatch.undo()
        fw, bw = mk(80), mk(90)
        loss = unFlowLoss(fused=fused)({"flow": fw, "flow_b": bw}, {"l_img": img1, "l_seq": img2})
        grads = torch.autograd.grad(loss, fw[:4] + bw[:4])
        res.append((float(loss.detach()), [g.cpu().numpy() for g in grads]))
    print("unFlowLoss fused %.9g unfused %.9g" % (res[0][0], res[1][0]))
    assert abs(res[0][0] - res[1][0]) <= 1e-5 * abs(res[1][0])
    for a, b in zip(res[0][1], res[1][1]):
        print("flow gradient l2_err fused vs unfused: %.3e" % l2_err(a, b))
        assert l2_err(a, b) < 5e-3


def test_photometric_loss_graphed_replay_is_bit_equal_to_eager():
    """Value + backward captured in ONE graph on a single stream (linear: no parallel branches), replayed on three
    different inputs with an eager call in between: the fixed-order reductions give the eager bits every time."""
    shape = (2, 3, 128, 256)
    s_orig = torch.zeros(shape, device=DEV)
    s_recons = torch.zeros(shape, device=DEV, requires_grad=True)

    def step():
        v = ca.photometric_loss(s_orig, s_recons, 0.15, 0.85)
        g, = torch.autograd.grad(v, s_recons)
        return v, g

    orig0, recons0 = _images(shape, "noise", 300)
    with torch.no_grad():
        s_orig.copy_(dev(orig0))
        s_recons.copy_(dev(recons0))
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
    for i, family in enumerate(("noise", "smooth", "noise")):
        orig, recons = _images(shape, family, 310 + 10 * i)
        with torch.no_grad():
            s_orig.copy_(dev(orig))
            s_recons.copy_(dev(recons))
        graph.replay()
        torch.cuda.synchronize()
        r = dev(recons).requires_grad_(True)
        v = ca.photometric_loss(dev(orig), r, 0.15, 0.85)          # the eager call in between
        g, = torch.autograd.grad(v, r)
        assert torch.equal(g_v, v.detach()), (i, float(g_v), float(v))
        assert torch.equal(g_g, g), i


# ---- held to the reference itself: tests/golden/photometric.npz holds what the reference's own SSIM module,
# smooth_grad_1st / smooth_grad_2nd and unFlowLoss compute on the CPU in float32 and in float64 for the cases of
# tests/photometric_cases.py.  Values: within VALUE_TOL of the reference's float64 value.  Gradients: l2_err and rel_err
# against the reference's float64 gradient, each at most GRAD_FACTOR x the same error of the reference's float32 gradient
# (formed on the CPU; the tests above take the stock chain on the GPU, whose error is printed beside it: no case needs it
# as a second yardstick). ----------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def ref(golden):
    return golden("photometric")


def _bracket(name, fused, stock_gpu, ref32, ref64):
    for metric in (l2_err, rel_err):
        ef, ec, eg = metric(fused, ref64), metric(ref32, ref64), metric(stock_gpu, ref64)
        print("%s %s: fused %.3e reference float32 %.3e (ratio %.2f) stock fp32 on the GPU %.3e" % (
            name, metric.__name__, ef, ec, ef / ec if ec else float(ef > 0), eg))
        assert ef <= GRAD_FACTOR * ec, (name, metric.__name__, ef, ec, eg)


@pytest.mark.parametrize("weights", pc.WEIGHT_PAIRS)
@pytest.mark.parametrize("i", range(len(pc.PHOTO_CASES)))
def test_photometric_loss_against_the_reference_golden(ref, i, weights):
    shape, family = pc.PHOTO_CASES[i]
    orig, recons = pc.photo_images(i)
    want_v, want64 = pc.photo_reference(ref, i, "f64", *weights)
    _, want32 = pc.photo_reference(ref, i, "f32", *weights)
    for k, which in enumerate(("im_orig", "im_recons")):          # one call per image that asks for a gradient
        pair = [dev(orig), dev(recons)]
        pair[k].requires_grad_(True)
        v = ca.photometric_loss(pair[0], pair[1], *weights)
        g, = torch.autograd.grad(v, pair[k])
        spair = [dev(orig), dev(recons)]
        spair[k].requires_grad_(True)
        vs = U._photometric_stock(spair[0], spair[1], *weights)
        gs, = torch.autograd.grad(vs, spair[k])
        name = "reference photometric %d %s %s %s d/d %s" % (i, shape, family, weights, which)
        print("%s value: fused rel %.3e stock fp32 on the GPU rel %.3e" % (name, abs(v.item() - want_v) / abs(want_v),
                                                                          abs(vs.item() - want_v) / abs(want_v)))
        assert v.shape == () and v.dtype == torch.float32
        assert abs(v.item() - want_v) <= VALUE_TOL * abs(want_v)
        _bracket(name, g.cpu().numpy(), gs.cpu().numpy(), want32[k], want64[k])


@pytest.mark.parametrize("i", range(len(pc.SMOOTH_CASES)))
def test_edge_smoothness_against_the_reference_golden(ref, i):
    shape, channels, degree, alpha, family = pc.SMOOTH_CASES[i]
    flow, image = pc.smooth_inputs(i)
    want_v = float(ref["s%d_f64_value" % i])
    f = dev(flow).requires_grad_(True)
    v = ca.edge_smoothness(f, dev(image), alpha, degree)
    g, = torch.autograd.grad(v, f)
    fs = dev(flow).requires_grad_(True)
    vs = U._edge_aware_smoothness(fs, dev(image), alpha, degree)
    gs, = torch.autograd.grad(vs, fs)
    name = "reference smoothness %d %s degree %d alpha %g %s" % (i, shape, degree, alpha, family)
    print("%s value: fused rel %.3e stock fp32 on the GPU rel %.3e" % (name, abs(v.item() - want_v) / abs(want_v),
                                                                      abs(vs.item() - want_v) / abs(want_v)))
    assert v.shape == () and v.dtype == torch.float32
    assert abs(v.item() - want_v) <= VALUE_TOL * abs(want_v)
    _bracket(name, g.cpu().numpy(), gs.cpu().numpy(), ref["s%d_f32_grad_flow" % i], ref["s%d_f64_grad_flow" % i])
    # an image that asks for a gradient takes the stock path by design: held to the reference's gradients all the same
    f2, im2 = dev(flow).requires_grad_(True), dev(image).requires_grad_(True)
    v2 = ca.edge_smoothness(f2, im2, alpha, degree)
    gf2, gi2 = torch.autograd.grad(v2, (f2, im2))
    ei, ef = rel_err(gi2.cpu().numpy(), ref["s%d_f64_grad_image" % i]), rel_err(gf2.cpu().numpy(), ref["s%d_f64_grad_flow" % i])
    print("%s with an image gradient: value rel %.3e image gradient rel_err %.3e flow gradient rel_err %.3e" % (
        name, abs(v2.item() - want_v) / abs(want_v), ei, ef))
    assert abs(v2.item() - want_v) <= VALUE_TOL * abs(want_v)
    assert ei < 1e-5 and ef < 1e-5


@pytest.mark.parametrize("name,fused", [("a", True), ("a", False), ("b", True), ("b", False), ("c", True)])
def test_unflow_loss_keywords_against_the_reference_golden(ref, monkeypatch, name, fused):
    """unFlowLoss(backend='hip') away from the default keywords (tests/photometric_cases.py: consistency, weight, smooth,
    w_sm_scales, w_wrp_scales) against the reference's own float64 run; bounds of
    test_unflow_loss_with_occlusion_matches_float64: value 1e-5 relative, flow gradients l2_err < 5e-3.  (c) carries a
    ternary weight, which needs fused=True.  With fused=True no stock formulation runs."""
    l_img, l_seq, fw, bw = pc.loss_inputs()
    fw = [f.detach().to(DEV).requires_grad_(True) for f in fw]
    bw = [f.detach().to(DEV).requires_grad_(True) for f in bw]
    if fused:
        def boom(*_a, **_k):
            raise AssertionError("a stock formulation was taken with fused=True")
        for fn in ("_ssim_distance", "_edge_aware_smoothness", "TernaryLoss", "_photometric_stock"):
            monkeypatch.setattr(U, fn, boom)
    loss = unFlowLoss(fused=fused, **pc.LOSS_CONFIGS[name])({"flow": fw, "flow_b": bw}, {"l_img": l_img.to(DEV), "l_seq": l_seq.to(DEV)})
    grads = torch.autograd.grad(loss, fw + bw, allow_unused=True)
    want = float(ref["l%s_f64_value" % name])
    print("reference unFlowLoss %s fused=%s: GPU %.9g reference float64 %.12g (rel %.3e)" % (
        name, fused, float(loss.detach()), want, abs(float(loss.detach()) - want) / abs(want)))
    assert abs(float(loss.detach()) - want) <= 1e-5 * abs(want)
    used = pc.loss_used(name)
    for j, g in enumerate(grads):
        if j not in used:
            assert g is None, (name, j)
            continue
        err = l2_err(g.cpu().numpy(), ref["l%s_grad%d" % (name, j)])
        print("  flow %d gradient l2_err vs the reference's float64: %.3e" % (j, err))
        assert err < 5e-3
