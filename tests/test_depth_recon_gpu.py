"""GPU tests of the stereo reprojection warp (csrc/reproject.hip: ``cerberus::reproject_warp``) and of
``DepthReconstructionLossV1(backend='hip')``.

Yardstick: the package's own stock-op formulation (``depth_losses._reproject_stock`` / ``backend='torch'``) evaluated in
float64 on the CPU, with the constants of test_photometric_gpu.py: loss values within 1e-5 relative; the warped image and
grad_depth by ``l2_err`` against float64, at most 4 x the same error of the stock fp32 chain run on the GPU in the same test
(the factor allows for another, equally valid operation order and nothing more); ``rel_err`` with the same factor on the
smooth image family only (the max-norm is not stable through a warp: conftest.l2_err).

Cameras (synth.stereo_camera): the Cityscapes rig scaled to the width with an off-centre principal point and an x baseline,
and the same rig with a small rotation and a y / z translation.  Depth fields (synth.stereo_depth): 'near' -- stereo shifts
of 1-6 px; where the image is narrower than that (W = 2, 3) the same field scaled to 0.15-0.45 of (W - 1), because at 1-6 px
every sample of such an image is clipped, its gradient is identically zero and what is left of either fp32 chain is
rounding noise of a term that cancels analytically, which no factor brackets -- and 'border': shifts from half a pixel to
1.2 W, past the border for most pixels, where the clipped taps have zero gradient.  Every case beyond 3 x 3 holds pixels of
both kinds (asserted on the float64 reference), and no sample position lies on a tap boundary (``_depth``)."""
import functools

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
from cerberusnet_amd.loss_functions import UnFlowLoss as U
from cerberusnet_amd.loss_functions import depth_losses as D
from cerberusnet_amd.synth import hash_uniform, stereo_camera, stereo_depth
from conftest import l2_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_TOL = 1e-5
GRAD_FACTOR = 4.0
EPS = 1e-7

SHAPES = [(1, 3, 2, 2), (1, 1, 3, 3),               # the smallest the op accepts
          (2, 3, 37, 53),                           # ragged: part of one 64-pixel segment, two items
          (1, 1, 5, 64),                            # exactly one segment per row
          (1, 4, 16, 200),                          # four segments, the last one ragged; one full channel trip
          (2, 8, 32, 128),                          # two channel trips
          (1, 3, 70, 40),                           # more rows than columns
          (4, 3, 128, 256)]                         # the loss's own layout, many workgroups
RIGS = ["cityscapes", "rotated"]
FIELDS = ["near", "border"]
FAMILIES = ["noise", "smooth"]


def dev(a, device=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device or DEV)


def _smooth_field(shape, seed, lo=-2.0, hi=2.0):
    B, C, H, W = shape
    coarse = torch.from_numpy(hash_uniform((B, C, max(2, H // 8), max(2, W // 8)), seed, lo, hi))
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).numpy()


def _image(shape, family, seed):
    if family == "noise":
        return hash_uniform(shape, seed, -2.0, 2.0)
    return (_smooth_field(shape, seed) + hash_uniform(shape, seed + 1, -0.02, 0.02)).astype(np.float32)


TAP_MARGIN = 2.0 ** -10


def _sample_positions(depth, mats, H, W):
    """The un-normalised, unclipped sample positions (x, y) of the stock chain in float64, as numpy (B,H,W) each."""
    d = torch.from_numpy(depth).double()
    inv_K, K, T = (torch.from_numpy(m).double() for m in mats)
    grid = D.Project3D(d.shape[0], H, W, EPS)(D.BackprojectDepth(d.shape[0], H, W)(d, inv_K), K, T).numpy()
    return ((grid[..., 0] + 1) * W - 1) / 2, ((grid[..., 1] + 1) * H - 1) / 2


def _near_a_tap_boundary(depth, mats, H, W, rig):
    """Pixels whose x position -- under the rotated rig also the y position -- lies within TAP_MARGIN of an integer.  Under
    the Cityscapes rig the row coordinate does not depend on the depth (the middle row of an odd H sits exactly on an
    integer, by quirk Q2), and its kink multiplies a derivative that is zero."""
    near = lambda s, size: (np.abs(s - np.rint(s)) < TAP_MARGIN) & (s > -1) & (s < size)
    sx, sy = _sample_positions(depth, mats, H, W)
    return (near(sx, W) | (near(sy, H) if rig == "rotated" else False))[:, None]


def _depth(shape, rig, field, pred_type="depth", seed=700):
    """A prediction of the field family whose sample positions all keep TAP_MARGIN away from the integers.  At an
    integer position the bilinear sample has a kink and the border clip switches: grad_depth is discontinuous there, and
    which side an fp32 chain lands on is decided by the last bit of its position -- at 4 x 128 x 256 pixels a handful of
    positions of a random field lie within an fp32 ulp of an integer, each moves l2_err by 1 / sqrt(pixels) ~ 3e-3
    whichever chain it hits, and the bracket would compare two coin tosses.  The margin is 10 x the fp32 position error
    at W = 256 (a few ulp of 256: 1e-4)."""
    B, _, H, W = shape
    if field == "near":
        lo, hi = min(1.0, 0.15 * (W - 1)), min(6.0, 0.45 * (W - 1))
    else:
        lo, hi = min(0.5, 0.15 * (W - 1)), (1.2 if W > 3 else 0.6) * W
    mats = stereo_camera(B, H, W, rig)
    depth = stereo_depth(B, H, W, seed, lo, hi, "depth")
    to_pred = (lambda d: d) if pred_type == "depth" else \
        (lambda d: (1.0 + 256.0 * (0.209313 * 2262.52) / d.astype(np.float64)).astype(np.float32))
    to_depth = (lambda p: p) if pred_type == "depth" else \
        (lambda p: ca.DepthReconstructionLossV1.depth_from_disparity(torch.from_numpy(p).double()).numpy())
    for trial in range(32):
        pred = to_pred(depth)
        bad = _near_a_tap_boundary(np.asarray(to_depth(pred), np.float64), mats, H, W, rig)
        if not bad.any():
            return pred
        depth = np.where(bad, depth * np.float32(1 + (trial + 1) * 2.0 ** -7), depth).astype(np.float32)
    raise AssertionError("no tap-safe depth field for %s %s %s" % (shape, rig, field))


@functools.lru_cache(maxsize=None)
def _case(shape, rig, field, family):
    """Inputs (numpy fp32) and the float64 CPU reference of the warp and of grad_depth for a fixed grad_out."""
    B, C, H, W = shape
    image, depth, gout = _image(shape, family, 600), _depth(shape, rig, field), hash_uniform(shape, 610)
    mats = stereo_camera(B, H, W, rig)
    d64 = torch.from_numpy(depth).double().requires_grad_(True)
    w64 = D._reproject_stock(torch.from_numpy(image).double(), d64, *(torch.from_numpy(m).double() for m in mats), EPS)
    g64, = torch.autograd.grad(w64, d64, torch.from_numpy(gout).double())
    return image, depth, mats, gout, w64.detach().numpy(), g64.numpy()


def _bracket(name, fused, stock, ref, metrics):
    for metric in metrics:
        ef, es = metric(fused, ref), metric(stock, ref)
        print("%s %s: hip %.3e stock fp32 %.3e" % (name, metric.__name__, ef, es))
        assert ef <= GRAD_FACTOR * es, (name, metric.__name__, ef, es)


def _run(fn, image, depth, mats, gout, device=None):
    """(warped, grad_depth) of fn(image, depth, inv_K, K, T, eps) on the device, as numpy"""
    d = dev(depth, device).requires_grad_(True)
    w = fn(dev(image, device), d, *(dev(m, device) for m in mats), EPS)
    g, = torch.autograd.grad(w, d, dev(gout, device))
    return w.detach().cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("rig", RIGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_warp_and_grad_depth_against_float64(shape, rig, field, family, monkeypatch):
    image, depth, mats, gout, ref_w, ref_g = _case(shape, rig, field, family)
    # the case itself: the gradient is signal (the stereo term is ~ shift / depth per unit of image slope and gradOutput;
    # what is left where x is clipped is 1e-6 of that under the Cityscapes rig), and pixels with and without it are
    # present.  At 2 x 2 the border field clips every pixel in x and y: both chains must give exact zeros.
    signal = np.abs(ref_g * depth) > 1e-3
    assert (signal.any() and (rig == "rotated" or not signal.all())) or (shape[3] == 2 and not ref_g.any()), float(signal.mean())
    sw, sg = _run(D._reproject_stock, image, depth, mats, gout)
    monkeypatch.setattr(D, "_reproject_stock", lambda *_a, **_k: pytest.fail("the stock path was taken"))
    hw, hg = _run(ca.reproject_warp, image, depth, mats, gout)
    assert hw.dtype == np.float32 and hw.shape == shape and hg.shape == (shape[0], 1) + shape[2:]
    metrics = (l2_err, rel_err) if family == "smooth" else (l2_err,)
    name = "%s %s %s %s" % (shape, rig, field, family)
    _bracket(name + " warped", hw, sw, ref_w, metrics)
    _bracket(name + " grad_depth", hg, sg, ref_g, metrics)


@pytest.mark.parametrize("rig", RIGS)
@pytest.mark.parametrize("shape", [(2, 3, 37, 53), (1, 4, 16, 200)])
def test_composition_with_flow_warp(shape, rig):
    """reproject_warp = flow_warp(image, positions - mesh, pad='border') with the positions of the stock chain: the two
    differ by no more than the bracket of the stock fp32 chain's own error against float64."""
    B, C, H, W = shape
    for field in FIELDS:
        image, depth, mats, gout, ref_w, _ = _case(shape, rig, field, "smooth")
        img, d = dev(image), dev(depth)
        inv_K, K, T = (dev(m) for m in mats)
        points = D.BackprojectDepth(B, H, W)(d, inv_K)
        cam = torch.matmul(torch.matmul(K, T)[:, :3, :], points)
        pos = (cam[:, :2] / (cam[:, 2:3] + EPS)).view(B, 2, H, W)
        comp = ca.flow_warp(img, pos - ca.mesh_grid(B, H, W, device=DEV).float(), pad="border").cpu().numpy()
        hip = ca.reproject_warp(img, d, inv_K, K, T, EPS).cpu().numpy()
        stock = D._reproject_stock(img, d, inv_K, K, T, EPS).cpu().numpy()
        es = l2_err(stock, ref_w)
        print("%s %s %s: hip vs composition %.3e, composition vs f64 %.3e, hip vs f64 %.3e, stock fp32 vs f64 %.3e" % (
            shape, rig, field, l2_err(hip, comp), l2_err(comp, ref_w), l2_err(hip, ref_w), es))
        assert l2_err(hip, comp) <= GRAD_FACTOR * es


def _targets(shape, rig, device, dtype):
    B, C, H, W = shape
    t = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)
    inv_K, K, T = stereo_camera(B, H, W, rig)
    return {"l_img": t(_image(shape, "smooth", 620)), "r_img": t(_image(shape, "smooth", 630)),
            "camera": {"inv_K": t(inv_K), "K": t(K), "baseline_T": t(T)}}


@pytest.mark.parametrize("ssim", [True, False])
@pytest.mark.parametrize("pred_type", ["depth", "disparity"])
@pytest.mark.parametrize("rig", RIGS)
@pytest.mark.parametrize("shape", [(2, 3, 37, 53), (4, 3, 128, 256)])
def test_module_value_and_gradient_against_float64(shape, rig, pred_type, ssim, monkeypatch):
    B, C, H, W = shape
    pred = _depth(shape, rig, "near", pred_type, 640)

    def run(backend, device, dtype):
        p = torch.from_numpy(pred).to(device=device, dtype=dtype).requires_grad_(True)
        fn = ca.DepthReconstructionLossV1(B, H, W, pred_type=pred_type, ssim=ssim, backend=backend)
        v = fn({"depth": p}, _targets(shape, rig, device, dtype))
        g, = torch.autograd.grad(v, p)
        return float(v.detach()), g.cpu().numpy()

    ref_v, ref_g = run("torch", "cpu", torch.float64)
    vs, gs = run("torch", DEV, torch.float32)
    for name in ("_reproject_stock",):
        monkeypatch.setattr(D, name, lambda *_a, **_k: pytest.fail("the stock warp was taken with backend='hip'"))
    monkeypatch.setattr(U, "_photometric_stock", lambda *_a, **_k: pytest.fail("the stock loss was taken with backend='hip'"))
    v, g = run("hip", DEV, torch.float32)
    name = "module %s %s %s ssim=%s" % (shape, rig, pred_type, ssim)
    print("%s value: hip rel %.3e stock fp32 rel %.3e" % (name, abs(v - ref_v) / abs(ref_v), abs(vs - ref_v) / abs(ref_v)))
    assert abs(v - ref_v) <= VALUE_TOL * abs(ref_v)
    _bracket(name + " grad", g, gs, ref_g, (l2_err, rel_err))


def test_two_eager_runs_and_a_graph_replay_give_the_same_bits():
    shape = (2, 3, 64, 200)
    B, C, H, W = shape
    mats = [dev(m) for m in stereo_camera(B, H, W, "rotated")]
    s_img = torch.zeros(shape, device=DEV)
    s_depth = torch.ones((B, 1, H, W), device=DEV, requires_grad=True)
    s_gout = torch.zeros(shape, device=DEV)

    def step(img, d, go):
        w = ca.reproject_warp(img, d, *mats, EPS)
        g, = torch.autograd.grad(w, d, go)
        return w.detach(), g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(s_img, s_depth, s_gout)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_w, g_g = step(s_img, s_depth, s_gout)
    for i, field in enumerate(FIELDS):
        image, depth, gout = dev(_image(shape, "noise", 650 + i)), dev(_depth(shape, "rotated", field, seed=660 + i)), dev(hash_uniform(shape, 670 + i))
        with torch.no_grad():
            s_img.copy_(image)
            s_depth.copy_(depth)
            s_gout.copy_(gout)
        graph.replay()
        torch.cuda.synchronize()
        runs = [step(image, depth.clone().requires_grad_(True), gout) for _ in range(2)]
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        assert torch.equal(g_w, runs[0][0]) and torch.equal(g_g, runs[0][1]), field
        assert float(runs[0][1].abs().sum()) > 0


def test_non_finite_depth_touches_its_own_pixels_only():
    """One NaN, one +Inf and one depth that makes p.z + eps exactly zero (-eps under the Cityscapes rig, whose ray has
    z = 1 and whose projection adds nothing to z): every other pixel of the output and of grad_depth keeps the bits of a
    clean run, and the device reports no error."""
    shape = (2, 3, 37, 53)
    B, C, H, W = shape
    image, depth, mats, gout, _, _ = _case(shape, "cityscapes", "near", "smooth")
    spots = [(0, 0, 5, 7), (1, 0, 36, 52), (1, 0, 18, 0)]
    bad = depth.copy()
    bad[spots[0]], bad[spots[1]], bad[spots[2]] = np.nan, np.inf, -np.float32(EPS)
    img, go = dev(image), dev(gout)
    m = [dev(a) for a in mats]
    outs = []
    for d_np in (depth, bad):
        d = dev(d_np).requires_grad_(True)
        w = ca.reproject_warp(img, d, *m, EPS)
        g, = torch.autograd.grad(w, d, go)
        torch.cuda.synchronize()
        outs.append((w.detach().cpu().numpy(), g.cpu().numpy()))
    keep = np.ones((B, 1, H, W), bool)
    for s in spots:
        keep[s] = False
    (w0, g0), (w1, g1) = outs
    assert np.isfinite(w0).all() and np.isfinite(g0).all()
    assert np.array_equal(w0[np.broadcast_to(keep, shape)], w1[np.broadcast_to(keep, shape)])
    assert np.array_equal(g0[keep], g1[keep])
    assert np.isnan(w1[0, :, 5, 7]).all()                       # the warp's NaN rule: a NaN position gives NaN there
    # the GPU still works and a fresh clean run gives the clean bits
    assert np.array_equal(ca.reproject_warp(img, dev(depth), *m, EPS).cpu().numpy(), w0)


def test_wrappers_fall_back_and_raw_ops_reject():
    shape = (1, 3, 16, 24)
    B, C, H, W = shape
    image, depth = dev(_image(shape, "smooth", 680)), dev(_depth(shape, "cityscapes", "near"))
    inv_K, K, T = (dev(m) for m in stereo_camera(B, H, W, "cityscapes"))
    ref = ca.reproject_warp(image, depth, inv_K, K, T)
    # 16-bit: stock ops
    w16 = ca.reproject_warp(image.half(), depth.half(), inv_K.half(), K.half(), T.half())
    assert w16.dtype == torch.float16 and bool(torch.isfinite(w16).all())
    # an image that asks for a gradient: stock ops, and it gets one
    img_g, d_g = image.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    w = ca.reproject_warp(img_g, d_g, inv_K, K, T)
    gi, gd = torch.autograd.grad(w.sum(), (img_g, d_g))
    assert float(gi.abs().sum()) > 0 and float(gd.abs().sum()) > 0
    assert l2_err(w.detach().cpu().numpy(), ref.cpu().numpy()) < 1e-5
    # the module: same rule
    fn = ca.DepthReconstructionLossV1(B, H, W, pred_type="depth")
    targets = {"l_img": img_g, "r_img": image, "camera": {"inv_K": inv_K, "K": K, "baseline_T": T}}
    gi, = torch.autograd.grad(fn({"depth": depth}, targets), img_g)
    assert float(gi.abs().sum()) > 0
    # the raw ops
    k3, proj = inv_K[:, :3, :3].contiguous(), torch.matmul(K, T)[:, :3, :].contiguous()
    op, op_b = torch.ops.cerberus.reproject_warp, torch.ops.cerberus.reproject_warp_backward
    assert torch.equal(op(image, depth, k3, proj, 1e-7), ref)
    with pytest.raises(RuntimeError, match="gradient for the depth only"):
        torch.autograd.grad(op(img_g, d_g, k3, proj, 1e-7).sum(), (img_g, d_g))
    with pytest.raises(RuntimeError, match="float32"):
        op(image.half(), depth.half(), k3.half(), proj.half(), 1e-7)
    with pytest.raises(RuntimeError, match="float32"):
        op(image, depth.double(), k3, proj, 1e-7)
    with pytest.raises(RuntimeError, match="depth must be"):
        op(image, torch.cat([depth, depth], 1), k3, proj, 1e-7)
    with pytest.raises(RuntimeError, match="inv_K must be"):
        op(image, depth, inv_K, proj, 1e-7)
    with pytest.raises(RuntimeError, match="proj must be"):
        op(image, depth, k3, torch.matmul(K, T), 1e-7)
    with pytest.raises(RuntimeError, match="grad_out"):
        op_b(image, depth, k3, proj, image[:, :2], 1e-7)
    with pytest.raises(RuntimeError, match="at least 2"):
        op(image[:, :, :1], depth[:, :, :1], k3, proj, 1e-7)
    with pytest.raises(RuntimeError, match="at least 2"):
        op_b(image[..., :1], depth[..., :1], k3, proj, image[..., :1], 1e-7)
    with pytest.raises(RuntimeError, match="different devices"):
        op(image, depth, k3.cpu(), proj, 1e-7)
