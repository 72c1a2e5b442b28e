"""flow_warp backward for reflection padding and nearest sampling (every pad x mode pair is differentiable, as with
grid_sample): every route of the backward against torch CPU autograd (oracle.flow_warp_grads_ref)."""
import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
from cerberusnet_amd import _lib
from cerberusnet_amd.synth import hash_uniform
from conftest import rel_err
import oracle

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"
PAD = {"zeros": 0, "border": 1, "reflection": 2}
MODE = {"bilinear": 0, "nearest": 1}
# the combinations that had no backward before: reflection x both modes, nearest x the two other pads
NEW = [("reflection", "bilinear"), ("reflection", "nearest"), ("border", "nearest"), ("zeros", "nearest")]
SHAPES = [(1, 1, 2, 2), (2, 3, 7, 9), (1, 16, 12, 20), (2, 5, 33, 65), (1, 130, 9, 17), (3, 32, 64, 128)]


def oracle_grads(img, flo, go, pad, mode):
    _, gi, gf = oracle.flow_warp_grads_ref(torch.as_tensor(img), torch.as_tensor(flo), torch.as_tensor(go), pad, mode)
    return gi.numpy(), gf.numpy()


def with_option(key, value, fn):
    _lib.set_option(key, value)
    try:
        return fn()
    finally:
        _lib.set_option(key, 0)


def backward(i, f, g, pad, mode, need_image=True, need_flow=True, ctx=True):
    """The raw ops: with the forward's context (flow_warp_ctx -> flow_warp_backward_ctx) or without it (the
    workspace path of flow_warp_backward)."""
    if ctx:
        _, c = torch.ops.cerberus.flow_warp_ctx(i, f, PAD[pad], MODE[mode])
        return torch.ops.cerberus.flow_warp_backward_ctx(i, f, c, g, PAD[pad], MODE[mode], need_image, need_flow)
    return torch.ops.cerberus.flow_warp_backward(i, f, g, PAD[pad], MODE[mode], need_image, need_flow)


def check_grads(gi, gf, rgi, rgf, mode, tol=TOL, gf_tol=None):
    if gi is not None:
        assert rel_err(gi.double().cpu().numpy(), rgi) < tol
    if gf is not None:
        if mode == "nearest":
            assert not rgf.any()
            assert not gf.view(torch.int16 if gf.element_size() == 2 else torch.int32 if gf.element_size() == 4
                               else torch.int64).any()   # +0.0 everywhere, as a bit pattern
        else:
            assert rel_err(gf.double().cpu().numpy(), rgf) < (gf_tol or tol)


@pytest.mark.parametrize("amp", ["small", "large"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pad,mode", NEW)
def test_parity_against_torch_cpu(pad, mode, shape, amp):
    """+-6 px, and +-3 max(H, W): several reflections and far-negative coordinates.  Through autograd (the public op)."""
    B, C, H, W = shape
    a = 6.0 if amp == "small" else 3.0 * max(H, W)
    img = hash_uniform(shape, 1)
    flo = hash_uniform((B, 2, H, W), 2, -a, a)
    go = hash_uniform(shape, 3)
    rgi, rgf = oracle_grads(img, flo, go, pad, mode)
    i = torch.from_numpy(img).to(DEV).requires_grad_(True)
    f = torch.from_numpy(flo).to(DEV).requires_grad_(True)
    out = ca.flow_warp(i, f, pad=pad, mode=mode)
    gi, gf = torch.autograd.grad(out, (i, f), torch.from_numpy(go).to(DEV))
    check_grads(gi, gf, rgi, rgf, mode)


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (2, 5, 33, 65), (3, 32, 64, 128)])
@pytest.mark.parametrize("pad,mode", NEW)
def test_every_route_of_the_backward(pad, mode, shape):
    """Both gradients / grad_image alone / grad_flow alone (C <= 4: the few-channel kernel; C > 4: the tile launch's
    flow role), with and without the forward's context, the per-pixel scatter kernel (warp_force_scatter), tile heights
    8 and 16: all against the oracle, and the deterministic routes agree with each other bit for bit."""
    B, C, H, W = shape
    img = hash_uniform(shape, 11)
    flo = hash_uniform((B, 2, H, W), 12, -2.0 * max(H, W), 2.0 * max(H, W))
    flo[:, :, : H // 2] /= 50.0   # half the map under a small flow: in-image taps as well as reflected ones
    go = hash_uniform(shape, 13)
    rgi, rgf = oracle_grads(img, flo, go, pad, mode)
    i, f, g = (torch.from_numpy(a).to(DEV) for a in (img, flo, go))
    gi, gf = backward(i, f, g, pad, mode)
    check_grads(gi, gf, rgi, rgf, mode)
    gi_n, gf_n = backward(i, f, g, pad, mode, ctx=False)
    assert torch.equal(gi_n, gi) and torch.equal(gf_n, gf)
    gi_a, _ = backward(i, f, g, pad, mode, need_flow=False)
    assert torch.equal(gi_a, gi)
    _, gf_a = backward(i, f, g, pad, mode, need_image=False)
    check_grads(None, gf_a, rgi, rgf, mode)
    if C > 4:
        assert torch.equal(gf_a, gf)
    _, gf_b = backward(i, f, g, pad, mode, need_image=False, ctx=False)
    assert torch.equal(gf_b, gf_a)
    for th in (8, 16):
        gi_t, gf_t = with_option("warp_tile_h", th, lambda: backward(i, f, g, pad, mode))
        check_grads(gi_t, gf_t, rgi, rgf, mode)
        assert torch.equal(gf_t, gf)
    gi_s, gf_s = with_option("warp_force_scatter", 1, lambda: backward(i, f, g, pad, mode))
    check_grads(gi_s, gf_s, rgi, rgf, mode)
    assert rel_err(gi_s.cpu().numpy(), gi.cpu().numpy()) < TOL


@pytest.mark.parametrize("pad,mode", NEW)
def test_fp64_and_half_dtypes(pad, mode):
    """fp64 (the per-pixel kernel with fp64 atomics) at 1e-12 / 1e-11; fp16 and bf16 against the fp64 oracle on the
    rounded inputs at the tolerances of test_warp_gpu.py::test_fp64_and_half_dtypes; an fp32 flow beside a 16-bit image."""
    shape = (1, 8, 20, 30)
    img = hash_uniform(shape, 9).astype(np.float64)
    flo = hash_uniform((1, 2, 20, 30), 10, -40.0, 40.0).astype(np.float64)
    go = hash_uniform(shape, 11).astype(np.float64)
    rgi, rgf = oracle_grads(img, flo, go, pad, mode)
    i, f, g = (torch.from_numpy(a).to(DEV) for a in (img, flo, go))
    gi, gf = backward(i, f, g, pad, mode)
    assert gi.dtype == torch.float64 and gf.dtype == torch.float64
    check_grads(gi, gf, rgi, rgf, mode, tol=1e-12, gf_tol=1e-11)
    for dt, tol in ((torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)):
        i16, f16, g16 = (torch.from_numpy(a).to(dt) for a in (img, flo, go))
        r16 = oracle_grads(i16.double(), f16.double(), g16.double(), pad, mode)
        gi, gf = backward(i16.to(DEV), f16.to(DEV), g16.to(DEV), pad, mode)
        assert gi.dtype == dt and gf.dtype == dt
        check_grads(gi, gf, *r16, mode, tol=tol)
        # an fp32 flow beside the 16-bit image: sampled at the flow's full precision
        f32 = torch.from_numpy(flo).float()
        r32 = oracle_grads(i16.double(), f32.double(), g16.double(), pad, mode)
        gi, gf = backward(i16.to(DEV), f32.to(DEV), g16.to(DEV), pad, mode)
        assert gi.dtype == dt and gf.dtype == torch.float32
        check_grads(gi, gf, *r32, mode, tol=tol)


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("cfg", ["config3_L3_fp32", "config5_L3_fp16"])
def test_full_size_levels_under_the_benched_smooth_flow(cfg, mode):
    from bench import Workload
    shape, dt, tol = {"config3_L3_fp32": ((4, 32, 128, 256), torch.float32, TOL),
                      "config5_L3_fp16": ((4, 32, 256, 512), torch.float16, 2e-3)}[cfg]
    B, C, H, W = shape
    img = torch.from_numpy(hash_uniform(shape, 51)).to(dt)
    go = torch.from_numpy(hash_uniform(shape, 53)).to(dt)
    flo = Workload._flow(B, H, W, 3, "smooth", "cpu").to(dt)
    rgi, rgf = oracle_grads(img.float(), flo.float(), go.float(), "reflection", mode)
    gi, gf = backward(img.to(DEV), flo.to(DEV), go.to(DEV), "reflection", mode)
    check_grads(gi, gf, rgi, rgf, mode, tol=tol)


@pytest.mark.parametrize("pad", ["zeros", "border", "reflection"])
def test_nearest_rounds_ties_to_even_as_aten_does(pad):
    """With W = 16, H = 8 a flow of (n + 1)(W - 1) / W - x puts the sample EXACTLY on n + 0.5 (every step of the
    reference's rounding sequence is exact there), and reflection keeps it on a half: the nearest tap is the even one.
    Half of the map sits on such ties, the other half under a random flow.  grad_image against the oracle, grad_flow all
    zero bits."""
    B, C, H, W = 2, 6, 8, 16
    img = hash_uniform((B, C, H, W), 61)
    go = hash_uniform((B, C, H, W), 63)
    n = np.rint(hash_uniform((B, 2, H, W), 62, -2.0 * W, 2.0 * W))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tie = np.stack([(n[:, 0] + 1) * (W - 1) / W - xs, (n[:, 1] + 1) * (H - 1) / H - ys], 1)
    flo = np.where(xs % 2 == 0, tie, hash_uniform((B, 2, H, W), 64, -2.0 * W, 2.0 * W)).astype(np.float32)
    v = (xs + flo[:, 0]).astype(np.float32)
    p = ((np.float32(2.0) * v / np.float32(W - 1) - np.float32(1.0)) + np.float32(1.0)) * W / 2 - np.float32(0.5)
    assert np.all((p - np.floor(p) == 0.5)[:, :, ::2])      # the ties are really there (exact arithmetic)
    rgi, rgf = oracle_grads(img, flo, go, pad, "nearest")
    i, f, g = (torch.from_numpy(a).to(DEV) for a in (img, flo, go))
    for ctx in (True, False):
        gi, gf = backward(i, f, g, pad, "nearest", ctx=ctx)
        check_grads(gi, gf, rgi, rgf, "nearest")
    gi, gf = with_option("warp_force_scatter", 1, lambda: backward(i, f, g, pad, "nearest"))
    check_grads(gi, gf, rgi, rgf, "nearest")


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (1, 12, 20, 36)])
def test_reflection_clip_kinks_at_zero_flow(shape):
    """With zero flow the first and last column reflect onto the edges and clip: grad_flow x is exactly 0 there, and
    grad_flow y in the first and last row -- as on torch CPU."""
    B, C, H, W = shape
    img = hash_uniform(shape, 71)
    go = hash_uniform(shape, 73)
    flo = np.zeros((B, 2, H, W), np.float32)
    rgi, rgf = oracle_grads(img, flo, go, "reflection", "bilinear")
    assert not rgf[:, 0, :, [0, -1]].any() and not rgf[:, 1, [0, -1], :].any()
    i, f, g = (torch.from_numpy(a).to(DEV) for a in (img, flo, go))
    for ctx in (True, False):
        gi, gf = backward(i, f, g, "reflection", "bilinear", ctx=ctx)
        check_grads(gi, gf, rgi, rgf, "bilinear")
        gf = gf.cpu()
        assert not gf[:, 0, :, [0, -1]].any() and not gf[:, 1, [0, -1], :].any()
        assert bool(gf[:, 0, :, 1:-1].ne(0).all())


@pytest.mark.parametrize("mag", [1e-20, 1.0, 3e18, 0.0])
@pytest.mark.parametrize("pad,mode", NEW)
def test_tiled_grad_image_fixed_point_is_scale_free_and_deterministic(pad, mode, mag):
    """test_warp_gpu.py's check for the new modes: independent of the gradient's magnitude, exactly linear in a
    power-of-two rescale, bit-reproducible run to run."""
    shape = (2, 9, 33, 70)
    img = hash_uniform(shape, 41)
    flo = hash_uniform((2, 2, 33, 70), 42, -7.0, 7.0)
    go = hash_uniform(shape, 43)
    rgi, _ = oracle_grads(img, flo, go, pad, mode)
    i, f = torch.from_numpy(img).to(DEV), torch.from_numpy(flo).to(DEV)
    g = torch.from_numpy(go).to(DEV) * mag
    a, _ = backward(i, f, g, pad, mode, need_flow=False, ctx=False)
    b, _ = backward(i, f, g, pad, mode, need_flow=False, ctx=False)
    assert torch.equal(a, b)
    if mag == 0.0:
        assert float(a.abs().max()) == 0.0
    else:
        assert rel_err(a.double().cpu().numpy() / mag, rgi) < TOL
    c, _ = backward(i, f, g * 8.0, pad, mode, need_flow=False, ctx=False)
    assert torch.equal(c, a * 8.0)


@pytest.mark.parametrize("pad,mode", NEW)
def test_nonfinite_grad_out_reaches_the_same_elements_as_the_oracle(pad, mode):
    shape = (2, 9, 40, 140)
    img = hash_uniform(shape, 81)
    flo = hash_uniform((2, 2, 40, 140), 82, -5.0, 5.0)
    go = hash_uniform(shape, 83)
    go[0, 1, 3, 3] = np.nan
    go[0, 5, 20, 77] = np.inf
    go[1, 8, 39, 139] = -np.inf
    go[1, 0, 17, 64] = np.nan
    rgi, rgf = oracle_grads(img, flo, go, pad, mode)
    i, f, g = (torch.from_numpy(a).to(DEV) for a in (img, flo, go))
    gi, gf = backward(i, f, g, pad, mode)
    gi, gf = gi.cpu().numpy(), gf.cpu().numpy()
    assert np.array_equal(np.isnan(gi), np.isnan(rgi))
    assert np.array_equal(np.isposinf(gi), np.isposinf(rgi))
    assert np.array_equal(np.isneginf(gi), np.isneginf(rgi))
    assert not np.isfinite(rgi).all()
    ok = np.isfinite(rgi)
    assert rel_err(np.where(ok, gi, 0), np.where(ok, rgi, 0)) < TOL
    assert np.array_equal(np.isfinite(gf), np.isfinite(rgf))
    if mode == "nearest":
        assert not gf.view(np.int32).any()
    else:
        okf = np.isfinite(rgf)
        assert rel_err(np.where(okf, gf, 0), np.where(okf, rgf, 0)) < TOL


def _gradcheck_inputs():
    img = torch.from_numpy(hash_uniform((1, 2, 5, 6), 201)).double()
    flo = torch.from_numpy(hash_uniform((1, 2, 5, 6), 202, -2.0, 2.0)).double()   # interior: no clip kink within eps
    return img, flo


def test_gradcheck_reflection_image_and_flow():
    img, flo = _gradcheck_inputs()
    ref = lambda i, f: oracle.flow_warp_ref(i, f, "reflection", "bilinear")   # noqa: E731
    assert torch.autograd.gradcheck(ref, (img.clone().requires_grad_(True), flo.clone().requires_grad_(True)))
    hip = lambda i, f: ca.flow_warp(i, f, pad="reflection", mode="bilinear")  # noqa: E731
    assert torch.autograd.gradcheck(hip, (img.to(DEV).requires_grad_(True), flo.to(DEV).requires_grad_(True)))


def test_gradcheck_nearest_image():
    img, flo = _gradcheck_inputs()
    for pad in ("reflection", "border", "zeros"):
        ref = lambda i: oracle.flow_warp_ref(i, flo, pad, "nearest")   # noqa: E731
        assert torch.autograd.gradcheck(ref, (img.clone().requires_grad_(True),))
        f = flo.to(DEV)
        hip = lambda i: ca.flow_warp(i, f, pad=pad, mode="nearest")   # noqa: E731
        assert torch.autograd.gradcheck(hip, (img.to(DEV).requires_grad_(True),))
