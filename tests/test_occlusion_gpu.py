"""GPU tests of the occlusion ops (csrc/occlusion.hip): ``cerberus::corresponding_map``, ``cerberus::occlusion_mask_bidirection``,
the public ``get_corresponding_map`` / ``get_occu_mask_backward`` / ``get_occu_mask_bidirection`` and ``unFlowLoss(occlusion=True)``.

Yardstick: the package's own stock-op formulations in float64 on the CPU.  Maps: max-abs error at most 4 x that of the
stock fp32 chain against the same float64 result (the factor of test_census_gpu.py, for its reason: another, equally valid
summation order and nothing more).  Masks: bracket tests -- a mask must be 1 where float64 says so by a margin, 0 where
float64 says so by a margin, the margin being 4 x the measured fp32 error of the stock chain; the pixels inside the margin
are the only undecided ones and may be at most 1 % of a case."""
import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import occlusion_cases as cases
from cerberusnet_amd.loss_functions import UnFlowLoss as U
from cerberusnet_amd.loss_functions.UnFlowLoss import unFlowLoss
from cerberusnet_amd.synth import hash_uniform
from conftest import l2_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0
UNDECIDED_CAP = 0.01

SHAPES = [(2, 37, 53), (1, 70, 40), (2, 17, 65),          # ragged
          (1, 16, 64),                                    # one tile
          (1, 1, 1), (1, 1, 7), (2, 3, 1),                # H or W of 1 .. 3
          (4, 512, 1024), (4, 256, 512), (4, 128, 256), (4, 64, 128)]      # the loss scales of the model step
MASK_SHAPES = [(2, 37, 53), (2, 128, 256), (4, 512, 1024), (4, 256, 512), (4, 128, 256), (4, 64, 128)]


def _map_field(shape, family):
    B, H, W = shape
    if family == "collapse":          # every source on one pixel pair: the accumulator's range
        return cases.collapse_flow(B, H, W, W // 2 + 0.25, H // 2 + 0.5 if H > 1 else 0.0)
    if family == "far":               # 1e6 px away, on every side
        sign = torch.from_numpy(np.where(hash_uniform((B, 2, H, W), 77, -1.0, 1.0) > 0, 1.0, -1.0).astype(np.float32))
        return sign * 1e6 + cases.noise(B, H, W, 78, 3.0)
    if family == "block":
        return cases.block_collapse_flow(B, H, W, 79)
    return cases.flow_pair(B, H, W, family, 900)[1]


def _map_errors(flow):
    """(float64 map, max-abs error of the stock fp32 chain against it), both on the CPU"""
    B, _, H, W = flow.shape
    mesh = cases.mesh(B, H, W)
    ref = U._corresponding_map_stock(mesh.double() + flow.double())
    stock = U._corresponding_map_stock(mesh + flow)
    return ref, float((stock.double() - ref).abs().max())


@pytest.mark.parametrize("family", ["independent", "noisy", "outward", "block", "collapse", "far"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_corresponding_map_against_float64(shape, family):
    B, H, W = shape
    flow = _map_field(shape, family)
    ref, stock_err = _map_errors(flow)
    got = torch.ops.cerberus.corresponding_map(flow.to(DEV), True)
    assert got.shape == (B, 1, H, W) and got.dtype == torch.float32
    err = float((got.cpu().double() - ref).abs().max())
    print("corresponding_map %s %s: map max %.6g, op err %.3e, stock fp32 err %.3e" % (shape, family, float(ref.max()), err, stock_err))
    assert err <= FACTOR * stock_err
    if family == "collapse":
        assert float(ref.max()) >= 0.25 * H * W        # one cell holds a fixed share of EVERY source
    if family == "far":
        assert float(ref.abs().max()) == 0 and float(got.abs().max()) == 0
    # absolute coordinates give the same bits as flow + the kernel's own mesh
    coords = (cases.mesh(B, H, W) + flow).to(DEV)
    assert torch.equal(torch.ops.cerberus.corresponding_map(coords, False), got)
    assert torch.equal(ca.get_corresponding_map(coords), got)


def _bidir_terms(f12, f21, scale, bias):
    """lhs, threshold of the stock formulation (U._occu_mask_bidirection_stock's steps) in the tensors' dtype"""
    b, _, h, w = f12.shape
    grid = U.norm_grid(U.mesh_grid(b, h, w).type_as(f12) + f12)
    warped = torch.nn.functional.grid_sample(f21, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    diff = f12 + warped
    mag = (f12 * f12).sum(1, keepdim=True) + (warped * warped).sum(1, keepdim=True)
    return (diff * diff).sum(1, keepdim=True), scale * mag + bias


def _bracket(name, mask, lo, hi):
    """lo <= mask <= hi everywhere; lo != hi on at most 1 % of the pixels; both values occur"""
    mask = mask.cpu().bool()
    undecided = float((lo != hi).double().mean())
    print("%s: undecided share %.4f %%, mask mean %.4f" % (name, 100 * undecided, float(mask.double().mean())))
    assert bool((mask | ~lo).all()), name + ": a pixel float64 sets by a margin is clear"
    assert bool((hi | ~mask).all()), name + ": a pixel float64 clears by a margin is set"
    assert undecided <= UNDECIDED_CAP, name
    assert bool(mask.any()) and not bool(mask.all()), name


@pytest.mark.parametrize("params", [(0.01, 0.5), (0.05, 0.25)], ids=["default", "other"])
@pytest.mark.parametrize("family", cases.FAMILIES)
@pytest.mark.parametrize("shape", MASK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bidirectional_mask_bracket(shape, family, params):
    B, H, W = shape
    scale, bias = params
    f12, f21 = cases.flow_pair(B, H, W, family, 900)
    lhs64, th64 = _bidir_terms(f12.double(), f21.double(), scale, bias)
    lhs32, th32 = _bidir_terms(f12, f21, scale, bias)
    e = float((((lhs32 - th32).double() - (lhs64 - th64)).abs() / th64).max())
    R = FACTOR * e
    got = torch.ops.cerberus.occlusion_mask_bidirection(f12.to(DEV), f21.to(DEV), scale, bias)
    assert got.shape == (B, 1, H, W) and got.dtype == torch.float32
    assert bool(((got == 0) | (got == 1)).all())
    name = "bidirection %s %s scale %g bias %g (e %.3e)" % (shape, family, scale, bias, e)
    _bracket(name, got, lhs64 > th64 * (1 + R), lhs64 > th64 * (1 - R))
    assert torch.equal(ca.get_occu_mask_bidirection(f12.to(DEV), f21.to(DEV), scale, bias), got)


@pytest.mark.parametrize("shape", [(2, 37, 53), (4, 128, 256)], ids=lambda s: "x".join(map(str, s)))
def test_bidirectional_mask_samples_what_flow_warp_returns(shape):
    """The op's sampled values are the bits of flow_warp(flow21, flow12, pad='zeros'): the stock elementwise chain on that
    warp, on the GPU, gives the same mask at every pixel."""
    B, H, W = shape
    for family in cases.FAMILIES:
        f12, f21 = (t.to(DEV) for t in cases.flow_pair(B, H, W, family, 940))
        warped = ca.flow_warp(f21, f12, pad="zeros")
        diff = f12 + warped
        mag = (f12 * f12).sum(1, keepdim=True) + (warped * warped).sum(1, keepdim=True)
        want = ((diff * diff).sum(1, keepdim=True) > 0.01 * mag + 0.5).float()
        got = ca.get_occu_mask_bidirection(f12, f21)
        print("bidirection vs chain on flow_warp %s %s: %d pixels differ" % (shape, family, int((got != want).sum())))
        assert torch.equal(got, want)


@pytest.mark.parametrize("theta", [0.2, 0.6])
@pytest.mark.parametrize("family", ["independent", "consistent", "noisy"])
@pytest.mark.parametrize("shape", MASK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_mask(shape, family, theta):
    B, H, W = shape
    flow = cases.flow_pair(B, H, W, family, 900)[1]
    got = ca.get_occu_mask_backward(flow.to(DEV), theta=theta)
    assert got.shape == (B, 1, H, W) and got.dtype == torch.float32
    # bit for bit the threshold of this package's own map of mesh + flow
    coords = (cases.mesh(B, H, W) + flow).to(DEV)
    assert torch.equal(got, (ca.get_corresponding_map(coords).clamp(0, 1) < theta).float())
    ref, stock_err = _map_errors(flow)
    band = FACTOR * stock_err
    ref = ref.clamp(0, 1)
    _bracket("backward %s %s theta %g (band %.3e)" % (shape, family, theta, band), got, ref < theta - band, ref < theta + band)


def test_both_ops_are_bit_reproducible_eager_and_graphed():
    """Two eager runs and a single-stream graph replay (linear: no parallel branches) give equal bits."""
    B, H, W = 2, 128, 256
    s12, s21 = torch.zeros(B, 2, H, W, device=DEV), torch.zeros(B, 2, H, W, device=DEV)

    def step():
        return (torch.ops.cerberus.corresponding_map(s21, True), torch.ops.cerberus.corresponding_map(s12, False),
                torch.ops.cerberus.occlusion_mask_bidirection(s12, s21, 0.01, 0.5), ca.get_occu_mask_backward(s21))

    f12, f21 = cases.flow_pair(B, H, W, "independent", 950)
    s12.copy_(f12.to(DEV))
    s21.copy_(f21.to(DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = step()
    for i, family in enumerate(("noisy", "consistent", "block")):
        if family == "block":
            f12, f21 = cases.flow_pair(B, H, W, "independent", 960)[0], cases.block_collapse_flow(B, H, W, 961)
        else:
            f12, f21 = cases.flow_pair(B, H, W, family, 960 + 10 * i)
        s12.copy_(f12.to(DEV))
        s21.copy_(f21.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        first, second = step(), step()
        assert float(first[0].max()) > 0
        for g, a, b in zip(g_out, first, second):
            assert torch.equal(a, b), (family, "eager vs eager")
            assert torch.equal(g, a), (family, "graph vs eager")


def test_non_finite_flows_add_nothing_and_disturb_nothing():
    B, H, W = 2, 37, 53
    f12, f21 = cases.flow_pair(B, H, W, "consistent", 970)
    bad, far = f21.clone(), f21.clone()
    spots = (((0, 0, 0, 0), float("nan")), ((0, 1, 20, 30), float("nan")), ((1, 0, 36, 52), float("inf")),
             ((1, 1, 5, 7), float("-inf")), ((0, 0, 17, 1), float("inf")))
    for (b, c, y, x), v in spots:
        bad[b, c, y, x] = v
        far[b, :, y, x] = 1e6
    got = torch.ops.cerberus.corresponding_map(bad.to(DEV), True)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, torch.ops.cerberus.corresponding_map(far.to(DEV), True))
    assert torch.equal(ca.get_occu_mask_backward(bad.to(DEV)), ca.get_occu_mask_backward(far.to(DEV)))
    # bidirectional: 0 where a term of the pixel is NaN (its own flow12; NaN * 0 is NaN, so also every pixel that samples a
    # non-finite flow21 value, even with weight 0); everything else as the clean field's mask
    clean = ca.get_occu_mask_bidirection(f12.to(DEV), f21.to(DEV))
    bad12 = f12.clone()
    for (b, c, y, x), v in spots:
        bad12[b, c, y, x] = float("nan")
    got = ca.get_occu_mask_bidirection(bad12.to(DEV), f21.to(DEV))
    touched = torch.zeros(B, 1, H, W, dtype=torch.bool)
    for (b, c, y, x), v in spots:
        touched[b, 0, y, x] = True
    assert float(got.cpu()[touched].abs().max()) == 0
    assert torch.equal(got.cpu()[~touched], clean.cpu()[~touched])
    lhs, th = _bidir_terms(f12, bad, 0.01, 0.5)
    got = ca.get_occu_mask_bidirection(f12.to(DEV), bad.to(DEV)).cpu()
    nan_terms = torch.isnan(lhs) | torch.isnan(th)
    assert bool(nan_terms.any()) and float(got[nan_terms].abs().max()) == 0
    assert bool(((got == 0) | (got == 1)).all())


def _loss_setup():
    B, H, W = 2, 128, 256
    img1, img2 = hash_uniform((B, 3, H, W), 71, 0.0, 1.0), hash_uniform((B, 3, H, W), 72, 0.0, 1.0)
    sizes = [(H, W), (H // 4, W // 4), (H // 8, W // 8), (H // 16, W // 16), (H // 32, W // 32)]
    pairs = [cases.flow_pair(B, h, w, "consistent", 980 + 10 * i) for i, (h, w) in enumerate(sizes)]
    return img1, img2, [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("back_occ_only", [False, True])
@pytest.mark.parametrize("fused", [True, False])
def test_unflow_loss_with_occlusion_matches_float64(monkeypatch, fused, back_occ_only):
    """unFlowLoss(occlusion=True) on the GPU against backend='torch' in float64 on the CPU with the float64 run's
    occlusion_masks patched to return the GPU run's masks (the masks are tested above; one flipped pixel must not decide
    this comparison).  Bounds of test_unflow_loss_fused_with_ternary_matches_float64: value 1e-5 relative, flow gradients
    l2_err < 5e-3.  With fused=True no stock formulation runs, of the terms or of the masks."""
    img1, img2, f12s, f21s = _loss_setup()
    weights = {"l1": .15, "ssim": .85, "ternary": 0.5} if fused else {"l1": .15, "ssim": .85}
    kept = []

    class Recording(unFlowLoss):
        def occlusion_masks(self, flow12, flow21):
            kept.append(super().occlusion_masks(flow12, flow21))
            return kept[-1]

    # the float64 side first (it uses the stock formulations of the terms), with masks filled in afterwards
    fw = [f.double().requires_grad_(True) for f in f12s]
    bw = [f.double().requires_grad_(True) for f in f21s]
    ref_mod = unFlowLoss(weights=weights, backend="torch", occlusion=True, back_occ_only=back_occ_only)
    ref_mod.occlusion_masks = lambda a, b: tuple(m.cpu().double() for m in kept[0])
    tgt64 = {"l_img": torch.from_numpy(img1).double(), "l_seq": torch.from_numpy(img2).double()}
    plain = unFlowLoss(weights=weights, backend="torch")({"flow": fw, "flow_b": bw}, tgt64).item()

    gfw = [f.to(DEV).requires_grad_(True) for f in f12s]
    gbw = [f.to(DEV).requires_grad_(True) for f in f21s]
    mod = Recording(weights=weights, fused=fused, occlusion=True, back_occ_only=back_occ_only)
    with monkeypatch.context() as mp:
        def boom(*_a, **_k):
            raise AssertionError("a stock formulation was taken")
        for name in ("_corresponding_map_stock", "_occu_mask_backward_stock", "_occu_mask_bidirection_stock"):
            mp.setattr(U, name, boom)
        if fused:
            for name in ("TernaryLoss", "_ssim_distance", "_edge_aware_smoothness"):
                mp.setattr(U, name, boom)
        loss = mod({"flow": gfw, "flow_b": gbw}, {"l_img": torch.from_numpy(img1).to(DEV), "l_seq": torch.from_numpy(img2).to(DEV)})
        grads = torch.autograd.grad(loss, gfw[:4] + gbw[:4])
    assert len(kept) == 1 and all(m.shape == (2, 1, 128, 256) and not m.requires_grad for m in kept[0])
    visible = [float(m.mean()) for m in kept[0]]
    assert all(0.02 < v < 0.98 for v in visible), visible

    ref = ref_mod({"flow": fw, "flow_b": bw}, tgt64)
    ref_grads = [g.numpy() for g in torch.autograd.grad(ref, fw[:4] + bw[:4])]
    print("unFlowLoss occlusion fused=%s back_occ_only=%s: GPU %.9g float64 %.9g (unmasked %.9g), visible %s" % (
        fused, back_occ_only, float(loss.detach()), ref.item(), plain, visible))
    assert abs(ref.item() - plain) > 1e-3 * abs(plain)                     # the masks carry weight here
    assert abs(float(loss.detach()) - ref.item()) <= 1e-5 * abs(ref.item())
    for a, b in zip(grads, ref_grads):
        print("flow gradient l2_err vs float64: %.3e" % l2_err(a.cpu().numpy(), b))
        assert float(np.abs(b).max()) > 0
        assert l2_err(a.cpu().numpy(), b) < 5e-3


def test_wrappers_fall_back_and_raw_ops_reject():
    B, H, W = 2, 24, 40
    f12, f21 = (t.to(DEV) for t in cases.flow_pair(B, H, W, "consistent", 990))
    coords = cases.mesh(B, H, W).to(DEV) + f21
    cmap = ca.get_corresponding_map(coords)
    # 16-bit: stock ops, in the tensor's dtype; masks float32
    for dt in (torch.float16, torch.bfloat16):
        assert ca.get_corresponding_map(coords.to(dt)).dtype == dt
        for m in (ca.get_occu_mask_backward(f21.to(dt)), ca.get_occu_mask_bidirection(f12.to(dt), f21.to(dt))):
            assert m.dtype == torch.float32 and m.shape == (B, 1, H, W) and m.is_cuda
        with pytest.raises(RuntimeError, match="float32"):
            torch.ops.cerberus.corresponding_map(coords.to(dt), False)
        with pytest.raises(RuntimeError, match="float32"):
            torch.ops.cerberus.occlusion_mask_bidirection(f12.to(dt), f21.to(dt), 0.01, 0.5)
    # CPU tensors: stock ops on the CPU; close to the op (another summation order)
    cpu = ca.get_corresponding_map(coords.cpu())
    assert not cpu.is_cuda and float((cpu - cmap.cpu()).abs().max()) < 1e-4
    assert not ca.get_occu_mask_bidirection(f12.cpu(), f21.cpu()).is_cuda
    # coordinates that require grad: the differentiable stock formulation, on the GPU
    c = coords.clone().requires_grad_(True)
    g, = torch.autograd.grad(ca.get_corresponding_map(c).square().sum(), c)
    assert g.is_cuda and float(g.abs().max()) > 0
    with pytest.raises(RuntimeError, match="not differentiable"):
        torch.ops.cerberus.corresponding_map(c, False).sum().backward()
    # non-contiguous views are made contiguous
    wide = torch.zeros(B, 2, H, W + 8, device=DEV)
    wide[..., :W] = coords
    assert torch.equal(ca.get_corresponding_map(wide[..., :W]), cmap)
    wide[..., :W] = f12
    wide21 = torch.zeros(B, 2, H, W + 8, device=DEV)
    wide21[..., :W] = f21
    assert torch.equal(ca.get_occu_mask_bidirection(wide[..., :W], wide21[..., :W]), ca.get_occu_mask_bidirection(f12, f21))
    # shapes the raw ops do not take
    for bad in (coords[:, :1], coords[0], torch.zeros(B, 3, H, W, device=DEV), torch.zeros(0, 2, H, W, device=DEV)):
        with pytest.raises(RuntimeError, match=r"\(B,2,H,W\)|no pixels"):
            torch.ops.cerberus.corresponding_map(bad, True)
    with pytest.raises(RuntimeError, match="shapes differ"):
        torch.ops.cerberus.occlusion_mask_bidirection(f12, f21[..., :-1], 0.01, 0.5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.corresponding_map(coords.cpu(), False)
