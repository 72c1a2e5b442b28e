"""CPU-side checks of the occlusion handling (csrc/occlusion.hip, loss_functions/UnFlowLoss.py): the three public functions
and the masked ``loss_photometric`` against results of the reference's own code (tests/golden/occlusion.npz, written by
tools/gen_golden_occlusion.py), the ``occlusion`` keyword of ``unFlowLoss``, op schemas, Meta shapes, loud CPU failure,
argument rejection in the C ABI before any launch and the workspace-size mirror."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import census_cases
import occlusion_cases as cases
from cerberusnet_amd import _lib
from cerberusnet_amd.loss_functions import UnFlowLoss as U
from cerberusnet_amd.loss_functions.UnFlowLoss import unFlowLoss
from conftest import rel_err

EINVAL, EDTYPE, EUNSUPPORTED, ETOOLARGE = -1, -2, -5, -6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "occlusion.npz")


def test_schemas_of_the_two_ops():
    s = lambda name: str(getattr(torch.ops.cerberus, name).default._schema)
    assert s("corresponding_map") == "cerberus::corresponding_map(Tensor data, bool is_flow) -> Tensor"
    assert s("occlusion_mask_bidirection") == ("cerberus::occlusion_mask_bidirection(Tensor flow12, Tensor flow21, float scale, "
                                               "float bias) -> Tensor")


def test_meta_shapes():
    a = torch.empty(2, 2, 37, 53, device="meta")
    for out in (torch.ops.cerberus.corresponding_map(a, True), torch.ops.cerberus.corresponding_map(a, False),
                torch.ops.cerberus.occlusion_mask_bidirection(a, a, 0.01, 0.5)):
        assert out.shape == (2, 1, 37, 53) and out.dtype == torch.float32


def test_cpu_tensors_fail_loudly():
    a = torch.rand(1, 2, 8, 8)
    for call in (lambda: torch.ops.cerberus.corresponding_map(a, True),
                 lambda: torch.ops.cerberus.corresponding_map(a.clone().requires_grad_(True), False),
                 lambda: torch.ops.cerberus.occlusion_mask_bidirection(a, a, 0.01, 0.5)):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


def test_argument_rejection_without_gpu():
    lib = _lib.get()
    one = ctypes.c_void_p(16)      # a non-null pointer that is never dereferenced: every call below is rejected first
    cm = lambda *a: lib.cerberus_corresponding_map(*a)
    bi = lambda *a: lib.cerberus_occlusion_mask_bidirection(*a)
    big = 1 << 40
    for dtype, want in ((9, EDTYPE), (-1, EDTYPE), (1, EUNSUPPORTED), (2, EUNSUPPORTED), (3, EUNSUPPORTED)):
        assert cm(one, one, one, big, 1, 8, 8, 1, dtype, None) == want
        assert bi(one, one, one, 1, 8, 8, 0.01, 0.5, dtype, None) == want
    for B, H, W in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8), (1, 8, -3)):
        assert cm(one, one, one, big, B, H, W, 1, 0, None) == EINVAL
        assert bi(one, one, one, B, H, W, 0.01, 0.5, 0, None) == EINVAL
    # what would let the fixed-point sum wrap, or floor(x) + 1 round: rejected, not computed
    for B, H, W in ((1, 1 << 15, 1 << 15), (1, 1, (1 << 24) + 1), (1, (1 << 24) + 1, 1), (1, 1 << 16, 1 << 16)):
        assert cm(one, one, one, big, B, H, W, 1, 0, None) == ETOOLARGE
        assert bi(one, one, one, B, H, W, 0.01, 0.5, 0, None) == ETOOLARGE
    for k in range(3):
        ptrs = [one] * 3
        ptrs[k] = None
        assert cm(*ptrs, big, 1, 8, 8, 1, 0, None) == EINVAL
        assert bi(*ptrs, 1, 8, 8, 0.01, 0.5, 0, None) == EINVAL
    for is_flow in (2, -1):
        assert cm(one, one, one, big, 1, 8, 8, is_flow, 0, None) == EINVAL
    assert cm(one, one, one, lib.cerberus_corresponding_map_workspace_bytes(2, 37, 53) - 1, 2, 37, 53, 1, 0, None) == EINVAL
    assert lib.cerberus_abi_version() == 7          # additions only


def test_workspace_size_equals_its_python_mirror():
    from cerberusnet_amd.ops import _corresponding_map_workspace_bytes
    lib = _lib.get()
    for shape in ((1, 1, 1), (2, 37, 53), (4, 512, 1024), (4, 64, 128), (1, 17, 65), (0, 8, 8), (2, 0, 8), (2, 8, 0), (-1, 8, 8),
                  (2, 8, -4), (2, -8, 4), (8, 2048, 4096)):
        assert _corresponding_map_workspace_bytes(*shape) == lib.cerberus_corresponding_map_workspace_bytes(*shape), shape
    assert lib.cerberus_corresponding_map_workspace_bytes(4, 512, 1024) == 4 * 512 * 1024 * 8


def _golden_cases():
    g = np.load(GOLDEN)
    assert int(g["n_cases"]) == len(cases.GOLDEN_CASES)
    for i, (shape, family, theta, scale, bias) in enumerate(cases.GOLDEN_CASES):
        assert tuple(g["c%d_shape" % i]) == shape and str(g["c%d_family" % i]) == family
        yield i, shape, family, theta, scale, bias, g


def test_the_three_functions_match_the_reference_golden():
    """Stock-op restatements of reference Python on fp32 CPU tensors: maps rel_err < 1e-6 (the bound of test_oracle.py and
    test_census_cpu.py), masks equal."""
    seen = set()
    for i, shape, family, theta, scale, bias, g in _golden_cases():
        B, H, W = shape
        f12, f21 = cases.golden_flows(i)
        coords = cases.mesh(B, H, W) + f21
        cmap = ca.get_corresponding_map(coords)
        want = g["c%d_map" % i]
        assert cmap.shape == (B, 1, H, W) and cmap.dtype == torch.float32
        err = rel_err(cmap.numpy(), want) if np.abs(want).max() > 0 else float(np.abs(cmap.numpy()).max())
        print("case %d %s %s: map rel_err %.3e, map max %.4g" % (i, shape, family, err, float(want.max())))
        assert err < 1e-6
        back = ca.get_occu_mask_backward(f21, theta=theta)
        bidir = ca.get_occu_mask_bidirection(f12, f21, scale=scale, bias=bias)
        for m, name in ((back, "backward"), (bidir, "bidirection")):
            assert m.shape == (B, 1, H, W) and m.dtype == torch.float32
            assert np.array_equal(m.numpy(), g["c%d_%s" % (i, name)]), (i, name)
        seen.add(family)
        if family == "outward":       # sources leave on every side: fewer than all of them are counted, some are
            assert 0 < float(cmap.sum()) < 0.7 * H * W
            gx, gy = coords[:, 0], coords[:, 1]
            assert bool((gx < -1).any() and (gx > W).any() and (gy < -1).any() and (gy > H).any())
        if family == "block":         # a whole block on one pixel
            assert float(cmap.max()) > 0.3 * (H // 4) * (W // 4)
    assert seen == {"independent", "consistent", "noisy", "outward", "block"}
    assert {(c[2], c[3], c[4]) for c in cases.GOLDEN_CASES} > {(0.2, 0.01, 0.5)}          # non-default parameters too
    assert min(min(c[0][1:]) for c in cases.GOLDEN_CASES) == 1
    # the defaults are the reference's
    f12, f21 = cases.golden_flows(0)
    assert torch.equal(ca.get_occu_mask_backward(f21), ca.get_occu_mask_backward(f21, theta=0.2))
    assert torch.equal(ca.get_occu_mask_bidirection(f12, f21), ca.get_occu_mask_bidirection(f12, f21, scale=0.01, bias=0.5))
    for name in ("get_corresponding_map", "get_occu_mask_backward", "get_occu_mask_bidirection"):
        assert name in U.__all__ and name in ca.__all__ and name in ca.loss_functions.__all__


def test_corresponding_map_is_differentiable_and_ignores_non_finite_targets():
    f21 = cases.flow_pair(1, 9, 11, "independent", 40)[1]
    coords = (cases.mesh(1, 9, 11) + f21).requires_grad_(True)
    cmap = ca.get_corresponding_map(coords)
    g, = torch.autograd.grad((cmap * torch.arange(99.).view(1, 1, 9, 11)).sum(), coords)
    assert float(g.abs().max()) > 0
    # NaN / +-Inf targets add nothing; the other pixels' contributions are those of the field with them sent far away
    bad, far = coords.detach().clone(), coords.detach().clone()
    for (y, x), v in (((0, 0), float("nan")), ((4, 5), float("inf")), ((8, 10), float("-inf"))):
        bad[0, 0, y, x] = v
        far[0, :, y, x] = 1e6
    assert torch.equal(ca.get_corresponding_map(bad), ca.get_corresponding_map(far))
    assert bool(torch.isfinite(ca.get_corresponding_map(bad)).all())
    # masks carry no gradient
    f = f21.clone().requires_grad_(True)
    assert not ca.get_occu_mask_backward(f).requires_grad and not ca.get_occu_mask_bidirection(f, f).requires_grad
    # 16-bit tensors: the stock formulation, mask in float32 as the reference's .float()
    assert ca.get_occu_mask_backward(f21.bfloat16()).dtype == torch.float32
    assert ca.get_corresponding_map(coords.detach().bfloat16()).dtype == torch.bfloat16


@pytest.mark.parametrize("w", range(len(cases.LOSS_WEIGHT_SETS)))
def test_masked_loss_photometric_matches_the_reference_golden(w):
    g = np.load(GOLDEN)
    a, b, masks = cases.photometric_inputs()
    mod = unFlowLoss(weights=dict(cases.LOSS_WEIGHT_SETS[w]), backend="torch")
    plain = mod.loss_photometric(a, b)
    got = {}
    for kind in cases.MASK_KINDS:
        want = float(g["p%d_%s" % (w, kind)])
        got[kind] = float(mod.loss_photometric(a, b, masks[kind]))
        print("weights %d mask %s: %.9g, reference %.9g" % (w, kind, got[kind], want))
        assert abs(got[kind] - want) <= 1e-6 * abs(want)
    # all ones = no mask; all zeros = the fallback to ones; a real mask changes the value
    assert abs(got["ones"] - float(plain)) <= 1e-6 * float(plain)
    assert abs(got["zeros"] - float(plain)) <= 1e-6 * float(plain)
    assert abs(got["random"] - float(plain)) > 1e-3 * float(plain)
    assert torch.equal(mod.loss_photometric(a, b, None), plain)


def _loss_io():
    l_img, l_seq, fw, bw = census_cases.loss_inputs()
    return {"flow": fw, "flow_b": bw}, {"l_img": l_img, "l_seq": l_seq}, fw, bw


def test_occlusion_keyword_of_unflowloss():
    pred, tgt, fw, bw = _loss_io()
    base = unFlowLoss(backend="torch")(pred, tgt)
    # default and explicit False: the bits of the loss as it was (the value asserted by the census golden's sibling test)
    off = unFlowLoss(backend="torch", occlusion=False)(pred, tgt)
    assert torch.equal(off, base) and unFlowLoss().occlusion is False
    on = unFlowLoss(backend="torch", occlusion=True)(pred, tgt)
    back = unFlowLoss(backend="torch", occlusion=True, back_occ_only=True)(pred, tgt)
    print("loss: plain %.9g, bidirectional masks %.9g, backward masks %.9g" % (base.item(), on.item(), back.item()))
    assert abs(on.item() - base.item()) > 1e-3 * base.item()
    assert abs(back.item() - base.item()) > 1e-3 * base.item()
    assert abs(back.item() - on.item()) > 1e-3 * base.item()
    # the schedule: masks from the first used scale's flows, argument order as upstream, nearest resize below
    f12, f21 = fw[0].detach(), bw[0].detach()
    m = unFlowLoss(backend="torch", occlusion=True).occlusion_masks(fw[0], bw[0])
    assert torch.equal(m[0], 1 - ca.get_occu_mask_bidirection(f12, f21)) and torch.equal(m[1], 1 - ca.get_occu_mask_bidirection(f21, f12))
    m = unFlowLoss(backend="torch", occlusion=True, back_occ_only=True).occlusion_masks(fw[0], bw[0])
    assert torch.equal(m[0], 1 - ca.get_occu_mask_backward(f21)) and torch.equal(m[1], 1 - ca.get_occu_mask_backward(f12))
    assert not m[0].requires_grad and 0 < float(m[0].mean()) < 1


def test_overriding_occlusion_masks_is_honoured_and_gradients_bypass_the_masks():
    pred, tgt, fw, bw = _loss_io()
    seen = []

    class Mine(unFlowLoss):
        def occlusion_masks(self, flow12, flow21):
            seen.append((tuple(flow12.shape), tuple(flow21.shape)))
            b, _, h, w = flow12.shape
            half = torch.zeros(b, 1, h, w)
            half[..., : w // 2] = 1
            return half, 1 - half

    mine = Mine(backend="torch", occlusion=True)(pred, tgt)
    assert seen == [(tuple(fw[0].shape), tuple(bw[0].shape))]           # once, at the first used scale
    on = unFlowLoss(backend="torch", occlusion=True)(pred, tgt)
    assert abs(mine.item() - on.item()) > 1e-4 * on.item()
    # all-ones masks through the seam: the unmasked loss
    class Ones(unFlowLoss):
        def occlusion_masks(self, flow12, flow21):
            return torch.ones_like(flow12[:, :1]), torch.ones_like(flow12[:, :1])
    plain = unFlowLoss(backend="torch")(pred, tgt)
    assert abs(Ones(backend="torch", occlusion=True)(pred, tgt).item() - plain.item()) <= 1e-6 * plain.item()
    # occlusion off: the seam is not called
    seen.clear()
    Mine(backend="torch")(pred, tgt)
    assert seen == []
    # gradients reach all eight used flows; masks are constants: the gradient equals the one with the same masks frozen
    grads = torch.autograd.grad(on, fw[:4] + bw[:4])
    assert all(float(x.abs().max()) > 0 for x in grads)
    frozen = unFlowLoss(backend="torch", occlusion=True)
    masks = tuple(t.clone() for t in frozen.occlusion_masks(fw[0], bw[0]))
    frozen.occlusion_masks = lambda a, b: masks
    grads2 = torch.autograd.grad(frozen(pred, tgt), fw[:4] + bw[:4])
    assert all(torch.equal(x, y) for x, y in zip(grads, grads2))
    # the unused fifth scale gets none
    assert torch.autograd.grad(unFlowLoss(backend="torch", occlusion=True)(pred, tgt), fw[4], allow_unused=True)[0] is None
