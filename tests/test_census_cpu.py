"""CPU-side checks of the census (ternary) term (csrc/census.hip): op schemas, Meta shapes, loud CPU failure, argument
rejection in the C ABI before any launch, the workspace-size mirror, the stock-op ``TernaryLoss`` and the whole
``unFlowLoss`` with a ternary weight against results of the reference's own code (tests/golden/census.npz, written by
tools/gen_golden_census.py), and the ``weights["ternary"]`` rules of ``unFlowLoss``."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import census_cases as cases
from cerberusnet_amd import _lib
from cerberusnet_amd.loss_functions import UnFlowLoss as U
from cerberusnet_amd.loss_functions.UnFlowLoss import unFlowLoss
from conftest import rel_err

EINVAL, EDTYPE, EUNSUPPORTED = -1, -2, -5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "census.npz")


def test_schemas_of_the_two_ops():
    s = lambda name: str(getattr(torch.ops.cerberus, name).default._schema)
    assert s("census_loss") == "cerberus::census_loss(Tensor im, Tensor im_warp, int max_distance) -> Tensor"
    assert s("census_loss_backward") == ("cerberus::census_loss_backward(Tensor im, Tensor im_warp, Tensor grad_loss, "
                                         "int max_distance, bool need_im, bool need_warp) -> (Tensor, Tensor)")


def test_meta_shapes():
    a = torch.empty(2, 3, 37, 53, device="meta")
    g = torch.empty((), device="meta")
    for d in (1, 2, 3):
        v = torch.ops.cerberus.census_loss(a, a, d)
        assert v.shape == () and v.dtype == torch.float32
        gi, gw = torch.ops.cerberus.census_loss_backward(a, a, g, d, True, True)
        assert gi.shape == a.shape and gw.shape == a.shape
        gi, gw = torch.ops.cerberus.census_loss_backward(a, a, g, d, False, True)
        assert gi.numel() == 0 and gw.shape == a.shape
        gi, gw = torch.ops.cerberus.census_loss_backward(a, a, g, d, True, False)
        assert gi.shape == a.shape and gw.numel() == 0


def test_cpu_tensors_fail_loudly():
    a, g = torch.rand(1, 3, 8, 8), torch.ones(())
    for call in (lambda: torch.ops.cerberus.census_loss(a, a, 1),
                 lambda: torch.ops.cerberus.census_loss_backward(a, a, g, 1, False, True),
                 lambda: torch.ops.cerberus.census_loss(a, a.clone().requires_grad_(True), 1)):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


def test_argument_rejection_without_gpu():
    lib = _lib.get()
    one = ctypes.c_void_p(16)      # a non-null pointer that is never dereferenced: every call below is rejected first
    cf = lambda *a: lib.cerberus_census_loss_forward(*a)
    cb = lambda *a: lib.cerberus_census_loss_backward(*a)
    big = 1 << 20
    # unknown dtype -> CERB_EDTYPE; known but not fp32 -> CERB_EUNSUPPORTED
    for dtype, want in ((9, EDTYPE), (-1, EDTYPE), (1, EUNSUPPORTED), (2, EUNSUPPORTED), (3, EUNSUPPORTED)):
        assert cf(one, one, one, one, big, 1, 8, 8, 1, dtype, None) == want
        assert cb(one, one, one, one, 1, 8, 8, 1, dtype, None) == want
    # max_distance outside the compiled windows
    for d in (0, -1, 4, 7):
        assert cf(one, one, one, one, big, 1, 64, 64, d, 0, None) == EINVAL
        assert cb(one, one, one, one, 1, 64, 64, d, 0, None) == EINVAL
    # sizes: an empty batch, H or W below 2 * max_distance + 1
    for B, H, W, d in ((0, 8, 8, 1), (-1, 8, 8, 1), (1, 2, 8, 1), (1, 8, 2, 1), (1, 0, 8, 1), (1, 4, 8, 2), (1, 8, 4, 2),
                       (1, 6, 8, 3), (1, 8, 6, 3)):
        assert cf(one, one, one, one, big, B, H, W, d, 0, None) == EINVAL
        assert cb(one, one, one, one, B, H, W, d, 0, None) == EINVAL
    # null pointers, one at a time
    for k in range(4):
        ptrs = [one] * 4
        ptrs[k] = None
        assert cf(*ptrs, big, 1, 8, 8, 1, 0, None) == EINVAL
        assert cb(*ptrs, 1, 8, 8, 1, 0, None) == EINVAL
    # a workspace smaller than the size function asks for
    assert cf(one, one, one, one, lib.cerberus_census_loss_workspace_bytes(2, 37, 53) - 1, 2, 37, 53, 1, 0, None) == EINVAL
    assert lib.cerberus_abi_version() == 7          # additions only


def test_workspace_size_equals_its_python_mirror():
    from cerberusnet_amd.ops import _census_workspace_bytes
    lib = _lib.get()
    for shape in ((1, 3, 3), (2, 37, 53), (4, 512, 1024), (4, 64, 128), (1, 16, 64), (1, 17, 65), (1, 1, 1), (0, 8, 8), (2, 0, 8),
                  (2, 8, 0), (-1, 8, 8), (2, 8, -4), (2, -8, 4)):
        assert _census_workspace_bytes(*shape) == lib.cerberus_census_loss_workspace_bytes(*shape), shape
    assert lib.cerberus_census_loss_workspace_bytes(4, 512, 1024) == 4 * 32 * 16 * 4


def _golden_cases():
    g = np.load(GOLDEN)
    assert int(g["n_cases"]) == len(cases.GOLDEN_CASES)
    for i, (shape, d, family) in enumerate(cases.GOLDEN_CASES):
        assert tuple(g["c%d_shape" % i]) == shape and int(g["c%d_max_distance" % i]) == d and str(g["c%d_family" % i]) == family
        yield i, shape, d, family, g


def test_ternary_loss_matches_the_reference_golden():
    """The package's TernaryLoss is the reference's op sequence in the same ATen ops: the map and the gradient are held to
    rel_err < 1e-6 (the bound of test_oracle.py for stock-op restatements of reference Python), the map also to bit-equality."""
    ds, ragged, tight = set(), False, False
    for i, shape, d, family, g in _golden_cases():
        im, im_warp = (torch.from_numpy(a) for a in cases.images(shape, family, cases.GOLDEN_SEED + 10 * i))
        im_warp.requires_grad_(True)
        out = ca.TernaryLoss(im, im_warp, d)
        assert out.shape == (shape[0], 1) + shape[2:] and out.dtype == torch.float32
        grad, = torch.autograd.grad(out.mean(), im_warp)
        want_map, want_grad = g["c%d_map" % i], g["c%d_grad_warp" % i]
        assert float(np.abs(want_grad).max()) > 0
        print("case %d %s d=%d %s: map rel_err %.3e grad rel_err %.3e" % (
            i, shape, d, family, rel_err(out.detach().numpy(), want_map), rel_err(grad.numpy(), want_grad)))
        assert rel_err(out.detach().numpy(), want_map) < 1e-6
        assert rel_err(grad.numpy(), want_grad) < 1e-6
        assert abs(float(out.detach().mean()) - float(g["c%d_mean" % i])) <= 1e-6 * abs(float(g["c%d_mean" % i]))
        assert np.array_equal(out.detach().numpy(), want_map)        # same op sequence on the same torch build
        # the border of width d is exactly zero, the interior is not
        m = out.detach().numpy()
        assert not m[:, :, :d].any() and not m[:, :, -d:].any() and not m[..., :d].any() and not m[..., -d:].any()
        assert m[:, :, d:-d, d:-d].all()
        ds.add(d)
        ragged |= shape[2] % 16 != 0 and shape[3] % 8 != 0
        tight |= min(shape[2:]) == 2 * d + 1
    assert ds == {1, 3} and ragged and tight


def test_unflow_loss_with_ternary_matches_the_reference_golden():
    g = np.load(GOLDEN)
    l_img, l_seq, fw, bw = cases.loss_inputs()
    loss = unFlowLoss(weights=dict(cases.LOSS_WEIGHTS), consistency=True, backend="torch")(
        {"flow": fw, "flow_b": bw}, {"l_img": l_img, "l_seq": l_seq})
    want = float(g["loss_value"])
    print("unFlowLoss with ternary: %.9g, reference %.9g" % (loss.item(), want))
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    grads = torch.autograd.grad(loss, fw[:4] + bw[:4])
    norms = np.array([float(x.double().norm()) for x in grads])
    assert np.allclose(norms, g["loss_flow_grad_norms"], rtol=2e-3, atol=1e-9)
    assert all(float(n) > 0 for n in norms)
    # the ternary term is part of that value: without it the loss differs
    plain = unFlowLoss(weights={"l1": 0.15, "ssim": 0.85}, consistency=True, backend="torch")(
        {"flow": fw, "flow_b": bw}, {"l_img": l_img, "l_seq": l_seq})
    assert abs(plain.item() - want) > 1e-3 * abs(want)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_census_loss_on_cpu_tensors_is_the_stock_formulation(d):
    a, b = (torch.from_numpy(x) for x in cases.images((2, 3, 13, 17), "unit", 700 + d))
    a.requires_grad_(True)
    b.requires_grad_(True)
    v = ca.census_loss(a, b, d)
    assert v.shape == () and torch.equal(v, ca.TernaryLoss(a, b, d).mean())
    ga, gb = torch.autograd.grad(v, (a, b))
    assert float(ga.abs().max()) > 0 and float(gb.abs().max()) > 0
    # symmetric in its two images
    assert torch.allclose(ca.census_loss(b, a, d), v, rtol=1e-6, atol=0)
    assert torch.equal(ca.census_loss(a, b), ca.census_loss(a, b, 1))
    assert "census_loss" in U.__all__ and "TernaryLoss" in U.__all__


def test_ternary_weight_of_unflowloss():
    assert unFlowLoss(weights={"ternary": 1.0}, backend="torch").ternary_weight == 1.0
    assert unFlowLoss(weights={"ternary": 1.0}, fused=True).ternary_weight == 1.0
    assert unFlowLoss().ternary_weight is None
    with pytest.raises(NotImplementedError, match="fused=True"):
        unFlowLoss(weights={"ternary": 1.0})
    with pytest.raises(NotImplementedError, match="fused=True"):
        unFlowLoss(weights={"l1": 0.15, "ssim": 0.85, "ternary": 1.0}, backend="hip", fused=False)
    # the term is added where the reference adds it: weight * TernaryLoss(im_recons, im_orig).mean(), beside L1 / SSIM
    a, b = (torch.from_numpy(x) for x in cases.images((1, 3, 9, 11), "unit", 710))
    only = unFlowLoss(weights={"ternary": 0.25}, backend="torch").loss_photometric(a, b)
    assert torch.equal(only, (0.25 * ca.TernaryLoss(b, a)).mean())
    both = unFlowLoss(weights={"l1": 0.15, "ssim": 0.85, "ternary": 0.25}, backend="torch").loss_photometric(a, b)
    plain = unFlowLoss(backend="torch").loss_photometric(a, b)
    assert torch.allclose(both, plain + only, rtol=1e-6, atol=0)
