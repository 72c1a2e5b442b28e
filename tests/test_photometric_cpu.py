"""CPU-side checks of the fused loss terms (csrc/photometric.hip): op schemas, Meta shapes, loud CPU failure, argument
rejection in the C ABI before any launch, the workspace-size mirrors, and the ``fused`` keyword of unFlowLoss."""
import ctypes

import pytest
import torch

import cerberusnet_amd as ca
from cerberusnet_amd import _lib
from cerberusnet_amd.loss_functions.UnFlowLoss import unFlowLoss

EINVAL, EDTYPE, EUNSUPPORTED = -1, -2, -5
F = ctypes.c_float


def test_schemas_of_the_four_ops():
    s = lambda name: str(getattr(torch.ops.cerberus, name).default._schema)
    assert s("photometric_loss") == ("cerberus::photometric_loss(Tensor im_orig, Tensor im_recons, float l1_weight, "
                                     "float ssim_weight) -> Tensor")
    assert s("photometric_loss_backward") == (
        "cerberus::photometric_loss_backward(Tensor im_orig, Tensor im_recons, Tensor grad_loss, float l1_weight, "
        "float ssim_weight, bool need_orig, bool need_recons) -> Tensor[]")
    assert s("edge_smoothness") == "cerberus::edge_smoothness(Tensor flow, Tensor image, float alpha, int degree) -> Tensor"
    assert s("edge_smoothness_backward") == ("cerberus::edge_smoothness_backward(Tensor flow, Tensor image, Tensor grad_loss, "
                                             "float alpha, int degree) -> Tensor")


def test_meta_shapes():
    a = torch.empty(2, 3, 37, 53, device="meta")
    f = torch.empty(2, 2, 37, 53, device="meta")
    g = torch.empty((), device="meta")
    v = torch.ops.cerberus.photometric_loss(a, a, 0.15, 0.85)
    assert v.shape == () and v.dtype == torch.float32
    go, gr = torch.ops.cerberus.photometric_loss_backward(a, a, g, 0.15, 0.85, True, True)
    assert go.shape == a.shape and gr.shape == a.shape
    go, gr = torch.ops.cerberus.photometric_loss_backward(a, a, g, 0.15, 0.85, False, True)
    assert go.numel() == 0 and gr.shape == a.shape
    v = torch.ops.cerberus.edge_smoothness(f, a, 0.2, 2)
    assert v.shape == () and v.dtype == torch.float32
    assert torch.ops.cerberus.edge_smoothness_backward(f, a, g, 0.2, 2).shape == f.shape


def test_cpu_tensors_fail_loudly():
    a, f, g = torch.randn(1, 3, 8, 8), torch.randn(1, 2, 8, 8), torch.ones(())
    for call in (lambda: torch.ops.cerberus.photometric_loss(a, a, 0.15, 0.85),
                 lambda: torch.ops.cerberus.photometric_loss_backward(a, a, g, 0.15, 0.85, False, True),
                 lambda: torch.ops.cerberus.edge_smoothness(f, a, 0.2, 2),
                 lambda: torch.ops.cerberus.edge_smoothness_backward(f, a, g, 0.2, 2),
                 lambda: torch.ops.cerberus.photometric_loss(a, a.clone().requires_grad_(True), 0.15, 0.85)):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


def test_public_wrappers_take_the_stock_path_where_the_ops_do_not_apply():
    """CPU tensors are outside the HIP ops: the public functions compute the stock formulation there (and agree with it)."""
    from cerberusnet_amd.loss_functions import UnFlowLoss as U
    torch.manual_seed(3)
    a, b = torch.randn(1, 3, 9, 11), torch.randn(1, 3, 9, 11, requires_grad=True)
    f = torch.randn(1, 2, 9, 11, requires_grad=True)
    ref = unFlowLoss(backend="torch").loss_photometric(a, b)
    assert torch.equal(ca.photometric_loss(a, b, 0.15, 0.85), ref)
    assert torch.equal(ca.photometric_loss(a, b, 1.0, None), (a - b).abs().mean())
    for degree in (1, 2):
        assert torch.equal(ca.edge_smoothness(f, a, 0.2, degree), U._edge_aware_smoothness(f, a, 0.2, degree))
    with pytest.raises(NotImplementedError):
        ca.edge_smoothness(f, a, 0.2, 3)
    assert "photometric_loss" in U.__all__ and "edge_smoothness" in U.__all__


def test_argument_rejection_without_gpu():
    lib = _lib.get()
    one = ctypes.c_void_p(16)      # a non-null pointer that is never dereferenced: every call below is rejected first
    pf = lambda *a: lib.cerberus_photometric_loss_forward(*a)
    pb = lambda *a: lib.cerberus_photometric_loss_backward(*a)
    sf = lambda *a: lib.cerberus_edge_smoothness_forward(*a)
    sb = lambda *a: lib.cerberus_edge_smoothness_backward(*a)
    big = 1 << 20
    # unknown dtype -> CERB_EDTYPE; known but not fp32 -> CERB_EUNSUPPORTED
    for dtype, want in ((9, EDTYPE), (-1, EDTYPE), (1, EUNSUPPORTED), (2, EUNSUPPORTED), (3, EUNSUPPORTED)):
        assert pf(one, one, one, one, big, 1, 3, 8, 8, F(0.15), F(0.85), dtype, None) == want
        assert pb(one, one, one, one, 1, 3, 8, 8, F(0.15), F(0.85), dtype, None) == want
        assert sf(one, one, one, one, big, 1, 2, 3, 8, 8, F(0.2), 2, dtype, None) == want
        assert sb(one, one, one, one, 1, 2, 3, 8, 8, F(0.2), 2, dtype, None) == want
    # sizes: empty tensors, H or W < 2 (photometric), H or W <= degree (smoothness), degree 3
    for B, C, H, W in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 1, 8), (1, 3, 8, 1), (1, 3, 0, 8), (-1, 3, 8, 8)):
        assert pf(one, one, one, one, big, B, C, H, W, F(0.15), F(0.85), 0, None) == EINVAL
        assert pb(one, one, one, one, B, C, H, W, F(0.15), F(0.85), 0, None) == EINVAL
    for B, H, W, degree in ((0, 8, 8, 2), (1, 2, 8, 2), (1, 8, 2, 2), (1, 1, 8, 1), (1, 8, 1, 1), (1, 8, 8, 3), (1, 8, 8, 0)):
        assert sf(one, one, one, one, big, B, 2, 3, H, W, F(0.2), degree, 0, None) == EINVAL
        assert sb(one, one, one, one, B, 2, 3, H, W, F(0.2), degree, 0, None) == EINVAL
    assert sf(one, one, one, one, big, 1, 0, 3, 8, 8, F(0.2), 2, 0, None) == EINVAL
    assert sf(one, one, one, one, big, 1, 2, 0, 8, 8, F(0.2), 2, 0, None) == EINVAL
    # null pointers, one at a time
    for k in range(4):
        ptrs = [one] * 4
        ptrs[k] = None
        assert pf(*ptrs, big, 1, 3, 8, 8, F(0.15), F(0.85), 0, None) == EINVAL
        assert pb(*ptrs, 1, 3, 8, 8, F(0.15), F(0.85), 0, None) == EINVAL
        assert sf(*ptrs, big, 1, 2, 3, 8, 8, F(0.2), 2, 0, None) == EINVAL
        assert sb(*ptrs, 1, 2, 3, 8, 8, F(0.2), 2, 0, None) == EINVAL
    # a workspace smaller than the size function asks for
    assert pf(one, one, one, one, lib.cerberus_photometric_loss_workspace_bytes(1, 3, 8, 8) - 1, 1, 3, 8, 8, F(0.15), F(0.85), 0,
              None) == EINVAL
    assert sf(one, one, one, one, lib.cerberus_edge_smoothness_workspace_bytes(1, 8, 8) - 1, 1, 2, 3, 8, 8, F(0.2), 2, 0,
              None) == EINVAL
    assert lib.cerberus_abi_version() == 7          # additions only


def test_workspace_sizes_equal_their_python_mirrors():
    from cerberusnet_amd.ops import _photometric_workspace_bytes, _smoothness_workspace_bytes
    lib = _lib.get()
    for shape in ((1, 1, 2, 2), (2, 3, 37, 53), (4, 3, 512, 1024), (4, 3, 64, 128), (1, 3, 16, 64), (1, 3, 17, 65), (1, 1, 1, 1),
                  (0, 3, 8, 8), (2, 0, 8, 8), (2, 3, 0, 8), (-1, 3, 8, 8), (2, 3, 8, -4)):
        assert _photometric_workspace_bytes(*shape) == lib.cerberus_photometric_loss_workspace_bytes(*shape), shape
    assert lib.cerberus_photometric_loss_workspace_bytes(4, 3, 512, 1024) == 4 * 3 * 32 * 16 * 4
    for shape in ((1, 2, 2), (2, 37, 53), (4, 512, 1024), (4, 64, 128), (1, 4, 64), (1, 5, 65), (0, 8, 8), (2, 0, 8), (-1, 8, 8),
                  (2, 8, -4)):
        assert _smoothness_workspace_bytes(*shape) == lib.cerberus_edge_smoothness_workspace_bytes(*shape), shape
    assert lib.cerberus_edge_smoothness_workspace_bytes(4, 512, 1024) == 4 * 128 * 16 * 8


def test_fused_keyword_of_unflowloss():
    assert unFlowLoss().fused is False
    assert unFlowLoss(fused=True).fused is True
    with pytest.raises(ValueError, match="fused"):
        unFlowLoss(backend="torch", fused=True)
    # `backend` is reassigned on live objects (the bench does): fused then has no effect, the stock path runs on the CPU
    loss_fn = unFlowLoss(fused=True)
    loss_fn.backend = "torch"
    torch.manual_seed(5)
    a, b = torch.randn(1, 3, 8, 12), torch.randn(1, 3, 8, 12)
    assert torch.equal(loss_fn.loss_photometric(a, b), unFlowLoss(backend="torch").loss_photometric(a, b))
    f = torch.randn(1, 2, 8, 12)
    assert torch.equal(loss_fn.loss_smooth(f, a), unFlowLoss(backend="torch").loss_smooth(f, a))
