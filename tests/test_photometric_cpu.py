"""CPU-side checks of the fused loss terms (csrc/photometric.hip): op schemas, Meta shapes, loud CPU failure, argument
rejection in the C ABI before any launch, the workspace-size mirrors, the ``fused`` keyword of unFlowLoss, and the stock-op
formulations of the two terms and of the whole loss against results of the reference's own code
(tests/golden/photometric.npz, written by tools/gen_golden_photometric.py from the table in tests/photometric_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import photometric_cases as pc
from cerberusnet_amd import _lib
from cerberusnet_amd.loss_functions import UnFlowLoss as U
from cerberusnet_amd.loss_functions.UnFlowLoss import unFlowLoss
from conftest import l2_err, rel_err

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


# ---- the stock-op restatements are the reference: tests/golden/photometric.npz, written by tools/gen_golden_photometric.py
# from the reference's own SSIM module, smooth_grad_1st / smooth_grad_2nd and unFlowLoss in float32 and float64 ----------
REF_TOL = 1e-6           # the bound of test_oracle.py for stock-op restatements of reference Python
F64_TOL = 1e-12


@pytest.fixture(scope="module")
def ref(golden):
    return golden("photometric")


def _close(a, b, tol):
    return abs(float(a) - float(b)) <= tol * abs(float(b))


def test_golden_file_agrees_with_the_case_table(ref):
    assert int(ref["n_photo"]) == len(pc.PHOTO_CASES) and int(ref["n_smooth"]) == len(pc.SMOOTH_CASES)
    assert list(ref["loss_configs"]) == sorted(pc.LOSS_CONFIGS)
    for i, (shape, family) in enumerate(pc.PHOTO_CASES):
        assert tuple(ref["p%d_shape" % i]) == shape and str(ref["p%d_family" % i]) == family
        assert float(ref["p%d_ssim_margin" % i]) >= pc.SSIM_MARGIN           # the clamp's corner at SSIM = -1 is not near
        for tag, dtype in (("f32", np.float32), ("f64", np.float64)):
            for key in ("map", "l1_grad_orig", "l1_grad_recons", "ssim_grad_orig", "ssim_grad_recons") + (
                    ("mix_grad_orig", "mix_grad_recons") if tag == "f32" else ()):
                a = ref["p%d_%s_%s" % (i, tag, key)]
                assert a.shape == shape and a.dtype == dtype and np.isfinite(a).all()
    for i, (shape, channels, degree, alpha, family) in enumerate(pc.SMOOTH_CASES):
        assert tuple(ref["s%d_shape" % i]) == shape and int(ref["s%d_channels" % i]) == channels
        assert int(ref["s%d_degree" % i]) == degree and float(ref["s%d_alpha" % i]) == alpha and str(ref["s%d_family" % i]) == family
        for tag, dtype in (("f32", np.float32), ("f64", np.float64)):
            assert ref["s%d_%s_grad_flow" % (i, tag)].shape == shape and ref["s%d_%s_grad_flow" % (i, tag)].dtype == dtype
            assert ref["s%d_%s_grad_image" % (i, tag)].shape == (shape[0], channels) + shape[2:]
    for name in pc.LOSS_CONFIGS:
        assert list(ref["l%s_used" % name]) == pc.loss_used(name)
        for j in pc.loss_used(name):
            assert ref["l%s_grad%d" % (name, j)].shape == (1, 2) + pc.LOSS_SIZES[j % 5]


def test_case_table_covers_what_the_kernels_can_get_wrong():
    crosses = lambda hw, tile, by=1: hw[0] >= tile[0] + by and hw[1] >= tile[1] + by         # a tile seam in each direction
    photo = pc.PHOTO_CASES
    assert {f for _, f in photo} == set(pc.FAMILIES)
    assert {f for s, f in photo if crosses(s[2:], pc.PHOTO_TILE)} == set(pc.FAMILIES)       # every family across a seam, both ways
    assert any(crosses(s[2:], pc.PHOTO_TILE, 2) for s, _ in photo)            # backward centres from the next tile's ring
    assert any(s[2:] == (2, 2) for s, _ in photo) and any(s[2:] == (3, 3) for s, _ in photo)
    assert any(s[0] > 1 for s, _ in photo) and any(s[3] > 2 * pc.PHOTO_TILE[1] and s[3] % pc.PHOTO_TILE[1] for s, _ in photo)
    smooth = pc.SMOOTH_CASES
    assert {(d, a) for _, _, d, a, _ in smooth} == {(1, 0.2), (1, 10.0), (2, 0.2), (2, 10.0)}
    assert {f for *_, f in smooth} == set(pc.FAMILIES)
    for degree in (1, 2):
        assert any(d == degree and s[2:] == (degree + 1, degree + 1) for s, _, d, _, _ in smooth)       # the smallest legal map
        assert any(d == degree and crosses(s[2:], pc.SMOOTH_TILE) for s, _, d, _, _ in smooth)
    assert any(c == 1 and s[1] == 3 for s, c, *_ in smooth)
    assert {c["smooth"]["degree"] for c in pc.LOSS_CONFIGS.values() if "smooth" in c} == {1}
    assert not all(c["consistency"] for c in pc.LOSS_CONFIGS.values())


def test_ssim_distance_is_the_reference_ssim_module(ref):
    """Same ATen op sequence on the same torch build: the float32 map equals the reference's bit for bit (the rule of
    test_ternary_loss_matches_the_reference_golden), the float64 map to rel_err < 1e-12.  No element is left out."""
    for i, (shape, family) in enumerate(pc.PHOTO_CASES):
        orig, recons = (torch.from_numpy(a) for a in pc.photo_images(i))
        m32 = U._ssim_distance(recons, orig).numpy()
        m64 = U._ssim_distance(recons.double(), orig.double()).numpy()
        e32, e64 = rel_err(m32, ref["p%d_f32_map" % i]), rel_err(m64, ref["p%d_f64_map" % i])
        print("photometric %d %s %s: map rel_err f32 %.3e f64 %.3e" % (i, shape, family, e32, e64))
        assert m32.dtype == np.float32 and np.array_equal(m32, ref["p%d_f32_map" % i])
        assert e64 < F64_TOL


@pytest.mark.parametrize("tag,dtype", pc.DTYPES)
def test_photometric_stock_matches_the_reference_golden(ref, tag, dtype):
    """``_photometric_stock`` and ``unFlowLoss(backend='torch').loss_photometric`` for every weight pair, in both dtypes,
    against the reference's results of the same dtype: values to 1e-6 relative, the gradients with respect to BOTH images
    to rel_err < 1e-6.  ``_ssim_distance`` is the reference's ATen op sequence, so in float32 values and gradients are the
    reference's bit for bit (the rule of test_ternary_loss_matches_the_reference_golden)."""
    for i, (shape, family) in enumerate(pc.PHOTO_CASES):
        for w1, w2 in pc.WEIGHT_PAIRS:
            want_v, want_g = pc.photo_reference(ref, i, tag, w1, w2)
            mod = unFlowLoss(backend="torch", weights={k: w for k, w in (("l1", w1), ("ssim", w2)) if w})
            for name, fn in (("_photometric_stock", lambda o, r: U._photometric_stock(o, r, w1, w2)), ("loss_photometric", mod.loss_photometric)):
                o, r = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in pc.photo_images(i))
                v = fn(o, r)
                grads = [g.numpy() for g in torch.autograd.grad(v, (o, r))]
                errs = [rel_err(g, w) for g, w in zip(grads, want_g)]
                print("photometric %d %s %s %s (%g, %g) %s: value rel %.3e grad rel_err orig %.3e recons %.3e" % (
                    i, shape, family, tag, w1, w2, name, abs(v.item() - want_v) / abs(want_v), errs[0], errs[1]))
                assert v.dtype == dtype and _close(v.item(), want_v, REF_TOL)
                assert all(float(np.abs(w).max()) > 0 for w in want_g) and max(errs) < REF_TOL
                if dtype == torch.float32:
                    assert v.item() == want_v and all(np.array_equal(g, w) for g, w in zip(grads, want_g))


@pytest.mark.parametrize("tag,dtype", pc.DTYPES)
def test_edge_aware_smoothness_matches_the_reference_golden(ref, tag, dtype):
    for i, (shape, channels, degree, alpha, family) in enumerate(pc.SMOOTH_CASES):
        flow, image = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in pc.smooth_inputs(i))
        assert flow.shape == shape and image.shape[1] == channels
        v = U._edge_aware_smoothness(flow, image, alpha, degree)
        gf, gi = torch.autograd.grad(v, (flow, image))
        want = float(ref["s%d_%s_value" % (i, tag)])
        ef, ei = rel_err(gf.numpy(), ref["s%d_%s_grad_flow" % (i, tag)]), rel_err(gi.numpy(), ref["s%d_%s_grad_image" % (i, tag)])
        print("smoothness %d %s degree %d alpha %g %s %s: value rel %.3e grad rel_err flow %.3e image %.3e" % (
            i, shape, degree, alpha, family, tag, abs(v.item() - want) / abs(want), ef, ei))
        assert v.dtype == dtype and _close(v.item(), want, REF_TOL)
        assert float(np.abs(ref["s%d_%s_grad_flow" % (i, tag)]).max()) > 0 and float(np.abs(ref["s%d_%s_grad_image" % (i, tag)]).max()) > 0
        assert max(ef, ei) < (REF_TOL if dtype == torch.float32 else F64_TOL)
        # the module's loss_smooth takes degree and alpha from its keywords
        mod = unFlowLoss(backend="torch", smooth={"degree": degree, "alpha": alpha, "weighting": 1.0})
        assert torch.equal(mod.loss_smooth(flow, image), v)


@pytest.mark.parametrize("name", sorted(pc.LOSS_CONFIGS))
def test_unflow_loss_keywords_match_the_reference_golden(ref, name):
    """consistency, weight, smooth (degree, alpha, weighting), w_sm_scales and w_wrp_scales (a skipped scale; a first scale
    that is off, which leaves the flow divisor at 1) against the reference's own unFlowLoss: the value in both dtypes, every
    used flow's float64 gradient per element, and no gradient for the flows the configuration does not use."""
    cfg = pc.LOSS_CONFIGS[name]
    l_img, l_seq, fw, bw = pc.loss_inputs(torch.float32)
    v32 = unFlowLoss(backend="torch", **cfg)({"flow": fw, "flow_b": bw}, {"l_img": l_img, "l_seq": l_seq}).item()
    l_img, l_seq, fw, bw = pc.loss_inputs(torch.float64)
    tgt = {"l_img": l_img, "l_seq": l_seq}
    loss = unFlowLoss(backend="torch", **cfg)({"flow": fw, "flow_b": bw}, tgt)
    want32, want64 = float(ref["l%s_f32_value" % name]), float(ref["l%s_f64_value" % name])
    print("unFlowLoss %s: float64 %.12g (reference %.12g) float32 %.9g (reference %.9g)" % (name, loss.item(), want64, v32, want32))
    assert loss.dtype == torch.float64 and _close(loss.item(), want64, 1e-10)
    assert _close(v32, want32, 1e-5)
    grads = torch.autograd.grad(loss, fw + bw, allow_unused=True)
    used = pc.loss_used(name)
    assert 4 not in used and 9 not in used and (name != "b" or 1 not in used)
    for j, g in enumerate(grads):
        if j not in used:
            assert g is None, (name, j)
            continue
        want = ref["l%s_grad%d" % (name, j)]
        print("  flow %d gradient l2_err %.3e rel_err %.3e" % (j, l2_err(g.numpy(), want), rel_err(g.numpy(), want)))
        assert float(np.abs(want).max()) > 0 and l2_err(g.numpy(), want) < 1e-6
    # the keywords carry weight: the default configuration gives another value on the same inputs
    plain = unFlowLoss(backend="torch")({"flow": fw, "flow_b": bw}, tgt).item()
    assert _close(plain, float(ref["ldefault_f64_value"]), 1e-10)
    assert abs(plain - want64) > 1e-3 * abs(want64)
