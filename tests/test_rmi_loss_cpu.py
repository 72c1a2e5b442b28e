"""CPU tests of the RMI losses (loss_functions/rmi.py, csrc/rmi_loss.hip): the stock-op formulation against results of the
reference's own RMILoss / RMILossAux / MultiScaleRMILoss (tests/golden/rmi_loss.npz, written by tools/gen_golden_rmi.py), the
classes' signatures, and the op / C-ABI layer as far as it goes without a GPU.

Bounds: the value within 1e-6 of the reference relative to S = |lambda bce| + |(1 - lambda) rmi| (the two terms have opposite
signs, the loss itself can be near 0), the gradient ``l2_err <= 1e-5`` (test_seg_loss_cpu.py's).  Measured on the build machine:
every one of the 13 cases gives the reference's value and gradient bit for bit (0.0 and 0.0) -- the formulation keeps the
reference's operation order."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import rmi_cases as cases
from cerberusnet_amd import _lib
from cerberusnet_amd import build as cbuild
from cerberusnet_amd import ops
from cerberusnet_amd.loss_functions import rmi as R
from conftest import REPO, l2_err

VALUE_TOL = 1e-6
GRAD_TOL = 1e-5


def test_the_golden_file_holds_the_inputs_of_the_cases(golden):
    g = golden("rmi_loss")
    for i, (_, shape, _, _, four_d) in enumerate(cases.GOLDEN_CASES):
        xs, t = cases.golden_inputs(i)
        for k, x in enumerate(xs):
            assert np.array_equal(g["c%d_logits%d" % (i, k)], x)
            assert x.shape == shape and x.dtype == np.float32 and -4.0 <= x.min() and x.max() < 4.0
        assert np.array_equal(g["c%d_target" % i], t)
        assert t.dtype == np.int64 and t.shape == ((shape[0], 1) + shape[2:] if four_d else (shape[0],) + shape[2:])
        assert 0.08 < float((t == cases.IGNORE).mean()) < 0.25
    names = {n for n, *_ in cases.GOLDEN_CASES}
    kw = [k for _, _, k, _, _ in cases.GOLDEN_CASES]
    assert names == {"RMILoss", "RMILossAux", "MultiScaleRMILoss"}
    assert {f.get("do_rmi", True) for *_, f, _ in cases.GOLDEN_CASES} == {True, False}
    assert {k.get("lambda_way", 1) for k in kw} == {0, 1} and {k.get("rmi_pool_size", 4) for k in kw} == {1, 2, 4}
    assert {k.get("rmi_pool_way", 1) for k in kw} == {0, 1, 2} and {k.get("rmi_radius", 3) for k in kw} == {1, 2, 3}
    assert any(four_d for *_, four_d in cases.GOLDEN_CASES)
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "rmi_loss.npz")) < (1 << 20)


@pytest.mark.parametrize("backend", ["torch", "hip"])       # on CPU tensors 'hip' falls back to the stock ops
@pytest.mark.parametrize("i", range(len(cases.GOLDEN_CASES)))
def test_stock_formulation_reproduces_the_reference(golden, i, backend):
    g = golden("rmi_loss")
    name, _, kwargs, fwd, _ = cases.GOLDEN_CASES[i]
    heads = len([k for k in g if k.startswith("c%d_logits" % i)])
    xs = [torch.from_numpy(g["c%d_logits%d" % (i, k)]).requires_grad_(True) for k in range(heads)]
    t = torch.from_numpy(g["c%d_target" % i])
    loss = cases.golden_call(getattr(ca, name)(backend=backend, **kwargs), name, fwd, xs, t)
    grads = torch.autograd.grad(loss, xs)
    lam, way = kwargs.get("loss_weight_lambda", 0.5), kwargs.get("lambda_way", 1)
    parts = []
    for k in range(heads):            # (bce, rmi) of every prediction from the reference's own values
        bce, full = float(g["c%d_bce%d" % (i, k)]), float(g["c%d_full%d" % (i, k)])
        parts.append((bce, (full - lam * bce) / (1 - lam) if way else (full - bce) / lam))
    S = cases.golden_scale(name, kwargs, fwd, parts)
    ref_v = float(g["c%d_value" % i])
    print("%d %s %s: value %.9g ref %.9g, |diff| / S %.3e" % (i, name, backend, loss.item(), ref_v, abs(loss.item() - ref_v) / S))
    assert loss.dtype == torch.float32 and loss.shape == () and S > 0
    assert abs(loss.item() - ref_v) <= VALUE_TOL * S
    for k, grad in enumerate(grads):
        ref_g = g["c%d_grad%d" % (i, k)]
        print("   grad%d l2_err %.3e" % (k, l2_err(grad.numpy(), ref_g)))
        assert l2_err(grad.numpy(), ref_g) <= GRAD_TOL and float(np.abs(ref_g).max()) > 0
        dead = (t.reshape(t.shape[0], 1, *t.shape[-2:]) == cases.IGNORE)
        assert float(grad.abs().mul(dead).max()) == 0.0


def test_the_restatement_agrees_with_the_reference(golden):
    """The float64 yardstick of the GPU tests (rmi_cases.restate) against the reference's fp32 values for the cases it covers
    (radius 3, average pooling): within 1e-5 S, the project's VALUE_TOL (measured 3.0e-9 .. 4.7e-8 S; gradient l2_err 4.8e-8 .. 3.6e-7)."""
    g = golden("rmi_loss")
    seen = 0
    for i, (name, shape, kwargs, fwd, _) in enumerate(cases.GOLDEN_CASES):
        if name != "RMILoss" or kwargs.get("rmi_pool_way", 1) != 1 or kwargs.get("rmi_radius", 3) != 3:
            continue
        x = torch.from_numpy(g["c%d_logits0" % i]).double().requires_grad_(True)
        t = torch.from_numpy(g["c%d_target" % i]).reshape(shape[0], *shape[2:])
        out = cases.restate(x, t, shape[1], p=kwargs.get("rmi_pool_size", 4), lam=kwargs.get("loss_weight_lambda", 0.5),
                            lambda_way=kwargs.get("lambda_way", 1), do_rmi=fwd.get("do_rmi", True))
        grad, = torch.autograd.grad(out["loss"], x)
        err = abs(float(out["loss"].detach()) - float(g["c%d_value" % i])) / out["S"]
        print("%d: |diff| / S %.3e, grad l2_err %.3e" % (i, err, l2_err(g["c%d_grad0" % i], grad.numpy())))
        assert err <= 1e-5 and l2_err(g["c%d_grad0" % i], grad.numpy()) <= 1e-5
        seen += 1
    assert seen >= 5


def test_negative_labels_are_ignored_on_the_stock_path():
    x = torch.from_numpy(cases.logits((1, 3, 12, 12), 980))
    t = torch.from_numpy(cases.labels((1, 3, 12, 12), 981))
    odd = t.clone()
    odd[t == cases.IGNORE] = torch.tensor([-1, -7, 3, 99, 1 << 40])[torch.arange(int((t == cases.IGNORE).sum())) % 5]
    assert torch.equal(ca.rmi_loss(x, t, num_classes=3), ca.rmi_loss(x, odd, num_classes=3))


def test_class_signatures_match_the_reference():
    # rmi.py:39-40, :63-64, :210, :217, :242, :248-249; `backend` comes after the reference's parameters
    params = [("num_classes", 21), ("rmi_radius", 3), ("rmi_pool_way", 1), ("rmi_pool_size", 4), ("rmi_pool_stride", 4),
              ("loss_weight_lambda", 0.5), ("lambda_way", 1), ("ignore_index", 255)]
    got = list(inspect.signature(ca.RMILoss.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in got] == params + [("backend", "hip")]
    fsig = inspect.signature(ca.RMILoss.forward)
    assert list(fsig.parameters) == ["self", "logits_4D", "labels_4D", "do_rmi"] and fsig.parameters["do_rmi"].default is True
    got = list(inspect.signature(ca.MultiScaleRMILoss.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in got[:3]] == [("ocr_aux_rmi", False), ("supervised_mscale_wt", 0.0), ("alpha", 0.4)]
    assert got[3].kind == inspect.Parameter.VAR_KEYWORD and len(got) == 4
    assert list(inspect.signature(ca.MultiScaleRMILoss.forward).parameters) == ["self", "seg_pred", "seg_gt", "kwargs"]
    got = list(inspect.signature(ca.RMILossAux.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in got[:2]] == [("weight", 1.0), ("aux_weight", 0.4)]
    assert got[2].kind == inspect.Parameter.VAR_KEYWORD and len(got) == 3
    assert list(inspect.signature(ca.RMILossAux.forward).parameters) == ["self", "predictions", "targets"]
    fn = ca.RMILoss()
    assert (fn.half_d, fn.d, fn.kernel_padding, fn.backend, len(fn.state_dict())) == (9, 18, 2, "hip", 0)
    assert ca.RMILossAux(num_classes=7, backend="torch").rmi.backend == "torch" and ca.MultiScaleRMILoss().rmi.num_classes == 21
    for bad in (dict(rmi_radius=11), dict(rmi_pool_way=4), dict(rmi_pool_size=4, rmi_pool_stride=2)):
        with pytest.raises(AssertionError):
            ca.RMILoss(**bad)
    with pytest.raises(ValueError):
        ca.RMILoss(backend="cuda")
    with pytest.raises(AssertionError):
        ca.RMILossAux()({"depth": torch.zeros(1)}, {"seg": torch.zeros(1)})
    with pytest.raises(NotImplementedError):
        ca.RMILoss(num_classes=3, rmi_pool_way=3)(torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, 16, dtype=torch.int64))
    sig = inspect.signature(ca.rmi_loss)
    assert [(p.name, p.default) for p in sig.parameters.values()][2:] == params[:7] + [("do_rmi", True), ("backend", "hip")]


def test_names_are_exported_and_the_source_is_built():
    names = ["rmi_loss", "RMILoss", "RMILossAux", "MultiScaleRMILoss"]
    assert R.__all__ == names
    for mod in (ca.loss_functions, ca):
        assert set(names) <= set(mod.__all__)
        for n in names:
            assert getattr(mod, n) is getattr(R, n)
    assert "rmi_loss.hip" in cbuild.SOURCES and "rmi_loss.hip" in cbuild.EXPERIMENT_SOURCES


def test_op_schemas():
    s = lambda n: str(getattr(torch.ops.cerberus, n).default._schema)
    assert s("rmi_moments") == ("cerberus::rmi_moments(Tensor logits, Tensor target, int radius, int pool, bool do_rmi) -> "
                                "(Tensor bce, Tensor la_cov, Tensor pr_cov, Tensor la_pr_cov, Tensor la_map, Tensor pr_map, "
                                "Tensor means, Tensor state)")
    assert s("rmi_moments_backward") == ("cerberus::rmi_moments_backward(Tensor logits, Tensor target, Tensor la_map, Tensor pr_map, "
                                         "Tensor means, Tensor state, Tensor grad_bce, Tensor grad_pr_cov, Tensor grad_la_pr_cov, "
                                         "int radius, int pool, bool do_rmi) -> Tensor")


def test_meta_implementations_give_the_shapes():
    m = lambda *shape, dtype=torch.float32: torch.empty(*shape, device="meta", dtype=dtype)
    x, t = m(2, 19, 15, 23), m(2, 15, 23, dtype=torch.int64)
    out = torch.ops.cerberus.rmi_moments(x, t, 3, 4, True)
    want = [((), torch.float32)] + [((2, 19, 9, 9), torch.float64)] * 3 + [((2, 19, 4, 6), torch.float32)] * 2 + [
        ((2, 19, 2, 9), torch.float64), ((4,), torch.float32)]
    assert [(tuple(o.shape), o.dtype) for o in out] == want and all(o.device.type == "meta" for o in out)
    g = torch.ops.cerberus.rmi_moments_backward(x, t, out[4], out[5], out[6], out[7], out[0], out[2], out[3], 3, 4, True)
    assert g.shape == x.shape and g.dtype == torch.float32 and g.device.type == "meta"
    off = torch.ops.cerberus.rmi_moments(x, t, 3, 4, False)
    assert off[0].shape == () and off[7].shape == (4,) and all(o.numel() == 0 for o in off[1:7])
    # the pooled size is avg_pool2d's: the divisor's window count, trailing rows in no window included
    for size in range(8, 40):
        for pool in range(1, 9):
            want = torch.nn.functional.avg_pool2d(torch.zeros(1, 1, size, size), pool, pool, pool // 2).shape[-1] if pool > 1 else size
            assert ops._rmi_pooled(size, pool) == want, (size, pool)


def test_cpu_tensors_through_the_raw_ops_raise():
    x, t = torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, 16, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.rmi_moments(x, t, 3, 4, True)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.rmi_moments(x.requires_grad_(True), t, 3, 4, True)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.rmi_moments_backward(x.detach(), t, torch.zeros(1, 3, 5, 5), torch.zeros(1, 3, 5, 5),
                                                torch.zeros(1, 3, 2, 9, dtype=torch.float64), torch.zeros(4), torch.ones(()),
                                                torch.zeros(1, 3, 9, 9, dtype=torch.float64),
                                                torch.zeros(1, 3, 9, 9, dtype=torch.float64), 3, 4, True)


def test_workspace_bytes_in_python_equal_the_library():
    lib = _lib.get()
    for shape in ((1, 2, 8, 8, 4), (1, 19, 13, 22, 4), (2, 19, 37, 53, 4), (2, 150, 9, 20, 4), (2, 4, 11, 13, 2), (2, 3, 17, 19, 3),
                  (1, 3, 7, 9, 1), (2, 19, 128, 256, 4), (4, 19, 512, 1024, 4), (2, 17, 150, 150, 1), (2, 19, 37, 53, 8),
                  (1, 2, 7, 8, 4), (0, 2, 8, 8, 4), (-1, 2, 8, 8, 4), (1, 0, 8, 8, 4), (2, 19, 37, 53, 9), (2, 19, 37, 53, 0),
                  (1, 2, 2, 2, 1), (70000, 2, 8, 8, 4), (1, 40000, 8, 8, 4), (1, 2, 65536, 32768, 4)):
        assert ops._rmi_workspace_bytes(*shape) == lib.cerberus_rmi_workspace_bytes(*shape), shape
    # (1,2,8,8): 1 workgroup x 1 class group x (bce, count) and 1 chunk of 243 products, float64
    assert ops._rmi_workspace_bytes(1, 2, 8, 8, 4) == 8 * (2 + 2 * 243)
    assert ops._rmi_workspace_bytes(1, 2, 7, 8, 4) == 0 and ops._rmi_workspace_bytes(2, 19, 37, 53, 9) == 0


def test_argument_rejection_without_gpu():
    lib = _lib.get()
    one = 4096                                                         # never dereferenced: every call below returns before a launch
    fwd = lambda ptrs, ws_bytes, B, C, H, W, radius, pool, do_rmi, dtype: lib.cerberus_rmi_forward(
        *ptrs, ws_bytes, B, C, H, W, radius, pool, do_rmi, dtype, None)
    bwd = lambda ptrs, B, C, H, W, radius, pool, do_rmi, dtype: lib.cerberus_rmi_backward(*ptrs, B, C, H, W, radius, pool, do_rmi,
                                                                                         dtype, None)
    null11, full11, null10, full10 = [None] * 11, [one] * 11, [None] * 10, [one] * 10
    ok = (2, 19, 16, 16, 3, 4, 1, 0)
    assert fwd(null11, 1 << 20, *ok) == -1 and bwd(null10, *ok) == -1  # CERB_EINVAL: null pointers
    for k in range(11):
        assert fwd(full11[:k] + [None] + full11[k + 1:], 1 << 20, *ok) == -1, k
    for k in range(10):
        assert bwd(full10[:k] + [None] + full10[k + 1:], *ok) == -1, k
    assert fwd(null11, 1 << 20, 2, 19, 16, 16, 3, 4, 1, 9) == -2 and bwd(null10, 2, 19, 16, 16, 3, 4, 1, 9) == -2    # CERB_EDTYPE
    for dtype in (1, 2, 3):                                            # fp16 / bf16 / fp64: CERB_EUNSUPPORTED
        assert fwd(full11, 1 << 20, 2, 19, 16, 16, 3, 4, 1, dtype) == -5 and bwd(full10, 2, 19, 16, 16, 3, 4, 1, dtype) == -5
    assert fwd(null11, 0, 0, 19, 16, 16, 3, 4, 1, 0) == 0 and bwd(null10, 0, 19, 16, 16, 3, 4, 1, 0) == 0   # an empty batch
    need = lib.cerberus_rmi_workspace_bytes(2, 19, 16, 16, 4)
    assert need == 8 * (2 * 2 * 3 + 2 * 19 * 243) and fwd(full11, need - 1, *ok) == -1       # workspace one byte short
    assert fwd([one] * 10 + [one + 4], 1 << 20, *ok) == -1                                   # workspace not 8-byte aligned
    for bad in ((-1, 19, 16, 16, 3, 4), (2, 0, 16, 16, 3, 4), (2, 19, 0, 16, 3, 4), (2, 19, 16, -3, 3, 4), (2, 19, 16, 16, 0, 4),
                (2, 19, 16, 16, 3, 0)):
        assert fwd(full11, 1 << 20, *bad, 1, 0) == -1 and bwd(full10, *bad, 1, 0) == -1, bad
    for unsupported in ((2, 19, 16, 16, 2, 4), (2, 19, 16, 16, 5, 4), (2, 19, 16, 16, 3, 9), (2, 19, 7, 16, 3, 4), (2, 19, 16, 2, 3, 1)):
        assert fwd(full11, 1 << 20, *unsupported, 1, 0) == -5 and bwd(full10, *unsupported, 1, 0) == -5, unsupported
    for large in ((70000, 2, 16, 16, 3, 4), (1, 40000, 16, 16, 3, 4), (1, 2, 65536, 32768, 3, 4)):
        assert fwd(full11, 1 << 40, *large, 1, 0) == -6 and bwd(full10, *large, 1, 0) == -6, large
    # with do_rmi off only the logits, the target, bce, state and the workspace are needed
    assert fwd([one, one, one, one] + [None] * 6 + [None], 1 << 20, 2, 19, 16, 16, 3, 4, 0, 0) == -1
    assert bwd([one, one, None] + [one] * 7, 2, 19, 16, 16, 3, 4, 0, 0) == -1


def test_header_and_binding_declare_the_symbols():
    with open(os.path.join(REPO, "include", "cerberus_hip.h")) as f:
        header = f.read()
    for name, nargs in (("cerberus_rmi_workspace_bytes", 5), ("cerberus_rmi_forward", 21), ("cerberus_rmi_backward", 19)):
        m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert "#define CERBERUS_HIP_ABI_VERSION 7 " in header            # additions only
