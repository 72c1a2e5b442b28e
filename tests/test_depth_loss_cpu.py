"""CPU tests of the supervised depth losses (loss_functions/depth_losses.py, csrc/depth_loss.hip): the stock-op formulations
against results of the reference's own InvHuberLoss / ScaleInvariantError / DepthAwareLoss (tests/golden/depth_loss.npz,
written by tools/gen_golden_depth_loss.py), the pyramid class against the sum over levels it is defined as, the classes'
signatures, and the op / C-ABI layer as far as it goes without a GPU.  Bounds of test_seg_loss_cpu.py: value 1e-6 relative,
gradient ``l2_err <= 1e-5``."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cerberusnet_amd as ca
import depth_loss_cases as cases
from cerberusnet_amd import _lib
from cerberusnet_amd import build as cbuild
from cerberusnet_amd import ops
from cerberusnet_amd.loss_functions import depth_losses as D
from conftest import REPO, l2_err

VALUE_TOL = 1e-6
GRAD_TOL = 1e-5
HUBER = [i for i, c in enumerate(cases.GOLDEN_CASES) if c[0] == "InvHuberLoss"]
STOCK_ONLY = [i for i, c in enumerate(cases.GOLDEN_CASES) if c[0] != "InvHuberLoss"]


def test_the_golden_file_holds_the_inputs_of_the_cases(golden):
    g = golden("depth_loss")
    for i, (name, shape, _kwargs, tie) in enumerate(cases.GOLDEN_CASES):
        p, t = cases.golden_inputs(i)
        assert np.array_equal(g["c%d_pred" % i], p) and np.array_equal(g["c%d_gt" % i], t)
        assert p.shape == shape and p.dtype == np.float32 and t.shape == (shape[0],) + shape[2:] and t.dtype == np.float32
        assert shape[0] * shape[2] * shape[3] <= 2 * 12 * 20
        assert 0.25 < float((t == 0).mean()) < 0.55 and 0.05 < float((p <= 0).mean()) < 0.25
        assert float(t[t > 0].min()) >= 0.01 and float(t.max()) < (10.0 if tie else 5.0)
        assert ("c%d_f32_grad" % i in g) == (name == "InvHuberLoss")
        if tie:
            err = np.abs(np.maximum(p[:, 0], 0) - t) * (t > 0)
            assert int((err == err.max()).sum()) == 2 and float(err.max()) == 9.0
    kinds = [(n, k.get("weight", 1.0), k.get("lmda", 1), tie) for n, _, k, tie in cases.GOLDEN_CASES]
    assert ("InvHuberLoss", 0.5, 1, False) in kinds and ("InvHuberLoss", 1.0, 1, True) in kinds
    assert {l for n, _, l, _ in kinds if n == "ScaleInvariantError"} == {1, 0.5} and "DepthAwareLoss" in {n for n, *_ in kinds}


@pytest.mark.parametrize("backend", ["torch", "hip"])       # on CPU tensors 'hip' falls back to the stock ops
@pytest.mark.parametrize("i", HUBER)
def test_inv_huber_stock_formulation_reproduces_the_reference(golden, i, backend):
    g = golden("depth_loss")
    _, _, kwargs, _ = cases.GOLDEN_CASES[i]
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        p = torch.from_numpy(g["c%d_pred" % i]).to(dtype).requires_grad_(True)
        t = torch.from_numpy(g["c%d_gt" % i]).to(dtype)
        loss = ca.InvHuberLoss(backend=backend, **kwargs)({"depth": p}, {"disparity": t})
        grad, = torch.autograd.grad(loss, p)
        ref_v, ref_g = float(g["c%d_%s_value" % (i, tag)]), g["c%d_%s_grad" % (i, tag)]
        print("%d %s %s: value rel %.3e grad l2_err %.3e" % (i, backend, tag, abs(loss.item() - ref_v) / abs(ref_v),
                                                            l2_err(grad.numpy(), ref_g)))
        assert loss.dtype == dtype and loss.shape == ()
        assert abs(loss.item() - ref_v) <= VALUE_TOL * abs(ref_v)
        assert l2_err(grad.numpy(), ref_g) <= GRAD_TOL
        dead = (t <= 0)[:, None] | (p.detach() <= 0)
        assert int(dead.sum()) > 0 and float(grad.abs().mul(dead).max()) == 0.0 and float(np.abs(ref_g).max()) > 0


@pytest.mark.parametrize("i", STOCK_ONLY)
def test_restated_losses_reproduce_the_reference_values(golden, i):
    g = golden("depth_loss")
    name, _, kwargs, _ = cases.GOLDEN_CASES[i]
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        p = torch.from_numpy(g["c%d_pred" % i]).to(dtype).requires_grad_(True)
        t = torch.from_numpy(g["c%d_gt" % i]).to(dtype)
        loss = getattr(ca, name)(**kwargs)({"depth": p}, {"disparity": t})
        ref_v = float(g["c%d_%s_value" % (i, tag)])
        print("%d %s %s: value rel %.3e" % (i, name, tag, abs(loss.item() - ref_v) / abs(ref_v)))
        assert loss.dtype == dtype and loss.shape == ()
        assert abs(loss.item() - ref_v) <= VALUE_TOL * abs(ref_v)
        grad, = torch.autograd.grad(loss, p)                    # the reference raises here
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
        assert float(grad.abs().mul((t <= 0)[:, None]).max()) == 0.0


@pytest.mark.parametrize("name,kwargs", [("ScaleInvariantError", dict()), ("ScaleInvariantError", dict(lmda=0.5, weight=2.0)),
                                         ("DepthAwareLoss", dict()), ("DepthAwareLoss", dict(weight=0.5))])
def test_restated_losses_are_differentiable_and_index_no_boolean_mask(monkeypatch, name, kwargs):
    """float64 ``gradcheck`` at (1,1,3,4), with invalid pixels and non-positive predictions, away from the kinks (prediction 0,
    prediction == ground truth, log == 0).  Boolean-mask indexing goes through ``nonzero`` (a host synchronisation on a GPU):
    both forms of it raise for the duration of the call."""
    p = torch.tensor([[[[0.7, 2.3, -0.5, 1.9], [3.1, 0.4, 2.6, -1.2], [1.4, 4.2, 0.6, 2.9]]]], dtype=torch.float64, requires_grad=True)
    t = torch.tensor([[[1.6, 0.0, 2.2, 3.3], [2.4, 1.7, 0.0, 0.8], [0.0, 3.6, 1.5, 2.1]]], dtype=torch.float64)
    fn = getattr(ca, name)(**kwargs)

    def boom(*_a, **_k):
        raise AssertionError("boolean-mask indexing in a restated loss")
    monkeypatch.setattr(torch.Tensor, "nonzero", boom)
    monkeypatch.setattr(torch, "nonzero", boom)
    value = fn({"depth": p}, {"disparity": t})
    grad, = torch.autograd.grad(value, p)
    monkeypatch.undo()
    assert bool(torch.isfinite(value)) and float(grad.abs().max()) > 0
    assert float(grad[0, 0][t[0] == 0].abs().max()) == 0.0
    assert torch.autograd.gradcheck(lambda x: fn({"depth": x}, {"disparity": t}), (p,), eps=1e-6, atol=1e-7, rtol=1e-5)


def _levels(shape, sizes, seed):
    return [torch.from_numpy(cases.prediction((shape[0], 1) + s, seed + k)) for k, s in enumerate(sizes)]


@pytest.mark.parametrize("backend", ["torch", "hip"])
@pytest.mark.parametrize("sizes", [((24, 40), (12, 20), (6, 10)), ((24, 40), (9, 13), (5, 40))])   # integer ratios; others
def test_pyramid_equals_the_sum_over_levels(backend, sizes):
    shape = (2, 24, 40)
    t = torch.from_numpy(cases.ground_truth(shape, 1900))
    levels = [p.requires_grad_(True) for p in _levels(shape, sizes, 1910)]
    lvl_weights = [1.0, 0.5, 0.25]
    got = ca.InvHuberLossPyr(lvl_weights, weight=0.5, backend=backend)({"depth": levels}, {"disparity": t})
    want = 0
    single = ca.InvHuberLoss(backend=backend)
    for lw, p in zip(lvl_weights, levels):
        resized = F.interpolate(t.unsqueeze(1), tuple(p.shape[2:]), mode="nearest").squeeze(1)
        want = want + lw * single({"depth": p}, {"disparity": resized})
    want = 0.5 * want
    assert got.shape == () and abs(got.item() - want.item()) <= VALUE_TOL * abs(want.item()) and got.item() > 0
    for a, b in zip(torch.autograd.grad(got, levels), torch.autograd.grad(want, levels)):
        assert l2_err(a.numpy(), b.numpy()) <= GRAD_TOL and float(b.abs().max()) > 0


def test_inv_huber_loss_wrapper_on_cpu():
    p = torch.from_numpy(cases.prediction((2, 1, 6, 8), 1920))
    t = torch.from_numpy(cases.ground_truth((2, 6, 8), 1921))
    want = ca.InvHuberLoss(backend="torch")({"depth": p}, {"disparity": t})
    assert torch.equal(ca.inv_huber_loss(p, t), want)
    assert torch.equal(ca.inv_huber_loss(p[:, 0], t), want) and torch.equal(ca.inv_huber_loss(p, t[:, None]), want)
    big = torch.from_numpy(cases.ground_truth((2, 12, 24), 1922))
    assert torch.equal(ca.inv_huber_loss(p, big), ca.inv_huber_loss(p, big[:, ::2, ::3]))        # nearest, integer ratios
    with pytest.raises(ValueError, match="Invalid prediction shape"):
        ca.inv_huber_loss(torch.zeros(2, 3, 6, 8), t)
    assert list(inspect.signature(ca.inv_huber_loss).parameters) == ["pred", "gt"]


# (name, default) of the reference's constructor parameters: depth_losses.py:17, :43, :68, :91
REFERENCE_PARAMS = {"InvHuberLoss": [("weight", 1.0)], "InvHuberLossPyr": [("lvl_weights", inspect.Parameter.empty), ("weight", 1.0)],
                    "ScaleInvariantError": [("weight", 1.0), ("lmda", 1)], "DepthAwareLoss": [("weight", 1.0)]}


def test_class_signatures_match_the_reference():
    # `backend` comes after the reference's parameters where there is a HIP path
    for name, has_backend in (("InvHuberLoss", True), ("InvHuberLossPyr", True), ("ScaleInvariantError", False),
                              ("DepthAwareLoss", False)):
        cls, params = getattr(ca, name), REFERENCE_PARAMS[name]
        got = list(inspect.signature(cls.__init__).parameters.values())[1:]
        assert [(p.name, p.default) for p in got[:len(params)]] == params
        if has_backend:
            assert (got[len(params)].name, got[len(params)].default) == ("backend", "hip")
        assert got[-1].kind == inspect.Parameter.VAR_KEYWORD and len(got) == len(params) + 1 + has_backend
        assert list(inspect.signature(cls.forward).parameters) == ["self", "predictions", "targets"]
        args = ([1.0],) if name == "InvHuberLossPyr" else ()
        fn = cls(*args, unknown_keyword=3)                             # **kwargs swallows what a config file carries
        assert fn.weight == 1.0 and len(fn.state_dict()) == 0
        if has_backend:
            with pytest.raises(ValueError):
                cls(*args, backend="cuda")
        with pytest.raises(AssertionError):
            fn({"seg": torch.zeros(1)}, {"disparity": torch.zeros(1)})
        with pytest.raises(AssertionError):
            fn({"depth": torch.zeros(1)}, {"depth": torch.zeros(1)})
    assert ca.ScaleInvariantError().lmda == 1 and ca.InvHuberLossPyr([1, 2]).lvl_weights == [1, 2]
    assert ca.InvHuberLoss().backend == ca.InvHuberLossPyr([1]).backend == "hip"


def test_names_are_exported_and_the_source_is_built():
    names = ["inv_huber_loss", "InvHuberLoss", "InvHuberLossPyr", "ScaleInvariantError", "DepthAwareLoss"]
    for mod in (D, ca.loss_functions, ca):
        assert set(names) <= set(mod.__all__)
        for n in names:
            assert getattr(mod, n) is getattr(D, n)
    assert "depth_loss.hip" in cbuild.SOURCES and "depth_loss.hip" in cbuild.EXPERIMENT_SOURCES


def test_op_schemas():
    s = lambda n: str(getattr(torch.ops.cerberus, n).default._schema)
    assert s("inv_huber") == "cerberus::inv_huber(Tensor pred, Tensor gt) -> (Tensor loss, Tensor state)"
    assert s("inv_huber_backward") == "cerberus::inv_huber_backward(Tensor pred, Tensor gt, Tensor state, Tensor grad_loss) -> Tensor"


def test_meta_implementations_give_the_shapes():
    m = lambda *shape: torch.empty(*shape, device="meta", dtype=torch.float32)
    for p, t in ((m(2, 1, 5, 7), m(2, 5, 7)), (m(2, 5, 7), m(2, 10, 21))):
        loss, state = torch.ops.cerberus.inv_huber(p, t)
        assert loss.shape == () and state.shape == (4,)
        assert all(o.dtype == torch.float32 and o.device.type == "meta" for o in (loss, state))
        g = torch.ops.cerberus.inv_huber_backward(p, t, state, loss)
        assert g.shape == p.shape and g.dtype == torch.float32 and g.device.type == "meta"


def test_cpu_tensors_through_the_raw_ops_raise():
    p, t = torch.ones(1, 1, 4, 4), torch.ones(1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.inv_huber(p, t)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.inv_huber(p.clone().requires_grad_(True), t)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.inv_huber_backward(p, t, torch.zeros(4), torch.ones(()))


def test_workspace_bytes_in_python_equal_the_library():
    lib = _lib.get()
    for shape in ((1, 1, 1), (1, 1, 4), (2, 37, 53), (1, 32, 32), (1, 32, 33), (2, 128, 256), (4, 512, 1024), (2, 1024, 2048),
                  (7, 1025, 31), (0, 8, 8), (-1, 8, 8), (1, 0, 8), (4, 32768, 32768)):
        assert ops._inv_huber_workspace_bytes(*shape) == lib.cerberus_inv_huber_workspace_bytes(*shape), shape
    assert ops._inv_huber_workspace_bytes(1, 32, 32) == 4096 + 12 and ops._inv_huber_workspace_bytes(1, 32, 33) == 4096 + 24
    assert ops._inv_huber_workspace_bytes(4, 32768, 32768) == 0


def test_argument_rejection_without_gpu():
    lib = _lib.get()
    one = 4096                                                         # never dereferenced: every call below returns before a launch
    fwd = lambda ptrs, ws_bytes, B, h, w, H, W, dtype: lib.cerberus_inv_huber_forward(*ptrs, ws_bytes, B, h, w, H, W, dtype, None)
    bwd = lambda ptrs, B, h, w, H, W, dtype: lib.cerberus_inv_huber_backward(*ptrs, B, h, w, H, W, dtype, None)
    null5, full5 = [None] * 5, [one] * 5
    assert fwd(null5, 1 << 20, 2, 8, 8, 8, 8, 0) == -1                # CERB_EINVAL: null pointers
    for k in range(5):
        assert fwd(full5[:k] + [None] + full5[k + 1:], 1 << 20, 2, 8, 8, 8, 8, 0) == -1, k
        assert bwd(full5[:k] + [None] + full5[k + 1:], 2, 8, 8, 8, 8, 0) == -1, k
    assert fwd(null5, 1 << 20, 2, 8, 8, 8, 8, 9) == -2                # CERB_EDTYPE: unknown dtype
    assert bwd(null5, 2, 8, 8, 8, 8, 9) == -2
    for dtype in (1, 2, 3):                                            # fp16 / bf16 / fp64: CERB_EUNSUPPORTED
        assert fwd(full5, 1 << 20, 2, 8, 8, 8, 8, dtype) == -5
        assert bwd(full5, 2, 8, 8, 8, 8, dtype) == -5
    assert fwd(null5, 0, 0, 8, 8, 8, 8, 0) == 0                       # an empty batch: 0, no launch
    assert bwd(null5, 0, 8, 8, 8, 8, 0) == 0
    need = lib.cerberus_inv_huber_workspace_bytes(2, 8, 8)
    assert need == 4096 + 12
    assert fwd(full5, need - 1, 2, 8, 8, 8, 8, 0) == -1               # workspace one byte short
    assert fwd(full5[:4] + [one + 4], 1 << 20, 2, 8, 8, 8, 8, 0) == -1     # workspace not 16-byte aligned
    for bad in ((-1, 8, 8, 8, 8), (2, 0, 8, 8, 8), (2, 8, -3, 8, 8), (2, 8, 8, 0, 8), (2, 8, 8, 8, -8)):
        assert fwd(full5, 1 << 20, *bad, 0) == -1 and bwd(full5, *bad, 0) == -1, bad
    for ratio in ((2, 8, 8, 12, 8), (2, 8, 8, 8, 20), (2, 8, 8, 4, 8)):    # a ground-truth size the prediction's does not divide
        assert fwd(full5, 1 << 20, *ratio, 0) == -5 and bwd(full5, *ratio, 0) == -5, ratio
    assert fwd(full5, 1 << 40, 4, 32768, 32768, 32768, 32768, 0) == -6    # CERB_ETOOLARGE: the pixel count does not fit an int
    assert bwd(full5, 4, 32768, 32768, 32768, 32768, 0) == -6


def test_header_and_binding_declare_the_symbols():
    with open(os.path.join(REPO, "include", "cerberus_hip.h")) as f:
        header = f.read()
    for name, nargs in (("cerberus_inv_huber_workspace_bytes", 3), ("cerberus_inv_huber_forward", 13),
                        ("cerberus_inv_huber_backward", 12)):
        m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert "#define CERBERUS_HIP_ABI_VERSION 7 " in header            # additions only
