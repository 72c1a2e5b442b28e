"""CPU tests of the segmentation losses (loss_functions/seg_losses.py, csrc/seg_loss.hip): the stock-op formulations against
results of the reference's own FocalLoss2D / SegCrossEntropy (tests/golden/seg_loss.npz, written by
tools/gen_golden_seg_loss.py), the dynamic class weights against the reference's ``unique`` formula, the classes' signatures,
and the op / C-ABI layer as far as it goes without a GPU.  Bounds of test_depth_recon_cpu.py: value 1e-6 relative, gradient
``l2_err <= 1e-5``."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import seg_loss_cases as cases
from cerberusnet_amd import _lib
from cerberusnet_amd import build as cbuild
from cerberusnet_amd import ops
from cerberusnet_amd.loss_functions import seg_losses as S
from conftest import REPO, l2_err

VALUE_TOL = 1e-6
GRAD_TOL = 1e-5


def test_the_golden_file_holds_the_inputs_of_the_cases(golden):
    g = golden("seg_loss")
    for i, (_, shape, kwargs, four_d) in enumerate(cases.GOLDEN_CASES):
        x, t = cases.golden_inputs(i)
        assert np.array_equal(g["c%d_logits" % i], x) and np.array_equal(g["c%d_target" % i], t)
        assert x.shape == shape and x.dtype == np.float32 and -4.0 <= x.min() and x.max() < 4.0
        assert t.dtype == np.int64 and t.shape == ((shape[0], 1) + shape[2:] if four_d else (shape[0],) + shape[2:])
        share = float((t == kwargs["ignore_index"]).mean())
        assert 0.08 < share < 0.25, share
        counts = np.bincount(t[t != kwargs["ignore_index"]], minlength=shape[1])
        # skewed: class 0 holds sqrt(1/C) of the labels, class C-1 holds 1 - sqrt(1 - 1/C), 5 times fewer at C = 7
        assert counts[0] > 2 * max(1, counts[-1])
    kinds = {(n, k["dynamic_weights"], k.get("gamma"), k["ignore_index"]) for n, _, k, _ in cases.GOLDEN_CASES}
    assert {n for n, *_ in kinds} == {"FocalLoss2D", "SegCrossEntropy"}
    assert {d for _, d, *_ in kinds} == {True, False} and {g_ for _, _, g_, _ in kinds} == {2.0, 0.5, None}
    assert {i for *_, i in kinds} == {255, -1} and any(f for *_, f in cases.GOLDEN_CASES)


@pytest.mark.parametrize("backend", ["torch", "hip"])       # on CPU tensors 'hip' falls back to the stock ops
@pytest.mark.parametrize("i", range(len(cases.GOLDEN_CASES)))
def test_stock_formulation_reproduces_the_reference(golden, i, backend):
    g = golden("seg_loss")
    name, _, kwargs, _ = cases.GOLDEN_CASES[i]
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        x = torch.from_numpy(g["c%d_logits" % i]).to(dtype).requires_grad_(True)
        loss = getattr(ca, name)(backend=backend, **kwargs)({"seg": x}, {"seg": torch.from_numpy(g["c%d_target" % i])})
        grad, = torch.autograd.grad(loss, x)
        ref_v, ref_g = float(g["c%d_%s_value" % (i, tag)]), g["c%d_%s_grad" % (i, tag)]
        print("%d %s %s %s: value rel %.3e grad l2_err %.3e" % (i, name, backend, tag, abs(loss.item() - ref_v) / abs(ref_v),
                                                                l2_err(grad.numpy(), ref_g)))
        assert loss.dtype == dtype and loss.shape == ()
        assert abs(loss.item() - ref_v) <= VALUE_TOL * abs(ref_v)
        assert l2_err(grad.numpy(), ref_g) <= GRAD_TOL
        assert float(np.abs(ref_g).max()) > 0
        if kwargs["ignore_index"] in g["c%d_target" % i]:
            dead = torch.from_numpy(g["c%d_target" % i]).reshape(x.shape[0], 1, *x.shape[2:]) == kwargs["ignore_index"]
            assert float(grad.abs().mul(dead).max()) == 0.0


def _reference_weights(target, num_classes, ignore_index, scale_factor):
    weights = torch.ones(num_classes)
    class_ids, counts = target[target != ignore_index].unique(return_counts=True)
    weights[class_ids] = scale_factor / (scale_factor + counts / float(target.nelement()))
    return weights


@pytest.mark.parametrize("ignore_index", [255, -1])
@pytest.mark.parametrize("shape,scale", [((2, 19, 9, 20), 0.125), ((1, 7, 16, 20), 0.25), ((3, 150, 11, 13), 0.125)])
def test_class_balance_weights_equal_the_reference_formula(shape, scale, ignore_index):
    """CPU tensors take the wrapper's stock form, which is the ``unique`` chain restated above: this pins the surface (dtype,
    shape, (B,1,H,W) targets, defaults) and that the restatement stays the reference's.  The independent check of the
    histogram path is on the GPU: ``_check_weights`` in tests/test_seg_loss_gpu.py, within 3 fp32 rounding units."""
    t = torch.from_numpy(cases.labels(shape, 800, ignore_index))
    got = ca.class_balance_weights(t, shape[1], ignore_index, scale)
    want = _reference_weights(t, shape[1], ignore_index, scale)
    assert got.dtype == torch.float32 and got.shape == (shape[1],)
    assert torch.equal(got, want)
    assert float(want.min()) < 1.0 and (shape[1] < 100 or float(want.max()) == 1.0)       # present and absent classes
    assert torch.equal(ca.class_balance_weights(t[:, None], shape[1], ignore_index, scale), want)
    sig = inspect.signature(ca.class_balance_weights)
    assert [(p.name, p.default) for p in sig.parameters.values()][2:] == [("ignore_index", 255), ("scale_factor", 0.125)]


def test_seg_cross_entropy_stock_path_on_cpu():
    x = torch.from_numpy(cases.logits((2, 5, 6, 7), 810)).requires_grad_(True)
    t = torch.from_numpy(cases.labels((2, 5, 6, 7), 811, 255))
    w = torch.tensor([1.0, 0.5, 0.0, 2.0, 1.0])
    ce = torch.nn.functional.cross_entropy(x, t, weight=w, ignore_index=255)
    assert torch.equal(ca.seg_cross_entropy(x, t, w), ce)                                 # gamma 0: exactly the mean
    assert torch.equal(ca.seg_cross_entropy(x, t, w, 255, 2.0), torch.pow(1 - torch.exp(-ce), 2.0) * ce)
    assert torch.equal(ca.seg_cross_entropy(x, t), torch.nn.functional.cross_entropy(x, t, ignore_index=255))
    sig = inspect.signature(ca.seg_cross_entropy)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("logits", inspect.Parameter.empty), ("target", inspect.Parameter.empty), ("weight", None), ("ignore_index", 255),
        ("gamma", 0.0)]
    all_ignored = torch.full_like(t, 255)
    assert bool(torch.isnan(ca.seg_cross_entropy(x, all_ignored)))
    # a weight that asks for a gradient gets one: F.cross_entropy refuses such a weight, so the same mean is written out
    wg = w.clone().requires_grad_(True)
    v = ca.seg_cross_entropy(x, t, wg, 255, 2.0)
    gx, gw = torch.autograd.grad(v, (x, wg))
    want = torch.pow(1 - torch.exp(-ce), 2.0) * ce
    assert abs(v.item() - want.item()) <= VALUE_TOL * want.item()
    assert l2_err(gx.numpy(), torch.autograd.grad(want, x)[0].numpy()) <= GRAD_TOL
    w64 = w.double().requires_grad_(True)                                  # the weight's gradient against float64 differences
    v64 = ca.seg_cross_entropy(x.detach().double(), t, w64, 255, 2.0)
    assert l2_err(gw.numpy(), torch.autograd.grad(v64, w64)[0].numpy()) <= GRAD_TOL and float(gw.abs().max()) > 0


def test_class_signatures_match_the_reference():
    # seg_losses.py:125-126 and :160-161; `backend` comes after the reference's parameters
    want = {ca.FocalLoss2D: [("weight", 1.0), ("gamma", 2.0), ("ignore_index", 255), ("dynamic_weights", False),
                             ("scale_factor", 0.125)],
            ca.SegCrossEntropy: [("weight", 1.0), ("ignore_index", 255), ("dynamic_weights", False), ("scale_factor", 0.125)]}
    for cls, params in want.items():
        got = list(inspect.signature(cls.__init__).parameters.values())[1:]
        assert [(p.name, p.default) for p in got[:len(params)]] == params
        assert (got[len(params)].name, got[len(params)].default) == ("backend", "hip")
        assert got[-1].kind == inspect.Parameter.VAR_KEYWORD and len(got) == len(params) + 2
        assert list(inspect.signature(cls.forward).parameters) == ["self", "predictions", "targets"]
        fn = cls(unknown_keyword=3)                                    # **kwargs swallows what a config file carries
        assert fn.backend == "hip" and fn.weight == 1.0 and len(fn.state_dict()) == 0
        with pytest.raises(ValueError):
            cls(backend="cuda")
        with pytest.raises(AssertionError):
            fn({"depth": torch.zeros(1)}, {"seg": torch.zeros(1)})
        with pytest.raises(ValueError, match="Invalid ground truth shape"):
            fn({"seg": torch.zeros(1, 3, 4, 4)}, {"seg": torch.zeros(1, 2, 4, 4, dtype=torch.int64)})
    assert ca.FocalLoss2D().gamma == 2.0 and ca.SegCrossEntropy().gamma == 0.0


def test_names_are_exported_and_the_source_is_built():
    names = ["seg_cross_entropy", "class_balance_weights", "FocalLoss2D", "SegCrossEntropy"]
    assert S.__all__ == names
    for mod in (ca.loss_functions, ca):
        assert set(names) <= set(mod.__all__)
        for n in names:
            assert getattr(mod, n) is getattr(S, n)
    assert "seg_loss.hip" in cbuild.SOURCES and "seg_loss.hip" in cbuild.EXPERIMENT_SOURCES


def test_op_schemas():
    s = lambda n: str(getattr(torch.ops.cerberus, n).default._schema)
    assert s("seg_cross_entropy") == ("cerberus::seg_cross_entropy(Tensor logits, Tensor target, Tensor weight, int ignore_index, "
                                      "float gamma) -> (Tensor loss, Tensor lse, Tensor state)")
    assert s("seg_cross_entropy_backward") == ("cerberus::seg_cross_entropy_backward(Tensor logits, Tensor target, Tensor weight, "
                                               "Tensor lse, Tensor state, Tensor grad_loss, int ignore_index) -> Tensor")
    assert s("class_histogram") == "cerberus::class_histogram(Tensor target, int num_classes, int ignore_index) -> Tensor"


def test_meta_implementations_give_the_shapes():
    m = lambda *shape, dtype=torch.float32: torch.empty(*shape, device="meta", dtype=dtype)
    x, t, w = m(2, 19, 5, 7), m(2, 5, 7, dtype=torch.int64), m(19)
    loss, lse, state = torch.ops.cerberus.seg_cross_entropy(x, t, w, 255, 2.0)
    assert loss.shape == () and lse.shape == (2, 5, 7) and state.shape == (4,)
    assert all(o.dtype == torch.float32 and o.device.type == "meta" for o in (loss, lse, state))
    g = torch.ops.cerberus.seg_cross_entropy_backward(x, t, w, lse, state, loss, 255)
    assert g.shape == x.shape and g.dtype == torch.float32 and g.device.type == "meta"
    h = torch.ops.cerberus.class_histogram(t, 19, 255)
    assert h.shape == (19,) and h.dtype == torch.int64 and h.device.type == "meta"


def test_cpu_tensors_through_the_raw_ops_raise():
    x, t, w = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.seg_cross_entropy(x, t, w, 255, 0.0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.seg_cross_entropy(x.requires_grad_(True), t, w, 255, 0.0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.seg_cross_entropy_backward(x.detach(), t, w, torch.zeros(1, 4, 4), torch.zeros(4), torch.ones(()), 255)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.class_histogram(t, 3, 255)


def test_workspace_bytes_in_python_equal_the_library():
    lib = _lib.get()
    for shape in ((1, 1, 1), (1, 1, 4), (2, 37, 53), (1, 32, 32), (1, 32, 33), (2, 128, 256), (4, 512, 1024), (2, 1024, 2048),
                  (7, 1025, 31), (0, 8, 8), (-1, 8, 8), (1, 0, 8), (4, 32768, 32768)):
        assert ops._seg_workspace_bytes(*shape) == lib.cerberus_seg_cross_entropy_workspace_bytes(*shape), shape
    assert ops._seg_workspace_bytes(1, 32, 32) == 8 and ops._seg_workspace_bytes(1, 32, 33) == 16
    assert ops._seg_workspace_bytes(4, 32768, 32768) == 0


def test_argument_rejection_without_gpu():
    lib = _lib.get()
    one = 4096                                                         # never dereferenced: every call below returns before a launch
    fwd = lambda ptrs, ws_bytes, B, C, H, W, gamma, dtype: lib.cerberus_seg_cross_entropy_forward(
        *ptrs, ws_bytes, B, C, H, W, -1, gamma, dtype, None)
    bwd = lambda ptrs, B, C, H, W, dtype: lib.cerberus_seg_cross_entropy_backward(*ptrs, B, C, H, W, 255, dtype, None)
    null7, full7 = [None] * 7, [one] * 7
    assert fwd(null7, 1 << 20, 2, 19, 8, 8, 2.0, 0) == -1             # CERB_EINVAL: null pointers
    for k in range(7):
        assert fwd(full7[:k] + [None] + full7[k + 1:], 1 << 20, 2, 19, 8, 8, 2.0, 0) == -1, k
        assert bwd(full7[:k] + [None] + full7[k + 1:], 2, 19, 8, 8, 0) == -1, k
    assert fwd(null7, 1 << 20, 2, 19, 8, 8, 2.0, 9) == -2             # CERB_EDTYPE: unknown dtype
    assert bwd(null7, 2, 19, 8, 8, 9) == -2
    for dtype in (1, 2, 3):                                            # fp16 / bf16 / fp64: CERB_EUNSUPPORTED
        assert fwd(full7, 1 << 20, 2, 19, 8, 8, 2.0, dtype) == -5
        assert bwd(full7, 2, 19, 8, 8, dtype) == -5
    assert fwd(null7, 0, 0, 19, 8, 8, 2.0, 0) == 0                    # an empty batch: 0, no launch
    assert bwd(null7, 0, 19, 8, 8, 0) == 0
    assert fwd(full7, 7, 2, 19, 8, 8, 2.0, 0) == -1                   # workspace one byte short
    assert lib.cerberus_seg_cross_entropy_workspace_bytes(2, 8, 8) == 8
    for bad in ((-1, 19, 8, 8), (2, 1, 8, 8), (2, 19, 0, 8), (2, 19, 8, -3)):
        assert fwd(full7, 1 << 20, *bad, 2.0, 0) == -1 and bwd(full7, *bad, 0) == -1, bad
    assert fwd(full7, 1 << 20, 2, 19, 8, 8, -0.5, 0) == -1 and fwd(full7, 1 << 20, 2, 19, 8, 8, float("nan"), 0) == -1
    assert fwd(full7, 1 << 40, 4, 19, 32768, 32768, 2.0, 0) == -6     # CERB_ETOOLARGE: the pixel count does not fit an int
    hist = lambda t, c, n, classes: lib.cerberus_class_histogram(t, c, n, classes, 255, None)
    assert hist(None, None, 64, 19) == -1 and hist(one, None, 64, 19) == -1 and hist(None, one, 64, 19) == -1
    assert hist(one, one, -1, 19) == -1 and hist(one, one, 64, 0) == -1
    assert hist(None, None, 0, 19) == 0                                # no labels: 0, no launch
    assert hist(None, None, 64, ops.HISTOGRAM_MAX_CLASSES) == -1 and hist(one, one, 64, ops.HISTOGRAM_MAX_CLASSES + 1) == -5
    assert ops.HISTOGRAM_MAX_CLASSES >= 1024


def test_header_and_binding_declare_the_symbols():
    with open(os.path.join(REPO, "include", "cerberus_hip.h")) as f:
        header = f.read()
    for name, nargs in (("cerberus_seg_cross_entropy_workspace_bytes", 3), ("cerberus_seg_cross_entropy_forward", 16),
                        ("cerberus_seg_cross_entropy_backward", 14), ("cerberus_class_histogram", 6)):
        m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert "#define CERBERUS_HIP_ABI_VERSION 7 " in header            # additions only
