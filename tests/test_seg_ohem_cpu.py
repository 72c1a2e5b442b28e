"""CPU tests of the OHEM cross-entropy (loss_functions/ohem_losses.py, csrc/seg_ohem.hip): the stock-op restatement against
results of the reference's own SoftmaxCrossEntropyOHEMLoss / MixSoftmaxCrossEntropyOHEMLoss (tests/golden/seg_ohem.npz, written
by tools/gen_golden_seg_ohem.py) -- kept masks exactly, value 1e-6 relative and gradient ``l2_err <= 1e-5`` as
tests/test_seg_loss_cpu.py --, the classes' signatures, the op / C-ABI layer as far as it goes without a GPU, the case table
of tests/seg_ohem_cases.py against the constants the kernels export, and a numpy model of the digit-wise select."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import seg_ohem_cases as oc
from cerberusnet_amd import _lib
from cerberusnet_amd import build as cbuild
from cerberusnet_amd import ops
from cerberusnet_amd.loss_functions import ohem_losses as O
from cerberusnet_amd.loss_functions import seg_losses as S
from conftest import REPO, l2_err

VALUE_TOL = 1e-6
GRAD_TOL = 1e-5
IGNORE = oc.IGNORE

# what each row is in the table for, keyed by the row itself
PURPOSE = {
    ((2, 19, 37, 53), 0.7, 256, True): ["scalar", "branch: thresh", "image boundary inside a chunk"],
    ((2, 19, 37, 53), 0.7, 2000, True): ["scalar", "branch: kth"],
    ((2, 19, 8, 64), 0.7, 600, True): ["vector", "branch: kth"],
    ((2, 2, 129, 1028), 0.7, 150000, False): ["vector", "branch: kth", "last digit decides", "more than 256 chunks",
                                              "image boundary inside a chunk"],
    ((1, 3, 601, 1023), 0.7, 400000, False): ["scalar", "branch: kth", "last digit decides", "more than 512 chunks"],
    ((1, 3, 601, 1023), 0.9, 100, False): ["branch: thresh", "more than 512 chunks"],
    ((2, 19, 8, 64), 0.7, 10 ** 6, True): ["branch: keep all"],
    ((2, 19, 8, 64), 0.7, 0, True): ["branch: thresh"],
}


def _t(a):
    return torch.from_numpy(np.array(a))


# ---- the stock restatement against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["torch", "hip"])       # on CPU tensors 'hip' falls back to the stock ops
@pytest.mark.parametrize("i", range(len(oc.GOLDEN_CASES)))
def test_stock_restatement_reproduces_the_reference(golden, i, backend):
    g = golden("seg_ohem")
    name, shape, kwargs, nheads = oc.GOLDEN_CASES[i]
    weights = g["c%d_weight" % i] if kwargs["use_weight"] else None
    assert g["c%d_weight" % i].shape == (shape[1],) and (kwargs["use_weight"] or (g["c%d_weight" % i] == 1).all())
    fn = getattr(ca, name)(backend=backend, class_weights=weights, **kwargs)
    target = _t(oc.inputs(shape)[1])
    heads = [_t(oc.inputs(shape, h)[0]).requires_grad_(True) for h in range(nheads)]
    loss = fn(heads if nheads > 1 else heads[0], target)
    grads = torch.autograd.grad(loss, heads)
    ref_v = float(g["c%d_value" % i])
    print("%d %s %s: value rel %.3e" % (i, name, backend, abs(loss.item() - ref_v) / abs(ref_v)))
    assert loss.dtype == torch.float32 and loss.shape == ()
    assert abs(loss.item() - ref_v) <= VALUE_TOL * abs(ref_v)
    ignore = kwargs.get("ignore_label", kwargs.get("ignore_index"))
    for h in range(nheads):
        kept_ref = g["c%d_kept" % i][h].astype(bool)
        kept, threshold, num_valid = O._ohem_selection(heads[h], target, ignore, kwargs["thresh"], kwargs["min_kept"])
        assert np.array_equal(kept.numpy(), kept_ref)                            # exactly the reference's rewritten target
        assert int(num_valid) == int((target != ignore).sum()) and int(kept.sum()) == kept_ref.sum() > 0
        assert l2_err(grads[h].numpy(), g["c%d_grad" % i][h]) <= GRAD_TOL and float(np.abs(g["c%d_grad" % i][h]).max()) > 0
        assert float(grads[h].abs().sum(1)[~kept].max()) == 0.0                  # exact zeros outside the kept set
    stats = ca.seg_ohem_cross_entropy(heads[0], target, None if weights is None else _t(weights), ignore, kwargs["thresh"],
                                      kwargs["min_kept"], return_stats=True)
    assert len(stats) == 4 and int(stats[3]) == g["c%d_kept" % i][0].sum()
    assert bool(torch.isinf(stats[1])) == (kwargs["min_kept"] >= int(stats[2]))


def test_the_golden_cases_are_those_of_the_issue():
    kinds = {(n, k["use_weight"], k["min_kept"]) for n, _, k, _ in oc.GOLDEN_CASES}
    assert {n for n, *_ in kinds} == {"SoftmaxCrossEntropyOHEMLoss", "MixSoftmaxCrossEntropyOHEMLoss"}
    assert {u for _, u, _ in kinds} == {True, False} and {0, 10 ** 6} < {m for *_, m in kinds}
    assert any(nheads > 1 and k.get("aux") for _, _, k, nheads in oc.GOLDEN_CASES)
    small = [(shape, k["thresh"], k["min_kept"], True) for n, shape, k, _ in oc.GOLDEN_CASES]
    assert all(r in small for r in oc.ROWS if r[3])
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "seg_ohem.npz")) < 1 << 20


def test_stock_restatement_branches_and_nan():
    """The table of the selection on a case small enough to read: 6 valid pixels with probabilities known in advance."""
    p = np.array([0.1, 0.2, 0.5, 0.8, 0.9, 0.95], dtype=np.float64)
    x = np.zeros((1, 2, 1, 8), dtype=np.float32)
    x[0, 0, 0, :6] = np.log(p / (1 - p))                                         # softmax over two classes: class 0 has p
    t = np.zeros((1, 1, 8), dtype=np.int64)
    t[0, 0, 6], t[0, 0, 7] = IGNORE, 5                                           # an ignored pixel and a label outside [0, C)
    xt, tt = torch.from_numpy(x), torch.from_numpy(t)
    sel = lambda thresh, k, xx=xt: O._ohem_selection(xx, tt, IGNORE, thresh, k)
    kept, th, nv = sel(0.7, 0)
    assert kept[0, 0].tolist() == [True] * 3 + [False] * 5 and float(th) == np.float32(0.7) and int(nv) == 6
    kept, th, _ = sel(0.7, 2)                                                    # kth = 0.2 is below thresh
    assert int(kept.sum()) == 3 and float(th) == np.float32(0.7)
    kept, th, _ = sel(0.7, 5)                                                    # kth = 0.9
    assert kept[0, 0].tolist() == [True] * 5 + [False] * 3 and abs(float(th) - 0.9) < 1e-6
    for k in (6, 7, 10 ** 9):                                                    # min_kept >= num_valid: everything valid, +inf
        kept, th, _ = sel(0.7, k)
        assert kept[0, 0].tolist() == [True] * 6 + [False] * 2 and float(th) == float("inf")
    kept, th, _ = sel(0.01, -4)
    assert int(kept.sum()) == 0 and float(th) == np.float32(0.01)
    xn = xt.clone()
    xn[0, 1, 0, 1] = float("nan")                                                # pixel 1's probability is NaN: above every number
    kept, th, _ = sel(0.7, 4, xn)                                                # the 4th smallest of {.1 .5 .8 .9 .95 NaN} is 0.9
    assert kept[0, 0].tolist() == [True, False, True, True, True, False, False, False] and abs(float(th) - 0.9) < 1e-6
    kept, th, _ = sel(0.7, 5, xn)
    assert int(kept.sum()) == 5 and abs(float(th) - 0.95) < 1e-6
    kept, th, _ = sel(0.7, 6, xn)                                                # min_kept >= num_valid keeps the NaN pixel too
    assert kept[0, 0, 1] and int(kept.sum()) == 6
    t2, xn2 = tt.clone(), xn.clone()
    t2[0, 0, 7], xn2[0, 0, 0, 7] = 0, float("nan")                               # 7 valid, two of them NaN: rank 6 is a NaN -> thresh
    kept, th, nv = O._ohem_selection(xn2, t2, IGNORE, 0.7, 6)
    assert int(nv) == 7 and float(th) == np.float32(0.7) and kept[0, 0].tolist() == [True, False, True] + [False] * 5
    assert bool(torch.isnan(ca.seg_ohem_cross_entropy(xt, torch.full_like(tt, IGNORE), None, IGNORE, 0.7, 3)))      # 0 / 0
    # the loss follows the logits: 16-bit, a single class, a weight that wants a gradient
    x4, t4 = _t(oc.inputs((2, 19, 8, 64))[0]), _t(oc.inputs((2, 19, 8, 64))[1])
    w = _t(oc.class_weights(19))
    base = ca.seg_ohem_cross_entropy(x4, t4, w, IGNORE, 0.7, 600)
    assert ca.seg_ohem_cross_entropy(x4.bfloat16(), t4, w, IGNORE, 0.7, 600).dtype == torch.bfloat16
    assert float(ca.seg_ohem_cross_entropy(x4[:, :1], t4.clamp(max=0), None, IGNORE, 0.7, 600)) == 0.0
    wg = w.clone().requires_grad_(True)
    v = ca.seg_ohem_cross_entropy(x4, t4, wg, IGNORE, 0.7, 600)
    gw, = torch.autograd.grad(v, wg)
    assert abs(float(v.detach()) - float(base)) <= VALUE_TOL * float(base) and float(gw.abs().max()) > 0


# ---- signatures ------------------------------------------------------------------------------------------------------------------
def test_class_signatures_match_the_reference():
    # seg_losses.py:17, :41 and :99; `backend` and `class_weights` come after the reference's parameters
    want = {ca.MixSoftmaxCrossEntropyLoss: [("aux", True), ("aux_weight", 0.2), ("ignore_label", 255)],
            ca.SoftmaxCrossEntropyOHEMLoss: [("ignore_label", -1), ("thresh", 0.7), ("min_kept", 256), ("use_weight", True),
                                             ("backend", "hip"), ("class_weights", None)],
            ca.MixSoftmaxCrossEntropyOHEMLoss: [("aux", False), ("aux_weight", 0.2), ("ignore_index", 255)]}
    for cls, params in want.items():
        got = list(inspect.signature(cls.__init__).parameters.values())[1:]
        assert [(p.name, p.default) for p in got[:len(params)]] == params
        assert got[-1].kind == inspect.Parameter.VAR_KEYWORD and len(got) == len(params) + 1
    assert list(inspect.signature(ca.SoftmaxCrossEntropyOHEMLoss.forward).parameters) == ["self", "predict", "target"]
    assert list(inspect.signature(ca.MixSoftmaxCrossEntropyOHEMLoss.forward).parameters) == ["self", "preds", "target"]
    assert list(inspect.signature(ca.MixSoftmaxCrossEntropyLoss.forward).parameters) == ["self", "preds", "target"]
    sig = inspect.signature(ca.seg_ohem_cross_entropy)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [
        ("weight", None), ("ignore_index", -1), ("thresh", 0.7), ("min_kept", 256), ("return_stats", False)]
    with pytest.raises(ValueError, match="class_weights"):
        ca.SoftmaxCrossEntropyOHEMLoss()                                         # the reference's table is not copied
    with pytest.raises(ValueError, match="class_weights"):
        ca.MixSoftmaxCrossEntropyOHEMLoss(ignore_index=255)
    with pytest.raises(ValueError, match="backend"):
        ca.SoftmaxCrossEntropyOHEMLoss(use_weight=False, backend="cuda")
    fn = ca.MixSoftmaxCrossEntropyOHEMLoss(use_weight=False, unknown_keyword=3)
    assert (fn.ignore_label, fn.thresh, fn.min_kept, fn.backend, fn.aux, fn.aux_weight) == (255, 0.7, 256, "hip", False, 0.2)
    assert fn.weight is None and len(fn.state_dict()) == 0
    fn = ca.SoftmaxCrossEntropyOHEMLoss(class_weights=[1.0, 2.0, 3.0])
    assert fn.weight.tolist() == [1.0, 2.0, 3.0] and fn.weight.dtype == torch.float32 and len(fn.state_dict()) == 0
    with pytest.raises(AssertionError):
        fn(torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 4, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="one head"):
        ca.MixSoftmaxCrossEntropyOHEMLoss(use_weight=False)([torch.zeros(1, 3, 4, 4)] * 2, torch.zeros(1, 4, 4, dtype=torch.int64))


def test_mix_softmax_cross_entropy_loss_is_the_aux_weighted_sum():
    shape = (2, 19, 8, 64)
    t = _t(oc.inputs(shape)[1])
    heads = [_t(oc.inputs(shape, h)[0]) for h in range(3)]
    ce = [torch.nn.functional.cross_entropy(h, t, ignore_index=IGNORE) for h in heads]
    assert torch.equal(ca.MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=0.4, ignore_label=IGNORE)(heads, t),
                       ce[0] + 0.4 * ce[1] + 0.4 * ce[2])
    assert torch.equal(ca.MixSoftmaxCrossEntropyLoss(aux=False, ignore_label=IGNORE)([heads[1]], t), ce[1])
    assert torch.equal(ca.MixSoftmaxCrossEntropyLoss(aux=False, ignore_label=IGNORE)(heads[1], t), ce[1])
    with pytest.raises(ValueError, match="one head"):
        ca.MixSoftmaxCrossEntropyLoss(aux=False)(heads, t)


def test_names_are_exported_and_the_source_is_built():
    names = ["seg_ohem_cross_entropy", "MixSoftmaxCrossEntropyLoss", "SoftmaxCrossEntropyOHEMLoss", "MixSoftmaxCrossEntropyOHEMLoss"]
    assert O.__all__ == names
    for mod in (ca.loss_functions, ca):
        assert set(names) <= set(mod.__all__)
        for n in names:
            assert getattr(mod, n) is getattr(O, n) is getattr(S, n)            # where the reference keeps them, too
    assert "seg_ohem.hip" in cbuild.SOURCES and "seg_ohem.hip" in cbuild.EXPERIMENT_SOURCES


# ---- ops and the C ABI ------------------------------------------------------------------------------------------------------------
def test_op_schemas():
    s = lambda n: str(getattr(torch.ops.cerberus, n).default._schema)
    assert s("seg_ohem_cross_entropy") == ("cerberus::seg_ohem_cross_entropy(Tensor logits, Tensor target, Tensor weight, "
                                           "int ignore_index, float thresh, int min_kept) -> (Tensor loss, Tensor prob, Tensor lse, "
                                           "Tensor state, Tensor counts)")
    assert s("seg_ohem_cross_entropy_backward") == ("cerberus::seg_ohem_cross_entropy_backward(Tensor logits, Tensor target, "
                                                    "Tensor weight, Tensor prob, Tensor lse, Tensor state, Tensor grad_loss, "
                                                    "int ignore_index) -> Tensor")


def test_meta_implementations_give_the_shapes():
    m = lambda *shape, dtype=torch.float32: torch.empty(*shape, device="meta", dtype=dtype)
    x, t, w = m(2, 19, 5, 7), m(2, 5, 7, dtype=torch.int64), m(19)
    loss, prob, lse, state, counts = torch.ops.cerberus.seg_ohem_cross_entropy(x, t, w, 255, 0.7, 100)
    assert loss.shape == () and prob.shape == lse.shape == (2, 5, 7) and state.shape == (ops.OHEM_STATE_FLOATS,)
    assert all(o.dtype == torch.float32 and o.device.type == "meta" for o in (loss, prob, lse, state))
    assert counts.shape == (2,) and counts.dtype == torch.int64 and ops.OHEM_STATE_FLOATS >= 4
    g = torch.ops.cerberus.seg_ohem_cross_entropy_backward(x, t, w, prob, lse, state, loss, 255)
    assert g.shape == x.shape and g.dtype == torch.float32 and g.device.type == "meta"


def test_cpu_tensors_through_the_raw_ops_raise():
    x, t, w = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.seg_ohem_cross_entropy(x, t, w, 255, 0.7, 4)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.seg_ohem_cross_entropy(x.requires_grad_(True), t, w, 255, 0.7, 4)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.seg_ohem_cross_entropy_backward(x.detach(), t, w, torch.zeros(1, 4, 4), torch.zeros(1, 4, 4),
                                                           torch.zeros(8), torch.ones(()), 255)


def test_workspace_bytes_in_python_equal_the_library():
    lib = _lib.get()
    for shape in ((1, 1, 1), (1, 1, 4), (2, 37, 53), (1, 32, 32), (1, 32, 33), (2, 128, 256), (4, 512, 1024), (2, 1024, 2048),
                  (7, 1025, 31), (0, 8, 8), (-1, 8, 8), (1, 0, 8), (4, 32768, 32768)):
        assert ops._seg_ohem_workspace_bytes(*shape) == lib.cerberus_seg_ohem_workspace_bytes(*shape), shape
    fixed = (len(ops.OHEM_DIGIT_BITS) * ops.OHEM_BINS + ops.OHEM_SELECT_WORDS) * 4
    assert ops._seg_ohem_workspace_bytes(1, 32, 32) == 1024 * 4 + 3 * 4 + fixed
    assert ops._seg_ohem_workspace_bytes(1, 32, 33) == 1056 * 4 + 6 * 4 + fixed
    assert ops._seg_ohem_workspace_bytes(1, 1, 1) == 4 * 4 + 3 * 4 + fixed and ops._seg_ohem_workspace_bytes(4, 32768, 32768) == 0
    assert ops._seg_ohem_workspace_bytes(1, 1, 1) % 16 == 12                    # nll is padded, so the partials stay 16-byte aligned
    # the constants of the select, exported by the library and restated in ops.py
    assert tuple(lib.cerberus_seg_ohem_digit_bits(d) for d in range(len(ops.OHEM_DIGIT_BITS))) == ops.OHEM_DIGIT_BITS
    assert lib.cerberus_seg_ohem_digit_bits(-1) == 0 and lib.cerberus_seg_ohem_digit_bits(len(ops.OHEM_DIGIT_BITS)) == 0
    assert lib.cerberus_seg_ohem_bins() == ops.OHEM_BINS and sum(ops.OHEM_DIGIT_BITS) == 32
    assert all(1 << b <= ops.OHEM_BINS for b in ops.OHEM_DIGIT_BITS)


def test_argument_rejection_without_gpu():
    lib = _lib.get()
    one = 4096                                                         # never dereferenced: every call below returns before a launch
    fwd = lambda ptrs, ws_bytes, B, C, H, W, thresh, dtype: lib.cerberus_seg_ohem_forward(
        *ptrs, ws_bytes, B, C, H, W, -1, thresh, 256, dtype, None)
    bwd = lambda ptrs, B, C, H, W, dtype: lib.cerberus_seg_ohem_backward(*ptrs, B, C, H, W, 255, dtype, None)
    null9, full9, null8, full8 = [None] * 9, [one] * 9, [None] * 8, [one] * 8
    assert fwd(null9, 1 << 20, 2, 19, 8, 8, 0.7, 0) == -1             # CERB_EINVAL: null pointers
    for k in range(9):
        assert fwd(full9[:k] + [None] + full9[k + 1:], 1 << 20, 2, 19, 8, 8, 0.7, 0) == -1, k
    for k in range(8):
        assert bwd(full8[:k] + [None] + full8[k + 1:], 2, 19, 8, 8, 0) == -1, k
    assert fwd(null9, 1 << 20, 2, 19, 8, 8, 0.7, 9) == -2 and bwd(null8, 2, 19, 8, 8, 9) == -2       # CERB_EDTYPE
    for dtype in (1, 2, 3):                                            # fp16 / bf16 / fp64: CERB_EUNSUPPORTED
        assert fwd(full9, 1 << 20, 2, 19, 8, 8, 0.7, dtype) == -5 and bwd(full8, 2, 19, 8, 8, dtype) == -5
    assert fwd(null9, 0, 0, 19, 8, 8, 0.7, 0) == 0 and bwd(null8, 0, 19, 8, 8, 0) == 0               # an empty batch: no launch
    need = lib.cerberus_seg_ohem_workspace_bytes(2, 8, 8)
    assert fwd(full9, need - 1, 2, 19, 8, 8, 0.7, 0) == -1            # workspace one byte short
    assert fwd(full9[:8] + [one + 4], 1 << 20, 2, 19, 8, 8, 0.7, 0) == -1       # workspace not 16-byte aligned
    for bad in ((-1, 19, 8, 8), (2, 0, 8, 8), (2, 19, 0, 8), (2, 19, 8, -3)):
        assert fwd(full9, 1 << 20, *bad, 0.7, 0) == -1 and bwd(full8, *bad, 0) == -1, bad
    assert fwd(full9, 1 << 20, 2, 19, 8, 8, float("nan"), 0) == -1
    # what the issue sets: a single class and B*H*W >= 2^31 are CERB_EUNSUPPORTED
    assert fwd(full9, 1 << 20, 2, 1, 8, 8, 0.7, 0) == -5 and bwd(full8, 2, 1, 8, 8, 0) == -5
    assert fwd(full9, 1 << 40, 4, 19, 32768, 32768, 0.7, 0) == -5 and bwd(full8, 2, 19, 32768, 32768, 0) == -5
    assert b"" != lib.cerberus_error_string(-5)


def test_header_and_binding_declare_the_symbols():
    with open(os.path.join(REPO, "include", "cerberus_hip.h")) as f:
        header = f.read()
    for name, nargs in (("cerberus_seg_ohem_workspace_bytes", 3), ("cerberus_seg_ohem_forward", 19),
                        ("cerberus_seg_ohem_backward", 15), ("cerberus_seg_ohem_digit_bits", 1)):
        m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert "#define CERBERUS_HIP_ABI_VERSION 7 " in header            # additions only


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_path():
    rows = oc.ROWS + oc.EXTRA_ROWS
    assert set(rows) == set(PURPOSE), "a row without a stated purpose"
    reached = set()
    for row, must in PURPOSE.items():
        got = oc.tiers(row)
        assert set(must) <= got and set(must) <= set(oc.TIERS), (row, sorted(got))
        reached |= got
    assert reached == set(oc.TIERS), "no row reaches: %s" % sorted(set(oc.TIERS) - reached)
    # both routes take the kth branch; the large rows cross the finish kernel's first and second wrap
    n = lambda s: (s[0] * s[2] * s[3] + ops.SEG_CHUNK_PIXELS - 1) // ops.SEG_CHUNK_PIXELS
    assert n((2, 2, 129, 1028)) == 260 and n((1, 3, 601, 1023)) == 601 and ops.SEG_CHUNK_PIXELS == 1024
    assert (129 * 1028) % 1024 and (37 * 53) % 1024 and (8 * 64) % 1024        # image 1 begins inside a chunk


def test_the_inputs_are_confident_and_the_small_rows_are_clear_of_the_threshold():
    for shape, thresh, min_kept, small in oc.ROWS:
        x, t = oc.inputs(shape)
        assert x.dtype == np.float32 and t.dtype == np.int64 and not x.flags.writeable
        p64, valid = oc.prob64(x, t)
        share = float((t == IGNORE).mean())
        assert 0.08 < share < 0.25 and valid.sum() == (t != IGNORE).sum()
        sure = float((p64[valid] > 0.99).mean())
        assert sure > (0.45 if shape[1] <= 3 else 0.15), (shape, sure)          # the dense cluster below 1
        th64, keep_all = oc.expected_threshold(p64[valid], thresh, min_kept, np.float64)
        gap = oc.nearest_gap(p64, valid, float(th64))
        p32 = np.take_along_axis(oc.prob32_numpy(x), np.where(valid, t, 0)[:, None], 1)[:, 0]
        e32 = float((np.abs(p32[valid] - p64[valid]) / p64[valid]).max())
        print("%s thresh %g min_kept %d: gap %.3e, numpy fp32 error %.3e" % (shape, thresh, min_kept, gap, e32))
        assert 1e-7 < e32 < 1e-6
        if small:
            assert gap >= 100 * e32                       # 25 times the GPU test's bound of 4 e32
        else:
            assert gap < 100 * e32                        # nothing here may compare kept sets with the reference


# ---- the digit-wise select, modelled in numpy --------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in oc.ROWS + oc.EXTRA_ROWS], ids=lambda r: "%s-%g-%d" % (r[0], r[1], r[2]))
def test_radix_select_model_equals_a_sort(row):
    shape, _thresh, min_kept, _ = row
    x, t = oc.inputs(shape)
    p64, valid = oc.prob64(x, t)
    key = oc.keys(p64[valid].astype(np.float32))
    ordered = np.sort(key)
    assert np.array_equal(np.argsort(key, kind="stable"), np.argsort(p64[valid].astype(np.float32), kind="stable"))     # monotonic
    for k in sorted({1, 2, min(max(min_kept, 1), key.size), key.size - 1, key.size}):
        kth, rank, counted = oc.radix_select(key, k)
        assert kth == ordered[k - 1] and rank == k - int((key < kth).sum()) and 1 <= rank <= int((key == kth).sum())
        assert counted[0] == key.size and counted[0] >= counted[1] >= counted[2] >= 1
    for bits in ((8, 8, 8, 8), (11, 11, 10), (10, 11, 11), (16, 16)):          # any split gives the same key
        if all(1 << b <= ops.OHEM_BINS for b in bits):
            assert oc.radix_select(key, min(max(min_kept, 1), key.size), bits)[0] == ordered[min(max(min_kept, 1), key.size) - 1]


def test_radix_select_model_on_ties_and_nan():
    p = np.array([0.5, 0.25, np.nan, 0.25, 0.75, 0.25, np.nan, 1.0, 0.0], dtype=np.float32)
    key = oc.keys(p)
    assert key[2] == key[6] == 0xffffffff and key[8] == 0
    want = np.sort(p)                                                            # NaN last, as numpy's argsort in the reference
    for k in range(1, p.size + 1):
        kth, rank, _ = oc.radix_select(key, k)
        got = kth.view(np.float32)
        assert (np.isnan(got) and np.isnan(want[k - 1])) or got == want[k - 1], k
    assert [oc.radix_select(key, k)[1] for k in (2, 3, 4)] == [1, 2, 3]          # the rank among the three ties at 0.25
    assert oc.expected_threshold(p, 0.3, 8)[0] == np.float32(0.3)               # a NaN kth gives thresh
    assert oc.expected_threshold(p, 0.3, 5)[0] == np.float32(0.5) and oc.expected_threshold(p, 0.3, 9) == (np.float32(np.inf), True)
