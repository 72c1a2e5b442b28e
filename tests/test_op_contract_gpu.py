"""The binding's contract on the GPU, for every ``cerberus::`` op of tests/op_cases.py in every layout:
"inputs of any strides, outputs contiguous, fake == real".

1. Metadata: the real outputs have the shapes, dtypes and default strides tests/test_op_contract_cpu.py demands of the fake
   ones.
2. Same bits as the contiguous call: outputs, what the call leaves in an argument it writes, and -- for an op with a
   gradient -- the gradients, with the upstream gradient of a non-scalar output itself in the layout and once more as an
   expanded (stride 0) tensor.  Equality, not a tolerance: the binding copies to a fresh contiguous allocation and runs the same
   kernels on the same values, and the kernels are bit-reproducible run to run.  That premise is asserted first (two
   contiguous calls give equal bits); no op needed another shape or a tolerance for it.
3. ``torch.library.opcheck``: schema, autograd registration, fake against real (sizes, strides, storage offsets, dtypes,
   devices) and AOT dispatch.  ``AOT_EXCLUDED`` lists the (op, util) pairs that cannot pass, each with its reason.
4. Same bits from an offset view: every tensor argument (and every upstream gradient) as a contiguous view that starts one
   element off a 16-byte boundary inside a buffer whose other elements are NaN (tests/alignment_cases.py: ``embed``).  The
   binding hands such a view's pointer to the kernels as it is, so their alignment gates decide; an op whose gate changes
   the summation order would be listed in ``OFFSET_EXCLUDED`` with its reason and held to its reference bound instead.
   (The correlation and warp kernels at every gate and shift: tests/test_alignment_gpu.py.)"""
import pytest
import torch

import cerberusnet_amd  # noqa: F401  (registers the ops)
import op_cases
from alignment_cases import embed
from op_cases import same_bits
from test_op_contract_cpu import check_outputs, flat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(name, layout) for name in op_cases.CASES for layout in op_cases.LAYOUTS]
IDS = ["%s-%s" % p for p in PAIRS]
UTILS = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_static")

# (op, util) -> why it cannot pass without restructuring the op (at most four; DESIGN.md 3.23 repeats the reasons)
AOT_EXCLUDED = {
    ("panoptic_targets", "test_aot_dispatch_static"):
        "center_points holds NaN for a table row without a centre (the reference's convention) and opcheck compares the "
        "eager with the compiled outputs by assert_close without equal_nan",
}


# op -> (why a misaligned pointer legitimately changes its summation order, the bound of the op's own test against its
# reference); at most six (a test holds the cap)
OFFSET_EXCLUDED = {}


def call(name, args):
    return flat(getattr(torch.ops.cerberus, name)(*args))


def fresh(name, args):
    """The arguments of one call: an argument the op writes is cloned, so that no two calls share it."""
    written = op_cases.MUTATED.get(name, ())
    return [a.clone() if i in written else a for i, a in enumerate(args)]


def contiguous_copies(args):
    return [a.contiguous() if isinstance(a, torch.Tensor) else a for a in args]


def upstream(out, k, layout, expanded):
    """The fixed upstream gradient of output ``k``: None for a scalar loss (the gradient of the loss itself), else a
    hash_uniform tensor in ``layout``, or one item of it expanded over the batch (stride 0)."""
    if out.dim() == 0:
        return None
    dtype = {torch.float32: "float32", torch.float64: "float64"}[out.dtype]
    if expanded:
        w = op_cases.on(DEV, op_cases.hash_uniform(tuple(out.shape[1:]), 900 + k, dtype=dtype))
        return w.expand(out.shape)
    full = op_cases.on(DEV, op_cases.hash_uniform(tuple(out.shape), 900 + k, dtype=dtype))
    return embed(full, 1) if layout == "offset" else op_cases.lay(full, layout)


def evaluate(name, args, differentiable, layout, materialise=False):
    """(results, gradients, gradients under an expanded upstream gradient) of one call.  ``results``: the outputs and what is
    left in the written arguments.  ``materialise``: the upstream gradients as contiguous copies (the reference call)."""
    args = fresh(name, args)
    for i in differentiable:
        args[i] = args[i].detach().requires_grad_(True)
    outs = call(name, args)
    results = [o.detach() for o in outs] + [args[i] for i in op_cases.MUTATED.get(name, ())]
    if not differentiable:
        return outs, results, [], []
    leaves = [args[i] for i in differentiable]
    heads = [(k, o) for k, o in enumerate(outs) if o.requires_grad]
    assert heads, name
    grads = []
    for expanded in (False, True):
        if expanded and all(o.dim() == 0 for _, o in heads):
            grads.append([])
            continue
        ups = [upstream(o, k, layout, expanded) for k, o in heads]
        if materialise:
            ups = [u.contiguous() if u is not None else None for u in ups]
        grads.append(list(torch.autograd.grad([o for _, o in heads], leaves, grad_outputs=ups, retain_graph=not expanded)))
    return outs, results, grads[0], grads[1]


def assert_same(name, layout, what, got, want):
    assert len(got) == len(want), (name, layout, what)
    for i, (a, b) in enumerate(zip(got, want)):
        assert same_bits(a, b), (name, layout, what, i, float((a.double() - b.double()).abs().max()) if a.shape == b.shape else None)


@pytest.mark.parametrize("name,layout", PAIRS, ids=IDS)
def test_real_outputs_have_the_stated_metadata(name, layout):
    args, _ = op_cases.case(name, DEV, layout)
    check_outputs(name, call(name, fresh(name, args)), "cuda")


@pytest.mark.parametrize("name,layout", PAIRS, ids=IDS)
def test_same_bits_as_the_contiguous_call(name, layout):
    args, differentiable = op_cases.case(name, DEV, layout)
    plain = contiguous_copies(args)
    _, res0, grad0, wide0 = evaluate(name, plain, differentiable, layout, materialise=True)
    _, res1, grad1, wide1 = evaluate(name, plain, differentiable, layout, materialise=True)
    # the premise: the kernels give the same bits run to run
    assert_same(name, layout, "premise: outputs", res1, res0)
    assert_same(name, layout, "premise: gradients", grad1, grad0)
    assert_same(name, layout, "premise: gradients (expanded)", wide1, wide0)
    outs, res, grad, wide = evaluate(name, args, differentiable, layout)
    check_outputs(name, outs, "cuda")
    assert_same(name, layout, "outputs", res, res0)
    assert_same(name, layout, "gradients", grad, grad0)
    assert_same(name, layout, "gradients (expanded)", wide, wide0)
    for i in differentiable:                # a gradient was really computed
        assert grad0[differentiable.index(i)].shape == plain[i].shape and bool(grad0[differentiable.index(i)].abs().sum() > 0)


def offset_views(name, args):
    """Every tensor argument one element off a 16-byte boundary, but for the arguments a binding takes in the form the forward
    returned (``NO_LAYOUT``: the concat buffers, the warp context, which must be 16-byte aligned)."""
    keep = op_cases.NO_LAYOUT.get(name, ())
    return [embed(a, 1) if isinstance(a, torch.Tensor) and i not in keep else a for i, a in enumerate(args)]


@pytest.mark.parametrize("name", list(op_cases.CASES))
def test_same_bits_from_an_offset_view(name):
    plain, differentiable = op_cases.case(name, DEV, "contiguous")
    args = offset_views(name, plain)
    for a, b in zip(args, plain):
        if isinstance(a, torch.Tensor) and a is not b:
            assert a.is_contiguous() and a.data_ptr() % 16 == a.element_size() % 16 and same_bits(a, b)
    _, res0, grad0, wide0 = evaluate(name, plain, differentiable, "contiguous", materialise=True)
    outs, res, grad, wide = evaluate(name, args, differentiable, "offset")
    check_outputs(name, outs, "cuda")
    if name in OFFSET_EXCLUDED:
        bound = OFFSET_EXCLUDED[name][1]
        for got, want in zip(res + grad + wide, res0 + grad0 + wide0):
            scale = float(want.double().abs().max()) or 1.0
            assert float((got.double() - want.double()).abs().max()) <= bound * scale, name
        return
    assert_same(name, "offset", "outputs", res, res0)
    assert_same(name, "offset", "gradients", grad, grad0)
    assert_same(name, "offset", "gradients (expanded)", wide, wide0)


def test_a_non_contiguous_concat_buffer_is_rejected():
    for layout in ("channels_last", "sliced"):
        args, _ = op_cases.case("correlation_leaky_into", DEV, "contiguous")
        args[0] = op_cases.lay(args[0], layout)
        with pytest.raises(RuntimeError, match="cannot hold channels"):
            torch.ops.cerberus.correlation_leaky_into(*args)


@pytest.mark.parametrize("name,layout", PAIRS, ids=IDS)
def test_opcheck(name, layout):
    args, differentiable = op_cases.case(name, DEV, layout)
    for i in differentiable:
        args[i] = args[i].detach().requires_grad_(True)
    utils = tuple(u for u in UTILS if (name, u) not in AOT_EXCLUDED)
    torch.library.opcheck(getattr(torch.ops.cerberus, name).default, tuple(args), test_utils=utils)


def test_the_exclusion_table_is_small_and_names_real_ops():
    assert len(AOT_EXCLUDED) <= 4
    for (name, util), reason in AOT_EXCLUDED.items():
        assert name in op_cases.CASES and util == "test_aot_dispatch_static" and reason
    assert len(OFFSET_EXCLUDED) <= 6
    for name, (reason, bound) in OFFSET_EXCLUDED.items():
        assert name in op_cases.CASES and reason and 0 < bound < 1
