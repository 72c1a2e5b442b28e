"""The binding's contract on the GPU for the five ``cerberus_detr::`` ops of tests/detr_op_cases.py in every layout,
as tests/test_op_contract_gpu.py states it for the ``cerberus::`` ops: "inputs of any strides, outputs contiguous, fake == real".

1. Metadata: the real outputs have the shapes, dtypes and default strides tests/test_detr_op_contract_cpu.py demands of the fake ones.
2. Same bits as the contiguous call: outputs and -- for set_loss, the op with a gradient -- the gradients, with the upstream gradient
   itself in the layout and once more as an expanded (stride 0) tensor.  The premise (two contiguous calls give equal bits) is
   asserted first.
3. ``torch.library.opcheck``: schema, autograd registration, fake against real, AOT dispatch.  Nothing is excluded."""
import pytest
import torch

import cerberusnet_amd  # noqa: F401  (registers the ops)
import detr_op_cases as dc
from cerberusnet_amd.synth import hash_uniform
from test_detr_op_contract_cpu import check_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(name, layout) for name in dc.CASES for layout in dc.LAYOUTS]
IDS = ["%s-%s" % p for p in PAIRS]
UTILS = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_static")


def upstream(out, k, layout, expanded):
    if expanded:
        return dc.on(DEV, hash_uniform(tuple(out.shape[1:]), 900 + k, 0.5, 2.0)).expand(out.shape)
    return dc.lay(dc.on(DEV, hash_uniform(tuple(out.shape), 900 + k, 0.5, 2.0)), layout)


def evaluate(name, args, differentiable, layout, materialise=False):
    """(outputs, gradients, gradients under an expanded upstream gradient) of one call."""
    args = list(args)
    for i in differentiable:
        args[i] = args[i].detach().requires_grad_(True)
    outs = dc.call(name, args)
    if not differentiable:
        return outs, [], []
    leaves = [args[i] for i in differentiable]
    heads = [(k, o) for k, o in enumerate(outs) if o.requires_grad]
    assert heads, name
    grads = []
    for expanded in (False, True):
        ups = [upstream(o, k, layout, expanded) for k, o in heads]
        if materialise:
            ups = [u.contiguous() for u in ups]
        grads.append(list(torch.autograd.grad([o for _, o in heads], leaves, grad_outputs=ups, retain_graph=not expanded)))
    return outs, grads[0], grads[1]


def assert_same(name, layout, what, got, want):
    assert len(got) == len(want), (name, layout, what)
    for i, (a, b) in enumerate(zip(got, want)):
        assert dc.same_bits(a.detach(), b.detach()), (name, layout, what, i)


@pytest.mark.parametrize("name,layout", PAIRS, ids=IDS)
def test_real_outputs_have_the_stated_metadata(name, layout):
    args, _ = dc.case(name, DEV, layout)
    check_outputs(name, dc.call(name, args), "cuda")


@pytest.mark.parametrize("name,layout", PAIRS, ids=IDS)
def test_same_bits_as_the_contiguous_call(name, layout):
    args, differentiable = dc.case(name, DEV, layout)
    plain = [a.contiguous() if isinstance(a, torch.Tensor) else a for a in args]
    out0, grad0, wide0 = evaluate(name, plain, differentiable, layout, materialise=True)
    out1, grad1, wide1 = evaluate(name, plain, differentiable, layout, materialise=True)
    assert_same(name, layout, "premise: outputs", out1, out0)
    assert_same(name, layout, "premise: gradients", grad1, grad0)
    assert_same(name, layout, "premise: gradients (expanded)", wide1, wide0)
    outs, grad, wide = evaluate(name, args, differentiable, layout)
    check_outputs(name, outs, "cuda")
    assert_same(name, layout, "outputs", outs, out0)
    assert_same(name, layout, "gradients", grad, grad0)
    assert_same(name, layout, "gradients (expanded)", wide, wide0)
    for j, i in enumerate(differentiable):                # a gradient was really computed
        assert grad0[j].shape == plain[i].shape and bool(grad0[j].abs().sum() > 0)


@pytest.mark.parametrize("name,layout", PAIRS, ids=IDS)
def test_opcheck(name, layout):
    args, differentiable = dc.case(name, DEV, layout)
    for i in differentiable:
        args[i] = args[i].detach().requires_grad_(True)
    torch.library.opcheck(getattr(torch.ops.cerberus_detr, name).default, tuple(args), test_utils=UTILS)


def test_the_backward_op_raises_on_double_backward():
    args, _ = dc.case("set_loss_backward", DEV, "contiguous")
    args[0] = args[0].detach().requires_grad_(True)
    gl, _ = dc.call("set_loss_backward", args)
    with pytest.raises(RuntimeError, match="double backward"):
        gl.sum().backward()
