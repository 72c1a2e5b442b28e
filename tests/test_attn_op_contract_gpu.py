"""The binding's contract on the GPU for the three ``cerberus_attn::`` ops of tests/attn_op_cases.py in every
layout: "inputs of any strides, outputs contiguous, fake == real".

1. Metadata: the real outputs have the shapes, dtypes and default strides tests/test_attn_op_contract_cpu.py demands of the fake ones.
2. Same bits as the contiguous call.  The premise (two contiguous calls give equal bits) is asserted first.
3. ``torch.library.opcheck``: schema and fake against real.  The raw ops have no autograd formula to check: the gradients are an op
   of their own in this table, and tests/test_detr_attn_gpu.py holds the ``autograd.Function`` wrapper to the float64 chain."""
import pytest
import torch

import attn_op_cases as pc
import cerberusnet_amd  # noqa: F401  (registers the ops)
from test_attn_op_contract_cpu import check_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(name, layout) for name in pc.CASES for layout in pc.LAYOUTS]
IDS = ["%s-%s" % p for p in PAIRS]
UTILS = ("test_schema", "test_faketensor")


@pytest.mark.parametrize("name,layout", PAIRS, ids=IDS)
def test_real_outputs_have_the_stated_metadata(name, layout):
    args, _ = pc.case(name, DEV, layout)
    check_outputs(name, pc.call(name, args), "cuda")


@pytest.mark.parametrize("name,layout", PAIRS, ids=IDS)
def test_same_bits_as_the_contiguous_call(name, layout):
    args, _ = pc.case(name, DEV, layout)
    plain = [a.contiguous() if isinstance(a, torch.Tensor) else a for a in args]
    out0, out1 = pc.call(name, plain), pc.call(name, plain)
    outs = pc.call(name, args)
    check_outputs(name, outs, "cuda")
    for i, (a, b, c) in enumerate(zip(out0, out1, outs)):
        assert pc.same_bits(a, b), (name, "premise", i)
        assert pc.same_bits(c, a), (name, layout, i)
        assert bool((a != 0).any()), (name, i)              # something was really computed


@pytest.mark.parametrize("name,layout", PAIRS, ids=IDS)
def test_opcheck(name, layout):
    args, _ = pc.case(name, DEV, layout)
    torch.library.opcheck(getattr(torch.ops.cerberus_attn, name).default, tuple(args), test_utils=UTILS)
