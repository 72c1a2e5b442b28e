"""The binding's contract for the three ``cerberus_attn::`` ops, checked without a GPU: every op has a sample call
in tests/attn_op_cases.py, and its fake (Meta) implementation returns, for inputs of any strides, fresh tensors of the shapes and
dtypes written out there, with the default strides and storage offset 0.  tests/test_attn_op_contract_gpu.py holds the real outputs
to the same statement."""
import pytest
import torch

import attn_op_cases as pc
import cerberusnet_amd  # noqa: F401  (registers the ops)
from test_pdl_op_contract_cpu import default_strides, registered_ops

PAIRS = [(name, layout) for name in pc.CASES for layout in pc.LAYOUTS]


def check_outputs(name, outs, device_type):
    want = pc.OUTPUTS[name]
    assert len(outs) == len(want), (name, len(outs), len(want))
    for i, (o, (shape, dtype)) in enumerate(zip(outs, want)):
        assert isinstance(o, torch.Tensor), (name, i, type(o))
        assert tuple(o.shape) == tuple(shape) and o.dtype == dtype, (name, i, tuple(o.shape), o.dtype, shape, dtype)
        assert o.device.type == device_type, (name, i, o.device)
        assert o.storage_offset() == 0 and tuple(o.stride()) == default_strides(o.shape), (name, i, o.stride(), o.storage_offset())


def test_every_registered_op_has_a_case():
    assert registered_ops("cerberus_attn::") == set(pc.CASES) == set(pc.OUTPUTS) and len(pc.CASES) == 3
    # the other namespaces keep their own tables
    for other in ("cerberus::", "cerberus_ocr::", "cerberus_detr::", "cerberus_pdl::"):
        assert not any("attn" in n or n.startswith("attention") for n in registered_ops(other)), other


@pytest.mark.parametrize("name", list(pc.CASES))
def test_the_layouts_change_strides_and_nothing_else(name):
    plain, diff = pc.case(name, "cpu", "contiguous")
    tensors = [i for i, a in enumerate(plain) if isinstance(a, torch.Tensor)]
    several = [i for i in tensors if plain[i].numel() > 1]            # a one-element tensor (the seed) has no layout
    assert set(diff) <= set(tensors)
    for layout in ("channels_last", "sliced"):
        args, _ = pc.case(name, "cpu", layout)
        for i in tensors:
            assert args[i].storage_offset() == 0 and args[i].shape == plain[i].shape and pc.same_bits(args[i], plain[i])
        if several:
            assert any(not args[i].is_contiguous() for i in several), (name, layout)
        if layout == "sliced":
            assert all(not args[i].is_contiguous() for i in several), (name, layout)


@pytest.mark.parametrize("name,layout", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_fake_outputs_are_fresh_contiguous_tensors_of_the_stated_shapes(name, layout):
    cpu, _ = pc.case(name, "cpu", layout)
    args, _ = pc.case(name, "meta", layout)
    for a, c in zip(args, cpu):
        if isinstance(a, torch.Tensor):
            assert a.device.type == "meta" and a.stride() == c.stride() and a.storage_offset() == 0
    check_outputs(name, pc.call(name, args), "meta")


def test_raw_ops_raise_on_cpu_tensors():
    for name in pc.CASES:
        args, _ = pc.case(name, "cpu", "contiguous")
        with pytest.raises(RuntimeError, match="cerberus_attn::%s has no CPU implementation" % name):
            pc.call(name, args)
