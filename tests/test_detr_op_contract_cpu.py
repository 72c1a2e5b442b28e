"""The binding's contract for the five ``cerberus_detr::`` ops, checked without a GPU: every op has a sample call in
tests/detr_op_cases.py, and its fake (Meta) implementation returns, for inputs of any strides, fresh tensors of the shapes and
dtypes written out there, with the default strides and storage offset 0.  tests/test_detr_op_contract_gpu.py holds the real outputs
to the same statement."""
import pytest
import torch

import cerberusnet_amd  # noqa: F401  (registers the ops)
import detr_op_cases as dc

PAIRS = [(name, layout) for name in dc.CASES for layout in dc.LAYOUTS]


def registered_ops():
    return {n.split("::", 1)[1].split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("cerberus_detr::")}


def default_strides(shape):
    strides, step = [], 1
    for n in reversed(shape):
        strides.append(step)
        step *= max(int(n), 1)
    return tuple(reversed(strides))


def check_outputs(name, outs, device_type):
    want = dc.OUTPUTS[name]
    assert len(outs) == len(want), (name, len(outs), len(want))
    for i, (o, (shape, dtype)) in enumerate(zip(outs, want)):
        assert isinstance(o, torch.Tensor), (name, i, type(o))
        assert tuple(o.shape) == tuple(shape) and o.dtype == dtype, (name, i, tuple(o.shape), o.dtype, shape, dtype)
        assert o.device.type == device_type, (name, i, o.device)
        assert o.storage_offset() == 0 and tuple(o.stride()) == default_strides(o.shape), (name, i, o.stride(), o.storage_offset())


def test_every_registered_op_has_a_case():
    assert registered_ops() == set(dc.CASES) == set(dc.OUTPUTS) and len(dc.CASES) == 5
    # the other namespaces keep their own tables
    assert not any(n.startswith("cerberus::hungarian") or n.startswith("cerberus::set_loss") or n.startswith("cerberus::lsap")
                   for n in torch._C._dispatch_get_all_op_names())


@pytest.mark.parametrize("name", list(dc.CASES))
def test_the_layouts_change_strides_and_nothing_else(name):
    plain, diff = dc.case(name, "cpu", "contiguous")
    tensors = [i for i, a in enumerate(plain) if isinstance(a, torch.Tensor)]
    assert set(diff) <= set(tensors)
    for layout in ("channels_last", "sliced"):
        args, _ = dc.case(name, "cpu", layout)
        moved = 0
        for i in tensors:
            assert args[i].storage_offset() == 0 and args[i].shape == plain[i].shape and dc.same_bits(args[i], plain[i])
            # op_cases.lay transposes tensors of three dimensions and up; "sliced" strides every tensor of more than one element
            if plain[i].numel() > 1 and (layout == "sliced" or plain[i].dim() >= 3):
                assert not args[i].is_contiguous(), (name, layout, i)
                moved += 1
        assert moved >= 1, (name, layout)


@pytest.mark.parametrize("name,layout", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_fake_outputs_are_fresh_contiguous_tensors_of_the_stated_shapes(name, layout):
    cpu, _ = dc.case(name, "cpu", layout)
    args, _ = dc.case(name, "meta", layout)
    for a, c in zip(args, cpu):
        if isinstance(a, torch.Tensor):
            assert a.device.type == "meta" and a.stride() == c.stride() and a.storage_offset() == 0
    check_outputs(name, dc.call(name, args), "meta")


@pytest.mark.parametrize("name", list(dc.CASES))
def test_cpu_tensors_fail_loudly(name):
    args, _ = dc.case(name, "cpu", "contiguous")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        dc.call(name, args)
