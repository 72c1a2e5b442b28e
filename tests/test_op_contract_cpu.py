"""The binding's contract, checked without a GPU: every ``cerberus::`` op has a sample call in
tests/op_cases.py, and its fake (Meta) implementation returns, for inputs of any strides, what the CUDA implementation
allocates -- fresh tensors of the stated shape and dtype with the default (NCHW) strides and storage offset 0.

The shapes and dtypes come from ``op_cases.OUTPUTS``, not from the Meta functions.  tests/test_op_contract_gpu.py holds the
real outputs to the same statement and the fake ones to the real ones (``torch.library.opcheck``)."""
import pytest
import torch

import cerberusnet_amd  # noqa: F401  (registers the ops)
import op_cases

PAIRS = [(name, layout) for name in op_cases.CASES for layout in op_cases.LAYOUTS]


def registered_ops():
    return {n.split("::", 1)[1].split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("cerberus::")}


def flat(out):
    if out is None:
        return []
    return [out] if isinstance(out, torch.Tensor) else list(out)


def default_strides(shape):
    strides, step = [], 1
    for n in reversed(shape):
        strides.append(step)
        step *= max(int(n), 1)
    return tuple(reversed(strides))


def check_outputs(name, outs, device_type):
    """``outs`` are fresh tensors of the stated shapes and dtypes with the default strides."""
    want = op_cases.OUTPUTS[name]
    assert len(outs) == len(want), (name, len(outs), len(want))
    for i, (o, (shape, dtype)) in enumerate(zip(outs, want)):
        assert isinstance(o, torch.Tensor), (name, i, type(o))
        assert tuple(o.shape) == tuple(shape) and o.dtype == dtype, (name, i, tuple(o.shape), o.dtype, shape, dtype)
        assert o.device.type == device_type, (name, i, o.device)
        assert o.storage_offset() == 0 and o.is_contiguous(), (name, i, o.stride(), o.storage_offset())
        assert tuple(o.stride()) == default_strides(o.shape), (name, i, tuple(o.shape), o.stride())


def test_every_registered_op_has_a_case():
    ops = registered_ops()
    assert len(ops) >= 43, sorted(ops)
    assert set(op_cases.CASES) == ops, (sorted(ops - set(op_cases.CASES)), sorted(set(op_cases.CASES) - ops))
    assert set(op_cases.OUTPUTS) == ops
    assert set(op_cases.NO_LAYOUT) <= ops and set(op_cases.MUTATED) <= ops


@pytest.mark.parametrize("name", list(op_cases.CASES))
def test_the_layouts_change_strides_and_nothing_else(name):
    """The table itself: a layout keeps every value, shifts no start address, and (but for the exempt arguments) leaves no
    tensor of rank >= 1 with more than one element per row contiguous under 'sliced'."""
    plain, diff = op_cases.case(name, "cpu", "contiguous")
    tensors = [i for i, a in enumerate(plain) if isinstance(a, torch.Tensor)]
    assert set(diff) <= set(tensors) and all(plain[i].is_floating_point() for i in diff)
    assert all(plain[i].is_contiguous() and plain[i].shape[-2:].numel() <= 64 * 128 for i in tensors)
    for layout in ("channels_last", "sliced"):
        args, _ = op_cases.case(name, "cpu", layout)
        for i in tensors:
            assert args[i].storage_offset() == 0 and args[i].shape == plain[i].shape and args[i].dtype == plain[i].dtype
            assert op_cases.same_bits(args[i], plain[i]), (name, layout, i)
            exempt = i in op_cases.NO_LAYOUT.get(name, ())
            if layout == "sliced" and plain[i].dim() >= 1 and plain[i].shape[-1] > 1:
                assert args[i].is_contiguous() == exempt, (name, i)
            if layout == "channels_last" and plain[i].dim() == 4 and min(plain[i].shape[1:]) > 1:
                assert args[i].is_contiguous() == exempt and (exempt or args[i].is_contiguous(memory_format=torch.channels_last))
            if layout == "channels_last" and plain[i].dim() == 3 and min(plain[i].shape[1:]) > 1:
                assert not args[i].is_contiguous() and args[i].transpose(1, 2).is_contiguous(), (name, i)


@pytest.mark.parametrize("name,layout", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_fake_outputs_are_fresh_contiguous_tensors_of_the_stated_shapes(name, layout):
    args, _ = op_cases.case(name, "meta", layout)
    for i, a in enumerate(args):            # the Meta run sees the layout, not a contiguous stand-in
        if isinstance(a, torch.Tensor):
            cpu = op_cases.case(name, "cpu", layout)[0][i]
            assert a.device.type == "meta" and a.stride() == cpu.stride() and a.storage_offset() == 0, (name, layout, i)
    outs = flat(getattr(torch.ops.cerberus, name)(*args))
    check_outputs(name, outs, "meta")
