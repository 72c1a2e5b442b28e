"""One sample call per ``cerberus_detr::`` op, in the three layouts of tests/op_cases.py (whose helpers are imported, not edited), and
the outputs each must return, written out by hand.  tests/test_detr_op_contract_cpu.py and tests/test_detr_op_contract_gpu.py hold the
five ops to the contract of DESIGN.md 3.23 with it."""
import torch

import detr_cases
from op_cases import LAYOUTS, lay, on, same_bits  # noqa: F401

F32, F64, I32 = torch.float32, torch.float64, torch.int32
L, B, Q, C1, COUNTS = 2, 2, 9, 6, (4, 2)
N, TMAX = L * B, max(COUNTS)
CASE = detr_cases.make_case(L, B, Q, C1, COUNTS, 5100)
WEIGHTS = (detr_cases.W_CLASS, detr_cases.W_BBOX, detr_cases.W_GIOU)

OUTPUTS = {
    "match_cost": [((N, Q, TMAX), F32)],
    "lsap": [((N, Q), I32)],
    "hungarian_match": [((N, Q), I32), ((N,), I32)],
    "set_loss": [((L, 4), F32), ((L,), F64)],
    "set_loss_backward": [((N, Q, C1), F32), ((N, Q, 4), F32)],
}


def call(name, args):
    out = getattr(torch.ops.cerberus_detr, name)(*args)
    return [out] if isinstance(out, torch.Tensor) else list(out)


def forward(device, name, args):
    """What the contiguous forward call leaves for the next op: the real outputs on a GPU, zeros of the stated shapes elsewhere."""
    if torch.device(device).type == "cuda":
        return call(name, args)
    return [torch.zeros(shape, dtype=dtype, device=device) for shape, dtype in OUTPUTS[name]]


def _inputs(d):
    return [on(d, CASE[k]) for k in ("logits", "boxes", "tgt_labels", "tgt_boxes", "tgt_count")]


def _match_cost(d):
    return [*_inputs(d), *WEIGHTS], ()


def _lsap(d):
    args, _ = _match_cost(d)
    cost, = forward(d, "match_cost", args)
    return [cost, args[4]], ()


def _hungarian_match(d):
    return [*_inputs(d), *WEIGHTS], ()


def _set_loss(d):
    x, p, tl, tb, tc = _inputs(d)
    match, _ = forward(d, "hungarian_match", [x, p, tl, tb, tc, *WEIGHTS])
    return [x, p, match, tl, tb, tc, on(d, CASE["weight"]), on(d, CASE["num_boxes"])], (0, 1)


def _set_loss_backward(d):
    args, _ = _set_loss(d)
    _, wsum = forward(d, "set_loss", args)
    return [on(d, detr_cases.upstream_of(CASE)), *args, wsum], ()


CASES = {
    "match_cost": _match_cost,
    "lsap": _lsap,
    "hungarian_match": _hungarian_match,
    "set_loss": _set_loss,
    "set_loss_backward": _set_loss_backward,
}


def case(name, device, layout):
    """(args, differentiable) of ``name`` with every tensor argument of more than one element (``num_boxes`` holds one) in ``layout``."""
    args, differentiable = CASES[name](device)
    return [lay(a, layout) if isinstance(a, torch.Tensor) and a.numel() > 1 else a for a in args], tuple(differentiable)
