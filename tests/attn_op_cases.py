"""One sample call per ``cerberus_attn::`` op, in the three layouts of tests/op_cases.py (whose helpers are imported, not edited), and
the outputs each must return, written out by hand.  tests/test_attn_op_contract_cpu.py and tests/test_attn_op_contract_gpu.py hold
the three ops to the contract of DESIGN.md 3.23 with it.  The raw ops carry no autograd formula (the differentiable entry point is
the ``autograd.Function`` wrapper of ops_attn.py), so no argument is differentiable here.

The seed is a one-element tensor: it has no layout to change (any view of one element is contiguous), so it stays as it is and the
statement "every tensor argument is non-contiguous in the sliced layout" is made of the tensors with more than one element."""
import torch

import attn_cases
from op_cases import LAYOUTS, lay, on, same_bits  # noqa: F401

F32, BOOL = torch.float32, torch.bool
LQ, LK, B, H = 37, 45, 2, 3             # more than one tile of 32 each way, fewer than one workgroup of 128
E = H * attn_cases.HEAD_DIM
Q = (LQ, B, E)
KV = (LK, B, E)
LSE = (B, H, LQ)
STATS = (B, H, LQ, 2)
KEEP = (B, H, LQ, LK)
SCALE, P, SEED = attn_cases.HEAD_DIM ** -0.5, 0.25, 4242

OUTPUTS = {
    "attention": [(Q, F32), (LSE, F32), (STATS, F32)],
    "attention_backward": [(Q, F32), (KV, F32), (KV, F32)],
    "attn_dropout_keep": [(KEEP, BOOL)],
}


def _inputs(d):
    q, k, v, up = (on(d, t.numpy()) for t in attn_cases.inputs(LQ, LK, B, H, 501))
    mask = on(d, attn_cases.padding_mask(B, LK, (33, 0), (0, 4)).numpy())
    return q, k, v, up, mask, on(d, torch.tensor([SEED], dtype=torch.int64).numpy())


def _attention(d):
    q, k, v, _, mask, seed = _inputs(d)
    return [q, k, v, H, mask, SCALE, P, seed], ()


def _attention_backward(d):
    q, k, v, up, mask, seed = _inputs(d)
    if torch.device(d).type == "cuda":
        out, _, stats = torch.ops.cerberus_attn.attention(q, k, v, H, mask, SCALE, P, seed)
    else:
        out, stats = torch.zeros(Q, dtype=F32, device=d), torch.zeros(STATS, dtype=F32, device=d)
    return [up, q, k, v, out, stats, H, mask, SCALE, P, seed, [True, True, True]], ()


def _attn_dropout_keep(d):
    return [_inputs(d)[5], B, H, LQ, LK, P], ()


CASES = {"attention": _attention, "attention_backward": _attention_backward, "attn_dropout_keep": _attn_dropout_keep}


def case(name, device, layout):
    """(args, differentiable) of ``name`` with every tensor argument of more than one element in ``layout``."""
    args, differentiable = CASES[name](device)
    return [lay(a, layout) if isinstance(a, torch.Tensor) and a.numel() > 1 else a for a in args], tuple(differentiable)


def call(name, args):
    out = getattr(torch.ops.cerberus_attn, name)(*args)
    return [out] if isinstance(out, torch.Tensor) else list(out)
