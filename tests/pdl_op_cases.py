"""One sample call per ``cerberus_pdl::`` op, in the three layouts of tests/op_cases.py (whose helpers are imported, not edited), and
the outputs each must return, written out by hand.  tests/test_pdl_op_contract_cpu.py and tests/test_pdl_op_contract_gpu.py hold the
four ops to the contract of DESIGN.md 3.23 with it.  The raw ops carry no autograd formula (the differentiable entry points are the
``autograd.Function`` wrappers of ops_pdl.py), so no argument is differentiable here."""
import torch

import pdl_cases
from op_cases import LAYOUTS, lay, on, same_bits  # noqa: F401

F32 = torch.float32
LOW = (2, 4, 5, 7)              # B, Ca, h, w
SKIP = (2, 3, 9, 12)            # B, Cb, H, W
OUT = (2, 7, 9, 12)             # B, Ca + Cb, H, W
WEIGHT = (7, 1, 5, 5)
PLAIN_WEIGHT = (3, 1, 5, 5)

OUTPUTS = {
    "dwconv5x5": [(SKIP, F32)],
    "dwconv5x5_backward": [(SKIP, F32), (PLAIN_WEIGHT, F32)],
    "upcat_dwconv5x5": [(OUT, F32)],
    "upcat_dwconv5x5_backward": [(LOW, F32), (SKIP, F32), (WEIGHT, F32)],
}


def _t(d, shape, seed):
    return on(d, pdl_cases.tensor(shape, seed).numpy())


CASES = {
    "dwconv5x5": lambda d: ([_t(d, SKIP, 401), _t(d, PLAIN_WEIGHT, 402)], ()),
    "dwconv5x5_backward": lambda d: ([_t(d, SKIP, 403), _t(d, SKIP, 401), _t(d, PLAIN_WEIGHT, 402), [True, True]], ()),
    "upcat_dwconv5x5": lambda d: ([_t(d, LOW, 411), _t(d, SKIP, 412), _t(d, WEIGHT, 413)], ()),
    "upcat_dwconv5x5_backward": lambda d: ([_t(d, OUT, 414), _t(d, LOW, 411), _t(d, SKIP, 412), _t(d, WEIGHT, 413), [True, True, True]],
                                           ()),
}


def case(name, device, layout):
    """(args, differentiable) of ``name`` with every tensor argument in ``layout``."""
    args, differentiable = CASES[name](device)
    return [lay(a, layout) if isinstance(a, torch.Tensor) else a for a in args], tuple(differentiable)


def call(name, args):
    out = getattr(torch.ops.cerberus_pdl, name)(*args)
    return [out] if isinstance(out, torch.Tensor) else list(out)
