"""One sample call per ``cerberus_ocr::`` op, in the three layouts of tests/op_cases.py (whose helpers are imported, not edited), and
the outputs each must return, written out by hand.  tests/test_ocr_op_contract_cpu.py and tests/test_ocr_op_contract_gpu.py hold the
four ops to the contract of DESIGN.md 3.23 with it."""
import torch

import ocr_cases
from op_cases import LAYOUTS, lay, on, same_bits  # noqa: F401

F32 = torch.float32
FEATS = (2, 6, 9, 12)           # B, C, H, W
LOGITS = (2, 5, 9, 12)          # B, K, H, W
TABLE = (2, 6, 5)               # B, C, K: the gathered context, and the attention's key / value
SCALE = 6 ** -0.5

OUTPUTS = {
    "spatial_gather": [(TABLE, F32), ((2, 5), F32)],
    "spatial_gather_backward": [(FEATS, F32), (LOGITS, F32)],
    "object_attention": [(FEATS, F32), (LOGITS, F32)],
    "object_attention_backward": [(FEATS, F32), (TABLE, F32), (TABLE, F32)],
}


def _t(d, shape, seed, lo=-1.0, hi=1.0):
    return on(d, ocr_cases.tensor(shape, seed, lo, hi).numpy())


def forward(device, name, args):
    """What the contiguous forward call leaves for its backward: the real outputs on a GPU, zeros of the stated shapes elsewhere."""
    if torch.device(device).type == "cuda":
        return list(getattr(torch.ops.cerberus_ocr, name)(*args))
    return [torch.zeros(shape, dtype=dtype, device=device) for shape, dtype in OUTPUTS[name]]


def _spatial_gather(d):
    return [_t(d, FEATS, 301), _t(d, LOGITS, 302, -3.0, 3.0), 1.0], (0, 1)


def _spatial_gather_backward(d):
    (f, x, s), _ = _spatial_gather(d)
    context, _ = forward(d, "spatial_gather", [f, x, s])
    return [f, x, context, _t(d, TABLE, 303), s], ()


def _object_attention(d):
    return [_t(d, FEATS, 311), _t(d, TABLE, 312), _t(d, TABLE, 313), SCALE], (0, 1, 2)


def _object_attention_backward(d):
    (q, k, v, s), _ = _object_attention(d)
    _, attn = forward(d, "object_attention", [q, k, v, s])
    return [_t(d, FEATS, 314), q, k, v, attn, s], ()


CASES = {
    "spatial_gather": _spatial_gather,
    "spatial_gather_backward": _spatial_gather_backward,
    "object_attention": _object_attention,
    "object_attention_backward": _object_attention_backward,
}


def case(name, device, layout):
    """(args, differentiable) of ``name`` with every tensor argument in ``layout``."""
    args, differentiable = CASES[name](device)
    return [lay(a, layout) if isinstance(a, torch.Tensor) else a for a in args], tuple(differentiable)
