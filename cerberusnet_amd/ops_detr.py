"""torch.ops.cerberus_detr.* -- the DETR set criterion (loss_functions/detr_loss.py, nnet_models/detr/matcher.py) bound to
csrc/detr_loss.hip through the C ABI (include/cerberus_hip.h):

    match_cost(logits, boxes, tgt_labels, tgt_boxes, tgt_count, w_class, w_bbox, w_giou) -> cost (N,Q,Tmax)
    lsap(cost, tgt_count) -> match (N,Q) int32
    hungarian_match(logits, boxes, tgt_labels, tgt_boxes, tgt_count, w_class, w_bbox, w_giou) -> (match (N,Q) int32, status (N,) int32)
    set_loss(logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes) -> (losses (L,4), wsum (L,) float64)
    set_loss_backward(grad_losses, logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes, wsum)
        -> (grad_logits, grad_boxes)

logits (N,Q,C1), boxes (N,Q,4) cxcywh, N = L B: the decoder layers stacked layer-major over the batch; tgt_labels (B,Tmax) int64,
tgt_boxes (B,Tmax,4), tgt_count (B,) int32: the targets padded per image; image n reads row n % B.  losses columns: loss_ce,
loss_bbox, loss_giou, cardinality_error.  num_boxes is a (1,) float32 tensor on the device.

The ops live in a library namespace of their own, ``cerberus_detr``, with a table of their own (tests/detr_op_cases.py) under the
contract of DESIGN.md 3.23, as ops_ocr.py's do: inputs of any strides, named ``.contiguous()`` copies kept alive until the launch,
outputs fresh with the default strides, fake == real.

fp32 CUDA tensors within the fused limits (``detr_fused_ok``): everything else is the caller's to route to the stock ops (the
modules do), and is rejected here.  CPU tensors are rejected with RuntimeError: there is no CPU path.
"""
import torch
from torch.library import Library

from . import _lib
from .ops import _stream_ptr

DETR_MAX_QUERIES = 256
DETR_MAX_TARGETS = 128
DETR_MAX_COST = 16384         # Q * Tmax: the 64 KiB fp32 cost matrix in LDS
DETR_MAX_CLASSES = 256
STATUS_NON_FINITE = 1         # bit 0 of status: a non-finite cost entry was replaced
STATUS_BAD_LABEL = 2          # bit 1: a counted target's label is outside [0, C1)

_def = Library("cerberus_detr", "DEF")
_def.define("match_cost(Tensor logits, Tensor boxes, Tensor tgt_labels, Tensor tgt_boxes, Tensor tgt_count, float w_class, "
            "float w_bbox, float w_giou) -> Tensor")
_def.define("lsap(Tensor cost, Tensor tgt_count) -> Tensor")
_def.define("hungarian_match(Tensor logits, Tensor boxes, Tensor tgt_labels, Tensor tgt_boxes, Tensor tgt_count, float w_class, "
            "float w_bbox, float w_giou) -> (Tensor match, Tensor status)")
_def.define("set_loss(Tensor logits, Tensor boxes, Tensor match, Tensor tgt_labels, Tensor tgt_boxes, Tensor tgt_count, Tensor weight, "
            "Tensor num_boxes) -> (Tensor losses, Tensor wsum)")
_def.define("set_loss_backward(Tensor grad_losses, Tensor logits, Tensor boxes, Tensor match, Tensor tgt_labels, Tensor tgt_boxes, "
            "Tensor tgt_count, Tensor weight, Tensor num_boxes, Tensor wsum) -> (Tensor grad_logits, Tensor grad_boxes)")


def _detr_fused_ok(Q, Tmax, C1):
    """cerberus_detr_fused_ok in pure Python (a test holds the two equal)."""
    return (1 <= Q <= DETR_MAX_QUERIES and 0 <= Tmax <= DETR_MAX_TARGETS and Q * Tmax <= DETR_MAX_COST
            and 2 <= C1 <= DETR_MAX_CLASSES)


def _detr_workspace_bytes(N):
    """cerberus_detr_workspace_bytes in pure Python: five float64 partial sums per image."""
    return 40 * N if N > 0 else 0


def detr_fused_ok(logits, boxes, Tmax):
    """What the fused route takes: fp32 CUDA logits (N,Q,C1) and boxes (N,Q,4) outside autocast, within the limits."""
    return (logits.dim() == 3 and logits.is_cuda and boxes.is_cuda and logits.dtype == torch.float32 and boxes.dtype == torch.float32
            and not torch.is_autocast_enabled() and _detr_fused_ok(logits.shape[1], Tmax, logits.shape[2]))


def _check_targets(what, first, tgt_labels, tgt_boxes, tgt_count):
    if tgt_count.dim() != 1 or tgt_count.shape[0] < 1 or tgt_count.dtype != torch.int32:
        raise RuntimeError("%s: tgt_count must be a (B,) int32 tensor, B >= 1, got %s %s" % (what, tuple(tgt_count.shape), tgt_count.dtype))
    B = tgt_count.shape[0]
    if tgt_labels is not None:
        if tgt_labels.dim() != 2 or tgt_labels.shape[0] != B or tgt_labels.dtype != torch.int64:
            raise RuntimeError("%s: tgt_labels must be a (B,Tmax) int64 tensor with B = %d, got %s %s"
                               % (what, B, tuple(tgt_labels.shape), tgt_labels.dtype))
        if tuple(tgt_boxes.shape) != (B, tgt_labels.shape[1], 4) or tgt_boxes.dtype != torch.float32:
            raise RuntimeError("%s: tgt_boxes must be a %s float32 tensor, got %s %s"
                               % (what, (B, tgt_labels.shape[1], 4), tuple(tgt_boxes.shape), tgt_boxes.dtype))
    for t in (tgt_labels, tgt_boxes, tgt_count):
        if t is not None and t.device != first.device:
            raise RuntimeError("%s: inputs on different devices: %s, %s" % (what, first.device, t.device))
    if first.shape[0] % B != 0:
        raise RuntimeError("%s: %d images are no multiple of the batch of %d target rows" % (what, first.shape[0], B))
    return B


def _check_predictions(what, logits, boxes, Tmax):
    if logits.dim() != 3 or tuple(boxes.shape) != (logits.shape[0], logits.shape[1], 4):
        raise RuntimeError("%s: logits must be (N,Q,C1) and boxes (N,Q,4), got %s and %s" % (what, tuple(logits.shape), tuple(boxes.shape)))
    for name, t in (("logits", logits), ("boxes", boxes)):
        if t.dtype != torch.float32:
            raise RuntimeError("%s: %s must be float32, got %s (16-bit tensors take the stock-op route of the modules)" % (what, name, t.dtype))
    if boxes.device != logits.device:
        raise RuntimeError("%s: inputs on different devices: %s, %s" % (what, logits.device, boxes.device))
    N, Q, C1 = logits.shape
    if not _detr_fused_ok(Q, Tmax, C1):
        raise RuntimeError("%s: Q = %d, Tmax = %d, C1 = %d is outside the fused limits (1..%d queries, 0..%d targets, Q Tmax <= %d, "
                           "2..%d classes): the modules take the stock-op route" % (what, Q, Tmax, C1, DETR_MAX_QUERIES, DETR_MAX_TARGETS,
                                                                                     DETR_MAX_COST, DETR_MAX_CLASSES))
    return N, Q, C1


def _match_cost_cuda(logits, boxes, tgt_labels, tgt_boxes, tgt_count, w_class, w_bbox, w_giou):
    what = "cerberus_detr::match_cost"
    B = _check_targets(what, logits, tgt_labels, tgt_boxes, tgt_count)
    Tmax = tgt_labels.shape[1]
    N, Q, C1 = _check_predictions(what, logits, boxes, Tmax)
    # named: every copy lives until the launch is enqueued
    x, p, tl, tb, tc = logits.contiguous(), boxes.contiguous(), tgt_labels.contiguous(), tgt_boxes.contiguous(), tgt_count.contiguous()
    cost = x.new_empty((N, Q, Tmax))
    with torch.cuda.device(x.device):
        rc = _lib.get().cerberus_detr_match_cost(x.data_ptr(), p.data_ptr(), tl.data_ptr(), tb.data_ptr(), tc.data_ptr(), cost.data_ptr(),
                                                 None, N, B, Q, C1, Tmax, float(w_class), float(w_bbox), float(w_giou), 0, _stream_ptr(x))
    _lib.check(rc, what)
    return cost


def _lsap_cuda(cost, tgt_count):
    what = "cerberus_detr::lsap"
    if cost.dim() != 3 or cost.dtype != torch.float32:
        raise RuntimeError("%s: cost must be a (N,Q,Tmax) float32 tensor, got %s %s" % (what, tuple(cost.shape), cost.dtype))
    B = _check_targets(what, cost, None, None, tgt_count)
    N, Q, Tmax = cost.shape
    if not _detr_fused_ok(Q, Tmax, 2):
        raise RuntimeError("%s: Q = %d, Tmax = %d is outside the fused limits (1..%d queries, 0..%d targets, Q Tmax <= %d)"
                           % (what, Q, Tmax, DETR_MAX_QUERIES, DETR_MAX_TARGETS, DETR_MAX_COST))
    c, tc = cost.contiguous(), tgt_count.contiguous()
    match = c.new_empty((N, Q), dtype=torch.int32)
    with torch.cuda.device(c.device):
        rc = _lib.get().cerberus_detr_lsap(c.data_ptr(), tc.data_ptr(), match.data_ptr(), None, N, B, Q, Tmax, _stream_ptr(c))
    _lib.check(rc, what)
    return match


def _hungarian_match_cuda(logits, boxes, tgt_labels, tgt_boxes, tgt_count, w_class, w_bbox, w_giou):
    what = "cerberus_detr::hungarian_match"
    B = _check_targets(what, logits, tgt_labels, tgt_boxes, tgt_count)
    Tmax = tgt_labels.shape[1]
    N, Q, C1 = _check_predictions(what, logits, boxes, Tmax)
    x, p, tl, tb, tc = logits.contiguous(), boxes.contiguous(), tgt_labels.contiguous(), tgt_boxes.contiguous(), tgt_count.contiguous()
    match, status = x.new_empty((N, Q), dtype=torch.int32), x.new_empty((N,), dtype=torch.int32)
    with torch.cuda.device(x.device):
        rc = _lib.get().cerberus_detr_hungarian_match(x.data_ptr(), p.data_ptr(), tl.data_ptr(), tb.data_ptr(), tc.data_ptr(),
                                                      match.data_ptr(), status.data_ptr(), N, B, Q, C1, Tmax, float(w_class),
                                                      float(w_bbox), float(w_giou), 0, _stream_ptr(x))
    _lib.check(rc, what)
    return match, status


def _check_loss(what, logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes):
    B = _check_targets(what, logits, tgt_labels, tgt_boxes, tgt_count)
    N, Q, C1 = _check_predictions(what, logits, boxes, tgt_labels.shape[1])
    if tuple(match.shape) != (N, Q) or match.dtype != torch.int32:
        raise RuntimeError("%s: match must be a %s int32 tensor, got %s %s" % (what, (N, Q), tuple(match.shape), match.dtype))
    if tuple(weight.shape) != (C1,) or weight.dtype != torch.float32:
        raise RuntimeError("%s: weight must be a (%d,) float32 tensor, got %s %s" % (what, C1, tuple(weight.shape), weight.dtype))
    if num_boxes.numel() != 1 or num_boxes.dtype != torch.float32:
        raise RuntimeError("%s: num_boxes must hold one float32, got %s %s" % (what, tuple(num_boxes.shape), num_boxes.dtype))
    for t in (match, weight, num_boxes):
        if t.device != logits.device:
            raise RuntimeError("%s: inputs on different devices: %s, %s" % (what, logits.device, t.device))
    return N, B, Q, C1, tgt_labels.shape[1]


def _set_loss_cuda(logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes):
    what = "cerberus_detr::set_loss"
    N, B, Q, C1, Tmax = _check_loss(what, logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes)
    # named: every copy lives until the launch is enqueued
    x, p, m, tl, tb = logits.contiguous(), boxes.contiguous(), match.contiguous(), tgt_labels.contiguous(), tgt_boxes.contiguous()
    tc, w, nb = tgt_count.contiguous(), weight.contiguous(), num_boxes.contiguous()
    L = N // B
    losses, wsum = x.new_empty((L, 4)), x.new_empty((L,), dtype=torch.float64)
    ws_bytes = _detr_workspace_bytes(N)
    ws = x.new_empty((max(ws_bytes, 8) // 8,), dtype=torch.float64)
    with torch.cuda.device(x.device):
        rc = _lib.get().cerberus_detr_set_loss_forward(x.data_ptr(), p.data_ptr(), m.data_ptr(), tl.data_ptr(), tb.data_ptr(), tc.data_ptr(),
                                                       w.data_ptr(), nb.data_ptr(), losses.data_ptr(), wsum.data_ptr(), ws.data_ptr(),
                                                       ws_bytes, N, B, Q, C1, Tmax, 0, _stream_ptr(x))
    _lib.check(rc, what)
    return losses, wsum


def _set_loss_backward_cuda(grad_losses, logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes, wsum):
    what = "cerberus_detr::set_loss_backward"
    N, B, Q, C1, Tmax = _check_loss(what, logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes)
    L = N // B
    if tuple(grad_losses.shape) != (L, 4) or grad_losses.dtype != torch.float32:
        raise RuntimeError("%s: grad_losses must be a %s float32 tensor, got %s %s" % (what, (L, 4), tuple(grad_losses.shape), grad_losses.dtype))
    if tuple(wsum.shape) != (L,) or wsum.dtype != torch.float64:
        raise RuntimeError("%s: wsum must be a (%d,) float64 tensor, got %s %s" % (what, L, tuple(wsum.shape), wsum.dtype))
    # named: every copy lives until the launch is enqueued
    g, x, p, m, tl = grad_losses.contiguous(), logits.contiguous(), boxes.contiguous(), match.contiguous(), tgt_labels.contiguous()
    tb, tc, w, nb, sw = tgt_boxes.contiguous(), tgt_count.contiguous(), weight.contiguous(), num_boxes.contiguous(), wsum.contiguous()
    grad_logits, grad_boxes = x.new_empty(x.shape), x.new_empty(p.shape)          # every element is written by the kernel
    with torch.cuda.device(x.device):
        rc = _lib.get().cerberus_detr_set_loss_backward(x.data_ptr(), p.data_ptr(), m.data_ptr(), tl.data_ptr(), tb.data_ptr(), tc.data_ptr(),
                                                        w.data_ptr(), nb.data_ptr(), sw.data_ptr(), g.data_ptr(), grad_logits.data_ptr(),
                                                        grad_boxes.data_ptr(), N, B, Q, C1, Tmax, 0, _stream_ptr(x))
    _lib.check(rc, what)
    return grad_logits, grad_boxes


def _match_cost_meta(logits, boxes, tgt_labels, tgt_boxes, tgt_count, w_class, w_bbox, w_giou):
    return logits.new_empty((logits.shape[0], logits.shape[1], tgt_labels.shape[1]))


def _hungarian_match_meta(logits, boxes, tgt_labels, tgt_boxes, tgt_count, w_class, w_bbox, w_giou):
    N, Q = logits.shape[0], logits.shape[1]
    return logits.new_empty((N, Q), dtype=torch.int32), logits.new_empty((N,), dtype=torch.int32)


def _set_loss_meta(logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes):
    L = logits.shape[0] // tgt_count.shape[0]
    return logits.new_empty((L, 4)), logits.new_empty((L,), dtype=torch.float64)


def _set_loss_backward_meta(grad_losses, logits, boxes, *_rest):
    return logits.new_empty(logits.shape), logits.new_empty(boxes.shape)


def _no_cpu(name):
    def _raise(*_a, **_k):
        raise RuntimeError("cerberus_detr::%s has no CPU implementation: this build is the MI355X HIP path only (move the tensors to "
                           "the GPU, or use backend='torch' of HungarianMatcher / DetrLoss, which take the stock ops there)" % name)
    return _raise


for _name, _cuda, _meta in (("match_cost", _match_cost_cuda, _match_cost_meta),
                            ("lsap", _lsap_cuda, lambda cost, tgt_count: cost.new_empty((cost.shape[0], cost.shape[1]), dtype=torch.int32)),
                            ("hungarian_match", _hungarian_match_cuda, _hungarian_match_meta),
                            ("set_loss", _set_loss_cuda, _set_loss_meta),
                            ("set_loss_backward", _set_loss_backward_cuda, _set_loss_backward_meta)):
    _def.impl(_name, _cuda, "CUDA")
    _def.impl(_name, _meta, "Meta")
    _def.impl(_name, _no_cpu(_name), "CPU")


def _set_loss_setup(ctx, inputs, output):
    logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes = inputs
    _losses, wsum = output
    ctx.save_for_backward(logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes, wsum)
    ctx.mark_non_differentiable(wsum)


def _set_loss_backward(ctx, grad_losses, _grad_wsum):
    logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes, wsum = ctx.saved_tensors
    if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
        return (None,) * 8
    gl, gb = torch.ops.cerberus_detr.set_loss_backward(grad_losses, logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight,
                                                       num_boxes, wsum)
    return (gl if ctx.needs_input_grad[0] else None, gb if ctx.needs_input_grad[1] else None) + (None,) * 6


def _no_double(name):
    def _raise(ctx, *grads):
        raise RuntimeError("cerberus_detr::%s is not differentiable (no double backward)" % name)
    return _raise


torch.library.register_autograd("cerberus_detr::set_loss", _set_loss_backward, setup_context=_set_loss_setup)
torch.library.register_autograd("cerberus_detr::set_loss_backward", _no_double("set_loss_backward"),
                                setup_context=lambda ctx, inputs, output: None)


def match_cost(logits, boxes, tgt_labels, tgt_boxes, tgt_count, w_class=1.0, w_bbox=1.0, w_giou=1.0):
    """The matcher's (N,Q,Tmax) cost matrix, padding columns zeroed (for inspection: ``hungarian_match`` never writes it)."""
    return torch.ops.cerberus_detr.match_cost(logits, boxes, tgt_labels, tgt_boxes, tgt_count, float(w_class), float(w_bbox), float(w_giou))


def lsap(cost, tgt_count):
    """match (N,Q) int32 of a caller-given (N,Q,Tmax) fp32 cost matrix: the column of each row's assignment, or -1."""
    return torch.ops.cerberus_detr.lsap(cost, tgt_count)


def hungarian_match(logits, boxes, tgt_labels, tgt_boxes, tgt_count, w_class=1.0, w_bbox=1.0, w_giou=1.0):
    """(match (N,Q) int32, status (N,) int32): the optimal assignment of every image of every layer, in one launch."""
    return torch.ops.cerberus_detr.hungarian_match(logits, boxes, tgt_labels, tgt_boxes, tgt_count, float(w_class), float(w_bbox),
                                                   float(w_giou))


def set_loss(logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes):
    """losses (L,4): loss_ce, loss_bbox, loss_giou, cardinality_error of every layer; differentiable in logits and boxes."""
    return torch.ops.cerberus_detr.set_loss(logits, boxes, match, tgt_labels, tgt_boxes, tgt_count, weight, num_boxes)[0]
