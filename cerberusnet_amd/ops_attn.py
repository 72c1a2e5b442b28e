"""torch.ops.cerberus_attn.* -- the multi-head attention core of the DETR head's transformer (nnet_models/detr/transformer.py) bound
to csrc/detr_attn.hip through the C ABI (include/cerberus_hip.h).  Per batch entry and head, with 32 channels per head,

    out = dropout(softmax(scale * q k^T + key_padding_mask)) v

without ever writing a tensor of size Lq x Lk.  ``q`` is (Lq,B,E), ``k`` and ``v`` are (Lk,B,E) with E = n_heads * 32: the tensors as
``F.linear`` leaves them and as ``out_proj`` wants them; ``key_padding_mask`` is (B,Lk) bool, True = the key is ignored.

    attention(q, k, v, n_heads, key_padding_mask, scale, dropout_p, seed) -> (out (Lq,B,E), lse (B,H,Lq), stats (B,H,Lq,2))
    attention_backward(grad_out, q, k, v, out, stats, n_heads, key_padding_mask, scale, dropout_p, seed, mask[3])
        -> (grad_q, grad_k, grad_v)
    attn_dropout_keep(seed, B, H, Lq, Lk, p) -> (B,H,Lq,Lk) bool

``lse`` is the log-sum-exp of every row of ``scale * q k^T + mask``; ``stats`` holds what it is made of, the row's maximum and its sum
of ``exp(. - maximum)``, and is what the backward recomputes the probabilities from: ``exp(s - max) / sum`` is the forward's own
expression, while ``exp(s - lse)`` would carry the rounding of ``lse`` and of ``s - lse`` (2^-22 for a hundred keys).

``mask`` says which gradients are wanted: the launches of the others are skipped, and a gradient that was not asked for comes back
as an empty (0,) tensor.  A gradient that is asked for has the same bits whatever else the mask asks for.

``seed`` is a one-element int64 tensor on the device: the kernels read it, the host never does, so a call can be captured in a
graph.  The keep decision is a stateless hash of (seed, b H + h, query, key) (csrc/attn_dropout.h); ``attn_dropout_keep`` writes it
out.  ``dropout_p == 0`` needs no seed.

A row whose keys are all masked gives zeros (``lse`` = -inf) and sends zero gradients; the stock chain gives NaN there.

The ops live in a library namespace of their own, ``cerberus_attn`` (tests/attn_op_cases.py is their table), under the contract of
DESIGN.md 3.23: inputs of any strides, named ``.contiguous()`` copies kept alive until the launch, outputs fresh with the default
strides, fake == real.  The raw ops carry no autograd formula; the differentiable entry point is ``detr_attention`` at the end (once
differentiable).

fp32 CUDA tensors with a head width of 32 only: everything else is the caller's to route to the stock ops (the modules do), and is
rejected here.  CPU tensors are rejected with RuntimeError: there is no CPU path.
"""
import torch
from torch.autograd.function import once_differentiable
from torch.library import Library

from . import _lib
from .ops import _stream_ptr

HEAD_DIM = 32                         # channels per head the kernels are built for

_def = Library("cerberus_attn", "DEF")
_def.define("attention(Tensor q, Tensor k, Tensor v, int n_heads, Tensor? key_padding_mask, float scale, float dropout_p, Tensor? seed)"
            " -> (Tensor out, Tensor lse, Tensor stats)")
_def.define("attention_backward(Tensor grad_out, Tensor q, Tensor k, Tensor v, Tensor out, Tensor stats, int n_heads, "
            "Tensor? key_padding_mask, float scale, float dropout_p, Tensor? seed, bool[3] mask) -> "
            "(Tensor grad_q, Tensor grad_k, Tensor grad_v)")
_def.define("attn_dropout_keep(Tensor seed, int B, int H, int Lq, int Lk, float p) -> Tensor")

_STOCK = "nn.MultiheadAttention, the backend='torch' route of nnet_models.detr.transformer"


def attn_fused_ok(q, k, v, n_heads):
    """What the fused route takes: fp32 CUDA tensors outside autocast, nothing empty, a head width of 32."""
    return (not torch.is_autocast_enabled() and q.dim() == 3 and n_heads > 0 and q.shape[-1] == n_heads * HEAD_DIM
            and all(t.is_cuda and t.dtype == torch.float32 and t.numel() > 0 for t in (q, k, v)))


def _check(what, q, k, v, n_heads, key_padding_mask, dropout_p, seed, extra=()):
    for name, t in (("q", q), ("k", k), ("v", v)) + tuple(extra):
        if t.dtype != torch.float32:
            raise RuntimeError("%s: %s must be float32, got %s (other types take the stock ops: %s)" % (what, name, t.dtype, _STOCK))
        if t.device != q.device:
            raise RuntimeError("%s: inputs on different devices: %s, %s" % (what, q.device, t.device))
    if q.dim() != 3 or k.dim() != 3:
        raise RuntimeError("%s: q and k must be (L, B, E) tensors, got %s and %s" % (what, tuple(q.shape), tuple(k.shape)))
    Lq, B, E = q.shape
    Lk = k.shape[0]
    if tuple(k.shape) != (Lk, B, E):
        raise RuntimeError("%s: k must be (Lk, %d, %d), got %s" % (what, B, E, tuple(k.shape)))
    if tuple(v.shape) != (Lk, B, E):
        raise RuntimeError("%s: v must be %s, got %s" % (what, (Lk, B, E), tuple(v.shape)))
    if n_heads < 1 or E % n_heads:
        raise RuntimeError("%s: %d channels do not split into %d heads" % (what, E, n_heads))
    if E // n_heads != HEAD_DIM:
        raise RuntimeError("%s: needs a head width of %d, got %d (other widths take the stock ops: %s)" % (what, HEAD_DIM, E // n_heads, _STOCK))
    if min(Lq, Lk, B) < 1:
        raise RuntimeError("%s: empty input %s, %s" % (what, tuple(q.shape), tuple(k.shape)))
    if key_padding_mask is not None:
        if key_padding_mask.dtype != torch.bool or tuple(key_padding_mask.shape) != (B, Lk) or key_padding_mask.device != q.device:
            raise RuntimeError("%s: key_padding_mask must be a (%d, %d) bool tensor on %s, got %s %s on %s" % (
                what, B, Lk, q.device, tuple(key_padding_mask.shape), key_padding_mask.dtype, key_padding_mask.device))
    if not 0.0 <= dropout_p < 1.0:
        raise RuntimeError("%s: dropout_p must be in [0, 1), got %r" % (what, dropout_p))
    if dropout_p > 0.0:
        if seed is None:
            raise RuntimeError("%s: dropout_p > 0 needs a seed tensor" % what)
        _check_seed(what, seed, q.device)
    return Lq, Lk, B, n_heads


def _check_seed(what, seed, device):
    if seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != device:
        raise RuntimeError("%s: seed must be a one-element int64 tensor on %s, got %s %s on %s" % (
            what, device, tuple(seed.shape), seed.dtype, seed.device))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _attention_cuda(q, k, v, n_heads, key_padding_mask, scale, dropout_p, seed):
    what = "cerberus_attn::attention"
    Lq, Lk, B, H = _check(what, q, k, v, n_heads, key_padding_mask, dropout_p, seed)
    # named: every copy lives until the launch is enqueued
    qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
    mc = None if key_padding_mask is None else key_padding_mask.contiguous()
    sc = seed.contiguous() if (seed is not None and dropout_p > 0.0) else None
    out = qc.new_empty(qc.shape)
    lse = qc.new_empty((B, H, Lq))
    stats = qc.new_empty((B, H, Lq, 2))
    with torch.cuda.device(qc.device):
        rc = _lib.get().cerberus_attn_forward(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), _ptr(mc), _ptr(sc), out.data_ptr(), lse.data_ptr(),
                                              stats.data_ptr(), Lq, Lk, B, H, HEAD_DIM, scale, dropout_p, 0, _stream_ptr(qc))
    _lib.check(rc, what)
    return out, lse, stats


def _masked(t, need):
    return t.new_empty(t.shape if need else (0,))


def _attention_backward_cuda(grad_out, q, k, v, out, stats, n_heads, key_padding_mask, scale, dropout_p, seed, mask):
    what = "cerberus_attn::attention_backward"
    Lq, Lk, B, H = _check(what, q, k, v, n_heads, key_padding_mask, dropout_p, seed, (("grad_out", grad_out), ("out", out), ("stats", stats)))
    if tuple(grad_out.shape) != tuple(q.shape) or tuple(out.shape) != tuple(q.shape):
        raise RuntimeError("%s: grad_out and out must be %s, got %s and %s" % (what, tuple(q.shape), tuple(grad_out.shape), tuple(out.shape)))
    if tuple(stats.shape) != (B, H, Lq, 2):
        raise RuntimeError("%s: stats must be %s, got %s" % (what, (B, H, Lq, 2), tuple(stats.shape)))
    need = [bool(m) for m in mask]
    # named: every copy lives until the launch is enqueued
    gc, qc, kc, vc, oc, lc = (t.contiguous() for t in (grad_out, q, k, v, out, stats))
    mc = None if key_padding_mask is None else key_padding_mask.contiguous()
    sc = seed.contiguous() if (seed is not None and dropout_p > 0.0) else None
    grad_q, grad_k, grad_v = _masked(qc, need[0]), _masked(kc, need[1]), _masked(vc, need[2])
    if any(need):
        delta = qc.new_empty((B, H, Lq))
        with torch.cuda.device(qc.device):
            rc = _lib.get().cerberus_attn_backward(gc.data_ptr(), qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), _ptr(mc), _ptr(sc), oc.data_ptr(),
                                                   lc.data_ptr(), grad_q.data_ptr() if need[0] else None,
                                                   grad_k.data_ptr() if need[1] else None, grad_v.data_ptr() if need[2] else None,
                                                   delta.data_ptr(), Lq, Lk, B, H, HEAD_DIM, scale, dropout_p, 0, _stream_ptr(qc))
        _lib.check(rc, what)
    return grad_q, grad_k, grad_v


def _keep_shape(what, B, H, Lq, Lk, p):
    if min(B, H, Lq, Lk) < 1:
        raise RuntimeError("%s: B, H, Lq and Lk must be positive, got %s" % (what, (B, H, Lq, Lk)))
    if not 0.0 <= p < 1.0:
        raise RuntimeError("%s: p must be in [0, 1), got %r" % (what, p))
    return (B, H, Lq, Lk)


def _attn_dropout_keep_cuda(seed, B, H, Lq, Lk, p):
    what = "cerberus_attn::attn_dropout_keep"
    shape = _keep_shape(what, B, H, Lq, Lk, p)
    _check_seed(what, seed, seed.device)
    sc = seed.contiguous()          # named: lives until the launch is enqueued
    keep = torch.empty(shape, dtype=torch.bool, device=sc.device)
    with torch.cuda.device(sc.device):
        rc = _lib.get().cerberus_attn_dropout_keep(sc.data_ptr(), keep.data_ptr(), B, H, Lq, Lk, p, _stream_ptr(sc))
    _lib.check(rc, what)
    return keep


def _attention_meta(q, k, v, n_heads, key_padding_mask, scale, dropout_p, seed):
    return q.new_empty(q.shape), q.new_empty((q.shape[1], n_heads, q.shape[0])), q.new_empty((q.shape[1], n_heads, q.shape[0], 2))


def _attention_backward_meta(grad_out, q, k, v, out, stats, n_heads, key_padding_mask, scale, dropout_p, seed, mask):
    return _masked(q, mask[0]), _masked(k, mask[1]), _masked(v, mask[2])


def _attn_dropout_keep_meta(seed, B, H, Lq, Lk, p):
    return torch.empty(_keep_shape("cerberus_attn::attn_dropout_keep", B, H, Lq, Lk, p), dtype=torch.bool, device=seed.device)


def _no_cpu(name):
    def _raise(*_a, **_k):
        raise RuntimeError("cerberus_attn::%s has no CPU implementation: this build is the MI355X HIP path only (move the tensors to "
                           "the GPU, or use the modules of nnet_models.detr, which take the stock ops there)" % name)
    return _raise


_def.impl("attention", _attention_cuda, "CUDA")
_def.impl("attention", _attention_meta, "Meta")
_def.impl("attention_backward", _attention_backward_cuda, "CUDA")
_def.impl("attention_backward", _attention_backward_meta, "Meta")
_def.impl("attn_dropout_keep", _attn_dropout_keep_cuda, "CUDA")
_def.impl("attn_dropout_keep", _attn_dropout_keep_meta, "Meta")
for _name in ("attention", "attention_backward", "attn_dropout_keep"):
    _def.impl(_name, _no_cpu(_name), "CPU")


def draw_seed(device):
    """A fresh one-element int64 seed on ``device``, drawn there from torch's generator: no host read, capturable."""
    return torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=device)


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, n_heads, key_padding_mask, scale, dropout_p, seed):
        out, lse, stats = torch.ops.cerberus_attn.attention(q, k, v, n_heads, key_padding_mask, scale, dropout_p, seed)
        ctx.save_for_backward(q, k, v, out, stats, key_padding_mask, seed)
        ctx.params = (n_heads, scale, dropout_p)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_lse):
        q, k, v, out, stats, key_padding_mask, seed = ctx.saved_tensors
        n_heads, scale, dropout_p = ctx.params
        need = list(ctx.needs_input_grad[:3])
        if not any(need):
            return (None,) * 8
        grads = torch.ops.cerberus_attn.attention_backward(grad_out, q, k, v, out, stats, n_heads, key_padding_mask, scale, dropout_p, seed,
                                                           need)
        return tuple(g if n else None for g, n in zip(grads, need)) + (None,) * 5


def detr_attention(q, k, v, n_heads, key_padding_mask=None, dropout_p=0.0, seed=None, scale=None):
    """``dropout(softmax(scale * q k^T + key_padding_mask)) v`` per batch entry and head, differentiable once: ``q`` (Lq,B,E), ``k`` and
    ``v`` (Lk,B,E), E = 32 ``n_heads``, ``key_padding_mask`` (B,Lk) bool with True = ignored -> (Lq,B,E).  ``scale`` defaults to
    32 ** -0.5.  With ``dropout_p > 0`` and no ``seed`` (a one-element int64 tensor on the device) one is drawn on the device."""
    dropout_p = float(dropout_p)
    if scale is None:
        scale = (q.shape[-1] // n_heads) ** -0.5
    if dropout_p > 0.0 and seed is None:
        seed = draw_seed(q.device)
    return _Attention.apply(q, k, v, int(n_heads), key_padding_mask, float(scale), dropout_p, seed)[0]
