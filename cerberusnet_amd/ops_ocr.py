"""torch.ops.cerberus_ocr.* -- the OCR segmentation head's two own steps (nnet_models/ocr_utils.py) bound to csrc/ocr_head.hip
through the C ABI (include/cerberus_hip.h):

    spatial_gather(feats, logits, scale) -> (context (B,C,K), lse (B,K))
    spatial_gather_backward(feats, logits, context, grad_context, scale) -> (grad_feats, grad_logits)
    object_attention(query, key, value, scale) -> (context (B,Kc,H,W), attn (B,R,H,W))
    object_attention_backward(grad_context, query, key, value, attn, scale) -> (grad_query, grad_key, grad_value)

The ops live in a library namespace of their own, ``cerberus_ocr``: tests/test_op_contract_cpu.py holds the set of ``cerberus::`` ops
equal to the table of tests/op_cases.py, and these ops have a table of their own (tests/ocr_op_cases.py) under the same contract
(DESIGN.md 3.23): inputs of any strides, named ``.contiguous()`` copies kept alive until the launch, outputs fresh with the default
strides, fake == real.  A later change may fold the two tables, and with them the two namespaces, into one.

fp32 CUDA tensors, 1 <= R <= 32 regions: everything else is the caller's to route to the stock ops (the modules do), and is rejected
here.  CPU tensors are rejected with RuntimeError: there is no CPU path.
"""
import torch
from torch.library import Library

from . import _lib
from .ops import _fresh_like, _stream_ptr

OCR_MAX_REGIONS = 32          # regions / classes of the fused route
OCR_CHUNK = 256               # P: pixels per pooling workgroup (one partial per chunk, image, channel and region)
OCR_TILE = 64                 # T: channels per LDS table of the lane-per-pixel kernels

_def = Library("cerberus_ocr", "DEF")
_def.define("spatial_gather(Tensor feats, Tensor logits, float scale) -> (Tensor context, Tensor lse)")
_def.define("spatial_gather_backward(Tensor feats, Tensor logits, Tensor context, Tensor grad_context, float scale) -> "
            "(Tensor grad_feats, Tensor grad_logits)")
_def.define("object_attention(Tensor query, Tensor key, Tensor value, float scale) -> (Tensor context, Tensor attn)")
_def.define("object_attention_backward(Tensor grad_context, Tensor query, Tensor key, Tensor value, Tensor attn, float scale) -> "
            "(Tensor grad_query, Tensor grad_key, Tensor grad_value)")


def ocr_fused_ok(*tensors, regions):
    """What the fused route takes: fp32 CUDA tensors outside autocast, 1 <= regions <= 32, nothing empty."""
    return (1 <= regions <= OCR_MAX_REGIONS and not torch.is_autocast_enabled()
            and all(t.is_cuda and t.dtype == torch.float32 and t.numel() > 0 for t in tensors))


def _ocr_workspace_bytes(B, C, R, HW):
    """cerberus_ocr_workspace_bytes in pure Python (a test holds the two equal): floats -- two row statistics and one dot product
    per (b, r), padded to 16 bytes, then one partial per (image, chunk of 256 pixels, channel, region)."""
    if min(B, C, R, HW) <= 0 or R > OCR_MAX_REGIONS:
        return 0
    chunks = (HW + OCR_CHUNK - 1) // OCR_CHUNK
    if (HW > 0x7fffffff - 1024 or C * R > 0x7fffffff or B * chunks > 0x7fffffff or B * ((C * R + 255) // 256) > 0x7fffffff
            or B * R > 0x7fffffff):
        return 0
    return 4 * (((3 * B * R + 3) // 4) * 4 + B * chunks * C * R)


def _workspace(B, C, R, HW, device):
    nbytes = _lib.get().cerberus_ocr_workspace_bytes(B, C, R, HW)
    return torch.empty((max(nbytes, 16) + 3) // 4, dtype=torch.float32, device=device), nbytes


def _check(what, maps, tables, regions):
    """``maps``: (name, tensor, channels or None) of the 4-D tensors, ``tables``: (name, tensor, shape) of the 3-D ones."""
    first = maps[0][1]
    if first.dim() != 4:
        raise RuntimeError("%s: %s must be a 4-D (B,C,H,W) tensor, got %s" % (what, maps[0][0], tuple(first.shape)))
    B, _, H, W = first.shape
    for name, t, channels in maps:
        want = (B, t.shape[1] if channels is None and t.dim() == 4 else channels, H, W)
        if t.dim() != 4 or tuple(t.shape) != want:
            raise RuntimeError("%s: %s must be %s, got %s" % (what, name, want, tuple(t.shape)))
    for name, t, shape in tables:
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError("%s: %s must be %s, got %s" % (what, name, tuple(shape), tuple(t.shape)))
    for name, t in [(n, t) for n, t, _ in maps] + [(n, t) for n, t, _ in tables]:
        if t.dtype != torch.float32:
            raise RuntimeError("%s: %s must be float32, got %s (16-bit tensors take the stock-op path of nnet_models.ocr_utils)"
                               % (what, name, t.dtype))
        if t.device != first.device:
            raise RuntimeError("%s: inputs on different devices: %s, %s" % (what, first.device, t.device))
    if not 1 <= regions <= OCR_MAX_REGIONS:
        raise RuntimeError("%s: needs 1..%d regions, got %d (nnet_models.ocr_utils takes the stock-op path)"
                           % (what, OCR_MAX_REGIONS, regions))
    if first.numel() == 0:
        raise RuntimeError("%s: empty input %s" % (what, tuple(first.shape)))


def _spatial_gather_cuda(feats, logits, scale):
    what = "cerberus_ocr::spatial_gather"
    _check(what, [("feats", feats, None), ("logits", logits, None)], [], logits.shape[1] if logits.dim() == 4 else 0)
    f, x = feats.contiguous(), logits.contiguous()
    B, C, H, W = f.shape
    K = x.shape[1]
    context, lse = f.new_empty((B, C, K)), f.new_empty((B, K))
    ws, ws_bytes = _workspace(B, C, K, H * W, f.device)
    with torch.cuda.device(f.device):
        rc = _lib.get().cerberus_ocr_gather_forward(f.data_ptr(), x.data_ptr(), context.data_ptr(), lse.data_ptr(), ws.data_ptr(),
                                                    ws_bytes, B, C, K, H * W, float(scale), 0, _stream_ptr(f))
    _lib.check(rc, what)
    return context, lse


def _spatial_gather_meta(feats, logits, scale):
    B, C, K = feats.shape[0], feats.shape[1], logits.shape[1]
    return feats.new_empty((B, C, K)), feats.new_empty((B, K))


def _spatial_gather_backward_cuda(feats, logits, context, grad_context, scale):
    what = "cerberus_ocr::spatial_gather_backward"
    K = logits.shape[1] if logits.dim() == 4 else 0
    table = (feats.shape[0], feats.shape[1], K) if feats.dim() == 4 else ()
    _check(what, [("feats", feats, None), ("logits", logits, None)], [("context", context, table), ("grad_context", grad_context, table)], K)
    # named: every copy lives until the launch is enqueued
    f, x, c, g = feats.contiguous(), logits.contiguous(), context.contiguous(), grad_context.contiguous()
    B, C, H, W = f.shape
    grad_feats, grad_logits = _fresh_like(f), _fresh_like(x)          # every element is written by the kernel
    ws, ws_bytes = _workspace(B, C, K, H * W, f.device)
    with torch.cuda.device(f.device):
        rc = _lib.get().cerberus_ocr_gather_backward(f.data_ptr(), x.data_ptr(), c.data_ptr(), g.data_ptr(), grad_feats.data_ptr(),
                                                     grad_logits.data_ptr(), ws.data_ptr(), ws_bytes, B, C, K, H * W, float(scale), 0,
                                                     _stream_ptr(f))
    _lib.check(rc, what)
    return grad_feats, grad_logits


def _attention_check(what, query, key, value, extra_maps=(), attn=None):
    R = key.shape[2] if key.dim() == 3 else 0
    table = (query.shape[0], query.shape[1], R) if query.dim() == 4 else ()
    maps = [("query", query, None)] + [(n, t, query.shape[1] if query.dim() == 4 else None) for n, t in extra_maps]
    if attn is not None:
        maps.append(("attn", attn, R))
    _check(what, maps, [("key", key, table), ("value", value, table)], R)
    return R


def _object_attention_cuda(query, key, value, scale):
    what = "cerberus_ocr::object_attention"
    R = _attention_check(what, query, key, value)
    q, k, v = query.contiguous(), key.contiguous(), value.contiguous()
    B, C, H, W = q.shape
    context, attn = _fresh_like(q), q.new_empty((B, R, H, W))
    with torch.cuda.device(q.device):
        rc = _lib.get().cerberus_ocr_attention_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), context.data_ptr(), attn.data_ptr(), B, C,
                                                       R, H * W, float(scale), 0, _stream_ptr(q))
    _lib.check(rc, what)
    return context, attn


def _object_attention_meta(query, key, value, scale):
    B, _, H, W = query.shape
    return _fresh_like(query), query.new_empty((B, key.shape[2], H, W))


def _object_attention_backward_cuda(grad_context, query, key, value, attn, scale):
    what = "cerberus_ocr::object_attention_backward"
    R = _attention_check(what, query, key, value, extra_maps=[("grad_context", grad_context)], attn=attn)
    # named: every copy lives until the launch is enqueued
    g, q, k, v, a = grad_context.contiguous(), query.contiguous(), key.contiguous(), value.contiguous(), attn.contiguous()
    B, C, H, W = q.shape
    grad_query, grad_key, grad_value = _fresh_like(q), _fresh_like(k), _fresh_like(v)
    dsim = q.new_empty((B, R, H, W))        # the scratch of the two poolings
    ws, ws_bytes = _workspace(B, C, R, H * W, q.device)
    with torch.cuda.device(q.device):
        rc = _lib.get().cerberus_ocr_attention_backward(g.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), a.data_ptr(),
                                                        grad_query.data_ptr(), grad_key.data_ptr(), grad_value.data_ptr(), dsim.data_ptr(),
                                                        ws.data_ptr(), ws_bytes, B, C, R, H * W, float(scale), 0, _stream_ptr(q))
    _lib.check(rc, what)
    return grad_query, grad_key, grad_value


def _no_cpu(name):
    def _raise(*_a, **_k):
        raise RuntimeError("cerberus_ocr::%s has no CPU implementation: this build is the MI355X HIP path only (move the tensors to "
                           "the GPU, or use the modules of nnet_models.ocr_utils, which take the stock ops there)" % name)
    return _raise


_def.impl("spatial_gather", _spatial_gather_cuda, "CUDA")
_def.impl("spatial_gather", _spatial_gather_meta, "Meta")
_def.impl("spatial_gather", _no_cpu("spatial_gather"), "CPU")
_def.impl("spatial_gather_backward", _spatial_gather_backward_cuda, "CUDA")
_def.impl("spatial_gather_backward", lambda f, x, c, g, s: (_fresh_like(f), _fresh_like(x)), "Meta")
_def.impl("spatial_gather_backward", _no_cpu("spatial_gather_backward"), "CPU")
_def.impl("object_attention", _object_attention_cuda, "CUDA")
_def.impl("object_attention", _object_attention_meta, "Meta")
_def.impl("object_attention", _no_cpu("object_attention"), "CPU")
_def.impl("object_attention_backward", _object_attention_backward_cuda, "CUDA")
_def.impl("object_attention_backward", lambda g, q, k, v, a, s: (_fresh_like(q), _fresh_like(k), _fresh_like(v)), "Meta")
_def.impl("object_attention_backward", _no_cpu("object_attention_backward"), "CPU")


def _gather_setup(ctx, inputs, output):
    feats, logits, scale = inputs
    context, lse = output
    ctx.save_for_backward(feats, logits, context)
    ctx.scale = scale
    ctx.mark_non_differentiable(lse)


def _gather_backward(ctx, grad_context, _grad_lse):
    feats, logits, context = ctx.saved_tensors
    if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
        return None, None, None
    gf, gl = torch.ops.cerberus_ocr.spatial_gather_backward(feats, logits, context, grad_context, ctx.scale)
    return (gf if ctx.needs_input_grad[0] else None, gl if ctx.needs_input_grad[1] else None, None)


def _attention_setup(ctx, inputs, output):
    query, key, value, scale = inputs
    _context, attn = output
    ctx.save_for_backward(query, key, value, attn)
    ctx.scale = scale
    ctx.mark_non_differentiable(attn)


def _attention_backward(ctx, grad_context, _grad_attn):
    query, key, value, attn = ctx.saved_tensors
    if not any(ctx.needs_input_grad[:3]):
        return None, None, None, None
    gq, gk, gv = torch.ops.cerberus_ocr.object_attention_backward(grad_context, query, key, value, attn, ctx.scale)
    return (gq if ctx.needs_input_grad[0] else None, gk if ctx.needs_input_grad[1] else None,
            gv if ctx.needs_input_grad[2] else None, None)


def _no_double(name):
    def _raise(ctx, *grads):
        raise RuntimeError("cerberus_ocr::%s is not differentiable (no double backward)" % name)
    return _raise


torch.library.register_autograd("cerberus_ocr::spatial_gather", _gather_backward, setup_context=_gather_setup)
torch.library.register_autograd("cerberus_ocr::spatial_gather_backward", _no_double("spatial_gather_backward"),
                                setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus_ocr::object_attention", _attention_backward, setup_context=_attention_setup)
torch.library.register_autograd("cerberus_ocr::object_attention_backward", _no_double("object_attention_backward"),
                                setup_context=lambda ctx, inputs, output: None)


def spatial_gather(feats, logits, scale=1.0):
    """context (B,C,K) = softmax over the pixels of ``scale * logits`` (B,K,H,W), times ``feats`` (B,C,H,W)."""
    return torch.ops.cerberus_ocr.spatial_gather(feats, logits, float(scale))[0]


def object_attention(query, key, value, scale):
    """context (B,Kc,H,W) = softmax over the regions of ``scale * query . key``, times ``value``; key / value are (B,Kc,R)."""
    return torch.ops.cerberus_ocr.object_attention(query, key, value, float(scale))[0]
