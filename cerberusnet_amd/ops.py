"""torch.ops.cerberus.* -- the reference's operator names and schemas, bound to
the HIP kernels through the C ABI (include/cerberus_hip.h).

Reference registration being replaced
(/root/reference/nnet_training/correlation_package/correlation_cuda.cpp:45-48):

    TORCH_LIBRARY(cerberus, m) {
        m.def("correlation", correlation_forward_cuda);            // :3-26
        m.def("correlation_backward", correlation_backward_cuda);  // :28-43
    }

Same names, same argument order (the ONNX symbolic in utilities/onnx_export.py:18-23
depends on it), same ownership (the op allocates and returns its outputs), same
threading contract (enqueue on the current stream, never synchronise).  Extra
ops ``cerberus::flow_warp`` / ``flow_warp_backward`` / ``correlation_leaky``
carry the fused warp (UnFlowLoss.py:83-94) and the fused LeakyReLU epilogue
(pwcnet_sfd.py:181-182).

CPU tensors are rejected with RuntimeError: the product has no CPU path.
PyTorch is plumbing here (device memory, streams, autograd graph) -- the
arithmetic is all in libcerberus_hip.so.
"""
import ctypes
from typing import List

import torch
from torch.library import Library

from . import _lib

_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float64: 3}
PAD_MODES = {"zeros": 0, "border": 1, "reflection": 2}
INTERP_MODES = {"bilinear": 0, "nearest": 1}

_CORR_ARGS = ("int pad_size, int kernel_size, int max_displacement, "
              "int stride1, int stride2, int corr_type_multiply")

_def = Library("cerberus", "DEF")
_def.define("correlation(Tensor input1, Tensor input2, %s) -> Tensor" % _CORR_ARGS)
_def.define("correlation_backward(Tensor input1, Tensor input2, Tensor gradOutput, %s) "
            "-> Tensor[]" % _CORR_ARGS)
_def.define("correlation_leaky(Tensor input1, Tensor input2, %s, float negative_slope) "
            "-> Tensor" % _CORR_ARGS)
_def.define("correlation_leaky_into(Tensor(a!) buffer, Tensor input1, Tensor input2, int channel_offset, "
            "%s, float negative_slope) -> ()" % _CORR_ARGS)
_def.define("correlation_backward_leaky(Tensor input1, Tensor input2, Tensor grad_buffer, Tensor fwd_buffer, "
            "int channel_offset, %s, float negative_slope) -> Tensor[]" % _CORR_ARGS)
_def.define("warp_correlation_leaky(Tensor input1, Tensor input2, Tensor flow, int pad_mode, float negative_slope) -> Tensor")
_def.define("area_pyramid(Tensor image, int[] sizes) -> Tensor[]")
_def.define("flow_upsample(Tensor flow, int factor) -> Tensor")
_def.define("flow_upsample_backward(Tensor grad_out, int factor) -> Tensor")
_def.define("area_resize(Tensor image, int out_h, int out_w) -> Tensor")
_def.define("flow_warp(Tensor image, Tensor flow, int pad_mode, int interp_mode) -> Tensor")
_def.define("flow_warp_ctx(Tensor image, Tensor flow, int pad_mode, int interp_mode) -> "
            "(Tensor, Tensor)")
_def.define("flow_warp_backward_ctx(Tensor image, Tensor flow, Tensor context, Tensor grad_out, "
            "int pad_mode, int interp_mode, bool need_image, bool need_flow) -> Tensor[]")
_def.define("flow_warp_backward(Tensor image, Tensor flow, Tensor grad_out, int pad_mode, "
            "int interp_mode, bool need_image, bool need_flow) -> Tensor[]")

_def.define("photometric_loss(Tensor im_orig, Tensor im_recons, float l1_weight, float ssim_weight) -> Tensor")
_def.define("photometric_loss_backward(Tensor im_orig, Tensor im_recons, Tensor grad_loss, float l1_weight, "
            "float ssim_weight, bool need_orig, bool need_recons) -> Tensor[]")
_def.define("census_loss(Tensor im, Tensor im_warp, int max_distance) -> Tensor")
_def.define("census_loss_backward(Tensor im, Tensor im_warp, Tensor grad_loss, int max_distance, bool need_im, "
            "bool need_warp) -> (Tensor, Tensor)")
_def.define("corresponding_map(Tensor data, bool is_flow) -> Tensor")
_def.define("occlusion_mask_bidirection(Tensor flow12, Tensor flow21, float scale, float bias) -> Tensor")
_def.define("reproject_warp(Tensor image, Tensor depth, Tensor inv_K, Tensor proj, float eps) -> Tensor")
_def.define("reproject_warp_backward(Tensor image, Tensor depth, Tensor inv_K, Tensor proj, Tensor grad_out, float eps) -> Tensor")
_def.define("seg_cross_entropy(Tensor logits, Tensor target, Tensor weight, int ignore_index, float gamma) -> "
            "(Tensor loss, Tensor lse, Tensor state)")
_def.define("seg_cross_entropy_backward(Tensor logits, Tensor target, Tensor weight, Tensor lse, Tensor state, Tensor grad_loss, "
            "int ignore_index) -> Tensor")
_def.define("class_histogram(Tensor target, int num_classes, int ignore_index) -> Tensor")
_def.define("seg_ohem_cross_entropy(Tensor logits, Tensor target, Tensor weight, int ignore_index, float thresh, int min_kept) -> "
            "(Tensor loss, Tensor prob, Tensor lse, Tensor state, Tensor counts)")
_def.define("seg_ohem_cross_entropy_backward(Tensor logits, Tensor target, Tensor weight, Tensor prob, Tensor lse, Tensor state, "
            "Tensor grad_loss, int ignore_index) -> Tensor")
_def.define("inv_huber(Tensor pred, Tensor gt) -> (Tensor loss, Tensor state)")
_def.define("inv_huber_backward(Tensor pred, Tensor gt, Tensor state, Tensor grad_loss) -> Tensor")
_def.define("seg_confusion(Tensor logits, Tensor target, int ignore_index) -> Tensor")
_def.define("depth_metric_sums(Tensor pred, Tensor gt, float min_depth, float max_depth) -> (Tensor sums, Tensor counts)")
_def.define("flow_metric_sums(Tensor flow_pred, Tensor flow_gt, Tensor mask) -> (Tensor sums, Tensor counts)")
_def.define("warp_sad(Tensor image, Tensor source, Tensor flow) -> Tensor")
_def.define("center_peaks(Tensor heatmap, float threshold, int nms_kernel) -> Tensor")
_def.define("group_pixels(Tensor offsets, Tensor centers, Tensor counts, Tensor? sem, int thing_mask) -> Tensor")
_def.define("instance_overlap(Tensor pred_inst, Tensor tgt_inst, Tensor pred_seg, Tensor tgt_seg, int max_ids, int num_classes) -> "
            "(Tensor inter, Tensor pred_cls, Tensor tgt_cls)")
_def.define("rmi_moments(Tensor logits, Tensor target, int radius, int pool, bool do_rmi) -> (Tensor bce, Tensor la_cov, "
            "Tensor pr_cov, Tensor la_pr_cov, Tensor la_map, Tensor pr_map, Tensor means, Tensor state)")
_def.define("rmi_moments_backward(Tensor logits, Tensor target, Tensor la_map, Tensor pr_map, Tensor means, Tensor state, "
            "Tensor grad_bce, Tensor grad_pr_cov, Tensor grad_la_pr_cov, int radius, int pool, bool do_rmi) -> Tensor")
_def.define("edge_smoothness(Tensor flow, Tensor image, float alpha, int degree) -> Tensor")
_def.define("edge_smoothness_backward(Tensor flow, Tensor image, Tensor grad_loss, float alpha, int degree) -> Tensor")
_def.define("panoptic_targets(Tensor ids, Tensor seg_ids, Tensor seg_category, Tensor seg_flags, Tensor seg_count, Tensor gauss, "
            "int ignore_label, int sigma, bool ignore_stuff_in_offset, int small_instance_area, float small_instance_weight, "
            "bool ignore_crowd_in_semantic) -> (Tensor semantic, Tensor foreground, Tensor center, Tensor offset, "
            "Tensor semantic_mask, Tensor center_mask, Tensor offset_mask, Tensor center_points)")
_def.define("panoptic_loss(Tensor center_pred, Tensor center_tgt, Tensor? center_mask, Tensor offset_pred, Tensor offset_tgt, "
            "Tensor? offset_mask, float center_weight, float offset_weight, int mode) -> (Tensor loss, Tensor state)")
_def.define("panoptic_loss_backward(Tensor center_pred, Tensor center_tgt, Tensor? center_mask, Tensor offset_pred, "
            "Tensor offset_tgt, Tensor? offset_mask, Tensor state, Tensor grad_loss, int mode) -> "
            "(Tensor grad_center, Tensor grad_offset)")


def _stream_ptr(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _dtype_code(t: torch.Tensor, what: str) -> int:
    try:
        return _DTYPES[t.dtype]
    except KeyError:
        raise RuntimeError("%s: unsupported dtype %s (float32/float16/bfloat16/float64)"
                           % (what, t.dtype)) from None


def _fresh_like(t: torch.Tensor, dtype=None) -> torch.Tensor:
    """An output "like ``t``" under the contract of every op here: ``t``'s shape, its dtype or ``dtype``, in a
    fresh allocation with the default (NCHW) strides and storage offset 0 -- whatever ``t``'s own strides are.  Both the CUDA
    and the Meta implementations allocate with it: ``torch.empty_like`` keeps the strides of a dense input (channels_last,
    a transposed map, a (B,1,H,W) tensor that passes for both formats), which is not what the kernels write."""
    return t.new_empty(t.shape, dtype=t.dtype if dtype is None else dtype)


def _check_pair(a: torch.Tensor, b: torch.Tensor, what: str):
    if a.dim() != 4 or b.dim() != 4:
        raise RuntimeError("%s: expected 4-D NCHW tensors, got %s and %s"
                           % (what, tuple(a.shape), tuple(b.shape)))
    if a.shape != b.shape:
        raise RuntimeError("%s: input shapes differ: %s vs %s"
                           % (what, tuple(a.shape), tuple(b.shape)))
    if a.dtype != b.dtype:
        raise RuntimeError("%s: input dtypes differ: %s vs %s" % (what, a.dtype, b.dtype))
    if a.device != b.device:
        raise RuntimeError("%s: inputs on different devices: %s vs %s"
                           % (what, a.device, b.device))


def _corr_out_shape(H, W, pad, k, d, s1, s2):
    lib = _lib.get()
    oc, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.cerberus_correlation_out_shape(H, W, pad, k, d, s1, s2, ctypes.byref(oc),
                                                  ctypes.byref(oh), ctypes.byref(ow)),
               "cerberus::correlation (output shape)")
    return oc.value, oh.value, ow.value


def _meta_out_shape(H, W, pad, k, d, s1, s2):
    # shape maths of correlation_cuda.cpp:6-14 without touching the library
    import math
    kr = (k - 1) // 2
    border = kr + d
    oc = ((d // s2) * 2 + 1) ** 2
    oh = math.ceil((H + 2 * pad - 2 * border) / s1)
    ow = math.ceil((W + 2 * pad - 2 * border) / s1)
    return oc, oh, ow


# ----------------------------------------------------------------------------
# correlation forward
# ----------------------------------------------------------------------------
def _correlation_impl(input1, input2, pad, k, d, s1, s2, mult, slope, what):
    _check_pair(input1, input2, what)
    code = _dtype_code(input1, what)
    x1 = input1.contiguous()   # the reference honours strides via accessors (.cu:271-272)
    x2 = input2.contiguous()
    B, C, H, W = x1.shape
    oc, oh, ow = _corr_out_shape(H, W, pad, k, d, s1, s2)
    out = torch.empty((B, oc, oh, ow), dtype=x1.dtype, device=x1.device)
    if out.numel() == 0:
        return out
    with torch.cuda.device(x1.device):
        rc = _lib.get().cerberus_correlation_forward_ex(
            x1.data_ptr(), x2.data_ptr(), out.data_ptr(), B, C, H, W, pad, k, d, s1, s2,
            ctypes.c_float(slope), 0, code, _stream_ptr(x1))
    _lib.check(rc, what)
    return out


def _correlation_cuda(input1, input2, pad_size, kernel_size, max_displacement, stride1,
                      stride2, corr_type_multiply):
    return _correlation_impl(input1, input2, pad_size, kernel_size, max_displacement, stride1,
                             stride2, corr_type_multiply, 1.0, "cerberus::correlation")


def _correlation_leaky_cuda(input1, input2, pad_size, kernel_size, max_displacement, stride1,
                            stride2, corr_type_multiply, negative_slope):
    return _correlation_impl(input1, input2, pad_size, kernel_size, max_displacement, stride1,
                             stride2, corr_type_multiply, float(negative_slope),
                             "cerberus::correlation_leaky")


def _correlation_leaky_into_cuda(buffer, input1, input2, channel_offset, pad_size, kernel_size,
                                 max_displacement, stride1, stride2, corr_type_multiply,
                                 negative_slope):
    """The cost volume (with the fused LeakyReLU) written straight into channels
    [channel_offset, channel_offset + oC) of a wider, caller-owned NCHW buffer: the
    ``torch.cat([out_corr, im1_1by1, flow])`` of pwcnet_sfd.py:186-187 without the pass that
    re-reads and re-writes the 81-channel volume."""
    what = "cerberus::correlation_leaky_into"
    _check_pair(input1, input2, what)
    code = _dtype_code(input1, what)
    x1, x2 = input1.contiguous(), input2.contiguous()
    B, C, H, W = x1.shape
    oc, oh, ow = _corr_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2)
    if (buffer.dim() != 4 or not buffer.is_contiguous() or buffer.dtype != x1.dtype or
            buffer.device != x1.device or buffer.shape[0] != B or
            tuple(buffer.shape[2:]) != (oh, ow) or channel_offset < 0 or
            channel_offset + oc > buffer.shape[1]):
        raise RuntimeError("%s: buffer %s (%s, contiguous=%s) cannot hold channels [%d, %d) of a "
                           "(%d, %d, %d, %d) %s cost volume"
                           % (what, tuple(buffer.shape), buffer.dtype, buffer.is_contiguous(),
                              channel_offset, channel_offset + oc, B, oc, oh, ow, x1.dtype))
    if B * oc * oh * ow == 0:
        return
    first = buffer[:, channel_offset]          # address of (0, channel_offset, 0, 0)
    with torch.cuda.device(x1.device):
        rc = _lib.get().cerberus_correlation_forward_ex(
            x1.data_ptr(), x2.data_ptr(), first.data_ptr(), B, C, H, W, pad_size, kernel_size,
            max_displacement, stride1, stride2, ctypes.c_float(float(negative_slope)),
            buffer.stride(0), code, _stream_ptr(x1))
    _lib.check(rc, what)


def _correlation_meta(input1, input2, pad_size, kernel_size, max_displacement, stride1,
                      stride2, corr_type_multiply, *_):
    B, _, H, W = input1.shape
    oc, oh, ow = _meta_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2)
    return input1.new_empty((B, oc, oh, ow))


# ----------------------------------------------------------------------------
# correlation backward
# ----------------------------------------------------------------------------
def _correlation_backward_cuda(input1, input2, gradOutput, pad_size, kernel_size,
                               max_displacement, stride1, stride2,
                               corr_type_multiply) -> List[torch.Tensor]:
    what = "cerberus::correlation_backward"
    _check_pair(input1, input2, what)
    code = _dtype_code(input1, what)
    if stride1 != 1:
        raise RuntimeError(what + ": stride1 must be 1 (the reference kernel writes out of "
                           "bounds for stride1 > 1, correlation_cuda_kernel.cu:106-107,169)")
    x1 = input1.contiguous()
    x2 = input2.contiguous()
    B, C, H, W = x1.shape
    oc, oh, ow = _corr_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2)
    if tuple(gradOutput.shape) != (B, oc, oh, ow):
        raise RuntimeError("%s: gradOutput shape %s, expected %s"
                           % (what, tuple(gradOutput.shape), (B, oc, oh, ow)))
    go = gradOutput.to(dtype=x1.dtype).contiguous()
    g1 = _fresh_like(x1)
    g2 = _fresh_like(x2)
    if x1.numel() == 0:
        return [g1, g2]
    with torch.cuda.device(x1.device):
        rc = _lib.get().cerberus_correlation_backward(
            x1.data_ptr(), x2.data_ptr(), go.data_ptr(), g1.data_ptr(), g2.data_ptr(), B, C, H,
            W, pad_size, kernel_size, max_displacement, stride1, stride2, corr_type_multiply,
            code, _stream_ptr(x1))
    _lib.check(rc, what)
    return [g1, g2]


def _correlation_backward_meta(input1, input2, gradOutput, *_):
    return [_fresh_like(input1), _fresh_like(input2)]


def _correlation_backward_leaky_cuda(input1, input2, grad_buffer, fwd_buffer, channel_offset, pad_size,
                                     kernel_size, max_displacement, stride1, stride2, corr_type_multiply,
                                     negative_slope) -> List[torch.Tensor]:
    """Backward of ``correlation_leaky_into``: ``grad_buffer`` is the gradient of the whole concatenation
    buffer, ``fwd_buffer`` the buffer the forward wrote; the cost volume is channels [channel_offset,
    channel_offset + oC) of both.  The LeakyReLU derivative (from the stored volume's sign) and the
    gather of the batch-strided slice happen in ONE pass of the library (cerberus_correlation_backward_ex)
    instead of ``g * slope``, ``torch.where`` and ``.contiguous()`` (pwcnet_sfd.py:181-187 seen from autograd)."""
    what = "cerberus::correlation_backward_leaky"
    _check_pair(input1, input2, what)
    code = _dtype_code(input1, what)
    if stride1 != 1:
        raise RuntimeError(what + ": stride1 must be 1 (the reference kernel writes out of "
                           "bounds for stride1 > 1, correlation_cuda_kernel.cu:106-107,169)")
    x1, x2 = input1.contiguous(), input2.contiguous()
    B, C, H, W = x1.shape
    oc, oh, ow = _corr_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2)
    for name, t in (("grad_buffer", grad_buffer), ("fwd_buffer", fwd_buffer)):
        if (t.dim() != 4 or t.shape[0] != B or tuple(t.shape[2:]) != (oh, ow) or t.device != x1.device or
                channel_offset < 0 or channel_offset + oc > t.shape[1]):
            raise RuntimeError("%s: %s %s cannot hold channels [%d, %d) of a (%d, %d, %d, %d) cost volume"
                               % (what, name, tuple(t.shape), channel_offset, channel_offset + oc, B, oc, oh, ow))
    # plane-dense AND one item per batch stride: an expanded gradient (``out.sum(0)`` hands over ``grad.expand(...)``
    # with batch stride 0) has dense planes but B items in ONE item's storage -- the library would read past it
    # (ADVICE r5), so it is materialised like any other non-dense layout
    def usable(t):
        return (t.stride(3) == 1 and t.stride(2) == ow and t.stride(1) == oh * ow and
                (B == 1 or t.stride(0) >= t.shape[1] * oh * ow))
    go = grad_buffer.to(dtype=x1.dtype)
    if not usable(go):
        go = go.contiguous()
    fo = fwd_buffer if (fwd_buffer.dtype == x1.dtype and usable(fwd_buffer)) else fwd_buffer.to(x1.dtype).contiguous()
    # the real batch stride always (the C ABI reads 0 as "dense": never hand it a Python-side 0)
    go_bs = go.stride(0) if B > 1 else go.shape[1] * oh * ow
    fo_bs = fo.stride(0) if B > 1 else fo.shape[1] * oh * ow
    g1, g2 = _fresh_like(x1), _fresh_like(x2)
    if x1.numel() == 0:
        return [g1, g2]
    lib = _lib.get()
    ws_bytes = lib.cerberus_correlation_backward_ex_workspace_bytes(B, H, W, pad_size, kernel_size, max_displacement,
                                                                    stride1, stride2, code)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=x1.device)   # caching allocator: 512-byte aligned
    with torch.cuda.device(x1.device):
        rc = lib.cerberus_correlation_backward_ex(
            x1.data_ptr(), x2.data_ptr(), go[:, channel_offset].data_ptr(), go_bs,
            fo[:, channel_offset].data_ptr(), fo_bs, ctypes.c_float(float(negative_slope)),
            ws.data_ptr(), ws_bytes, g1.data_ptr(), g2.data_ptr(), B, C, H, W, pad_size, kernel_size,
            max_displacement, stride1, stride2, code, _stream_ptr(x1))
    _lib.check(rc, what)
    return [g1, g2]


# ----------------------------------------------------------------------------
# flow warp
# ----------------------------------------------------------------------------
def _warp_check(image, flow, what):
    if image.dim() != 4 or flow.dim() != 4:
        raise RuntimeError("%s: expected image (B,C,H,W) and flow (B,2,H,W)" % what)
    B, _, H, W = image.shape
    if tuple(flow.shape) != (B, 2, H, W):
        raise RuntimeError("%s: flow shape %s, expected %s"
                           % (what, tuple(flow.shape), (B, 2, H, W)))
    if image.device != flow.device:
        raise RuntimeError("%s: image and flow on different devices" % what)


def _flow_for(img, flow):
    """The flow as the kernels take it: in the image's dtype, except that an fp32 flow stays
    fp32 beside a 16-bit image.  (Reference, UnFlowLoss.py:89-93: ``base_grid.type_as(image) +
    flow12`` promotes to fp32 and grid_sample is on autocast's fp32 list, so a half image with
    an fp32 flow is sampled at full flow precision -- rounding the flow to fp16/bf16 would
    cost 0.03-0.25 px at |flow| of 32-512 px.)  The output keeps the image's dtype: the
    reference's caller casts it back at once (pwcnet_sfd.py:178 ``.type(im1.dtype)``)."""
    if flow.dtype == torch.float32 and img.dtype in (torch.float16, torch.bfloat16):
        return flow.contiguous()
    return flow.to(dtype=img.dtype).contiguous()


def _check_aligned16(t, what, name):
    """The warp kernels read the context / workspace header as int4 (ABI v4: CERB_EINVAL otherwise).
    torch's caching allocator hands out 512-byte aligned blocks; a sliced or re-viewed tensor may not be."""
    if t is not None and t.numel() and t.data_ptr() % 16:
        raise RuntimeError("%s: the warp %s must be 16-byte aligned (got an address ending in 0x%x): "
                           "pass the tensor the forward returned, not a slice of it" % (what, name, t.data_ptr() % 16))


def _flow_warp_run(image, flow, pad_mode, interp_mode, want_ctx, what):
    _warp_check(image, flow, what)
    code = _dtype_code(image, what)
    img = image.contiguous()
    flo = _flow_for(img, flow)
    out = _fresh_like(img)
    B, C, H, W = img.shape
    lib = _lib.get()
    ctx_bytes = lib.cerberus_flow_warp_context_bytes(B, H, W) if want_ctx else 0
    # int64 elements; the kernels need 16-byte alignment (checked below: the caching allocator gives 512)
    ctx = torch.empty((ctx_bytes + 7) // 8, dtype=torch.int64, device=img.device) if want_ctx else None
    if want_ctx:
        _check_aligned16(ctx, what, "context")
    if out.numel() == 0:
        return out, ctx
    with torch.cuda.device(img.device):
        rc = lib.cerberus_flow_warp_forward_ctx(
            img.data_ptr(), flo.data_ptr(), out.data_ptr(),
            ctx.data_ptr() if want_ctx else None, ctx_bytes, B, C, H, W, pad_mode, interp_mode,
            code, _DTYPES[flo.dtype], _stream_ptr(img))
    _lib.check(rc, what)
    return out, ctx


def _flow_warp_cuda(image, flow, pad_mode, interp_mode):
    return _flow_warp_run(image, flow, pad_mode, interp_mode, False, "cerberus::flow_warp")[0]


def _flow_warp_ctx_cuda(image, flow, pad_mode, interp_mode):
    """Forward that also returns the backward context (sample positions + tap extents):
    the analogue of what autograd saves for grid_sample in the reference."""
    return _flow_warp_run(image, flow, pad_mode, interp_mode, True, "cerberus::flow_warp_ctx")


def _warp_context_bytes(B, H, W):
    """Size of the warp backward's context in pure Python (what cerberus_flow_warp_context_bytes returns; a test holds
    the two equal): one int4 tap range per 2 x 32 pixel strip + two fp32 sample-position planes per image.  Meta /
    fake-tensor tracing must not need the shared library."""
    if B <= 0 or H <= 0 or W <= 0:
        return 0
    strips = ((W + 31) // 32) * ((H + 1) // 2)
    return B * strips * 16 + B * 2 * H * W * 4


def _flow_warp_ctx_meta(image, flow, pad_mode, interp_mode):
    B, _, H, W = image.shape
    n = (_warp_context_bytes(B, H, W) + 7) // 8
    return _fresh_like(image), image.new_empty((n,), dtype=torch.int64)


def _flow_warp_backward_run(image, flow, context, grad_out, pad_mode, interp_mode, need_image,
                            need_flow, what) -> List[torch.Tensor]:
    _warp_check(image, flow, what)
    code = _dtype_code(image, what)
    img = image.contiguous()
    flo = _flow_for(img, flow)
    go = grad_out.to(dtype=img.dtype).contiguous()
    if go.shape != img.shape:
        raise RuntimeError("%s: grad_out shape %s, expected %s"
                           % (what, tuple(go.shape), tuple(img.shape)))
    gi = _fresh_like(img) if need_image else img.new_empty(0)
    gf = _fresh_like(flo) if need_flow else flo.new_empty(0)
    if img.numel() == 0 or not (need_image or need_flow):
        return [gi, gf]
    B, C, H, W = img.shape
    lib = _lib.get()
    ctx_ptr, ctx_bytes = None, 0
    if context is not None:
        ctx_bytes = lib.cerberus_flow_warp_context_bytes(B, H, W)
        if (context.device != img.device or not context.is_contiguous()
                or context.numel() * context.element_size() < ctx_bytes):
            raise RuntimeError("%s: context does not belong to this image/flow shape" % what)
        _check_aligned16(context, what, "context")
        ctx_ptr = context.data_ptr()
    # device scratch in which the tiled grad_image builds its context when the forward saved
    # none (caching allocator: no sync, graph-capturable; stream-ordered reuse keeps it
    # private to this call)
    ws, ws_bytes = None, 0
    if (need_image or (need_flow and C > 4)) and context is None:   # (round 6: grad_flow alone takes the tile launch's flow role too)
        ws_bytes = lib.cerberus_flow_warp_backward_workspace_bytes(B, C, H, W)
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=img.device)
        _check_aligned16(ws, what, "workspace")
    with torch.cuda.device(img.device):
        rc = lib.cerberus_flow_warp_backward(
            img.data_ptr(), flo.data_ptr(), go.data_ptr(),
            gi.data_ptr() if need_image else None, gf.data_ptr() if need_flow else None,
            ctx_ptr, ctx_bytes,
            ws.data_ptr() if ws is not None else None, ws_bytes,
            B, C, H, W, pad_mode, interp_mode, code, _DTYPES[flo.dtype], _stream_ptr(img))
    _lib.check(rc, what)
    return [gi, gf]


def _flow_warp_backward_cuda(image, flow, grad_out, pad_mode, interp_mode, need_image,
                             need_flow) -> List[torch.Tensor]:
    return _flow_warp_backward_run(image, flow, None, grad_out, pad_mode, interp_mode,
                                   need_image, need_flow, "cerberus::flow_warp_backward")


def _flow_warp_backward_ctx_cuda(image, flow, context, grad_out, pad_mode, interp_mode,
                                 need_image, need_flow) -> List[torch.Tensor]:
    return _flow_warp_backward_run(image, flow, context, grad_out, pad_mode, interp_mode,
                                   need_image, need_flow, "cerberus::flow_warp_backward_ctx")


def _flow_warp_backward_meta(image, flow, need_image, need_flow):
    """What ``_flow_warp_backward_run`` returns: grad_image like the image, grad_flow in the dtype ``_flow_for`` hands the
    kernels (fp32 beside a 16-bit image, else the image's), and an empty (0,) tensor for a gradient that is not asked for."""
    keep = flow.dtype == torch.float32 and image.dtype in (torch.float16, torch.bfloat16)
    fdtype = flow.dtype if keep else image.dtype
    return [_fresh_like(image) if need_image else image.new_empty(0),
            _fresh_like(flow, fdtype) if need_flow else flow.new_empty(0, dtype=fdtype)]


# ----------------------------------------------------------------------------
# f2: the warp fused into the correlation forward (pwcnet_sfd.py:178 -> :181-182, d = 4)
# ----------------------------------------------------------------------------
def _warp_correlation_leaky_cuda(input1, input2, flow, pad_mode, negative_slope):
    """LeakyReLU(correlation(input1, flow_warp(input2, flow))) with pad = d = 4, k = s1 = s2 = 1, without writing the
    warped features (cerberus_warp_correlation_forward).  Opt-in: measured slower than the two tuned launches."""
    what = "cerberus::warp_correlation_leaky"
    _check_pair(input1, input2, what)
    _warp_check(input2, flow, what)
    code = _dtype_code(input1, what)
    x1, x2 = input1.contiguous(), input2.contiguous()
    flo = _flow_for(x2, flow)
    B, C, H, W = x1.shape
    out = x1.new_empty((B, 81, H, W))
    if out.numel() == 0:
        return out
    lib = _lib.get()
    ws_bytes = lib.cerberus_warp_correlation_workspace_bytes(B, C, H, W)    # small maps: fp32 volume for the split channel sum
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=x1.device) if ws_bytes else None
    with torch.cuda.device(x1.device):
        rc = lib.cerberus_warp_correlation_forward(
            x1.data_ptr(), x2.data_ptr(), flo.data_ptr(), out.data_ptr(), ws.data_ptr() if ws is not None else None, ws_bytes,
            B, C, H, W, pad_mode, ctypes.c_float(float(negative_slope)), 0, code, _DTYPES[flo.dtype], _stream_ptr(x1))
    _lib.check(rc, what)
    return out


# ----------------------------------------------------------------------------
# flow upsample (pwcnet_sfd.py:176, :199-201): factor 2 and 4 in the model, any integer factor >= 1 here
# (tests/test_resample_gpu.py runs 1 - 8; exactly F.interpolate(flow * k) for powers of two, within one
# rounding of a multiply otherwise)
# ----------------------------------------------------------------------------
def _flow_upsample_run(t, factor, forward, what):
    if t.dim() != 4:
        raise RuntimeError("%s: expected a 4-D NCHW tensor, got %s" % (what, tuple(t.shape)))
    if factor < 1:
        raise RuntimeError("%s: factor must be >= 1" % what)
    code = _dtype_code(t, what)
    if code == 3:
        raise RuntimeError("%s: float64 is not supported" % what)
    x = t.contiguous()
    B, C, H, W = x.shape
    if forward:
        h, w = H, W
        out = x.new_empty((B, C, H * factor, W * factor))
    else:
        if H % factor or W % factor:
            raise RuntimeError("%s: grad shape %s is not a multiple of the factor %d"
                               % (what, tuple(x.shape), factor))
        h, w = H // factor, W // factor
        out = x.new_empty((B, C, h, w))
    if out.numel() == 0 or x.numel() == 0:
        return out
    fn = _lib.get().cerberus_flow_upsample_forward if forward else _lib.get().cerberus_flow_upsample_backward
    with torch.cuda.device(x.device):
        rc = fn(x.data_ptr(), out.data_ptr(), B * C, h, w, factor, code, _stream_ptr(x))
    _lib.check(rc, what)
    return out


def _flow_upsample_cuda(flow, factor):
    return _flow_upsample_run(flow, factor, True, "cerberus::flow_upsample")


def _flow_upsample_backward_cuda(grad_out, factor):
    return _flow_upsample_run(grad_out, factor, False, "cerberus::flow_upsample_backward")


def _area_resize_cuda(image, out_h, out_w):
    """F.interpolate(image, (out_h, out_w), mode='area') (UnFlowLoss.py:279-280)."""
    what = "cerberus::area_resize"
    if image.dim() != 4:
        raise RuntimeError("%s: expected a 4-D NCHW tensor, got %s" % (what, tuple(image.shape)))
    if out_h < 1 or out_w < 1:
        raise RuntimeError("%s: output size must be positive, got (%d, %d)" % (what, out_h, out_w))
    code = _dtype_code(image, what)
    if code == 3:
        raise RuntimeError("%s: float64 is not supported" % what)
    x = image.contiguous()
    B, C, H, W = x.shape
    out = x.new_empty((B, C, out_h, out_w))
    if out.numel() == 0:
        return out
    if H == 0 or W == 0:
        raise RuntimeError("%s: input has no pixels" % what)
    with torch.cuda.device(x.device):
        rc = _lib.get().cerberus_area_resize(x.data_ptr(), out.data_ptr(), B * C, H, W, out_h, out_w,
                                             code, _stream_ptr(x))
    _lib.check(rc, what)
    return out


def _area_pyramid_cuda(image, sizes) -> List[torch.Tensor]:
    """``[F.interpolate(image, (h, w), mode='area') for (h, w) in sizes]`` (``sizes`` flat: h0, w0, h1, w1, ...):
    how unFlowLoss brings a target image to every flow scale (UnFlowLoss.py:279-280).  A scale of the image's
    own size is a copy of the image; the others come from one pass over the source when they
    are integer ratios of it (cerberus_area_pyramid), bit-identical to ``area_resize`` scale by scale."""
    what = "cerberus::area_pyramid"
    if image.dim() != 4:
        raise RuntimeError("%s: expected a 4-D NCHW tensor, got %s" % (what, tuple(image.shape)))
    if len(sizes) % 2:
        raise RuntimeError("%s: sizes must be a flat list of (height, width) pairs" % what)
    code = _dtype_code(image, what)
    if code == 3:
        raise RuntimeError("%s: float64 is not supported" % what)
    x = image.contiguous()
    B, C, H, W = x.shape
    pairs = [(int(sizes[i]), int(sizes[i + 1])) for i in range(0, len(sizes), 2)]
    if any(h < 1 or w < 1 for h, w in pairs):
        raise RuntimeError("%s: output sizes must be positive, got %s" % (what, pairs))
    # a scale of the image's own size is a COPY (F.interpolate returns one; a custom op must not return an alias of
    # its input: ADVICE r5) -- unFlowLoss asks for it at most once per step and only on pyramids that start at 1/1
    outs = [x.clone(memory_format=torch.contiguous_format) if (h, w) == (H, W) else x.new_empty((B, C, h, w)) for h, w in pairs]
    todo = [(o, hw) for o, hw in zip(outs, pairs) if hw != (H, W) and o.numel()]
    if not todo:
        return outs
    if H == 0 or W == 0:
        raise RuntimeError("%s: input has no pixels" % what)
    lib = _lib.get()
    with torch.cuda.device(x.device):
        for i in range(0, len(todo), 4):        # one launch holds up to four scales
            chunk = todo[i:i + 4]
            n = len(chunk)
            dsts = (ctypes.c_void_p * n)(*[o.data_ptr() for o, _ in chunk])
            hs = (ctypes.c_int * n)(*[hw[0] for _, hw in chunk])
            ws = (ctypes.c_int * n)(*[hw[1] for _, hw in chunk])
            _lib.check(lib.cerberus_area_pyramid(x.data_ptr(), dsts, hs, ws, n, B * C, H, W, code, _stream_ptr(x)), what)
    return outs


def _area_pyramid_meta(image, sizes):
    B, C, _, _ = image.shape
    return [image.new_empty((B, C, int(sizes[i]), int(sizes[i + 1]))) for i in range(0, len(sizes), 2)]


# ----------------------------------------------------------------------------
# unFlowLoss's scalar terms (UnFlowLoss.py:162-187, :236-255; loss_functions.py:47-77), csrc/photometric.hip
# ----------------------------------------------------------------------------
def _photometric_workspace_bytes(B, C, H, W):
    """cerberus_photometric_loss_workspace_bytes in pure Python (a test holds the two equal): one fp32 partial per
    16 x 64 tile of every image plane."""
    if B <= 0 or C <= 0 or H <= 0 or W <= 0:
        return 0
    return ((W + 63) // 64) * ((H + 15) // 16) * B * C * 4


def _smoothness_workspace_bytes(B, H, W):
    """cerberus_edge_smoothness_workspace_bytes in pure Python: an x and a y partial per 4 x 64 tile of every batch item."""
    if B <= 0 or H <= 0 or W <= 0:
        return 0
    return ((W + 63) // 64) * ((H + 3) // 4) * B * 8


def _loss_check(a, b, what, names):
    for t, name in zip((a, b), names):
        if t.dim() != 4:
            raise RuntimeError("%s: %s must be a 4-D NCHW tensor, got %s" % (what, name, tuple(t.shape)))
        if t.dtype != torch.float32:
            raise RuntimeError("%s: %s must be float32, got %s (16-bit tensors take the stock-op path of "
                               "loss_functions.photometric_loss / edge_smoothness)" % (what, name, t.dtype))
    if a.device != b.device:
        raise RuntimeError("%s: inputs on different devices: %s vs %s" % (what, a.device, b.device))


def _grad_scalar(grad_loss, like, what):
    if grad_loss.numel() != 1:
        raise RuntimeError("%s: grad_loss must hold one element, got %s" % (what, tuple(grad_loss.shape)))
    # stays on the device: the kernel reads it (no .item(), no synchronisation -- capturable)
    return grad_loss.to(device=like.device, dtype=torch.float32).contiguous()


def _photometric_loss_cuda(im_orig, im_recons, l1_weight, ssim_weight):
    what = "cerberus::photometric_loss"
    _loss_check(im_orig, im_recons, what, ("im_orig", "im_recons"))
    if im_orig.shape != im_recons.shape:
        raise RuntimeError("%s: image shapes differ: %s vs %s" % (what, tuple(im_orig.shape), tuple(im_recons.shape)))
    a, b = im_orig.contiguous(), im_recons.contiguous()
    B, C, H, W = a.shape
    lib = _lib.get()
    ws_bytes = lib.cerberus_photometric_loss_workspace_bytes(B, C, H, W)
    ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=a.device)
    out = torch.empty((), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = lib.cerberus_photometric_loss_forward(a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_bytes, B, C, H, W,
                                                   float(l1_weight), float(ssim_weight), 0, _stream_ptr(a))
    _lib.check(rc, what)
    return out


def _photometric_loss_backward_cuda(im_orig, im_recons, grad_loss, l1_weight, ssim_weight, need_orig,
                                    need_recons) -> List[torch.Tensor]:
    what = "cerberus::photometric_loss_backward"
    _loss_check(im_orig, im_recons, what, ("im_orig", "im_recons"))
    if im_orig.shape != im_recons.shape:
        raise RuntimeError("%s: image shapes differ: %s vs %s" % (what, tuple(im_orig.shape), tuple(im_recons.shape)))
    a, b = im_orig.contiguous(), im_recons.contiguous()
    g = _grad_scalar(grad_loss, a, what)
    B, C, H, W = a.shape
    lib = _lib.get()
    outs = []
    # the loss is symmetric in the two images: the gradient of im_orig is the same launch with the roles exchanged
    for need, first, second in ((need_orig, b, a), (need_recons, a, b)):
        if not need:
            outs.append(a.new_empty((0,)))
            continue
        grad = _fresh_like(second)
        with torch.cuda.device(a.device):
            rc = lib.cerberus_photometric_loss_backward(first.data_ptr(), second.data_ptr(), g.data_ptr(), grad.data_ptr(), B, C, H, W,
                                                        float(l1_weight), float(ssim_weight), 0, _stream_ptr(a))
        _lib.check(rc, what)
        outs.append(grad)
    return outs


def _photometric_loss_backward_meta(im_orig, im_recons, grad_loss, l1_weight, ssim_weight, need_orig, need_recons):
    return [_fresh_like(im_orig) if need_orig else im_orig.new_empty((0,)),
            _fresh_like(im_recons) if need_recons else im_recons.new_empty((0,))]


def _smoothness_check(flow, image, degree, what):
    _loss_check(flow, image, what, ("flow", "image"))
    if flow.shape[0] != image.shape[0] or flow.shape[2:] != image.shape[2:]:
        raise RuntimeError("%s: flow %s and image %s differ in batch or size" % (what, tuple(flow.shape), tuple(image.shape)))
    if degree not in (1, 2):
        raise RuntimeError("%s: degree must be 1 or 2, got %s" % (what, degree))


def _edge_smoothness_cuda(flow, image, alpha, degree):
    what = "cerberus::edge_smoothness"
    _smoothness_check(flow, image, degree, what)
    f, img = flow.contiguous(), image.contiguous()
    B, Cf, H, W = f.shape
    lib = _lib.get()
    ws_bytes = lib.cerberus_edge_smoothness_workspace_bytes(B, H, W)
    ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=f.device)
    out = torch.empty((), dtype=torch.float32, device=f.device)
    with torch.cuda.device(f.device):
        rc = lib.cerberus_edge_smoothness_forward(f.data_ptr(), img.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_bytes, B, Cf,
                                                  img.shape[1], H, W, float(alpha), int(degree), 0, _stream_ptr(f))
    _lib.check(rc, what)
    return out


def _edge_smoothness_backward_cuda(flow, image, grad_loss, alpha, degree):
    what = "cerberus::edge_smoothness_backward"
    _smoothness_check(flow, image, degree, what)
    f, img = flow.contiguous(), image.contiguous()
    g = _grad_scalar(grad_loss, f, what)
    B, Cf, H, W = f.shape
    grad = _fresh_like(f)
    with torch.cuda.device(f.device):
        rc = _lib.get().cerberus_edge_smoothness_backward(f.data_ptr(), img.data_ptr(), g.data_ptr(), grad.data_ptr(), B, Cf,
                                                          img.shape[1], H, W, float(alpha), int(degree), 0, _stream_ptr(f))
    _lib.check(rc, what)
    return grad


# the census (ternary) term (UnFlowLoss.py:119-156), csrc/census.hip
CENSUS_MAX_DISTANCES = (1, 2, 3)        # the compiled window sizes: 3 x 3, 5 x 5, 7 x 7


def _census_workspace_bytes(B, H, W):
    """cerberus_census_loss_workspace_bytes in pure Python (a test holds the two equal): one fp32 partial per 16 x 64
    tile of every batch item."""
    if B <= 0 or H <= 0 or W <= 0:
        return 0
    return ((W + 63) // 64) * ((H + 15) // 16) * B * 4


def _census_check(im, im_warp, max_distance, what):
    for t, name in zip((im, im_warp), ("im", "im_warp")):
        if t.dim() != 4:
            raise RuntimeError("%s: %s must be a 4-D NCHW tensor, got %s" % (what, name, tuple(t.shape)))
        if t.dtype != torch.float32:
            raise RuntimeError("%s: %s must be float32, got %s (16-bit tensors take the stock-op path of "
                               "loss_functions.census_loss)" % (what, name, t.dtype))
    if im.device != im_warp.device:
        raise RuntimeError("%s: inputs on different devices: %s vs %s" % (what, im.device, im_warp.device))
    if im.shape != im_warp.shape:
        raise RuntimeError("%s: image shapes differ: %s vs %s" % (what, tuple(im.shape), tuple(im_warp.shape)))
    if im.shape[1] != 3:
        raise RuntimeError("%s: the grayscale conversion needs 3 channels, got %d" % (what, im.shape[1]))
    if max_distance not in CENSUS_MAX_DISTANCES:
        raise RuntimeError("%s: max_distance must be one of %s, got %s (other windows take the stock-op path of "
                           "loss_functions.census_loss)" % (what, CENSUS_MAX_DISTANCES, max_distance))
    patch = 2 * max_distance + 1
    if im.shape[0] < 1 or min(im.shape[2:]) < patch:
        raise RuntimeError("%s: max_distance=%d needs a non-empty batch of maps of at least %d x %d, got %s"
                           % (what, max_distance, patch, patch, tuple(im.shape)))


def _census_loss_cuda(im, im_warp, max_distance):
    what = "cerberus::census_loss"
    _census_check(im, im_warp, max_distance, what)
    a, b = im.contiguous(), im_warp.contiguous()
    B, _, H, W = a.shape
    lib = _lib.get()
    ws_bytes = lib.cerberus_census_loss_workspace_bytes(B, H, W)
    ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=a.device)
    out = torch.empty((), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = lib.cerberus_census_loss_forward(a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_bytes, B, H, W,
                                              int(max_distance), 0, _stream_ptr(a))
    _lib.check(rc, what)
    return out


def _census_loss_backward_cuda(im, im_warp, grad_loss, max_distance, need_im, need_warp):
    what = "cerberus::census_loss_backward"
    _census_check(im, im_warp, max_distance, what)
    a, b = im.contiguous(), im_warp.contiguous()
    g = _grad_scalar(grad_loss, a, what)
    B, _, H, W = a.shape
    lib = _lib.get()
    outs = []
    # the loss is symmetric in the two images: the gradient of im is the same launch with the roles exchanged
    for need, first, second in ((need_im, b, a), (need_warp, a, b)):
        if not need:
            outs.append(a.new_empty((0,)))
            continue
        grad = _fresh_like(second)
        with torch.cuda.device(a.device):
            rc = lib.cerberus_census_loss_backward(first.data_ptr(), second.data_ptr(), g.data_ptr(), grad.data_ptr(), B, H, W,
                                                   int(max_distance), 0, _stream_ptr(a))
        _lib.check(rc, what)
        outs.append(grad)
    return outs[0], outs[1]


def _census_loss_backward_meta(im, im_warp, grad_loss, max_distance, need_im, need_warp):
    return (_fresh_like(im) if need_im else im.new_empty((0,)),
            _fresh_like(im_warp) if need_warp else im_warp.new_empty((0,)))


# the occlusion masks (UnFlowLoss.py:34-81, :96-117), csrc/occlusion.hip: forward only
def _corresponding_map_workspace_bytes(B, H, W):
    """cerberus_corresponding_map_workspace_bytes in pure Python (a test holds the two equal): one 64-bit fixed-point
    accumulator per pixel of the map."""
    if B <= 0 or H <= 0 or W <= 0:
        return 0
    return 8 * B * H * W


def _occlusion_check(t, name, what):
    if t.dim() != 4 or t.shape[1] != 2:
        raise RuntimeError("%s: %s must be a (B,2,H,W) tensor, got %s" % (what, name, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise RuntimeError("%s: %s must be float32, got %s (16-bit tensors take the stock-op path of the wrappers in "
                           "loss_functions.UnFlowLoss)" % (what, name, t.dtype))
    if t.numel() == 0:
        raise RuntimeError("%s: %s has no pixels: %s" % (what, name, tuple(t.shape)))


def _corresponding_map_cuda(data, is_flow):
    what = "cerberus::corresponding_map"
    _occlusion_check(data, "data", what)
    x = data.contiguous()
    B, _, H, W = x.shape
    lib = _lib.get()
    ws_bytes = lib.cerberus_corresponding_map_workspace_bytes(B, H, W)
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=x.device)      # zeroed on the stream by the library
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.cerberus_corresponding_map(x.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_bytes, B, H, W, int(bool(is_flow)),
                                            0, _stream_ptr(x))
    _lib.check(rc, what)
    return out


def _occlusion_mask_bidirection_cuda(flow12, flow21, scale, bias):
    what = "cerberus::occlusion_mask_bidirection"
    _occlusion_check(flow12, "flow12", what)
    _occlusion_check(flow21, "flow21", what)
    if flow12.shape != flow21.shape:
        raise RuntimeError("%s: flow shapes differ: %s vs %s" % (what, tuple(flow12.shape), tuple(flow21.shape)))
    if flow12.device != flow21.device:
        raise RuntimeError("%s: inputs on different devices: %s vs %s" % (what, flow12.device, flow21.device))
    a, b = flow12.contiguous(), flow21.contiguous()
    B, _, H, W = a.shape
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = _lib.get().cerberus_occlusion_mask_bidirection(a.data_ptr(), b.data_ptr(), out.data_ptr(), B, H, W, float(scale),
                                                            float(bias), 0, _stream_ptr(a))
    _lib.check(rc, what)
    return out


def _occlusion_meta(t, *_):
    return t.new_empty((t.shape[0], 1, t.shape[2], t.shape[3]), dtype=torch.float32)


# the stereo reprojection warp of the depth reconstruction loss (depth_losses.py:112-206), csrc/reproject.hip
def _reproject_check(image, depth, inv_K, proj, what, grad_out=None):
    named = [("image", image), ("depth", depth), ("inv_K", inv_K), ("proj", proj)]
    if grad_out is not None:
        named.append(("grad_out", grad_out))
    for name, t in named:
        if t.dtype != torch.float32:
            raise RuntimeError("%s: %s must be float32, got %s (16-bit tensors take the stock-op path of "
                               "loss_functions.reproject_warp)" % (what, name, t.dtype))
        if t.device != image.device:
            raise RuntimeError("%s: inputs on different devices: image on %s, %s on %s" % (what, image.device, name, t.device))
    if image.dim() != 4 or image.numel() == 0:
        raise RuntimeError("%s: image must be a non-empty 4-D NCHW tensor, got %s" % (what, tuple(image.shape)))
    B, C, H, W = image.shape
    if tuple(depth.shape) != (B, 1, H, W):
        raise RuntimeError("%s: depth must be %s for an image of %s, got %s" % (what, (B, 1, H, W), tuple(image.shape),
                                                                               tuple(depth.shape)))
    if tuple(inv_K.shape) != (B, 3, 3):
        raise RuntimeError("%s: inv_K must be %s (the upper-left 3 x 3 of the inverse intrinsics), got %s"
                           % (what, (B, 3, 3), tuple(inv_K.shape)))
    if tuple(proj.shape) != (B, 3, 4):
        raise RuntimeError("%s: proj must be %s ((K @ T)[:, :3, :]), got %s" % (what, (B, 3, 4), tuple(proj.shape)))
    if grad_out is not None and grad_out.shape != image.shape:
        raise RuntimeError("%s: grad_out %s does not match the image %s" % (what, tuple(grad_out.shape), tuple(image.shape)))
    if H < 2 or W < 2:
        raise RuntimeError("%s: H and W must be at least 2 (positions are normalised by W - 1 and H - 1), got %s"
                           % (what, tuple(image.shape)))


def _reproject_warp_cuda(image, depth, inv_K, proj, eps):
    what = "cerberus::reproject_warp"
    _reproject_check(image, depth, inv_K, proj, what)
    img, d, k, p = image.contiguous(), depth.contiguous(), inv_K.contiguous(), proj.contiguous()
    B, C, H, W = img.shape
    out = _fresh_like(img)
    with torch.cuda.device(img.device):
        rc = _lib.get().cerberus_reproject_warp_forward(img.data_ptr(), d.data_ptr(), k.data_ptr(), p.data_ptr(), out.data_ptr(),
                                                        B, C, H, W, float(eps), 0, _stream_ptr(img))
    _lib.check(rc, what)
    return out


def _reproject_warp_backward_cuda(image, depth, inv_K, proj, grad_out, eps):
    what = "cerberus::reproject_warp_backward"
    _reproject_check(image, depth, inv_K, proj, what, grad_out)
    img, d, k, p, g = (t.contiguous() for t in (image, depth, inv_K, proj, grad_out))
    B, C, H, W = img.shape
    grad = _fresh_like(d)
    with torch.cuda.device(img.device):
        rc = _lib.get().cerberus_reproject_warp_backward(img.data_ptr(), d.data_ptr(), k.data_ptr(), p.data_ptr(), g.data_ptr(),
                                                         grad.data_ptr(), B, C, H, W, float(eps), 0, _stream_ptr(img))
    _lib.check(rc, what)
    return grad


# the segmentation loss (seg_losses.py:121-190), csrc/seg_loss.hip
SEG_CHUNK_PIXELS = 1024                 # pixels per workgroup of the forward: one num and one den partial each
HISTOGRAM_MAX_CLASSES = 2048            # the LDS bins of class_histogram; more classes: torch.bincount in the wrapper


def _seg_workspace_bytes(B, H, W):
    """cerberus_seg_cross_entropy_workspace_bytes in pure Python (a test holds the two equal): an fp32 num and an fp32 den
    partial per 1024 pixels of the flattened (B,H,W) map."""
    if B <= 0 or H <= 0 or W <= 0 or B * H * W > 0x7fffffff - 1024:
        return 0
    return 2 * ((B * H * W + SEG_CHUNK_PIXELS - 1) // SEG_CHUNK_PIXELS) * 4


def _seg_check(logits, target, weight, what):
    if logits.dim() != 4:
        raise RuntimeError("%s: logits must be a 4-D (B,C,H,W) tensor, got %s" % (what, tuple(logits.shape)))
    if logits.dtype != torch.float32:
        raise RuntimeError("%s: logits must be float32, got %s (16-bit logits take the stock-op path of "
                           "loss_functions.seg_cross_entropy)" % (what, logits.dtype))
    if target.dtype != torch.int64:
        raise RuntimeError("%s: target must be int64, got %s" % (what, target.dtype))
    if weight.dtype != torch.float32:
        raise RuntimeError("%s: weight must be float32, got %s" % (what, weight.dtype))
    if target.device != logits.device or weight.device != logits.device:
        raise RuntimeError("%s: inputs on different devices: %s, %s, %s" % (what, logits.device, target.device, weight.device))
    B, C, H, W = logits.shape
    if tuple(target.shape) != (B, H, W):
        raise RuntimeError("%s: target must be (B,H,W) = %s, got %s" % (what, (B, H, W), tuple(target.shape)))
    if tuple(weight.shape) != (C,):
        raise RuntimeError("%s: weight must hold one value per class, (%d,), got %s" % (what, C, tuple(weight.shape)))
    if C < 2 or logits.numel() == 0:
        raise RuntimeError("%s: needs at least 2 classes and one pixel, got %s (loss_functions.seg_cross_entropy takes the "
                           "stock-op path)" % (what, tuple(logits.shape)))


def _seg_cross_entropy_cuda(logits, target, weight, ignore_index, gamma):
    what = "cerberus::seg_cross_entropy"
    _seg_check(logits, target, weight, what)
    x, t, w = logits.contiguous(), target.contiguous(), weight.contiguous()
    B, C, H, W = x.shape
    lib = _lib.get()
    ws_bytes = lib.cerberus_seg_cross_entropy_workspace_bytes(B, H, W)
    ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    lse = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    state = torch.empty((4,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.cerberus_seg_cross_entropy_forward(x.data_ptr(), t.data_ptr(), w.data_ptr(), loss.data_ptr(), lse.data_ptr(),
                                                    state.data_ptr(), ws.data_ptr(), ws_bytes, B, C, H, W, int(ignore_index),
                                                    ctypes.c_float(gamma), 0, _stream_ptr(x))
    _lib.check(rc, what)
    return loss, lse, state


def _seg_cross_entropy_meta(logits, target, weight, ignore_index, gamma):
    B, _, H, W = logits.shape
    f = lambda *shape: logits.new_empty(shape, dtype=torch.float32)
    return f(), f(B, H, W), f(4)


def _seg_cross_entropy_backward_cuda(logits, target, weight, lse, state, grad_loss, ignore_index):
    what = "cerberus::seg_cross_entropy_backward"
    _seg_check(logits, target, weight, what)
    B, C, H, W = logits.shape
    for t, name, shape in ((lse, "lse", (B, H, W)), (state, "state", (4,))):
        if t.dtype != torch.float32 or t.device != logits.device or tuple(t.shape) != shape:
            raise RuntimeError("%s: %s must be the float32 %s tensor of the forward, got %s %s" % (what, name, shape, t.dtype,
                                                                                                  tuple(t.shape)))
    x, t, w = logits.contiguous(), target.contiguous(), weight.contiguous()
    # named, so that each copy lives until the launch is enqueued: a temporary ``v.contiguous().data_ptr()`` is freed at once,
    # and the next copy may be handed its block while the first pointer is still to be read
    ls, st = lse.contiguous(), state.contiguous()
    g = _grad_scalar(grad_loss, x, what)
    grad = _fresh_like(x)          # every element is written by the kernel
    with torch.cuda.device(x.device):
        rc = _lib.get().cerberus_seg_cross_entropy_backward(x.data_ptr(), t.data_ptr(), w.data_ptr(), ls.data_ptr(),
                                                            st.data_ptr(), g.data_ptr(), grad.data_ptr(), B, C, H,
                                                            W, int(ignore_index), 0, _stream_ptr(x))
    _lib.check(rc, what)
    return grad


# OHEM cross-entropy (seg_losses.py:40-119), csrc/seg_ohem.hip
OHEM_DIGIT_BITS = (11, 11, 10)          # the radix select fixes the 32 bits of a probability in three digits, from the top
OHEM_BINS = 2048                        # bins of one digit's histogram (LDS per workgroup, then global)
OHEM_SELECT_WORDS = 8                   # the select state in the workspace: prefix, rank, num_valid, branch
OHEM_STATE_FLOATS = 8                   # [ce, den, 1 / den, threshold, keep_all, rank left among the ties at kth, 0, 0]


def _seg_ohem_workspace_bytes(B, H, W):
    """cerberus_seg_ohem_workspace_bytes in pure Python (a test holds the two equal): lse - x_t per pixel (the pixels rounded
    up to a multiple of 4), an fp32 num, an fp32 den and a uint32 kept partial per 1024 pixels, the bins of the three digits
    and the select state."""
    if B <= 0 or H <= 0 or W <= 0 or B * H * W > 0x7fffffff - 1024:
        return 0
    n = B * H * W
    words = (n + 3) // 4 * 4 + 3 * ((n + SEG_CHUNK_PIXELS - 1) // SEG_CHUNK_PIXELS) + len(OHEM_DIGIT_BITS) * OHEM_BINS
    return (words + OHEM_SELECT_WORDS) * 4


def _seg_ohem_cuda(logits, target, weight, ignore_index, thresh, min_kept):
    what = "cerberus::seg_ohem_cross_entropy"
    _seg_check(logits, target, weight, what)
    if thresh != thresh:
        raise RuntimeError("%s: thresh is NaN" % what)
    x, t, w = logits.contiguous(), target.contiguous(), weight.contiguous()
    B, C, H, W = x.shape
    lib = _lib.get()
    ws_bytes = lib.cerberus_seg_ohem_workspace_bytes(B, H, W)
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
    ws = f((max(ws_bytes, 4) + 3) // 4)
    loss, prob, lse, state = f(), f(B, H, W), f(B, H, W), f(OHEM_STATE_FLOATS)
    counts = torch.empty((2,), dtype=torch.int64, device=x.device)
    min_kept = max(-1, min(int(min_kept), 2 ** 62))       # what the kernels compare with a count below 2^31
    with torch.cuda.device(x.device):
        rc = lib.cerberus_seg_ohem_forward(x.data_ptr(), t.data_ptr(), w.data_ptr(), loss.data_ptr(), prob.data_ptr(), lse.data_ptr(),
                                           state.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes, B, C, H, W,
                                           int(ignore_index), ctypes.c_float(thresh), min_kept, 0, _stream_ptr(x))
    _lib.check(rc, what)
    return loss, prob, lse, state, counts


def _seg_ohem_meta(logits, target, weight, ignore_index, thresh, min_kept):
    B, _, H, W = logits.shape
    f = lambda *shape: logits.new_empty(shape, dtype=torch.float32)
    return f(), f(B, H, W), f(B, H, W), f(OHEM_STATE_FLOATS), logits.new_empty((2,), dtype=torch.int64)


def _seg_ohem_backward_cuda(logits, target, weight, prob, lse, state, grad_loss, ignore_index):
    what = "cerberus::seg_ohem_cross_entropy_backward"
    _seg_check(logits, target, weight, what)
    B, C, H, W = logits.shape
    for t, name, shape in ((prob, "prob", (B, H, W)), (lse, "lse", (B, H, W)), (state, "state", (OHEM_STATE_FLOATS,))):
        if t.dtype != torch.float32 or t.device != logits.device or tuple(t.shape) != shape:
            raise RuntimeError("%s: %s must be the float32 %s tensor of the forward, got %s %s" % (what, name, shape, t.dtype,
                                                                                                  tuple(t.shape)))
    x, t, w = logits.contiguous(), target.contiguous(), weight.contiguous()
    pr, ls, st = prob.contiguous(), lse.contiguous(), state.contiguous()      # named: alive until the launch (see above)
    g = _grad_scalar(grad_loss, x, what)
    grad = _fresh_like(x)          # every element is written by the kernel
    with torch.cuda.device(x.device):
        rc = _lib.get().cerberus_seg_ohem_backward(x.data_ptr(), t.data_ptr(), w.data_ptr(), pr.data_ptr(),
                                                   ls.data_ptr(), st.data_ptr(), g.data_ptr(),
                                                   grad.data_ptr(), B, C, H, W, int(ignore_index), 0, _stream_ptr(x))
    _lib.check(rc, what)
    return grad


# the RMI loss (rmi.py:33-207), csrc/rmi_loss.hip
RMI_RADIUS = 3                          # the radius of the fused route
RMI_MAX_POOL = 8                        # its largest pooling window (the labels of a window are staged in LDS)
RMI_CELLS_PER_WORKGROUP = 256           # pooling windows per front-end workgroup
RMI_CLASS_GROUP = 8                     # class planes per front-end workgroup
RMI_POSITIONS_PER_WORKGROUP = 1024      # positions of the 3 x 3 slices per moment workgroup
RMI_ENTRIES = 3 * 81                    # la_cov, pr_cov, la_pr_cov


def _rmi_pooled(size, pool):
    return (size + 2 * (pool // 2) - pool) // pool + 1


def rmi_fused_shape_ok(C, H, W, radius, pool):
    """The shapes cerberus::rmi_moments takes: radius 3, pool 1..8, a pooled map of at least 3 x 3 (the C ABI's own limits)."""
    return (radius == RMI_RADIUS and 1 <= pool <= RMI_MAX_POOL and 1 <= C <= 32767 and H > 0 and W > 0
            and H * W <= 0x7fffffff - 1024 and _rmi_pooled(H, pool) >= radius and _rmi_pooled(W, pool) >= radius)


def _rmi_workspace_bytes(B, C, H, W, pool):
    """cerberus_rmi_workspace_bytes in pure Python (a test holds the two equal): float64 -- a BCE and a count partial per
    front-end workgroup (256 windows of 8 class planes of one image), 243 partial products per moment workgroup (1024 positions
    of one (n, c))."""
    if not (0 < B <= 65535 and pool >= 1 and rmi_fused_shape_ok(C, H, W, RMI_RADIUS, pool)):
        return 0
    pad = pool // 2
    cells = ((H - 1 + pad) // pool + 1) * ((W - 1 + pad) // pool + 1)
    parts = B * ((C + RMI_CLASS_GROUP - 1) // RMI_CLASS_GROUP) * ((cells + RMI_CELLS_PER_WORKGROUP - 1) // RMI_CELLS_PER_WORKGROUP)
    positions = (_rmi_pooled(H, pool) - 2) * (_rmi_pooled(W, pool) - 2)
    chunks = (positions + RMI_POSITIONS_PER_WORKGROUP - 1) // RMI_POSITIONS_PER_WORKGROUP
    if B * C * chunks > 0x7fffffff:
        return 0
    return 8 * (2 * parts + B * C * chunks * RMI_ENTRIES)


def _rmi_check(logits, target, radius, pool, what):
    if logits.dim() != 4:
        raise RuntimeError("%s: logits must be a 4-D (B,C,H,W) tensor, got %s" % (what, tuple(logits.shape)))
    if logits.dtype != torch.float32:
        raise RuntimeError("%s: logits must be float32, got %s (16-bit logits take the stock-op path of "
                           "loss_functions.rmi_loss)" % (what, logits.dtype))
    if target.dtype != torch.int64:
        raise RuntimeError("%s: target must be int64, got %s" % (what, target.dtype))
    if target.device != logits.device:
        raise RuntimeError("%s: inputs on different devices: %s, %s" % (what, logits.device, target.device))
    B, C, H, W = logits.shape
    if tuple(target.shape) != (B, H, W):
        raise RuntimeError("%s: target must be (B,H,W) = %s, got %s" % (what, (B, H, W), tuple(target.shape)))
    if B == 0 or not rmi_fused_shape_ok(C, H, W, radius, pool):
        raise RuntimeError("%s: needs radius 3, a pool of 1..8 and a pooled map of at least 3 x 3, got %s, radius %d, pool %d "
                           "(loss_functions.rmi_loss takes the stock-op path)" % (what, tuple(logits.shape), radius, pool))


def _rmi_shapes(B, C, H, W, pool, do_rmi):
    if not do_rmi:
        return (0,), (0,), (0,)
    return (B, C, 9, 9), (B, C, _rmi_pooled(H, pool), _rmi_pooled(W, pool)), (B, C, 2, 9)


def _rmi_moments_cuda(logits, target, radius, pool, do_rmi):
    what = "cerberus::rmi_moments"
    _rmi_check(logits, target, radius, pool, what)
    x, t = logits.contiguous(), target.contiguous()
    B, C, H, W = x.shape
    lib = _lib.get()
    ws_bytes = lib.cerberus_rmi_workspace_bytes(B, C, H, W, pool)
    ws = torch.empty((max(ws_bytes, 8) + 7) // 8, dtype=torch.float64, device=x.device)
    cov_shape, map_shape, mean_shape = _rmi_shapes(B, C, H, W, pool, do_rmi)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=x.device)
    bce, state = f32(), f32(4)
    la_cov, pr_cov, la_pr_cov, means = f64(*cov_shape), f64(*cov_shape), f64(*cov_shape), f64(*mean_shape)
    la_map, pr_map = f32(*map_shape), f32(*map_shape)          # with do_rmi off: empty, and never written
    ptr = lambda v: v.data_ptr() if do_rmi else None
    with torch.cuda.device(x.device):
        rc = lib.cerberus_rmi_forward(x.data_ptr(), t.data_ptr(), bce.data_ptr(), state.data_ptr(), ptr(la_map), ptr(pr_map),
                                      ptr(means), ptr(la_cov), ptr(pr_cov), ptr(la_pr_cov), ws.data_ptr(), ws_bytes, B, C, H, W,
                                      int(radius), int(pool), int(bool(do_rmi)), 0, _stream_ptr(x))
    _lib.check(rc, what)
    return bce, la_cov, pr_cov, la_pr_cov, la_map, pr_map, means, state


def _rmi_moments_meta(logits, target, radius, pool, do_rmi):
    B, C, H, W = logits.shape
    cov_shape, map_shape, mean_shape = _rmi_shapes(B, C, H, W, pool, do_rmi)
    f32 = lambda *shape: logits.new_empty(shape, dtype=torch.float32)
    f64 = lambda *shape: logits.new_empty(shape, dtype=torch.float64)
    return f32(), f64(*cov_shape), f64(*cov_shape), f64(*cov_shape), f32(*map_shape), f32(*map_shape), f64(*mean_shape), f32(4)


def _rmi_moments_backward_cuda(logits, target, la_map, pr_map, means, state, grad_bce, grad_pr_cov, grad_la_pr_cov, radius, pool,
                               do_rmi):
    what = "cerberus::rmi_moments_backward"
    _rmi_check(logits, target, radius, pool, what)
    B, C, H, W = logits.shape
    cov_shape, map_shape, mean_shape = _rmi_shapes(B, C, H, W, pool, do_rmi)
    for v, name, shape, dtype in ((la_map, "la_map", map_shape, torch.float32), (pr_map, "pr_map", map_shape, torch.float32),
                                  (means, "means", mean_shape, torch.float64), (state, "state", (4,), torch.float32),
                                  (grad_pr_cov, "grad_pr_cov", cov_shape, torch.float64),
                                  (grad_la_pr_cov, "grad_la_pr_cov", cov_shape, torch.float64)):
        if v.dtype != dtype or v.device != logits.device or tuple(v.shape) != shape:
            raise RuntimeError("%s: %s must be the %s %s tensor of the forward, got %s %s" % (what, name, dtype, shape, v.dtype,
                                                                                           tuple(v.shape)))
    x, t = logits.contiguous(), target.contiguous()
    g = _grad_scalar(grad_bce, x, what)
    grad = _fresh_like(x)          # every element is written by the kernel
    # named: every copy lives until the launch is enqueued (see _seg_cross_entropy_backward_cuda)
    st = state.contiguous()
    la, pr, mu, gp, glp = (v.contiguous() for v in (la_map, pr_map, means, grad_pr_cov, grad_la_pr_cov))
    ptr = lambda v: v.data_ptr() if do_rmi else None
    with torch.cuda.device(x.device):
        rc = _lib.get().cerberus_rmi_backward(x.data_ptr(), t.data_ptr(), st.data_ptr(), ptr(la), ptr(pr),
                                              ptr(mu), g.data_ptr(), ptr(gp), ptr(glp), grad.data_ptr(), B, C,
                                              H, W, int(radius), int(pool), int(bool(do_rmi)), 0, _stream_ptr(x))
    _lib.check(rc, what)
    return grad


def _class_histogram_cuda(target, num_classes, ignore_index):
    what = "cerberus::class_histogram"
    if target.dtype != torch.int64:
        raise RuntimeError("%s: target must be int64, got %s" % (what, target.dtype))
    if not 1 <= num_classes <= HISTOGRAM_MAX_CLASSES:
        raise RuntimeError("%s: num_classes must lie in 1..%d, got %d (loss_functions.class_balance_weights takes "
                           "torch.bincount above it)" % (what, HISTOGRAM_MAX_CLASSES, num_classes))
    t = target.contiguous()
    if t.numel() == 0:
        return torch.zeros((num_classes,), dtype=torch.int64, device=t.device)
    counts = torch.empty((num_classes,), dtype=torch.int64, device=t.device)      # zeroed on the stream by the call
    with torch.cuda.device(t.device):
        rc = _lib.get().cerberus_class_histogram(t.data_ptr(), counts.data_ptr(), t.numel(), int(num_classes), int(ignore_index),
                                                 _stream_ptr(t))
    _lib.check(rc, what)
    return counts


# the supervised depth loss InvHuberLoss (depth_losses.py:64-88), csrc/depth_loss.hip
INV_HUBER_CHUNK_PIXELS = 1024           # pixels per workgroup of the sum pass: a partial of sum(term), of S and of ties each
INV_HUBER_MAX_PARTS = 1024              # partial maxima of the max pass


def _inv_huber_workspace_bytes(B, h, w):
    """cerberus_inv_huber_workspace_bytes in pure Python (a test holds the two equal): 1024 partial maxima, then an fp32
    sum(term), an fp32 S and a uint32 ties partial per 1024 pixels of the flattened (B,h,w) prediction."""
    if B <= 0 or h <= 0 or w <= 0 or B * h * w > 0x7fffffff - 1024:
        return 0
    return (INV_HUBER_MAX_PARTS + 3 * ((B * h * w + INV_HUBER_CHUNK_PIXELS - 1) // INV_HUBER_CHUNK_PIXELS)) * 4


def _inv_huber_check(pred, gt, what):
    """(B, h, w, H, W) of a prediction (B,1,h,w) or (B,h,w) and a ground truth (B,H,W) the op takes."""
    if pred.dim() == 4 and pred.shape[1] == 1:
        shape = (pred.shape[0],) + tuple(pred.shape[2:])
    elif pred.dim() == 3:
        shape = tuple(pred.shape)
    else:
        raise RuntimeError("%s: pred must be (B,1,h,w) or (B,h,w), got %s" % (what, tuple(pred.shape)))
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError("%s: pred and gt must be float32, got %s and %s (16-bit and 64-bit tensors take the stock-op path "
                           "of loss_functions.inv_huber_loss)" % (what, pred.dtype, gt.dtype))
    if gt.device != pred.device:
        raise RuntimeError("%s: inputs on different devices: %s, %s" % (what, pred.device, gt.device))
    if gt.dim() != 3 or gt.shape[0] != shape[0]:
        raise RuntimeError("%s: gt must be (B,H,W) with B = %d, got %s" % (what, shape[0], tuple(gt.shape)))
    B, h, w = shape
    H, W = gt.shape[1:]
    if pred.numel() == 0 or gt.numel() == 0:
        raise RuntimeError("%s: needs at least one pixel, got %s and %s" % (what, tuple(pred.shape), tuple(gt.shape)))
    if H % h != 0 or W % w != 0:
        raise RuntimeError("%s: the gt size %s must be an integer multiple of the prediction's %s (loss_functions.inv_huber_loss "
                           "resizes the ground truth for any other ratio)" % (what, (H, W), (h, w)))
    if B * h * w > 0x7fffffff - 1024:
        raise RuntimeError("%s: %d pixels do not fit the kernels' 32-bit pixel index" % (what, B * h * w))
    return B, h, w, H, W


def _inv_huber_cuda(pred, gt):
    what = "cerberus::inv_huber"
    B, h, w, H, W = _inv_huber_check(pred, gt, what)
    p, g = pred.contiguous(), gt.contiguous()
    lib = _lib.get()
    ws_bytes = lib.cerberus_inv_huber_workspace_bytes(B, h, w)
    ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=p.device)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    state = torch.empty((4,), dtype=torch.float32, device=p.device)
    with torch.cuda.device(p.device):
        rc = lib.cerberus_inv_huber_forward(p.data_ptr(), g.data_ptr(), loss.data_ptr(), state.data_ptr(), ws.data_ptr(), ws_bytes,
                                            B, h, w, H, W, 0, _stream_ptr(p))
    _lib.check(rc, what)
    return loss, state


def _inv_huber_meta(pred, gt):
    return pred.new_empty((), dtype=torch.float32), pred.new_empty((4,), dtype=torch.float32)


def _inv_huber_backward_cuda(pred, gt, state, grad_loss):
    what = "cerberus::inv_huber_backward"
    B, h, w, H, W = _inv_huber_check(pred, gt, what)
    if state.dtype != torch.float32 or state.device != pred.device or tuple(state.shape) != (4,):
        raise RuntimeError("%s: state must be the float32 (4,) tensor of the forward, got %s %s" % (what, state.dtype,
                                                                                                   tuple(state.shape)))
    p, g, st = pred.contiguous(), gt.contiguous(), state.contiguous()
    gl = _grad_scalar(grad_loss, p, what)
    grad = _fresh_like(p)          # every element is written by the kernel
    with torch.cuda.device(p.device):
        rc = _lib.get().cerberus_inv_huber_backward(p.data_ptr(), g.data_ptr(), st.data_ptr(), gl.data_ptr(),
                                                    grad.data_ptr(), B, h, w, H, W, 0, _stream_ptr(p))
    _lib.check(rc, what)
    return grad


# the training metrics (nnet_training/statistics/), csrc/metrics.hip
METRIC_CHUNK_PIXELS = 1024              # pixels of ONE image per workgroup: a partial per sum and count each
SEG_CONFUSION_MAX_CLASSES = 64          # C*C 32-bit LDS bins (16 KiB); more classes: the stock chain in statistics.SegmentationMetric
METRIC_MAX_BATCH = 65535                # the image is the launch grid's second dimension


def _metric_workspace_bytes(B, H, W, nsums, ncounts):
    if B <= 0 or B > METRIC_MAX_BATCH or H <= 0 or W <= 0 or H * W > 0x7fffffff - 1024:
        return 0
    return B * ((H * W + METRIC_CHUNK_PIXELS - 1) // METRIC_CHUNK_PIXELS) * (8 * nsums + 4 * ncounts)


def _depth_metric_workspace_bytes(B, h, w):
    """cerberus_depth_metric_workspace_bytes in pure Python (a test holds the two equal): five float64 sums and four uint32
    counts per 1024 pixels of each image."""
    return _metric_workspace_bytes(B, h, w, 5, 4)


def _flow_metric_workspace_bytes(B, H, W):
    """cerberus_flow_metric_workspace_bytes in pure Python: two float64 sums and one uint32 count per 1024 pixels of each image."""
    return _metric_workspace_bytes(B, H, W, 2, 1)


def _warp_sad_workspace_bytes(B, H, W):
    """cerberus_warp_sad_workspace_bytes in pure Python: one float64 sum per 1024 pixels of each image."""
    return _metric_workspace_bytes(B, H, W, 1, 0)


def _metric_check(what, tensors, shapes, dtypes=None):
    """Every (name, tensor) of ``tensors`` is on the first one's device, has the shape of ``shapes`` and is float32 (or the
    dtype of ``dtypes``); the batch and the image fit the launch grid."""
    first = tensors[0][1]
    for i, (name, t) in enumerate(tensors):
        want = (dtypes or {}).get(name, torch.float32)
        if t.dtype != want:
            raise RuntimeError("%s: %s must be %s, got %s (other dtypes take the stock-op path of cerberusnet_amd.statistics)"
                               % (what, name, str(want).replace("torch.", ""), t.dtype))
        if t.device != first.device:
            raise RuntimeError("%s: inputs on different devices: %s, %s" % (what, first.device, t.device))
        if tuple(t.shape) != tuple(shapes[i]):
            raise RuntimeError("%s: %s must be %s, got %s" % (what, name, tuple(shapes[i]), tuple(t.shape)))
    if first.numel() == 0:
        raise RuntimeError("%s: needs at least one pixel, got %s" % (what, tuple(first.shape)))
    B, H, W = first.shape[0], first.shape[-2], first.shape[-1]
    if B > METRIC_MAX_BATCH or H * W > 0x7fffffff - 1024:
        raise RuntimeError("%s: %d images of %d pixels do not fit the kernels' launch grid" % (what, B, H * W))


def _metric_workspace(nbytes, device):
    return torch.empty((max(nbytes, 8) + 7) // 8, dtype=torch.float64, device=device)     # 8-byte aligned, never zeroed


def _seg_confusion_cuda(logits, target, ignore_index):
    what = "cerberus::seg_confusion"
    if logits.dim() != 4:
        raise RuntimeError("%s: logits must be a 4-D (B,C,H,W) tensor, got %s" % (what, tuple(logits.shape)))
    B, C, H, W = logits.shape
    _metric_check(what, [("logits", logits), ("target", target)], [(B, C, H, W), (B, H, W)], {"target": torch.int64})
    if not 2 <= C <= SEG_CONFUSION_MAX_CLASSES:
        raise RuntimeError("%s: the class count must lie in 2..%d, got %d (statistics.SegmentationMetric takes the stock-op path "
                           "outside it)" % (what, SEG_CONFUSION_MAX_CLASSES, C))
    x, t = logits.contiguous(), target.contiguous()
    conf = torch.empty((B, C, C), dtype=torch.int64, device=x.device)            # zeroed on the stream by the call
    with torch.cuda.device(x.device):
        rc = _lib.get().cerberus_seg_confusion(x.data_ptr(), t.data_ptr(), conf.data_ptr(), B, C, H, W, int(ignore_index), 0,
                                               _stream_ptr(x))
    _lib.check(rc, what)
    return conf


def _depth_metric_shape(pred, what):
    if pred.dim() == 4 and pred.shape[1] == 1:
        return (pred.shape[0],) + tuple(pred.shape[2:])
    if pred.dim() == 3:
        return tuple(pred.shape)
    raise RuntimeError("%s: pred must be (B,1,h,w) or (B,h,w), got %s" % (what, tuple(pred.shape)))


def _depth_metric_sums_cuda(pred, gt, min_depth, max_depth):
    what = "cerberus::depth_metric_sums"
    B, h, w = _depth_metric_shape(pred, what)
    _metric_check(what, [("pred", pred), ("gt", gt)], [tuple(pred.shape), (B, h, w)])
    if not min_depth < max_depth:
        raise RuntimeError("%s: min_depth %r must lie below max_depth %r" % (what, min_depth, max_depth))
    p, g = pred.contiguous(), gt.contiguous()
    lib = _lib.get()
    ws_bytes = lib.cerberus_depth_metric_workspace_bytes(B, h, w)
    ws = _metric_workspace(ws_bytes, p.device)
    sums = torch.empty((B, 5), dtype=torch.float64, device=p.device)
    counts = torch.empty((B, 4), dtype=torch.int64, device=p.device)
    with torch.cuda.device(p.device):
        rc = lib.cerberus_depth_metric_sums(p.data_ptr(), g.data_ptr(), sums.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes,
                                            B, h, w, ctypes.c_float(min_depth), ctypes.c_float(max_depth), 0, _stream_ptr(p))
    _lib.check(rc, what)
    return sums, counts


def _flow_metric_sums_cuda(flow_pred, flow_gt, mask):
    what = "cerberus::flow_metric_sums"
    if flow_pred.dim() != 4 or flow_pred.shape[1] != 2:
        raise RuntimeError("%s: flow_pred must be a 4-D (B,2,H,W) tensor, got %s" % (what, tuple(flow_pred.shape)))
    B, _, H, W = flow_pred.shape
    _metric_check(what, [("flow_pred", flow_pred), ("flow_gt", flow_gt), ("mask", mask)], [(B, 2, H, W), (B, 2, H, W), (B, H, W)])
    fp, fg, m = flow_pred.contiguous(), flow_gt.contiguous(), mask.contiguous()
    lib = _lib.get()
    ws_bytes = lib.cerberus_flow_metric_workspace_bytes(B, H, W)
    ws = _metric_workspace(ws_bytes, fp.device)
    sums = torch.empty((B, 2), dtype=torch.float64, device=fp.device)
    counts = torch.empty((B, 1), dtype=torch.int64, device=fp.device)
    with torch.cuda.device(fp.device):
        rc = lib.cerberus_flow_metric_sums(fp.data_ptr(), fg.data_ptr(), m.data_ptr(), sums.data_ptr(), counts.data_ptr(),
                                           ws.data_ptr(), ws_bytes, B, H, W, 0, _stream_ptr(fp))
    _lib.check(rc, what)
    return sums, counts


def _warp_sad_cuda(image, source, flow):
    what = "cerberus::warp_sad"
    if image.dim() != 4:
        raise RuntimeError("%s: image must be a 4-D (B,C,H,W) tensor, got %s" % (what, tuple(image.shape)))
    B, C, H, W = image.shape
    _metric_check(what, [("image", image), ("source", source), ("flow", flow)], [(B, C, H, W), (B, C, H, W), (B, 2, H, W)])
    im, src, fl = image.contiguous(), source.contiguous(), flow.contiguous()
    lib = _lib.get()
    ws_bytes = lib.cerberus_warp_sad_workspace_bytes(B, H, W)
    ws = _metric_workspace(ws_bytes, im.device)
    sad = torch.empty((B,), dtype=torch.float64, device=im.device)
    with torch.cuda.device(im.device):
        rc = lib.cerberus_warp_sad(im.data_ptr(), src.data_ptr(), fl.data_ptr(), sad.data_ptr(), ws.data_ptr(), ws_bytes, B, C, H, W,
                                   0, _stream_ptr(im))
    _lib.check(rc, what)
    return sad


def _seg_confusion_meta(logits, target, ignore_index):
    return logits.new_empty((logits.shape[0], logits.shape[1], logits.shape[1]), dtype=torch.int64)


def _depth_metric_sums_meta(pred, gt, min_depth, max_depth):
    return pred.new_empty((pred.shape[0], 5), dtype=torch.float64), pred.new_empty((pred.shape[0], 4), dtype=torch.int64)


def _flow_metric_sums_meta(flow_pred, flow_gt, mask):
    B = flow_pred.shape[0]
    return flow_pred.new_empty((B, 2), dtype=torch.float64), flow_pred.new_empty((B, 1), dtype=torch.int64)


# the panoptic metric (nnet_training/statistics/panoptic.py, utilities/panoptic_post_processing.py), csrc/panoptic.hip
CENTER_PEAKS_MAX_KERNEL = 15            # odd NMS windows 1..15: the halo of a 16 x 64 LDS tile
GROUP_PIXELS_MAX_CENTERS = 4096         # centres per image, walked through LDS 256 at a time; more: the stock chain
INSTANCE_OVERLAP_MAX_BINS = 16128       # max_ids * (max_ids + 2 * num_classes) 32-bit LDS bins (63 KiB): 101 ids x 19 classes fit


def thing_mask_of(thing_list):
    """The 64-bit mask ``group_pixels`` takes: bit c set for every thing class c; None if a class lies outside [0, 64) (the
    caller takes the stock ops then)."""
    mask = 0
    for c in thing_list:
        c = int(c)
        if not 0 <= c < 64:
            return None
        mask |= 1 << c
    return mask


def _heatmap_shape(heatmap, what):
    if heatmap.dim() == 4 and heatmap.shape[1] == 1:
        return (heatmap.shape[0],) + tuple(heatmap.shape[2:])
    if heatmap.dim() == 3:
        return tuple(heatmap.shape)
    raise RuntimeError("%s: heatmap must be (B,1,H,W) or (B,H,W), got %s" % (what, tuple(heatmap.shape)))


def _center_peaks_cuda(heatmap, threshold, nms_kernel):
    what = "cerberus::center_peaks"
    B, H, W = _heatmap_shape(heatmap, what)
    _metric_check(what, [("heatmap", heatmap)], [tuple(heatmap.shape)])
    if nms_kernel < 1 or nms_kernel % 2 == 0 or nms_kernel > CENTER_PEAKS_MAX_KERNEL:
        raise RuntimeError("%s: nms_kernel must be odd and lie in 1..%d, got %d" % (what, CENTER_PEAKS_MAX_KERNEL, nms_kernel))
    x = heatmap.contiguous()
    out = _fresh_like(x)               # every element is written by the kernel; the input never is
    with torch.cuda.device(x.device):
        rc = _lib.get().cerberus_center_peaks(x.data_ptr(), out.data_ptr(), B, H, W, ctypes.c_float(threshold), int(nms_kernel), 0,
                                              _stream_ptr(x))
    _lib.check(rc, what)
    return out


def _group_pixels_cuda(offsets, centers, counts, sem, thing_mask):
    what = "cerberus::group_pixels"
    if offsets.dim() != 4 or offsets.shape[1] != 2:
        raise RuntimeError("%s: offsets must be a 4-D (B,2,H,W) tensor, got %s" % (what, tuple(offsets.shape)))
    B, _, H, W = offsets.shape
    if centers.dim() != 3 or centers.shape[0] != B or centers.shape[2] != 2:
        raise RuntimeError("%s: centers must be (B,Kmax,2) with B = %d, got %s" % (what, B, tuple(centers.shape)))
    kmax = centers.shape[1]
    tensors = [("offsets", offsets), ("centers", centers), ("counts", counts)] + ([("sem", sem)] if sem is not None else [])
    shapes = [(B, 2, H, W), (B, kmax, 2), (B,)] + ([(B, H, W)] if sem is not None else [])
    _metric_check(what, tensors, shapes, {"centers": torch.int64, "counts": torch.int64, "sem": torch.int64})
    if kmax > GROUP_PIXELS_MAX_CENTERS:
        raise RuntimeError("%s: at most %d centres per image, got %d (utilities.panoptic_post_processing takes the stock-op path "
                           "above it)" % (what, GROUP_PIXELS_MAX_CENTERS, kmax))
    thing_mask = int(thing_mask) & 0xFFFFFFFFFFFFFFFF      # the schema's int is signed: bit 63 arrives as the sign
    if kmax == 0:                          # no centre anywhere: nothing to launch
        return torch.zeros((B, H, W), dtype=torch.int64, device=offsets.device)
    off, ctr, cnt = offsets.contiguous(), centers.contiguous(), counts.contiguous()
    sm = sem.contiguous() if sem is not None else None
    out = torch.empty((B, H, W), dtype=torch.int64, device=off.device)
    with torch.cuda.device(off.device):
        rc = _lib.get().cerberus_group_pixels(off.data_ptr(), ctr.data_ptr(), cnt.data_ptr(), sm.data_ptr() if sm is not None else None,
                                              out.data_ptr(), B, H, W, kmax, int(thing_mask), 0, _stream_ptr(off))
    _lib.check(rc, what)
    return out


def _instance_overlap_cuda(pred_inst, tgt_inst, pred_seg, tgt_seg, max_ids, num_classes):
    what = "cerberus::instance_overlap"
    if pred_inst.dim() != 3:
        raise RuntimeError("%s: pred_inst must be a 3-D (B,H,W) tensor, got %s" % (what, tuple(pred_inst.shape)))
    B, H, W = pred_inst.shape
    names = ("pred_inst", "tgt_inst", "pred_seg", "tgt_seg")
    _metric_check(what, list(zip(names, (pred_inst, tgt_inst, pred_seg, tgt_seg))), [(B, H, W)] * 4, dict.fromkeys(names, torch.int64))
    M, C = int(max_ids), int(num_classes)
    if M < 1 or C < 1 or M * (M + 2 * C) > INSTANCE_OVERLAP_MAX_BINS:
        raise RuntimeError("%s: max_ids and num_classes must be positive with max_ids * (max_ids + 2 * num_classes) <= %d, got %d "
                           "and %d" % (what, INSTANCE_OVERLAP_MAX_BINS, M, C))
    maps = [t.contiguous() for t in (pred_inst, tgt_inst, pred_seg, tgt_seg)]
    dev = maps[0].device
    inter = torch.empty((B, M, M), dtype=torch.int64, device=dev)               # zeroed on the stream by the call
    pred_cls = torch.empty((B, M, C), dtype=torch.int64, device=dev)
    tgt_cls = torch.empty((B, M, C), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.get().cerberus_instance_overlap(*[m.data_ptr() for m in maps], inter.data_ptr(), pred_cls.data_ptr(),
                                                  tgt_cls.data_ptr(), B, H, W, M, C, _stream_ptr(maps[0]))
    _lib.check(rc, what)
    return inter, pred_cls, tgt_cls


def _group_pixels_meta(offsets, centers, counts, sem, thing_mask):
    return offsets.new_empty((offsets.shape[0],) + tuple(offsets.shape[2:]), dtype=torch.int64)


def _instance_overlap_meta(pred_inst, tgt_inst, pred_seg, tgt_seg, max_ids, num_classes):
    B = pred_inst.shape[0]
    return (pred_inst.new_empty((B, max_ids, max_ids), dtype=torch.int64), pred_inst.new_empty((B, max_ids, num_classes), dtype=torch.int64),
            pred_inst.new_empty((B, max_ids, num_classes), dtype=torch.int64))


def center_peaks(heatmap, threshold=0.1, nms_kernel=3):
    """``cerberus::center_peaks``: the thresholded, non-maximum-suppressed copy of a (B,1,H,W) or (B,H,W) float32 CUDA heat
    map (-1 everywhere but at the peaks); the input is not written."""
    return torch.ops.cerberus.center_peaks(heatmap, float(threshold), int(nms_kernel))


def group_pixels(offsets, centers, counts, sem=None, thing_mask=0xFFFFFFFFFFFFFFFF):
    """``cerberus::group_pixels``: the (B,H,W) int64 instance ids (1 + the index of the nearest centre) of (B,2,H,W) float32
    CUDA offsets for (B,Kmax,2) int64 centres of which ``counts[b]`` are valid; with ``sem`` only pixels of a class whose bit
    is set in ``thing_mask`` keep their id."""
    mask = int(thing_mask)
    return torch.ops.cerberus.group_pixels(offsets, centers, counts, sem, mask - (1 << 64) if mask >= 1 << 63 else mask)


def instance_overlap(pred_inst, tgt_inst, pred_seg, tgt_seg, max_ids, num_classes):
    """``cerberus::instance_overlap``: the (B,M,M) intersection counts of two (B,H,W) int64 CUDA id maps and the (B,M,C) class
    histograms of each one's instances."""
    return torch.ops.cerberus.instance_overlap(pred_inst, tgt_inst, pred_seg, tgt_seg, int(max_ids), int(num_classes))


# the training side of the panoptic branch (datasets/cityscapes_panoptic_transform.py, loss_functions/panoptic_loss.py),
# csrc/panoptic_train.hip
PANOPTIC_TARGETS_MAX_SEGMENTS = 256     # rows of an image's segment table: one per thread of a workgroup; more: the stock route
PANOPTIC_CHUNK_PIXELS = 1024            # pixels (elements) per workgroup: three fp32 partials each in the loss
PANOPTIC_LOSS_MODES = {"reference": 0, "pixel": 1}
_PANOPTIC_TARGET_NAMES = ("semantic", "foreground", "center", "offset", "semantic_mask", "center_mask", "offset_mask", "center_points")


def _panoptic_targets_workspace_bytes(B, H, W, S):
    """cerberus_panoptic_targets_workspace_bytes in pure Python (a test holds the two equal): per row three 64-bit moments, an
    int64 category, two int32 centre coordinates and an int32 flag word; a 32-bit row per pixel, padded to 16 bytes."""
    if B <= 0 or B > METRIC_MAX_BATCH or H <= 0 or W <= 0 or S <= 0 or S > PANOPTIC_TARGETS_MAX_SEGMENTS or H * W > 0x7fffffff - 1024:
        return 0
    return B * S * (24 + 8 + 8 + 4) + (B * H * W * 4 + 15) // 16 * 16


def _panoptic_loss_workspace_bytes(B, H, W):
    """cerberus_panoptic_loss_workspace_bytes in pure Python: an fp32 partial of sum f, sum m f and sum m per 1024 elements of
    the centre term (B*H*W elements) and of the offset term (2*B*H*W)."""
    if B <= 0 or H <= 0 or W <= 0 or 2 * B * H * W > 0x7fffffff - 1024:
        return 0
    n = B * H * W
    return 3 * ((n + PANOPTIC_CHUNK_PIXELS - 1) // PANOPTIC_CHUNK_PIXELS + (2 * n + PANOPTIC_CHUNK_PIXELS - 1) // PANOPTIC_CHUNK_PIXELS) * 4


def _panoptic_targets_check(ids, seg_ids, seg_category, seg_flags, seg_count, gauss, sigma, what):
    if ids.dim() != 3 or ids.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("%s: ids must be a (B,H,W) int32 or int64 tensor, got %s %s" % (what, tuple(ids.shape), ids.dtype))
    B, H, W = ids.shape
    if seg_ids.dim() != 2 or seg_ids.shape[0] != B:
        raise RuntimeError("%s: seg_ids must be (B,S) with B = %d, got %s" % (what, B, tuple(seg_ids.shape)))
    S = seg_ids.shape[1]
    size = 6 * int(sigma) + 3
    for name, t, shape, dtype in (("seg_ids", seg_ids, (B, S), torch.int64), ("seg_category", seg_category, (B, S), torch.int64),
                                  ("seg_flags", seg_flags, (B, S), torch.int32), ("seg_count", seg_count, (B,), torch.int64),
                                  ("gauss", gauss, (size, size), torch.float32)):
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise RuntimeError("%s: %s must be %s %s, got %s %s" % (what, name, str(dtype).replace("torch.", ""), shape, t.dtype,
                                                                    tuple(t.shape)))
        if t.device != ids.device:
            raise RuntimeError("%s: inputs on different devices: %s, %s" % (what, ids.device, t.device))
    if sigma < 1:
        raise RuntimeError("%s: sigma must be a positive integer, got %d" % (what, sigma))
    if ids.numel() == 0 or S == 0:
        raise RuntimeError("%s: needs at least one pixel and one table row, got ids %s and S = %d" % (what, tuple(ids.shape), S))
    if S > PANOPTIC_TARGETS_MAX_SEGMENTS:
        raise RuntimeError("%s: at most %d table rows per image, got %d (utilities.panoptic_targets takes the stock-op route "
                           "above it)" % (what, PANOPTIC_TARGETS_MAX_SEGMENTS, S))
    if B > METRIC_MAX_BATCH or H * W > 0x7fffffff - 1024:
        raise RuntimeError("%s: %d images of %d pixels do not fit the kernels' launch grid" % (what, B, H * W))
    return B, H, W, S


def _panoptic_targets_empty(ids, S):
    B, H, W = ids.shape
    new = lambda shape, dtype: ids.new_empty(shape, dtype=dtype)
    return (new((B, H, W), torch.int64), new((B, H, W), torch.int64), new((B, 1, H, W), torch.float32), new((B, 2, H, W), torch.float32),
            new((B, H, W), torch.float32), new((B, H, W), torch.float32), new((B, H, W), torch.float32), new((B, S, 2), torch.float64))


def _panoptic_targets_cuda(ids, seg_ids, seg_category, seg_flags, seg_count, gauss, ignore_label, sigma, ignore_stuff_in_offset,
                           small_instance_area, small_instance_weight, ignore_crowd_in_semantic):
    what = "cerberus::panoptic_targets"
    B, H, W, S = _panoptic_targets_check(ids, seg_ids, seg_category, seg_flags, seg_count, gauss, sigma, what)
    x = ids.contiguous()
    tables = [t.contiguous() for t in (seg_ids, seg_category, seg_flags, seg_count, gauss)]
    outs = _panoptic_targets_empty(x, S)            # every element is written by the kernels
    lib = _lib.get()
    ws_bytes = lib.cerberus_panoptic_targets_workspace_bytes(B, H, W, S)
    ws = torch.empty((max(ws_bytes, 16) + 7) // 8, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.cerberus_panoptic_targets(x.data_ptr(), 1 if x.dtype == torch.int64 else 0, *[t.data_ptr() for t in tables],
                                           *[o.data_ptr() for o in outs], ws.data_ptr(), ws_bytes, B, H, W, S, int(sigma),
                                           int(ignore_label), int(bool(ignore_stuff_in_offset)), int(small_instance_area),
                                           ctypes.c_float(small_instance_weight), int(bool(ignore_crowd_in_semantic)), _stream_ptr(x))
    _lib.check(rc, what)
    return outs


def _panoptic_targets_meta(ids, seg_ids, seg_category, seg_flags, seg_count, gauss, ignore_label, sigma, ignore_stuff_in_offset,
                           small_instance_area, small_instance_weight, ignore_crowd_in_semantic):
    return _panoptic_targets_empty(ids, seg_ids.shape[1])


def _panoptic_loss_check(center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask, mode, what):
    if center_pred.dim() != 4 or center_pred.shape[1] != 1:
        raise RuntimeError("%s: center_pred must be a 4-D (B,1,H,W) tensor, got %s" % (what, tuple(center_pred.shape)))
    B, _, H, W = center_pred.shape
    for name, t, shape in (("center_pred", center_pred, (B, 1, H, W)), ("center_tgt", center_tgt, (B, 1, H, W)),
                           ("center_mask", center_mask, (B, H, W)), ("offset_pred", offset_pred, (B, 2, H, W)),
                           ("offset_tgt", offset_tgt, (B, 2, H, W)), ("offset_mask", offset_mask, (B, H, W))):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise RuntimeError("%s: %s must be float32, got %s (16-bit and 64-bit tensors take the stock-op chain of "
                               "loss_functions.deeplab_panoptic_loss)" % (what, name, t.dtype))
        if t.device != center_pred.device:
            raise RuntimeError("%s: inputs on different devices: %s, %s" % (what, center_pred.device, t.device))
        if tuple(t.shape) != shape:
            raise RuntimeError("%s: %s must be %s, got %s" % (what, name, shape, tuple(t.shape)))
    if mode not in (0, 1):
        raise RuntimeError("%s: mode must be 0 (reference) or 1 (pixel), got %d" % (what, mode))
    if center_pred.numel() == 0:
        raise RuntimeError("%s: needs at least one pixel, got %s" % (what, tuple(center_pred.shape)))
    if 2 * B * H * W > 0x7fffffff - 1024:
        raise RuntimeError("%s: %d elements do not fit the kernels' 32-bit element index" % (what, 2 * B * H * W))
    return B, H, W


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _panoptic_loss_cuda(center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask, center_weight, offset_weight, mode):
    what = "cerberus::panoptic_loss"
    B, H, W = _panoptic_loss_check(center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask, mode, what)
    ts = [t.contiguous() if t is not None else None for t in (center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask)]
    dev = ts[0].device
    lib = _lib.get()
    ws_bytes = lib.cerberus_panoptic_loss_workspace_bytes(B, H, W)
    ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    state = torch.empty((2,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.cerberus_panoptic_loss_forward(*[_ptr(t) for t in ts], loss.data_ptr(), state.data_ptr(), ws.data_ptr(), ws_bytes, B, H, W,
                                                ctypes.c_float(center_weight), ctypes.c_float(offset_weight), int(mode), 0,
                                                _stream_ptr(ts[0]))
    _lib.check(rc, what)
    return loss, state


def _panoptic_loss_meta(center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask, center_weight, offset_weight, mode):
    return center_pred.new_empty((), dtype=torch.float32), center_pred.new_empty((2,), dtype=torch.float32)


def _panoptic_loss_backward_cuda(center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask, state, grad_loss, mode):
    what = "cerberus::panoptic_loss_backward"
    B, H, W = _panoptic_loss_check(center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask, mode, what)
    if state.dtype != torch.float32 or state.device != center_pred.device or tuple(state.shape) != (2,):
        raise RuntimeError("%s: state must be the float32 (2,) tensor of the forward, got %s %s" % (what, state.dtype,
                                                                                                   tuple(state.shape)))
    ts = [t.contiguous() if t is not None else None for t in (center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask)]
    gl = _grad_scalar(grad_loss, ts[0], what)
    st = state.contiguous()
    gc, go = _fresh_like(ts[0]), _fresh_like(ts[3])       # every element is written by the kernel
    with torch.cuda.device(ts[0].device):
        rc = _lib.get().cerberus_panoptic_loss_backward(*[_ptr(t) for t in ts], st.data_ptr(), gl.data_ptr(),
                                                        gc.data_ptr(), go.data_ptr(), B, H, W, int(mode), 0, _stream_ptr(ts[0]))
    _lib.check(rc, what)
    return gc, go


def _panoptic_loss_backward_meta(center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask, state, grad_loss, mode):
    return _fresh_like(center_pred), _fresh_like(offset_pred)


def _no_cpu(name):
    def _raise(*_a, **_k):
        raise RuntimeError("cerberus::%s has no CPU implementation: this build is the "
                           "MI355X HIP path only (move the tensors to the GPU)" % name)
    return _raise


_def.impl("correlation", _correlation_cuda, "CUDA")
_def.impl("correlation", _correlation_meta, "Meta")
_def.impl("correlation", _no_cpu("correlation"), "CPU")
_def.impl("correlation_leaky", _correlation_leaky_cuda, "CUDA")
_def.impl("correlation_leaky", _correlation_meta, "Meta")
_def.impl("correlation_leaky", _no_cpu("correlation_leaky"), "CPU")
_def.impl("warp_correlation_leaky", _warp_correlation_leaky_cuda, "CUDA")
_def.impl("warp_correlation_leaky", lambda a, b, f, p, sl: a.new_empty((a.shape[0], 81, a.shape[2], a.shape[3])), "Meta")
_def.impl("warp_correlation_leaky", _no_cpu("warp_correlation_leaky"), "CPU")
_def.impl("correlation_leaky_into", _correlation_leaky_into_cuda, "CUDA")
_def.impl("correlation_leaky_into", lambda *a: None, "Meta")
_def.impl("correlation_leaky_into", _no_cpu("correlation_leaky_into"), "CPU")
_def.impl("photometric_loss", _photometric_loss_cuda, "CUDA")
_def.impl("photometric_loss", lambda a, b, l1, ss: a.new_empty((), dtype=torch.float32), "Meta")
_def.impl("photometric_loss", _no_cpu("photometric_loss"), "CPU")
_def.impl("photometric_loss_backward", _photometric_loss_backward_cuda, "CUDA")
_def.impl("photometric_loss_backward", _photometric_loss_backward_meta, "Meta")
_def.impl("photometric_loss_backward", _no_cpu("photometric_loss_backward"), "CPU")
_def.impl("census_loss", _census_loss_cuda, "CUDA")
_def.impl("census_loss", lambda a, b, d: a.new_empty((), dtype=torch.float32), "Meta")
_def.impl("census_loss", _no_cpu("census_loss"), "CPU")
_def.impl("census_loss_backward", _census_loss_backward_cuda, "CUDA")
_def.impl("census_loss_backward", _census_loss_backward_meta, "Meta")
_def.impl("census_loss_backward", _no_cpu("census_loss_backward"), "CPU")
_def.impl("corresponding_map", _corresponding_map_cuda, "CUDA")
_def.impl("corresponding_map", _occlusion_meta, "Meta")
_def.impl("corresponding_map", _no_cpu("corresponding_map"), "CPU")
_def.impl("occlusion_mask_bidirection", _occlusion_mask_bidirection_cuda, "CUDA")
_def.impl("occlusion_mask_bidirection", _occlusion_meta, "Meta")
_def.impl("occlusion_mask_bidirection", _no_cpu("occlusion_mask_bidirection"), "CPU")
_def.impl("reproject_warp", _reproject_warp_cuda, "CUDA")
_def.impl("reproject_warp", lambda image, depth, k, p, eps: image.new_empty(image.shape), "Meta")
_def.impl("reproject_warp", _no_cpu("reproject_warp"), "CPU")
_def.impl("reproject_warp_backward", _reproject_warp_backward_cuda, "CUDA")
_def.impl("reproject_warp_backward", lambda image, depth, k, p, g, eps: depth.new_empty(depth.shape), "Meta")
_def.impl("reproject_warp_backward", _no_cpu("reproject_warp_backward"), "CPU")
_def.impl("seg_cross_entropy", _seg_cross_entropy_cuda, "CUDA")
_def.impl("seg_cross_entropy", _seg_cross_entropy_meta, "Meta")
_def.impl("seg_cross_entropy", _no_cpu("seg_cross_entropy"), "CPU")
_def.impl("seg_cross_entropy_backward", _seg_cross_entropy_backward_cuda, "CUDA")
_def.impl("seg_cross_entropy_backward", lambda x, t, w, lse, st, g, i: _fresh_like(x), "Meta")
_def.impl("seg_cross_entropy_backward", _no_cpu("seg_cross_entropy_backward"), "CPU")
_def.impl("rmi_moments", _rmi_moments_cuda, "CUDA")
_def.impl("rmi_moments", _rmi_moments_meta, "Meta")
_def.impl("rmi_moments", _no_cpu("rmi_moments"), "CPU")
_def.impl("rmi_moments_backward", _rmi_moments_backward_cuda, "CUDA")
_def.impl("rmi_moments_backward", lambda x, *a: _fresh_like(x), "Meta")
_def.impl("rmi_moments_backward", _no_cpu("rmi_moments_backward"), "CPU")
_def.impl("seg_ohem_cross_entropy", _seg_ohem_cuda, "CUDA")
_def.impl("seg_ohem_cross_entropy", _seg_ohem_meta, "Meta")
_def.impl("seg_ohem_cross_entropy", _no_cpu("seg_ohem_cross_entropy"), "CPU")
_def.impl("seg_ohem_cross_entropy_backward", _seg_ohem_backward_cuda, "CUDA")
_def.impl("seg_ohem_cross_entropy_backward", lambda x, t, w, p, lse, st, g, i: _fresh_like(x), "Meta")
_def.impl("seg_ohem_cross_entropy_backward", _no_cpu("seg_ohem_cross_entropy_backward"), "CPU")
_def.impl("class_histogram", _class_histogram_cuda, "CUDA")
_def.impl("class_histogram", lambda t, c, i: t.new_empty((c,), dtype=torch.int64), "Meta")
_def.impl("class_histogram", _no_cpu("class_histogram"), "CPU")
_def.impl("edge_smoothness", _edge_smoothness_cuda, "CUDA")
_def.impl("edge_smoothness", lambda f, i, al, d: f.new_empty((), dtype=torch.float32), "Meta")
_def.impl("edge_smoothness", _no_cpu("edge_smoothness"), "CPU")
_def.impl("inv_huber", _inv_huber_cuda, "CUDA")
_def.impl("inv_huber", _inv_huber_meta, "Meta")
_def.impl("inv_huber", _no_cpu("inv_huber"), "CPU")
_def.impl("inv_huber_backward", _inv_huber_backward_cuda, "CUDA")
_def.impl("inv_huber_backward", lambda p, g, st, gl: _fresh_like(p), "Meta")
_def.impl("inv_huber_backward", _no_cpu("inv_huber_backward"), "CPU")
_def.impl("seg_confusion", _seg_confusion_cuda, "CUDA")
_def.impl("seg_confusion", _seg_confusion_meta, "Meta")
_def.impl("seg_confusion", _no_cpu("seg_confusion"), "CPU")
_def.impl("depth_metric_sums", _depth_metric_sums_cuda, "CUDA")
_def.impl("depth_metric_sums", _depth_metric_sums_meta, "Meta")
_def.impl("depth_metric_sums", _no_cpu("depth_metric_sums"), "CPU")
_def.impl("flow_metric_sums", _flow_metric_sums_cuda, "CUDA")
_def.impl("flow_metric_sums", _flow_metric_sums_meta, "Meta")
_def.impl("flow_metric_sums", _no_cpu("flow_metric_sums"), "CPU")
_def.impl("warp_sad", _warp_sad_cuda, "CUDA")
_def.impl("warp_sad", lambda im, src, fl: im.new_empty((im.shape[0],), dtype=torch.float64), "Meta")
_def.impl("warp_sad", _no_cpu("warp_sad"), "CPU")
_def.impl("center_peaks", _center_peaks_cuda, "CUDA")
_def.impl("center_peaks", lambda h, t, k: _fresh_like(h), "Meta")
_def.impl("center_peaks", _no_cpu("center_peaks"), "CPU")
_def.impl("group_pixels", _group_pixels_cuda, "CUDA")
_def.impl("group_pixels", _group_pixels_meta, "Meta")
_def.impl("group_pixels", _no_cpu("group_pixels"), "CPU")
_def.impl("instance_overlap", _instance_overlap_cuda, "CUDA")
_def.impl("instance_overlap", _instance_overlap_meta, "Meta")
_def.impl("instance_overlap", _no_cpu("instance_overlap"), "CPU")
_def.impl("panoptic_targets", _panoptic_targets_cuda, "CUDA")
_def.impl("panoptic_targets", _panoptic_targets_meta, "Meta")
_def.impl("panoptic_targets", _no_cpu("panoptic_targets"), "CPU")
_def.impl("panoptic_loss", _panoptic_loss_cuda, "CUDA")
_def.impl("panoptic_loss", _panoptic_loss_meta, "Meta")
_def.impl("panoptic_loss", _no_cpu("panoptic_loss"), "CPU")
_def.impl("panoptic_loss_backward", _panoptic_loss_backward_cuda, "CUDA")
_def.impl("panoptic_loss_backward", _panoptic_loss_backward_meta, "Meta")
_def.impl("panoptic_loss_backward", _no_cpu("panoptic_loss_backward"), "CPU")
_def.impl("edge_smoothness_backward", _edge_smoothness_backward_cuda, "CUDA")
_def.impl("edge_smoothness_backward", lambda f, i, g, al, d: _fresh_like(f), "Meta")
_def.impl("edge_smoothness_backward", _no_cpu("edge_smoothness_backward"), "CPU")
_def.impl("correlation_backward", _correlation_backward_cuda, "CUDA")
_def.impl("correlation_backward", _correlation_backward_meta, "Meta")
_def.impl("correlation_backward", _no_cpu("correlation_backward"), "CPU")
_def.impl("correlation_backward_leaky", _correlation_backward_leaky_cuda, "CUDA")
_def.impl("correlation_backward_leaky", _correlation_backward_meta, "Meta")
_def.impl("correlation_backward_leaky", _no_cpu("correlation_backward_leaky"), "CPU")
_def.impl("area_pyramid", _area_pyramid_cuda, "CUDA")
_def.impl("area_pyramid", _area_pyramid_meta, "Meta")
_def.impl("area_pyramid", _no_cpu("area_pyramid"), "CPU")
_def.impl("flow_upsample", _flow_upsample_cuda, "CUDA")
_def.impl("flow_upsample", lambda f, k: f.new_empty((f.shape[0], f.shape[1], f.shape[2] * k, f.shape[3] * k)), "Meta")
_def.impl("flow_upsample", _no_cpu("flow_upsample"), "CPU")
_def.impl("flow_upsample_backward", _flow_upsample_backward_cuda, "CUDA")
_def.impl("flow_upsample_backward",
          lambda g, k: g.new_empty((g.shape[0], g.shape[1], g.shape[2] // k, g.shape[3] // k)), "Meta")
_def.impl("flow_upsample_backward", _no_cpu("flow_upsample_backward"), "CPU")
_def.impl("area_resize", _area_resize_cuda, "CUDA")
_def.impl("area_resize", lambda x, h, w: x.new_empty((x.shape[0], x.shape[1], h, w)), "Meta")
_def.impl("area_resize", _no_cpu("area_resize"), "CPU")
_def.impl("flow_warp", _flow_warp_cuda, "CUDA")
_def.impl("flow_warp", lambda image, flow, p, m: _fresh_like(image), "Meta")
_def.impl("flow_warp", _no_cpu("flow_warp"), "CPU")
_def.impl("flow_warp_backward", _flow_warp_backward_cuda, "CUDA")
_def.impl("flow_warp_backward", lambda image, flow, go, p, m, ni, nf: _flow_warp_backward_meta(image, flow, ni, nf), "Meta")
_def.impl("flow_warp_backward", _no_cpu("flow_warp_backward"), "CPU")
_def.impl("flow_warp_ctx", _flow_warp_ctx_cuda, "CUDA")
_def.impl("flow_warp_ctx", _flow_warp_ctx_meta, "Meta")
_def.impl("flow_warp_ctx", _no_cpu("flow_warp_ctx"), "CPU")
_def.impl("flow_warp_backward_ctx", _flow_warp_backward_ctx_cuda, "CUDA")
_def.impl("flow_warp_backward_ctx", lambda image, flow, ctx, go, p, m, ni, nf: _flow_warp_backward_meta(image, flow, ni, nf), "Meta")
_def.impl("flow_warp_backward_ctx", _no_cpu("flow_warp_backward_ctx"), "CPU")


# ----------------------------------------------------------------------------
# autograd formulas for the raw ops.  The reference registers none (its raw op
# is only differentiable through CorrelationFunction); having them makes the
# eval-mode path of Correlation.forward (correlation.py:78-80) differentiable
# too and costs nothing.
# ----------------------------------------------------------------------------
def _corr_setup(ctx, inputs, output):
    input1, input2, *params = inputs
    ctx.save_for_backward(input1, input2)
    ctx.params = tuple(params[:6])


def _corr_backward(ctx, grad):
    input1, input2 = ctx.saved_tensors
    g1, g2 = torch.ops.cerberus.correlation_backward(input1, input2, grad, *ctx.params)
    return (g1, g2) + (None,) * 6


def _corr_leaky_setup(ctx, inputs, output):
    input1, input2, *params = inputs
    ctx.save_for_backward(input1, input2, output)
    ctx.params = tuple(params[:6])
    ctx.slope = params[6]


def _corr_leaky_backward(ctx, grad):
    input1, input2, output = ctx.saved_tensors
    # d leaky(v)/dv from the sign of the output (slope > 0 keeps the sign), applied by the library in one pass
    g1, g2 = torch.ops.cerberus.correlation_backward_leaky(input1, input2, grad, output, 0, *ctx.params, ctx.slope)
    return (g1, g2) + (None,) * 7


def _warp_setup(ctx, inputs, output):
    image, flow, pad_mode, interp_mode = inputs
    ctx.save_for_backward(image, flow)
    ctx.modes = (pad_mode, interp_mode)


def _warp_backward(ctx, grad):
    image, flow = ctx.saved_tensors
    need_image, need_flow = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    gi, gf = torch.ops.cerberus.flow_warp_backward(image, flow, grad, ctx.modes[0],
                                                   ctx.modes[1], need_image, need_flow)
    return (gi if need_image else None, gf.to(flow.dtype) if need_flow else None, None, None)


def _warp_corr_setup(ctx, inputs, output):
    input1, input2, flow, pad_mode, slope = inputs
    # f2's point in training: neither the warped features nor the warp's context are kept -- only the three inputs and the
    # (81-channel) result, whose sign carries the LeakyReLU derivative
    ctx.save_for_backward(input1, input2, flow, output)
    ctx.pad_mode, ctx.slope = pad_mode, slope


def _warp_corr_backward(ctx, grad):
    input1, input2, flow, output = ctx.saved_tensors
    bil = INTERP_MODES["bilinear"]
    # recompute the warp (the tuned kernels, with its context), then the tuned correlation and warp backward
    warped, context = torch.ops.cerberus.flow_warp_ctx(input2, flow, ctx.pad_mode, bil)
    g1, gw = torch.ops.cerberus.correlation_backward_leaky(input1, warped, grad, output, 0, 4, 1, 4, 1, 1, 1, ctx.slope)
    need_image, need_flow = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
    g2 = gf = None
    if need_image or need_flow:
        gi, gfl = torch.ops.cerberus.flow_warp_backward_ctx(input2, flow, context, gw, ctx.pad_mode, bil, need_image, need_flow)
        g2 = gi if need_image else None
        gf = gfl.to(flow.dtype) if need_flow else None
    return g1, g2, gf, None, None


torch.library.register_autograd("cerberus::warp_correlation_leaky", _warp_corr_backward, setup_context=_warp_corr_setup)
torch.library.register_autograd("cerberus::correlation", _corr_backward,
                                setup_context=_corr_setup)
torch.library.register_autograd("cerberus::correlation_leaky", _corr_leaky_backward,
                                setup_context=_corr_leaky_setup)
def _warp_ctx_setup(ctx, inputs, output):
    image, flow, pad_mode, interp_mode = inputs
    ctx.save_for_backward(image, flow, output[1])
    ctx.modes = (pad_mode, interp_mode)
    ctx.mark_non_differentiable(output[1])


def _warp_ctx_backward(ctx, grad, _grad_context):
    image, flow, context = ctx.saved_tensors
    need_image, need_flow = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    gi, gf = torch.ops.cerberus.flow_warp_backward_ctx(image, flow, context, grad,
                                                       ctx.modes[0], ctx.modes[1],
                                                       need_image, need_flow)
    return (gi if need_image else None, gf.to(flow.dtype) if need_flow else None, None, None)


def _upsample_setup(ctx, inputs, output):
    ctx.factor = inputs[1]


def _upsample_backward(ctx, grad):
    return torch.ops.cerberus.flow_upsample_backward(grad, ctx.factor), None


def _upsample_bwd_setup(ctx, inputs, output):
    ctx.factor = inputs[1]


def _upsample_bwd_backward(ctx, grad):
    # the adjoint of the adjoint is the forward (the op is linear)
    return torch.ops.cerberus.flow_upsample(grad, ctx.factor), None


def _area_resize_backward(ctx, grad):
    raise RuntimeError("cerberus::area_resize is not differentiable: the reference resizes the "
                       "TARGET images with it (UnFlowLoss.py:279-280), which carry no gradient")


torch.library.register_autograd("cerberus::area_resize", _area_resize_backward,
                                setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::area_pyramid", _area_resize_backward,
                                setup_context=lambda ctx, inputs, output: None)
def _occlusion_backward(ctx, grad):
    raise RuntimeError("the cerberus:: occlusion ops are not differentiable: a mask is a constant of the loss (the reference "
                       "builds it with a comparison, UnFlowLoss.py:105, :116); for a map that is differentiable through "
                       "its weights call loss_functions.get_corresponding_map on a tensor that requires grad")


torch.library.register_autograd("cerberus::corresponding_map", _occlusion_backward,
                                setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::occlusion_mask_bidirection", _occlusion_backward,
                                setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::flow_upsample", _upsample_backward,
                                setup_context=_upsample_setup)
torch.library.register_autograd("cerberus::flow_upsample_backward", _upsample_bwd_backward,
                                setup_context=_upsample_bwd_setup)
torch.library.register_autograd("cerberus::flow_warp", _warp_backward,
                                setup_context=_warp_setup)
torch.library.register_autograd("cerberus::flow_warp_ctx", _warp_ctx_backward,
                                setup_context=_warp_ctx_setup)


def _photometric_setup(ctx, inputs, output):
    im_orig, im_recons, l1_weight, ssim_weight = inputs
    ctx.save_for_backward(im_orig, im_recons)       # nothing but the inputs: the backward recomputes
    ctx.weights = (l1_weight, ssim_weight)


def _photometric_backward(ctx, grad):
    im_orig, im_recons = ctx.saved_tensors
    need_orig, need_recons = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    go, gr = torch.ops.cerberus.photometric_loss_backward(im_orig, im_recons, grad, ctx.weights[0], ctx.weights[1],
                                                          need_orig, need_recons)
    return (go if need_orig else None, gr if need_recons else None, None, None)


def _census_setup(ctx, inputs, output):
    im, im_warp, max_distance = inputs
    ctx.save_for_backward(im, im_warp)              # nothing but the inputs: the backward recomputes
    ctx.max_distance = max_distance


def _census_backward(ctx, grad):
    im, im_warp = ctx.saved_tensors
    need_im, need_warp = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    gi, gw = torch.ops.cerberus.census_loss_backward(im, im_warp, grad, ctx.max_distance, need_im, need_warp)
    return (gi if need_im else None, gw if need_warp else None, None)


def _smoothness_setup(ctx, inputs, output):
    flow, image, alpha, degree = inputs
    ctx.save_for_backward(flow, image)
    ctx.params = (alpha, degree)


def _smoothness_backward(ctx, grad):
    flow, image = ctx.saved_tensors
    if ctx.needs_input_grad[1]:
        raise RuntimeError("cerberus::edge_smoothness has no gradient for its image (a target image in unFlowLoss): "
                           "loss_functions.edge_smoothness takes the stock-op path for an image that requires grad")
    gf = torch.ops.cerberus.edge_smoothness_backward(flow, image, grad, *ctx.params) if ctx.needs_input_grad[0] else None
    return gf, None, None, None


def _reproject_setup(ctx, inputs, output):
    image, depth, inv_K, proj, eps = inputs
    ctx.save_for_backward(image, depth, inv_K, proj)      # nothing but the inputs: the backward recomputes the positions
    ctx.eps = eps


def _reproject_backward(ctx, grad):
    image, depth, inv_K, proj = ctx.saved_tensors
    if ctx.needs_input_grad[0] or ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
        raise RuntimeError("cerberus::reproject_warp has a gradient for the depth only (the image is a target, the camera "
                           "matrices are data): loss_functions.reproject_warp takes the stock-op path for an image or a "
                           "matrix that requires grad")
    gd = torch.ops.cerberus.reproject_warp_backward(image, depth, inv_K, proj, grad, ctx.eps) if ctx.needs_input_grad[1] else None
    return None, gd, None, None, None


def _seg_setup(ctx, inputs, output):
    logits, target, weight, ignore_index, _gamma = inputs
    loss, lse, state = output
    # the logits, and what the forward left for the backward: lse (4 B per pixel against 4 C) and the scalars on the device
    ctx.save_for_backward(logits, target, weight, lse, state)
    ctx.ignore_index = ignore_index
    ctx.mark_non_differentiable(lse, state)


def _seg_backward(ctx, grad_loss, _grad_lse, _grad_state):
    logits, target, weight, lse, state = ctx.saved_tensors
    if ctx.needs_input_grad[2]:
        raise RuntimeError("cerberus::seg_cross_entropy has no gradient for its class weights: "
                           "loss_functions.seg_cross_entropy takes the stock-op path for a weight that requires grad")
    gx = None
    if ctx.needs_input_grad[0]:
        gx = torch.ops.cerberus.seg_cross_entropy_backward(logits, target, weight, lse, state, grad_loss, ctx.ignore_index)
    return gx, None, None, None, None


def _seg_ohem_setup(ctx, inputs, output):
    logits, target, weight, ignore_index, _thresh, _min_kept = inputs
    _loss, prob, lse, state, counts = output
    # the logits, and what the forward left: prob and lse (8 B per pixel against 4 C), the threshold and 1 / den on the device
    ctx.save_for_backward(logits, target, weight, prob, lse, state)
    ctx.ignore_index = ignore_index
    ctx.mark_non_differentiable(prob, lse, state, counts)


def _seg_ohem_backward(ctx, grad_loss, *_grads):
    logits, target, weight, prob, lse, state = ctx.saved_tensors
    if ctx.needs_input_grad[2]:
        raise RuntimeError("cerberus::seg_ohem_cross_entropy has no gradient for its class weights: "
                           "loss_functions.seg_ohem_cross_entropy takes the stock-op path for a weight that requires grad")
    gx = None
    if ctx.needs_input_grad[0]:
        gx = torch.ops.cerberus.seg_ohem_cross_entropy_backward(logits, target, weight, prob, lse, state, grad_loss, ctx.ignore_index)
    return gx, None, None, None, None, None


def _rmi_setup(ctx, inputs, output):
    logits, target, radius, pool, do_rmi = inputs
    _bce, la_cov, _pr_cov, _la_pr_cov, la_map, pr_map, means, state = output
    # the logits, and what the forward left: two pooled maps (1 / pool^2 of the logits each), 18 means per (n, c), the scalars
    ctx.save_for_backward(logits, target, la_map, pr_map, means, state)
    ctx.radius, ctx.pool, ctx.do_rmi = radius, pool, do_rmi
    ctx.mark_non_differentiable(la_cov, la_map, pr_map, means, state)      # la_cov depends on the labels only


def _rmi_backward(ctx, grad_bce, _g_la_cov, grad_pr_cov, grad_la_pr_cov, *_rest):
    logits, target, la_map, pr_map, means, state = ctx.saved_tensors
    if not ctx.needs_input_grad[0]:
        return None, None, None, None, None
    if grad_bce is None:
        grad_bce = torch.zeros((), dtype=torch.float32, device=logits.device)
    if ctx.do_rmi:
        zeros = lambda: torch.zeros(logits.shape[:2] + (9, 9), dtype=torch.float64, device=logits.device)
        grad_pr_cov = zeros() if grad_pr_cov is None else grad_pr_cov
        grad_la_pr_cov = zeros() if grad_la_pr_cov is None else grad_la_pr_cov
    else:
        grad_pr_cov = grad_la_pr_cov = torch.empty((0,), dtype=torch.float64, device=logits.device)
    gx = torch.ops.cerberus.rmi_moments_backward(logits, target, la_map, pr_map, means, state, grad_bce, grad_pr_cov, grad_la_pr_cov,
                                                 ctx.radius, ctx.pool, ctx.do_rmi)
    return gx, None, None, None, None


def _inv_huber_setup(ctx, inputs, output):
    pred, gt = inputs
    _loss, state = output
    # the inputs and the four scalars the forward left on the device: the backward recomputes every pixel's terms
    ctx.save_for_backward(pred, gt, state)
    ctx.mark_non_differentiable(state)


def _inv_huber_backward(ctx, grad_loss, _grad_state):
    pred, gt, state = ctx.saved_tensors
    if ctx.needs_input_grad[1]:
        raise RuntimeError("cerberus::inv_huber has no gradient for the ground truth: loss_functions.inv_huber_loss takes the "
                           "stock-op path for a gt that requires grad")
    gp = torch.ops.cerberus.inv_huber_backward(pred, gt, state, grad_loss) if ctx.needs_input_grad[0] else None
    return gp, None


def _panoptic_loss_setup(ctx, inputs, output):
    center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask, _cw, _ow, mode = inputs
    _loss, state = output
    ctx.mode = mode
    # the inputs and the two scales the forward left on the device: the backward recomputes every element's difference
    ctx.save_for_backward(center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask, state)
    ctx.mark_non_differentiable(state)


def _panoptic_loss_backward(ctx, grad_loss, _grad_state):
    center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask, state = ctx.saved_tensors
    if any(ctx.needs_input_grad[i] for i in (1, 2, 4, 5)):
        raise RuntimeError("cerberus::panoptic_loss has no gradient for a target or a mask: loss_functions.deeplab_panoptic_loss "
                           "takes the stock-op chain for targets that require grad")
    gc = go = None
    if ctx.needs_input_grad[0] or ctx.needs_input_grad[3]:
        gc, go = torch.ops.cerberus.panoptic_loss_backward(center_pred, center_tgt, center_mask, offset_pred, offset_tgt, offset_mask,
                                                           state, grad_loss, ctx.mode)
    return (gc if ctx.needs_input_grad[0] else None, None, None, go if ctx.needs_input_grad[3] else None, None, None, None, None, None)


def _histogram_backward(ctx, grad):
    raise RuntimeError("cerberus::class_histogram is not differentiable: it counts integer labels")


def _metric_backward(name):
    def _raise(ctx, *grads):
        raise RuntimeError("cerberus::%s is not differentiable: it is a training metric (counts and per-image sums for the "
                           "logger), not a loss" % name)
    return _raise


def _no_double_backward(name):
    def _raise(ctx, *grads):
        raise RuntimeError("cerberus::%s is not differentiable (no double backward)" % name)
    return _raise


torch.library.register_autograd("cerberus::photometric_loss", _photometric_backward, setup_context=_photometric_setup)
torch.library.register_autograd("cerberus::edge_smoothness", _smoothness_backward, setup_context=_smoothness_setup)
torch.library.register_autograd("cerberus::census_loss", _census_backward, setup_context=_census_setup)
torch.library.register_autograd("cerberus::reproject_warp", _reproject_backward, setup_context=_reproject_setup)
torch.library.register_autograd("cerberus::reproject_warp_backward", _no_double_backward("reproject_warp_backward"),
                                setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::census_loss_backward", _no_double_backward("census_loss_backward"),
                                setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::photometric_loss_backward", _no_double_backward("photometric_loss_backward"),
                                setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::edge_smoothness_backward", _no_double_backward("edge_smoothness_backward"),
                                setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::seg_cross_entropy", _seg_backward, setup_context=_seg_setup)
torch.library.register_autograd("cerberus::seg_cross_entropy_backward", _no_double_backward("seg_cross_entropy_backward"),
                                setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::seg_ohem_cross_entropy", _seg_ohem_backward, setup_context=_seg_ohem_setup)
torch.library.register_autograd("cerberus::seg_ohem_cross_entropy_backward", _no_double_backward("seg_ohem_cross_entropy_backward"),
                                setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::rmi_moments", _rmi_backward, setup_context=_rmi_setup)
torch.library.register_autograd("cerberus::rmi_moments_backward", _no_double_backward("rmi_moments_backward"),
                                setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::class_histogram", _histogram_backward, setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::inv_huber", _inv_huber_backward, setup_context=_inv_huber_setup)
torch.library.register_autograd("cerberus::inv_huber_backward", _no_double_backward("inv_huber_backward"),
                                setup_context=lambda ctx, inputs, output: None)
for _name in ("seg_confusion", "depth_metric_sums", "flow_metric_sums", "warp_sad", "center_peaks", "group_pixels", "instance_overlap"):
    torch.library.register_autograd("cerberus::" + _name, _metric_backward(_name), setup_context=lambda ctx, inputs, output: None)
torch.library.register_autograd("cerberus::panoptic_loss", _panoptic_loss_backward, setup_context=_panoptic_loss_setup)
torch.library.register_autograd("cerberus::panoptic_loss_backward", _no_double_backward("panoptic_loss_backward"),
                                setup_context=lambda ctx, inputs, output: None)


def _targets_backward(ctx, *grads):
    raise RuntimeError("cerberus::panoptic_targets is not differentiable: it makes training targets from integer labels")


torch.library.register_autograd("cerberus::panoptic_targets", _targets_backward, setup_context=lambda ctx, inputs, output: None)
