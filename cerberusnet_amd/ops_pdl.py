"""torch.ops.cerberus_pdl.* -- the Panoptic-DeepLab decoder head's own step (nnet_models/deeplab_panoptic.py) bound to
csrc/pdl_head.hip through the C ABI (include/cerberus_hip.h): the depthwise 5x5 convolution (stride 1, padding 2, no bias), alone
or over ``cat(interpolate(low, skip.shape[2:], bilinear, align_corners=True), skip)`` without writing that tensor.

    dwconv5x5(x, weight) -> y
    dwconv5x5_backward(grad_y, x, weight, mask[2]) -> (grad_x, grad_weight)
    upcat_dwconv5x5(low, skip, weight) -> y (B,Ca+Cb,H,W)
    upcat_dwconv5x5_backward(grad_y, low, skip, weight, mask[3]) -> (grad_low, grad_skip, grad_weight)

``mask`` says which gradients are wanted: the launches of the others are skipped, and a gradient that was not asked for comes back
as an empty (0,) tensor.  A gradient that is asked for has the same bits whatever else the mask asks for.

The ops live in a library namespace of their own, ``cerberus_pdl`` (tests/pdl_op_cases.py is their table), under the contract of
DESIGN.md 3.23: inputs of any strides, named ``.contiguous()`` copies kept alive until the launch, outputs fresh with the default
strides, fake == real.  The raw ops carry no autograd formula; the differentiable entry points are the two ``autograd.Function``
wrappers at the end, ``dwconv5x5(x, weight)`` and ``upcat_dwconv5x5(low, skip, weight)`` (once differentiable).

fp32 CUDA tensors only: everything else is the caller's to route to the stock ops (the modules do), and is rejected here.  CPU
tensors are rejected with RuntimeError: there is no CPU path.
"""
import torch
from torch.autograd.function import once_differentiable
from torch.library import Library

from . import _lib
from .ops import _stream_ptr

PDL_TILE_H, PDL_TILE_W = 32, 64       # one workgroup's pixels: one grad_weight partial per (channel, tap, image, tile)
PDL_FOLD = 256                        # partials per round of the finishing fold (loss_reduce.h: kReduceThreads)

_def = Library("cerberus_pdl", "DEF")
_def.define("dwconv5x5(Tensor x, Tensor weight) -> Tensor")
_def.define("dwconv5x5_backward(Tensor grad_y, Tensor x, Tensor weight, bool[2] mask) -> (Tensor grad_x, Tensor grad_weight)")
_def.define("upcat_dwconv5x5(Tensor low, Tensor skip, Tensor weight) -> Tensor")
_def.define("upcat_dwconv5x5_backward(Tensor grad_y, Tensor low, Tensor skip, Tensor weight, bool[3] mask) -> "
            "(Tensor grad_low, Tensor grad_skip, Tensor grad_weight)")

_STOCK = "F.interpolate + torch.cat + F.conv2d(padding=2, groups=C), the backend='torch' route of nnet_models.deeplab_panoptic"


def pdl_fused_ok(*tensors):
    """What the fused route takes: fp32 CUDA tensors outside autocast, nothing empty."""
    return (not torch.is_autocast_enabled()
            and all(t.is_cuda and t.dtype == torch.float32 and t.numel() > 0 for t in tensors))


def _pdl_workspace_bytes(B, Ca, Cb, H, W):
    """cerberus_pdl_workspace_bytes in pure Python (a test holds the two equal): the gradient of the upsampled channels, B Ca H W
    floats padded to 16 bytes, then one float64 partial per (channel, tap, image, tile of 32 x 64 pixels)."""
    if min(B, Cb, H, W) <= 0 or Ca < 0:
        return 0
    tiles = ((H + PDL_TILE_H - 1) // PDL_TILE_H) * ((W + PDL_TILE_W - 1) // PDL_TILE_W)
    lim = 0x7fffffff
    if H * W > lim - 1024 or W > lim - 1024 or B * (Ca + Cb) > lim or (Ca + Cb) * 25 > lim or tiles > 65535 or B * tiles > lim:
        return 0
    return 4 * ((B * Ca * H * W + 3) // 4 * 4) + 8 * (Ca + Cb) * 25 * B * tiles


def _check(what, low, skip, weight, grad_y=None):
    tensors = [("skip" if low is not None else "x", skip), ("weight", weight)]
    if low is not None:
        tensors.insert(0, ("low", low))
    if grad_y is not None:
        tensors.insert(0, ("grad_y", grad_y))
    for name, t in tensors:
        if t.dim() != 4:
            raise RuntimeError("%s: %s must be a 4-D tensor, got %s" % (what, name, tuple(t.shape)))
        if t.dtype != torch.float32:
            raise RuntimeError("%s: %s must be float32, got %s (other types take the stock ops: %s)" % (what, name, t.dtype, _STOCK))
        if t.device != skip.device:
            raise RuntimeError("%s: inputs on different devices: %s, %s" % (what, skip.device, t.device))
    B, Cb, H, W = skip.shape
    Ca = 0
    if low is not None:
        Ca = low.shape[1]
        if low.shape[0] != B or Ca < 1:
            raise RuntimeError("%s: low must be (%d, Ca >= 1, h, w), got %s" % (what, B, tuple(low.shape)))
    if tuple(weight.shape) != (Ca + Cb, 1, 5, 5):
        raise RuntimeError("%s: weight must be %s, got %s" % (what, (Ca + Cb, 1, 5, 5), tuple(weight.shape)))
    if grad_y is not None and tuple(grad_y.shape) != (B, Ca + Cb, H, W):
        raise RuntimeError("%s: grad_y must be %s, got %s" % (what, (B, Ca + Cb, H, W), tuple(grad_y.shape)))
    if skip.numel() == 0 or (low is not None and low.numel() == 0):
        raise RuntimeError("%s: empty input %s" % (what, tuple(skip.shape)))
    return B, Ca, Cb, H, W


def _forward(what, low, skip, weight):
    B, Ca, Cb, H, W = _check(what, low, skip, weight)
    # named: every copy lives until the launch is enqueued
    lo, sk, wt = (None if low is None else low.contiguous()), skip.contiguous(), weight.contiguous()
    out = sk.new_empty((B, Ca + Cb, H, W))
    h, w = (lo.shape[2], lo.shape[3]) if lo is not None else (0, 0)
    with torch.cuda.device(sk.device):
        rc = _lib.get().cerberus_pdl_dwconv_forward(lo.data_ptr() if lo is not None else None, sk.data_ptr(), wt.data_ptr(), out.data_ptr(),
                                                    B, Ca, Cb, h, w, H, W, 0, _stream_ptr(sk))
    _lib.check(rc, what)
    return out


def _backward(what, grad_y, low, skip, weight, need_low, need_skip, need_weight):
    B, Ca, Cb, H, W = _check(what, low, skip, weight, grad_y)
    # named: every copy lives until the launch is enqueued
    gy, lo, sk, wt = grad_y.contiguous(), (None if low is None else low.contiguous()), skip.contiguous(), weight.contiguous()
    grad_low = lo.new_empty(lo.shape if need_low else (0,)) if lo is not None else None
    grad_skip = sk.new_empty(sk.shape if need_skip else (0,))
    grad_weight = wt.new_empty(wt.shape if need_weight else (0,))
    if need_low or need_skip or need_weight:
        nbytes = _lib.get().cerberus_pdl_workspace_bytes(B, Ca, Cb, H, W)
        ws = torch.empty((max(nbytes, 16) + 7) // 8, dtype=torch.float64, device=sk.device)
        h, w = (lo.shape[2], lo.shape[3]) if lo is not None else (0, 0)
        ptr = lambda t, need: t.data_ptr() if need else None
        with torch.cuda.device(sk.device):
            rc = _lib.get().cerberus_pdl_dwconv_backward(gy.data_ptr(), lo.data_ptr() if lo is not None else None, sk.data_ptr(),
                                                         wt.data_ptr(), ptr(grad_low, need_low) if lo is not None else None,
                                                         ptr(grad_skip, need_skip), ptr(grad_weight, need_weight), ws.data_ptr(), nbytes,
                                                         B, Ca, Cb, h, w, H, W, 0, _stream_ptr(sk))
        _lib.check(rc, what)
    return grad_low, grad_skip, grad_weight


def _dwconv5x5_cuda(x, weight):
    return _forward("cerberus_pdl::dwconv5x5", None, x, weight)


def _dwconv5x5_backward_cuda(grad_y, x, weight, mask):
    _, gx, gw = _backward("cerberus_pdl::dwconv5x5_backward", grad_y, None, x, weight, False, bool(mask[0]), bool(mask[1]))
    return gx, gw


def _upcat_cuda(low, skip, weight):
    return _forward("cerberus_pdl::upcat_dwconv5x5", low, skip, weight)


def _upcat_backward_cuda(grad_y, low, skip, weight, mask):
    return _backward("cerberus_pdl::upcat_dwconv5x5_backward", grad_y, low, skip, weight, bool(mask[0]), bool(mask[1]), bool(mask[2]))


def _masked(t, need):
    return t.new_empty(t.shape if need else (0,))


def _no_cpu(name):
    def _raise(*_a, **_k):
        raise RuntimeError("cerberus_pdl::%s has no CPU implementation: this build is the MI355X HIP path only (move the tensors to "
                           "the GPU, or use the modules of nnet_models.deeplab_panoptic, which take the stock ops there)" % name)
    return _raise


_def.impl("dwconv5x5", _dwconv5x5_cuda, "CUDA")
_def.impl("dwconv5x5", lambda x, weight: x.new_empty(x.shape), "Meta")
_def.impl("dwconv5x5_backward", _dwconv5x5_backward_cuda, "CUDA")
_def.impl("dwconv5x5_backward", lambda g, x, weight, mask: (_masked(x, mask[0]), _masked(weight, mask[1])), "Meta")
_def.impl("upcat_dwconv5x5", _upcat_cuda, "CUDA")
_def.impl("upcat_dwconv5x5", lambda low, skip, weight: skip.new_empty((skip.shape[0], low.shape[1] + skip.shape[1]) + tuple(skip.shape[2:])),
          "Meta")
_def.impl("upcat_dwconv5x5_backward", _upcat_backward_cuda, "CUDA")
_def.impl("upcat_dwconv5x5_backward",
          lambda g, low, skip, weight, mask: (_masked(low, mask[0]), _masked(skip, mask[1]), _masked(weight, mask[2])), "Meta")
for _name in ("dwconv5x5", "dwconv5x5_backward", "upcat_dwconv5x5", "upcat_dwconv5x5_backward"):
    _def.impl(_name, _no_cpu(_name), "CPU")


class _DwConv5x5(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return torch.ops.cerberus_pdl.dwconv5x5(x, weight)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        need = list(ctx.needs_input_grad[:2])
        if not any(need):
            return None, None
        gx, gw = torch.ops.cerberus_pdl.dwconv5x5_backward(grad_y, x, weight, need)
        return (gx if need[0] else None, gw if need[1] else None)


class _UpcatDwConv5x5(torch.autograd.Function):
    @staticmethod
    def forward(ctx, low, skip, weight):
        ctx.save_for_backward(low, skip, weight)
        return torch.ops.cerberus_pdl.upcat_dwconv5x5(low, skip, weight)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        low, skip, weight = ctx.saved_tensors
        need = list(ctx.needs_input_grad[:3])
        if not any(need):
            return None, None, None
        grads = torch.ops.cerberus_pdl.upcat_dwconv5x5_backward(grad_y, low, skip, weight, need)
        return tuple(g if n else None for g, n in zip(grads, need))


def dwconv5x5(x, weight):
    """``F.conv2d(x, weight, padding=2, groups=C)`` for ``weight`` (C,1,5,5): the depthwise 5x5 convolution, differentiable once."""
    return _DwConv5x5.apply(x, weight)


def upcat_dwconv5x5(low, skip, weight):
    """The depthwise 5x5 convolution of ``cat(interpolate(low, skip.shape[2:], bilinear, align_corners=True), skip)`` with
    ``weight`` (Ca+Cb,1,5,5), differentiable once; neither the upsampled map nor the concatenation is written."""
    return _UpcatDwConv5x5.apply(low, skip, weight)
