"""The hot-path kernels on misaligned pointers, at every alignment gate (cases: tests/alignment_cases.py).

The correlation and warp kernels choose their routes by per-pointer alignment tests, each over another subset of the
pointers.  Every case forces one route, asserts on the 16-byte-aligned call that ``cerberus_last_kernel`` names it, and then
moves each pointer alone and all of them together off the boundary by every amount an element-aligned pointer can have
(and by a whole 16 bytes, which must change nothing).  Inputs go through ``torch.ops.cerberus``; output and gradient
pointers, which the bindings always allocate aligned, through the C ABI.  Per call:

  (a) the result is finite and within the bound of the op's own test against the same oracle (fp32 1e-5, fp16 2e-3, bf16
      1.6e-2 of the result's maximum), the bands around every written tensor are untouched;
  (b) where the call reports the aligned call's kernel, or one the suite pins as bit-identical to it, the bits are equal;
  (c) where a shifted pointer fails the route's gate the reported kernel changed (the gate fired), otherwise it did not.

flow_warp reports no kernel: (a) always, (b) for the shifts that pass every gate of the forced route."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import alignment_cases as ac
import cerberusnet_amd  # noqa: F401  (registers the ops)
import oracle
from alignment_cases import F32, embed
from cerberusnet_amd import _lib
from cerberusnet_amd.synth import hash_uniform
from conftest import rel_err
from op_cases import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = (4, 1, 4, 1, 1)
CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
SLOPE = 0.1


def dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def f64(t):
    return t.double().cpu().numpy()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def options(opts):
    for k, v in opts.items():
        _lib.set_option(k, v)
    try:
        yield
    finally:
        for k in opts:
            _lib.set_option(k, 0)


def subsets(pointers):
    """Each pointer alone, then all together."""
    return [(p,) for p in pointers] + [tuple(pointers)]


def fired(case, shifted, nbytes):
    return any(ac.misaligned(nbytes, case["gates"][p]) for p in shifted if p in case["gates"])


def check_route(case, name, name0, shifted, nbytes):
    """(c): the gate fired exactly when a shifted pointer fails it."""
    tag = (case["name"], shifted, nbytes, name, name0)
    if not fired(case, shifted, nbytes):
        assert name == name0, tag
    elif case["renames"]:
        assert name != name0, tag
    must_pair = set(shifted) <= set(case["pinned"]) and nbytes in (case["pinned_bytes"] or (nbytes,))
    if must_pair and fired(case, shifted, nbytes):
        assert (name0, name) in ac.PINNED, tag         # the bit comparison below is known to run
    return name == name0 or (name0, name) in ac.PINNED


def check_result(tag, got, ref, bound, base=None):
    """(a) and, with ``base``, (b)."""
    assert bool(torch.isfinite(got).all()), tag
    err = rel_err(f64(got), ref)
    assert err < bound, (tag, err)
    if base is not None:
        assert same_bits(got.contiguous(), base), (tag, float((got.double() - base.double()).abs().max()))


# ---- correlation forward -----------------------------------------------------------------------------------------------------
FWD = ac.per_dtype(ac.CORR_FORWARD)


@pytest.mark.parametrize("case,dtype", FWD, ids=ac.ids(FWD))
def test_correlation_forward(case, dtype):
    B, C, H, W = case["shape"]
    x1, x2 = dev(hash_uniform(case["shape"], 3101), dtype), dev(hash_uniform(case["shape"], 3102), dtype)
    ref = oracle.corr_forward_ref(f64(x1), f64(x2), *P)
    lib, esz, bound = _lib.get(), x1.element_size(), ac.BOUND[dtype]
    with options(case["options"]):
        base = torch.ops.cerberus.correlation(x1, x2, *P, 1)
        name0 = _lib.last_kernel(0)
        assert name0 == case["kernel"], (name0, case["kernel"])
        check_result((case["name"], "aligned"), base, ref, bound)
        for shift in ac.SHIFTS[dtype]:
            for shifted in subsets(("in1", "in2", "out")):
                a = embed(x1, shift) if "in1" in shifted else x1
                b = embed(x2, shift) if "in2" in shifted else x2
                if "out" in shifted:
                    out = embed(torch.empty_like(base), shift, written=True)
                    rc = lib.cerberus_correlation_forward_ex(a.data_ptr(), b.data_ptr(), out.data_ptr(), B, C, H, W, *P,
                                                             ctypes.c_float(1.0), 0, CODE[dtype], stream())
                    torch.cuda.synchronize()
                    assert rc == 0 and ac.bands_untouched(out), (case["name"], shifted, shift, rc)
                else:
                    out = torch.ops.cerberus.correlation(a, b, *P, 1)
                name = _lib.last_kernel(0)
                same = check_route(case, name, name0, shifted, shift * esz)
                check_result((case["name"], shifted, shift, name), out, ref, bound, base if same else None)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
@pytest.mark.parametrize("offset", [0, 5])
def test_correlation_leaky_into_a_shifted_buffer(offset, dtype):
    """The caller-owned concatenation buffer with a shifted BASE (tests/test_corr_gpu.py shifts its batch stride only): the
    volume lands in channels [offset, offset + 81), every other channel and the bands keep the sentinel.  The `out` gate of
    the forward (16 bytes fp32, 8 bytes 16-bit storage) sees the address of channel `offset`."""
    shape = (2, 32, 13, 72) if dtype == torch.float32 else (1, 20, 13, 72)
    B, C, H, W = shape
    case = ac.CORR_FORWARD[0] if dtype == torch.float32 else ac.CORR_FORWARD[6]
    assert case["shape"] == shape
    x1, x2 = dev(hash_uniform(shape, 3111), dtype), dev(hash_uniform(shape, 3112), dtype)
    ref = oracle.corr_forward_ref(f64(x1), f64(x2), *P)
    ref = np.where(ref > 0, ref, ref * SLOPE)
    total, esz = 81 + 9, x1.element_size()
    assert offset * H * W * esz % 16 == 0            # channel `offset` of an aligned buffer is aligned
    plain = torch.full((B, total, H, W), ac.SENTINEL, dtype=dtype, device=DEV)
    torch.ops.cerberus.correlation_leaky_into(plain, x1, x2, offset, *P, 1, SLOPE)
    name0 = _lib.last_kernel(0)
    assert name0 == case["kernel"], name0
    base = plain[:, offset:offset + 81].contiguous()
    check_result(("aligned", offset), base, ref, ac.BOUND[dtype])
    for shift in ac.SHIFTS[dtype]:
        buf = embed(plain, shift, written=True)
        torch.ops.cerberus.correlation_leaky_into(buf, x1, x2, offset, *P, 1, SLOPE)
        name = _lib.last_kernel(0)
        same = check_route(case, name, name0, ("out",), shift * esz)
        check_result((offset, shift, name), buf[:, offset:offset + 81], ref, ac.BOUND[dtype], base if same else None)
        rest = torch.cat([buf[:, :offset], buf[:, offset + 81:]], dim=1)
        assert bool((rest == ac.SENTINEL).all()) and ac.bands_untouched(buf), (offset, shift)


# ---- correlation backward ----------------------------------------------------------------------------------------------------
BWD = ac.per_dtype(ac.CORR_BACKWARD)


@pytest.mark.parametrize("case,dtype", BWD, ids=ac.ids(BWD))
def test_correlation_backward(case, dtype):
    B, C, H, W = case["shape"]
    x1, x2 = dev(hash_uniform(case["shape"], 3121), dtype), dev(hash_uniform(case["shape"], 3122), dtype)
    go = dev(hash_uniform((B, 81, H, W), 3123), dtype)
    refs = oracle.corr_backward_ref(f64(x1), f64(x2), f64(go), *P)
    lib, esz, bound = _lib.get(), x1.element_size(), ac.BOUND[dtype]
    with options(case["options"]):
        base = torch.ops.cerberus.correlation_backward(x1, x2, go, *P, 1)
        name0 = _lib.last_kernel(1)
        assert name0 == case["kernel"], (name0, case["kernel"])
        for k in range(2):
            check_result((case["name"], "aligned", k), base[k], refs[k], bound)
        for shift in ac.SHIFTS[dtype]:
            for shifted in subsets(("in1", "in2", "gout", "gin1", "gin2")):
                a = embed(x1, shift) if "in1" in shifted else x1
                b = embed(x2, shift) if "in2" in shifted else x2
                g = embed(go, shift) if "gout" in shifted else go
                if "gin1" in shifted or "gin2" in shifted:
                    outs = [embed(torch.empty_like(x1), shift if p in shifted else 0, written=True) for p in ("gin1", "gin2")]
                    rc = lib.cerberus_correlation_backward(a.data_ptr(), b.data_ptr(), g.data_ptr(), outs[0].data_ptr(),
                                                           outs[1].data_ptr(), B, C, H, W, *P, 1, CODE[dtype], stream())
                    torch.cuda.synchronize()
                    assert rc == 0 and all(ac.bands_untouched(o) for o in outs), (case["name"], shifted, shift, rc)
                else:
                    outs = torch.ops.cerberus.correlation_backward(a, b, g, *P, 1)
                name = _lib.last_kernel(1)
                same = check_route(case, name, name0, shifted, shift * esz)
                for k in range(2):
                    check_result((case["name"], shifted, shift, name, k), outs[k], refs[k], bound, base[k] if same else None)


def test_correlation_backward_leaky_with_shifted_buffers():
    """`grad_buffer` and `fwd_buffer` are read in place by corr_grad_prep alone (its `vec4` test: 16 bytes on both and on the
    workspace, which the binding allocates); the backward proper sees the workspace.  A shifted buffer therefore changes the
    copy's width and nothing else: the same backward kernel, the same bits."""
    shape, offset, total = (2, 32, 13, 72), 5, 90
    B, C, H, W = shape
    x1, x2 = dev(hash_uniform(shape, 3131)), dev(hash_uniform(shape, 3132))
    fwd = torch.full((B, total, H, W), ac.SENTINEL, device=DEV)
    torch.ops.cerberus.correlation_leaky_into(fwd, x1, x2, offset, *P, 1, SLOPE)
    gbuf = dev(hash_uniform((B, total, H, W), 3133))
    vol, g = f64(fwd[:, offset:offset + 81]), f64(gbuf[:, offset:offset + 81])
    refs = oracle.corr_backward_ref(f64(x1), f64(x2), np.where(vol > 0, g, g * np.float32(SLOPE)), *P)
    with options({"corr_bwd_variant": 4}):
        base = torch.ops.cerberus.correlation_backward_leaky(x1, x2, gbuf, fwd, offset, *P, 1, SLOPE)
        name0 = _lib.last_kernel(1)
        assert name0 == "corr_bwd_d4_dma_8x64", name0
        for k in range(2):
            check_result(("aligned", k), base[k], refs[k], ac.BOUND[F32])
        for shift in ac.SHIFTS[F32]:
            for shifted in subsets(("grad_buffer", "fwd_buffer")):
                gb = embed(gbuf, shift) if "grad_buffer" in shifted else gbuf
                fb = embed(fwd, shift) if "fwd_buffer" in shifted else fwd
                outs = torch.ops.cerberus.correlation_backward_leaky(x1, x2, gb, fb, offset, *P, 1, SLOPE)
                assert _lib.last_kernel(1) == name0, (shifted, shift, _lib.last_kernel(1))
                for k in range(2):
                    check_result((shifted, shift, k), outs[k], refs[k], ac.BOUND[F32], base[k])


# ---- the warp fused into the correlation ---------------------------------------------------------------------------------------
def test_warp_correlation_leaky_forward():
    """warp_corr.hip tests no pointer (scalar loads and stores): every shift gives the aligned call's bits.  (C = 8: one
    launch, no channel slices summed by float atomics.)"""
    shape = (2, 8, 13, 72)
    B, C, H, W = shape
    x1, x2 = dev(hash_uniform(shape, 3141)), dev(hash_uniform(shape, 3142))
    flo = dev(hash_uniform((B, 2, H, W), 3143, -3.0, 3.0))
    w_ref = oracle.flow_warp_ref(x2.cpu(), flo.cpu(), "border").numpy()
    ref = oracle.corr_forward_ref(x1.cpu().numpy(), w_ref, *P)
    ref = np.where(ref > 0, ref, ref * np.float32(SLOPE))
    lib = _lib.get()
    assert lib.cerberus_warp_correlation_workspace_bytes(B, C, H, W) == 0
    base = torch.ops.cerberus.warp_correlation_leaky(x1, x2, flo, 1, SLOPE)
    assert _lib.last_kernel(0) == "warp_corr_fwd_8x32"
    check_result("aligned", base, ref, ac.BOUND[F32])
    for shift in ac.SHIFTS[F32]:
        for shifted in subsets(("in1", "in2", "flow", "out")):
            a = embed(x1, shift) if "in1" in shifted else x1
            b = embed(x2, shift) if "in2" in shifted else x2
            f = embed(flo, shift) if "flow" in shifted else flo
            if "out" in shifted:
                out = embed(torch.empty_like(base), shift, written=True)
                rc = lib.cerberus_warp_correlation_forward(a.data_ptr(), b.data_ptr(), f.data_ptr(), out.data_ptr(), None, 0, B, C, H,
                                                           W, 1, ctypes.c_float(SLOPE), 0, 0, 0, stream())
                torch.cuda.synchronize()
                assert rc == 0 and ac.bands_untouched(out), (shifted, shift, rc)
            else:
                out = torch.ops.cerberus.warp_correlation_leaky(a, b, f, 1, SLOPE)
            check_result((shifted, shift), out, ref, ac.BOUND[F32], base)


def test_warp_correlation_leaky_backward():
    """The fused op's backward recomputes the warp and runs the tuned backward kernels: against the unfused chain's gradients
    within the bound of tests/test_corr_gpu.py (1e-4: the LeakyReLU mask comes from the stored result's sign); a shift of a
    whole 16 bytes gives the aligned call's bits."""
    shape = (2, 32, 24, 64)
    B, C, H, W = shape
    x1, x2 = dev(hash_uniform(shape, 3151)), dev(hash_uniform(shape, 3152))
    flo = dev(hash_uniform((B, 2, H, W), 3153, -3.0, 3.0))
    go = dev(hash_uniform((B, 81, H, W), 3154))

    def grads(a, b, f, g, fused=True):
        a, b, f = (t.detach().requires_grad_(True) for t in (a, b, f))
        if fused:
            out = torch.ops.cerberus.warp_correlation_leaky(a, b, f, 1, SLOPE)
        else:
            out = torch.ops.cerberus.correlation_leaky(a, torch.ops.cerberus.flow_warp(b, f, 1, 0), *P, 1, SLOPE)
        return torch.autograd.grad(out, (a, b, f), g)

    refs = [f64(t) for t in grads(x1, x2, flo, go, fused=False)]
    base = grads(x1, x2, flo, go)
    for k in range(3):
        check_result(("aligned", k), base[k], refs[k], 1e-4)
    for shift in ac.SHIFTS[F32]:
        for shifted in subsets(("in1", "in2", "flow", "gout")):
            a = embed(x1, shift) if "in1" in shifted else x1
            b = embed(x2, shift) if "in2" in shifted else x2
            f = embed(flo, shift) if "flow" in shifted else flo
            g = embed(go, shift) if "gout" in shifted else go
            outs = grads(a, b, f, g)
            for k in range(3):
                check_result((shifted, shift, k), outs[k], refs[k], 1e-4, base[k] if shift * 4 % 16 == 0 else None)


# ---- flow_warp ---------------------------------------------------------------------------------------------------------------
def warp_inputs(case, dtype, seed):
    B, C, H, W = case["shape"]
    fdt = case["flow"] or dtype
    img = dev(hash_uniform(case["shape"], seed), dtype)
    flo = dev(hash_uniform((B, 2, H, W), seed + 1, -6.0, 6.0), fdt)
    go = dev(hash_uniform(case["shape"], seed + 2), dtype)
    return img, flo, go


WFWD = ac.per_dtype(ac.WARP_FORWARD)


@pytest.mark.parametrize("case,dtype", WFWD, ids=ac.ids(WFWD))
def test_flow_warp_forward(case, dtype):
    B, C, H, W = case["shape"]
    img, flo, _ = warp_inputs(case, dtype, 3201)
    ref = oracle.flow_warp_ref(img.float().cpu(), flo.float().cpu(), "border").numpy()
    lib, bound = _lib.get(), ac.BOUND[dtype]
    with options(case["options"]):
        base = torch.ops.cerberus.flow_warp(img, flo, 1, 0)
        check_result((case["name"], "aligned"), base, ref, bound)
        for shift in ac.SHIFTS[dtype]:
            for shifted in subsets(("image", "flow", "out")):
                i = embed(img, shift) if "image" in shifted else img
                f = embed(flo, shift) if "flow" in shifted else flo
                if "out" in shifted:
                    out = embed(torch.empty_like(base), shift, written=True)
                    rc = lib.cerberus_flow_warp_forward_ctx(i.data_ptr(), f.data_ptr(), out.data_ptr(), None, 0, B, C, H, W, 1, 0,
                                                            CODE[dtype], CODE[flo.dtype], stream())
                    torch.cuda.synchronize()
                    assert rc == 0 and ac.bands_untouched(out), (case["name"], shifted, shift, rc)
                else:
                    out = torch.ops.cerberus.flow_warp(i, f, 1, 0)
                nbytes = {"image": shift * img.element_size(), "flow": shift * flo.element_size(), "out": shift * img.element_size()}
                same = not any(ac.misaligned(nbytes[p], case["gates"][p]) for p in shifted if p in case["gates"])
                check_result((case["name"], shifted, shift), out, ref, bound, base if same else None)


WBWD = ac.per_dtype(ac.WARP_BACKWARD)


@pytest.mark.parametrize("case,dtype", WBWD, ids=ac.ids(WBWD))
def test_flow_warp_backward(case, dtype):
    B, C, H, W = case["shape"]
    img, flo, go = warp_inputs(case, dtype, 3211)
    _, rgi, rgf = oracle.flow_warp_grads_ref(img.float().cpu(), flo.float().cpu(), go.float().cpu(), "border")
    refs = (rgi.numpy(), rgf.numpy())
    lib, bound = _lib.get(), ac.BOUND[dtype]
    ws_bytes = lib.cerberus_flow_warp_backward_workspace_bytes(B, C, H, W)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=DEV)
    assert ws.data_ptr() % 16 == 0
    with options(case["options"]):
        base = torch.ops.cerberus.flow_warp_backward(img, flo, go, 1, 0, True, True)
        assert base[0].dtype == dtype and base[1].dtype == flo.dtype
        for k in range(2):
            check_result((case["name"], "aligned", k), base[k], refs[k], bound)
        for shift in ac.SHIFTS[dtype]:
            for shifted in subsets(("image", "flow", "gout", "gimage", "gflow")):
                i = embed(img, shift) if "image" in shifted else img
                f = embed(flo, shift) if "flow" in shifted else flo
                g = embed(go, shift) if "gout" in shifted else go
                if "gimage" in shifted or "gflow" in shifted:
                    outs = [embed(torch.empty_like(img), shift if "gimage" in shifted else 0, written=True),
                            embed(torch.empty_like(flo), shift if "gflow" in shifted else 0, written=True)]
                    rc = lib.cerberus_flow_warp_backward(i.data_ptr(), f.data_ptr(), g.data_ptr(), outs[0].data_ptr(),
                                                         outs[1].data_ptr(), None, 0, ws.data_ptr(), ws_bytes, B, C, H, W, 1, 0,
                                                         CODE[dtype], CODE[flo.dtype], stream())
                    torch.cuda.synchronize()
                    assert rc == 0 and all(ac.bands_untouched(o) for o in outs), (case["name"], shifted, shift, rc)
                else:
                    outs = torch.ops.cerberus.flow_warp_backward(i, f, g, 1, 0, True, True)
                esz = {"image": img.element_size(), "gout": img.element_size(), "gimage": img.element_size(),
                       "flow": flo.element_size(), "gflow": flo.element_size()}
                same = case["deterministic"] and not any(ac.misaligned(shift * esz[p], case["gates"][p])
                                                         for p in shifted if p in case["gates"])
                for k in range(2):
                    check_result((case["name"], shifted, shift, k), outs[k], refs[k], bound, base[k] if same else None)


def test_a_shifted_warp_workspace_counts_as_none():
    """cerberus_flow_warp_backward without a context builds one in the caller's workspace.  A workspace that is not 16-byte
    aligned is no error (include/cerberus_hip.h): like one that is too small (tests/test_warp_gpu.py) it counts as none, the
    call returns CERB_OK and runs the scatter kernel -- grad_image within the bound of the oracle (float atomics: no fixed
    order), grad_flow the per-pixel gathers' bits, i.e. those of the same call with no workspace at all."""
    case = ac.WARP_BACKWARD[0]
    B, C, H, W = case["shape"]
    img, flo, go = warp_inputs(case, F32, 3241)
    _, rgi, rgf = oracle.flow_warp_grads_ref(img.cpu(), flo.cpu(), go.cpu(), "border")
    lib = _lib.get()
    ws_bytes = lib.cerberus_flow_warp_backward_workspace_bytes(B, C, H, W)
    ws = embed(torch.zeros((ws_bytes + 7) // 8, dtype=torch.int64, device=DEV), 1)
    assert ws.data_ptr() % 16 == 8
    res = []
    for ptr, nbytes in ((ws.data_ptr(), ws_bytes), (None, 0)):
        gi, gf = embed(torch.empty_like(img), 0, written=True), embed(torch.empty_like(flo), 0, written=True)
        rc = lib.cerberus_flow_warp_backward(img.data_ptr(), flo.data_ptr(), go.data_ptr(), gi.data_ptr(), gf.data_ptr(), None, 0,
                                             ptr, nbytes, B, C, H, W, 1, 0, 0, 0, stream())
        torch.cuda.synchronize()
        assert rc == 0 and ac.bands_untouched(gi) and ac.bands_untouched(gf)
        check_result(("grad_image", ptr is None), gi, rgi.numpy(), ac.BOUND[F32])
        check_result(("grad_flow", ptr is None), gf, rgf.numpy(), ac.BOUND[F32])
        res.append(gf.clone())
    assert same_bits(res[0], res[1])
    assert bool((ac.bands(ws) == ac.INT_FILL).all()) and bool((ws == 0).all())      # the shifted workspace was not used


def test_a_shifted_warp_context_keeps_being_rejected():
    """The context is read as int4: 16 bytes or CERB_EINVAL, from the binding (a clear message) and from the C ABI."""
    shape = (1, 4, 12, 40)
    img, flo, go = dev(hash_uniform(shape, 3221)), dev(hash_uniform((1, 2, 12, 40), 3222, -2.0, 2.0)), dev(hash_uniform(shape, 3223))
    _, ctx = torch.ops.cerberus.flow_warp_ctx(img, flo, 1, 0)
    shifted = embed(ctx, 1)
    assert shifted.data_ptr() % 16 == 8
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        torch.ops.cerberus.flow_warp_backward_ctx(img, flo, shifted, go, 1, 0, True, True)
    gi, gf = embed(torch.empty_like(img), 0, written=True), embed(torch.empty_like(flo), 0, written=True)
    lib = _lib.get()
    nbytes = lib.cerberus_flow_warp_context_bytes(1, 12, 40)
    rc = lib.cerberus_flow_warp_backward(img.data_ptr(), flo.data_ptr(), go.data_ptr(), gi.data_ptr(), gf.data_ptr(),
                                         shifted.data_ptr(), nbytes, None, 0, 1, 4, 12, 40, 1, 0, 0, 0, stream())
    torch.cuda.synchronize()
    assert rc == -1                                                       # CERB_EINVAL, before any launch
    assert bool((gi == ac.SENTINEL).all()) and bool((gf == ac.SENTINEL).all())
    out = embed(torch.empty_like(img), 0, written=True)
    rc = lib.cerberus_flow_warp_forward_ctx(img.data_ptr(), flo.data_ptr(), out.data_ptr(), shifted.data_ptr(), nbytes, 1, 4, 12, 40,
                                            1, 0, 0, 0, stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == ac.SENTINEL).all())


# ---- flow_upsample -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("factor", [2, 4])
def test_flow_upsample_forward(factor, dtype):
    """upsample_fwd_kernel loads and stores single elements: no gate, the aligned call's bits at every shift.  Bounds and
    reference of tests/test_warp_gpu.py (F.interpolate of the rounded input; fp32 1e-6)."""
    import torch.nn.functional as F
    shape = (2, 2, 9, 20)
    B, C, H, W = shape
    x = dev(hash_uniform(shape, 3231, -8.0, 8.0), dtype)
    ref = F.interpolate(x.float().cpu() * factor, scale_factor=factor, mode="bilinear", align_corners=True).numpy()
    bound = 1e-6 if dtype == torch.float32 else ac.BOUND[dtype]
    base = torch.ops.cerberus.flow_upsample(x, factor)
    check_result("aligned", base, ref, bound)
    lib = _lib.get()
    for shift in ac.SHIFTS[dtype]:
        for shifted in subsets(("src", "dst")):
            s = embed(x, shift) if "src" in shifted else x
            if "dst" in shifted:
                out = embed(torch.empty_like(base), shift, written=True)
                rc = lib.cerberus_flow_upsample_forward(s.data_ptr(), out.data_ptr(), B * C, H, W, factor, CODE[dtype], stream())
                torch.cuda.synchronize()
                assert rc == 0 and ac.bands_untouched(out), (shifted, shift, rc)
            else:
                out = torch.ops.cerberus.flow_upsample(s, factor)
            check_result((shifted, shift), out, ref, bound, base)
