"""The OCR head's fused steps on the GPU (csrc/ocr_head.hip) against the float64 restatement of the reference's
operation order on the CPU (tests/ocr_cases.py).

The bound.  The same chain in stock fp32 ops runs on the GPU in the same test; its own error against float64 is ``e_stock``, and
every output and gradient of the fused route must have ``l2_err`` and ``rel_err`` of at most ``4 x max(e_stock, 2^-23)`` -- the
rule and the floor of test_seg_loss_gpu.py and test_rmi_loss_gpu.py.

The shapes.  The pooling kernel gives a workgroup a chunk of P = 256 pixels and walks the channels in LDS tiles of 32; the
lane-per-pixel kernels (gather backward, attention forward and backward) give a workgroup 256 pixels and keep key / value / the
context gradient in LDS tables of T = 64 channels; the fold adds the chunks' partials 8 per round; the regions live in registers in
groups of 4.  From that (B, C, R, H, W):
    (1, 3, 2, 5, 7)        35 pixels: fewer than a wave, one ragged chunk, 3 channels, R = 2, odd H W: the 4-byte loads
    (2, 19, 19, 37, 53)    1961 = 7 x 256 + 169 pixels: 8 chunks with a ragged tail, not a multiple of 64, one fold round exactly
    (1, 17, 32, 150, 150)  22500 pixels: 88 chunks = 11 fold rounds, R = 32 (the > 64 KiB LDS opt-in), H W % 4 == 0: the row
                           statistics' 16-byte loads
    (3, 65, 1, 16, 20)     320 pixels (a multiple of 64, not of P), T + 1 = 65 channels (3 pooling tiles, 2 tables), R = 1, B = 3
    (2, 1, 19, 9, 31)      one channel, 279 pixels, odd W
    (1, 40, 7, 24, 44)     1056 pixels: 4 chunks + 32, a partial fold round only, R = 7 (a ragged register group), 16-byte loads
Odd W (5 x 7, 37 x 53, 9 x 31) takes the row statistics' 4-byte loads with their ragged last quad.

Measured on an MI355X (this file's own prints; fused / stock fp32 / bound, the worst entry of each case; DESIGN.md 3.24 has all):
gather 1.6e-7 / 1.0e-7 / 4.8e-7 at (1,3,2,5,7), 2.0e-7 / 1.8e-7 / 7.1e-7 at (2,19,19,37,53), 1.9e-7 / 1.9e-7 / 7.7e-7 at
(1,17,32,150,150); attention 2.8e-7 / 1.9e-7 / 7.6e-7 at (2,19,19,37,53), 4.3e-7 / 2.9e-7 / 1.2e-6 at (1,17,32,150,150); x 60: gather
1.3e-7 / 1.3e-7 / 5.0e-7, attention 6.8e-6 / 6.8e-6 / 2.7e-5; OCR_block 9.2e-7 / 6.0e-7 / 2.4e-6 (golden sizes), 1.78e-3 / 1.78e-3 /
7.1e-3 (the input gradient at (2,48,33,47)); attention peak memory at (2,256,32,64), R = 19: 9.71 MB (allowed 10.32 MB; stock 8.78 MB).
"""
import functools

import pytest
import torch

import cerberusnet_amd as ca
import ocr_cases as cases
from cerberusnet_amd import _lib, ops_ocr
from conftest import l2_err, rel_err
from op_cases import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 3, 2, 5, 7), (2, 19, 19, 37, 53), (1, 17, 32, 150, 150), (3, 65, 1, 16, 20), (2, 1, 19, 9, 31), (1, 40, 7, 24, 44)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def fused_gather(feats, logits, scale=1.0):
    return ca.spatial_gather(feats, logits, scale).unsqueeze(3)


@functools.lru_cache(maxsize=None)
def gather_case(shape, logit_range=3.0):
    B, C, K, H, W = shape
    *inputs, up = cases.gather_inputs(B, C, K, H, W, 500 + C, logit_range)
    ref = cases.run(cases.gather_chain, inputs, up, "cpu", torch.float64)
    stock = cases.run(cases.gather_chain, inputs, up, DEV, torch.float32)
    return inputs, up, ref, stock


@functools.lru_cache(maxsize=None)
def attention_case(shape, query_range=1.0, scale=None):
    B, C, R, H, W = shape
    scale = C ** -0.5 if scale is None else scale
    *inputs, up = cases.attention_inputs(B, C, R, H, W, 600 + C, query_range)
    chain = lambda q, k, v: cases.attention_chain(q, k, v, scale)
    ref = cases.run(chain, inputs, up, "cpu", torch.float64)
    stock = cases.run(chain, inputs, up, DEV, torch.float32)
    return inputs, up, ref, stock, scale


def check(tag, names, got, stock, ref):
    failed = []
    for name, g, s, r in zip(names, got, stock, ref):
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), (tag, name)
        for metric in (l2_err, rel_err):
            e, e_stock = metric(g.numpy(), r.numpy()), metric(s.numpy(), r.numpy())
            print("%s %s %s: fused %.3e stock fp32 %.3e (bound %.3e)" % (tag, name, metric.__name__, e, e_stock, cases.bound(e_stock)))
            if not e <= cases.bound(e_stock):
                failed.append((tag, name, metric.__name__, e, e_stock))
    assert not failed, failed


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_spatial_gather_matches_float64_within_the_stock_chains_error(shape):
    inputs, up, ref, stock = gather_case(shape)
    got = cases.run(fused_gather, inputs, up, DEV, torch.float32)
    check("gather %s" % (shape,), ("context", "grad_feats", "grad_logits"), got, stock, ref)
    # the second output: the log-sum-exp of every class plane
    f, x = (t.to(DEV) for t in inputs)
    lse = torch.ops.cerberus_ocr.spatial_gather(f, x, 1.0)[1].double().cpu()
    want = torch.logsumexp(inputs[1].double().flatten(2), dim=2)
    e, e_stock = rel_err(lse.numpy(), want.numpy()), rel_err(torch.logsumexp(x.flatten(2), dim=2).double().cpu().numpy(), want.numpy())
    print("gather %s lse rel_err: fused %.3e stock %.3e" % (shape, e, e_stock))
    assert e <= cases.bound(e_stock)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_object_attention_matches_float64_within_the_stock_chains_error(shape):
    inputs, up, ref, stock, scale = attention_case(shape)
    got = cases.run(lambda q, k, v: ca.object_attention(q, k, v, scale), inputs, up, DEV, torch.float32)
    check("attention %s" % (shape,), ("context", "grad_query", "grad_key", "grad_value"), got, stock, ref)
    q, k, v = (t.to(DEV) for t in inputs)
    attn = torch.ops.cerberus_ocr.object_attention(q, k, v, scale)[1]
    want = torch.softmax(scale * torch.einsum("bchw,bcr->brhw", inputs[0].double(), inputs[1].double()), dim=1)
    stock_attn = torch.softmax(scale * torch.einsum("bchw,bcr->brhw", q, k), dim=1)
    e, e_stock = rel_err(attn.double().cpu().numpy(), want.numpy()), rel_err(stock_attn.double().cpu().numpy(), want.numpy())
    print("attention %s attn rel_err: fused %.3e stock %.3e" % (shape, e, e_stock))
    assert e <= cases.bound(e_stock)


def test_one_region_is_exact():
    """R = 1: the attention weights are exactly 1, the context is the value column, grad_query and grad_key are exactly zero."""
    B, C, H, W = 3, 65, 16, 20
    q, k, v, up = (t.to(DEV) for t in cases.attention_inputs(B, C, 1, H, W, 700))
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    context, attn = torch.ops.cerberus_ocr.object_attention(q, k, v, C ** -0.5)
    assert bool((attn == 1.0).all())
    assert same_bits(context.detach(), v.detach().view(B, C, 1, 1).expand(B, C, H, W))
    gq, gk, gv = torch.autograd.grad(context, [q, k, v], up)
    assert int(torch.count_nonzero(gq)) == 0 and int(torch.count_nonzero(gk)) == 0
    want = up.double().flatten(2).sum(2, keepdim=True).cpu().numpy()             # grad_value is the sum of the upstream gradient
    e_stock = l2_err(up.flatten(2).sum(2, keepdim=True).double().cpu().numpy(), want)
    assert l2_err(gv.double().cpu().numpy(), want) <= cases.bound(e_stock)


def test_one_pixel_gathers_the_features_themselves():
    """H W = 1: every class's softmax is exactly 1, the gathered context equals the features bit for bit."""
    feats, logits, _ = (t.to(DEV) for t in cases.gather_inputs(2, 65, 19, 1, 1, 710))
    context, lse = torch.ops.cerberus_ocr.spatial_gather(feats, logits, 1.0)
    assert same_bits(context, feats.view(2, 65, 1).expand(2, 65, 19))
    assert same_bits(lse, logits.view(2, 19))


def test_large_logits_and_queries_stay_finite_and_within_the_bound():
    """x 60: exp overflows fp32 unless the maximum is subtracted first."""
    shape = (2, 19, 19, 37, 53)
    inputs, up, ref, stock = gather_case(shape, 180.0)
    assert float(inputs[1].max()) > 89.0
    got = cases.run(fused_gather, inputs, up, DEV, torch.float32)
    check("gather x60", ("context", "grad_feats", "grad_logits"), got, stock, ref)
    inputs, up, ref, stock, scale = attention_case(shape, 60.0, 1.0)
    sim = torch.einsum("bchw,bcr->brhw", inputs[0].double(), inputs[1].double())
    assert float(sim.max()) > 89.0
    got = cases.run(lambda q, k, v: ca.object_attention(q, k, v, scale), inputs, up, DEV, torch.float32)
    check("attention x60", ("context", "grad_query", "grad_key", "grad_value"), got, stock, ref)


def _shifted(t):
    """``t``'s values in a view that starts 4 bytes into a larger buffer."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _all_results(fn, inputs, up, shift):
    prep = _shifted if shift else (lambda t: t.clone())
    leaves = [prep(t.to(DEV)).requires_grad_(True) for t in inputs]
    outs = fn(*leaves)
    grads = torch.autograd.grad(outs[0], leaves, prep(up.to(DEV)))
    return [o.detach() for o in outs] + list(grads)


@pytest.mark.parametrize("shape", [(2, 65, 19, 36, 52), (1, 17, 32, 150, 150)], ids=["2x65x19x36x52", "1x17x32x150x150"])
def test_two_calls_and_a_misaligned_call_give_the_same_bits(shape):
    """H W % 4 == 0: the aligned call takes the 16-byte loads, the shifted one the 4-byte loads."""
    B, C, R, H, W = shape
    for tag, fn, (*inputs, up) in (
            ("gather", lambda f, x: torch.ops.cerberus_ocr.spatial_gather(f, x, 1.0), cases.gather_inputs(B, C, R, H, W, 720)),
            ("attention", lambda q, k, v: torch.ops.cerberus_ocr.object_attention(q, k, v, C ** -0.5), cases.attention_inputs(B, C, R, H, W, 730))):
        up = up.view(B, C, R) if tag == "gather" else up
        first, second, shifted = (_all_results(fn, inputs, up, s) for s in (False, False, True))
        for i, (a, b, c) in enumerate(zip(first, second, shifted)):
            assert same_bits(a, b), (tag, "second call", i)
            assert same_bits(a, c), (tag, "4 bytes into a buffer", i)


def _peak(fn, q, k, v, up):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(q, k, v)
    grads = torch.autograd.grad(out, [q, k, v], up)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out, grads
    return peak


def test_attention_peak_memory_has_no_second_full_size_temporary():
    B, C, R, H, W = 2, 256, 19, 32, 64
    q, k, v, up = (t.to(DEV) for t in cases.attention_inputs(B, C, R, H, W, 740))
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    scale = C ** -0.5
    fused = lambda q, k, v: ca.object_attention(q, k, v, scale)
    _peak(fused, q, k, v, up)                          # warm the allocator and the library
    full = 4 * B * C * H * W                           # one (B,Kc,H,W) fp32 tensor: 4 MiB
    regions = 4 * B * R * H * W                        # one (B,R,H,W) fp32 tensor: 311,296 B
    workspace = _lib.get().cerberus_ocr_workspace_bytes(B, C, R, H * W)
    assert workspace == ops_ocr._ocr_workspace_bytes(B, C, R, H * W) == 4 * (116 + B * 8 * C * R)
    # the output + grad_query, attn + dsim, the workspace, and 1 MB for grad_key, grad_value and the allocator's rounding
    allowed = 2 * full + 2 * regions + workspace + 1000000
    got = _peak(fused, q, k, v, up)
    stock = _peak(lambda q, k, v: cases.attention_chain(q, k, v, scale), q, k, v, up)
    print("attention forward + backward at %s: peak excess fused %d B (allowed %d B), stock chain %d B" % ((B, C, R, H, W), got, allowed, stock))
    assert got <= allowed
    assert allowed < 3 * full                           # the bound itself leaves no room for a third (B,Kc,H,W) tensor


@functools.lru_cache(maxsize=None)
def block_reference(sizes, shape):
    x = cases.block_input(shape)
    block = cases.make_block(ca.OCR_block, "torch", **dict(sizes)).double()
    xd = x.double().requires_grad_(True)
    outs = block(xd)
    grad, = torch.autograd.grad(cases.block_loss(*outs), xd)
    return x, [o.detach() for o in outs] + [grad]


@pytest.mark.parametrize("sizes,shape", [((), cases.BLOCK_INPUT),
                                         ((("high_level_ch", 48), ("mid_channels", 32), ("key_channels", 16), ("classes", 19)), (2, 48, 33, 47))],
                         ids=["golden", "2x48x33x47"])
def test_whole_block_hip_against_torch_against_float64(sizes, shape):
    x, ref = block_reference(sizes, shape)
    results = {}
    for backend in ("hip", "torch"):
        block = cases.make_block(ca.OCR_block, backend, **dict(sizes)).to(DEV)
        xg = x.to(DEV).requires_grad_(True)
        outs = block(xg)
        grad, = torch.autograd.grad(cases.block_loss(*outs), xg)
        results[backend] = [o.detach().double().cpu() for o in outs] + [grad.double().cpu()]
    check("block %s" % (shape,), ("cls_out", "aux_out", "ocr_feats", "grad_input"), results["hip"], results["torch"], ref)


def test_the_hip_backend_takes_the_fused_ops_and_the_torch_backend_does_not(monkeypatch):
    seen = []
    gather, attention = ops_ocr.spatial_gather, ops_ocr.object_attention
    monkeypatch.setattr(ops_ocr, "spatial_gather", lambda *a: (seen.append("gather"), gather(*a))[1])
    monkeypatch.setattr(ops_ocr, "object_attention", lambda *a: (seen.append("attention"), attention(*a))[1])
    x = cases.block_input().to(DEV)
    cases.make_block(ca.OCR_block, "torch").to(DEV)(x)
    assert seen == []
    cases.make_block(ca.OCR_block, "hip").to(DEV)(x)
    assert seen == ["gather", "attention"]


def test_raw_ops_reject_what_the_modules_route_elsewhere():
    f, x = torch.zeros(1, 4, 6, 7, device=DEV), torch.zeros(1, 3, 6, 7, device=DEV)
    k = torch.zeros(1, 4, 3, device=DEV)
    with pytest.raises(RuntimeError, match="cerberus_ocr::spatial_gather: .*float32"):
        torch.ops.cerberus_ocr.spatial_gather(f.half(), x.half(), 1.0)
    with pytest.raises(RuntimeError, match="cerberus_ocr::object_attention: .*float32"):
        torch.ops.cerberus_ocr.object_attention(f.half(), k.half(), k.half(), 0.5)
    with pytest.raises(RuntimeError, match="cerberus_ocr::spatial_gather: needs 1..32 regions, got 33"):
        torch.ops.cerberus_ocr.spatial_gather(f, torch.zeros(1, 33, 6, 7, device=DEV), 1.0)
    with pytest.raises(RuntimeError, match="cerberus_ocr::object_attention: needs 1..32 regions, got 33"):
        torch.ops.cerberus_ocr.object_attention(f, torch.zeros(1, 4, 33, device=DEV), torch.zeros(1, 4, 33, device=DEV), 0.5)
    with pytest.raises(RuntimeError, match="cerberus_ocr::spatial_gather: logits must be"):
        torch.ops.cerberus_ocr.spatial_gather(f, torch.zeros(1, 3, 6, 8, device=DEV), 1.0)
    with pytest.raises(RuntimeError, match="cerberus_ocr::object_attention: value must be"):
        torch.ops.cerberus_ocr.object_attention(f, k, torch.zeros(1, 4, 2, device=DEV), 0.5)
    with pytest.raises(RuntimeError, match="cerberus_ocr::object_attention_backward: grad_context must be"):
        torch.ops.cerberus_ocr.object_attention_backward(torch.zeros(1, 4, 6, 8, device=DEV), f, k, k, x, 0.5)
    # the modules route all of it to the stock ops
    m = ca.SpatialGather_Module(33, backend="hip")
    assert m(f, torch.zeros(1, 33, 6, 7, device=DEV)).shape == (1, 4, 33, 1)
    assert m(f.half(), x.half()).dtype == torch.float16
