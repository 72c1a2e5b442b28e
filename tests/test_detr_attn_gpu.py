"""The DETR attention core on the GPU (csrc/detr_attn.hip) against the float64 restatement of the stock chain on
the CPU (tests/attn_cases.py).

The bound.  The same chain in stock fp32 ops runs on the GPU in the same test; its own error against float64 is ``e_stock``, and the
output and every gradient of the fused route must have ``l2_err`` and ``rel_err`` of at most ``4 x max(e_stock, 2^-23)`` -- the rule
and the floor of tests/ocr_cases.py.

The shapes.  A workgroup owns 128 rows (4 waves x 32: queries in the forward and the dq kernel, keys in the dk / dv kernel) and
walks the other side in tiles of 32 rows.  From that (Lq, Lk, B, H):
    (1, 1, 1, 1)          one row each way: 31 of a wave's 32 rows and of a tile's 32 rows are padding
    (5, 7, 2, 3)          less than one wave and one tile each way, B H = 6 planes
    (100, 100, 2, 8)      the decoder's self-attention: 3 waves + 4 rows, 3 tiles + 4
    (100, 561, 2, 8)      the decoder's cross-attention on a 17 x 33 map: 17 tiles + 17 keys; 4 key-owning workgroups + 49 keys
    (130, 65, 2, 1)       two rows past one workgroup of queries, one key past two tiles
    (257, 257, 1, 1)      one row past two workgroups both ways, one past eight tiles
    (257, 1031, 1, 2)     several workgroups and 32 tiles + 7 with a prime key count

Measured on an MI355X (this file's own prints; fused / stock fp32 / bound, the entry of each case nearest its bound): (1,1,1,1) exact;
(5,7,2,3) 1.9e-7 / 1.3e-7 / 5.2e-7 (grad_q); (100,100,2,8) 5.3e-7 / 4.2e-7 / 1.7e-6 (out); (100,561,2,8) 1.1e-6 / 8.7e-7 / 3.5e-6
(grad_q); (130,65,2,1) 3.6e-7 / 3.1e-7 / 1.2e-6 (out); (257,257,1,1) 6.4e-7 / 4.6e-7 / 1.8e-6 (grad_k); (257,1031,1,2) 1.7e-6 / 5.3e-7 /
2.1e-6 (out: 1031 keys are one fmaf chain of 33 rescaled tiles per output); masked 8.0e-7 / 6.9e-7 / 2.8e-6; x 60 1.7e-5 / 1.6e-5 /
6.2e-5 (grad_q); dropout 0.1 5.3e-7 / 4.6e-7 / 1.9e-6, with the mask 8.2e-7 / 7.5e-7 / 3.0e-6; dropout 0.5 3.5e-7 / 2.8e-7 / 1.1e-6, with
the mask 3.8e-7 / 3.0e-7 / 1.2e-6; lse 1.6e-7 .. 2.4e-7 against 8.4e-8 .. 1.6e-7; kept share 0.89912 (p = 0.1) and 0.49357 (p = 0.5) of
54600; peak memory at L = 2048, H = 8: 8.7 MB fused (allowed 33.6 MB), 545 MB through nn.MultiheadAttention.
"""
import functools

import pytest
import torch

import attn_cases as cases
import cerberusnet_amd as ca
from cerberusnet_amd import ops_attn
from conftest import l2_err, rel_err
from op_cases import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = cases.HEAD_DIM
SCALE = D ** -0.5

SHAPES = [(1, 1, 1, 1), (5, 7, 2, 3), (100, 100, 2, 8), (100, 561, 2, 8), (130, 65, 2, 1), (257, 257, 1, 1), (257, 1031, 1, 2)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
NAMES = ("out", "grad_q", "grad_k", "grad_v")


def seed_tensor(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def fused(H, mask=None, p=0.0, seed=None, scale=SCALE):
    m = None if mask is None else mask.to(DEV)
    return lambda q, k, v: ca.detr_attention(q, k, v, H, m, p, seed, scale)


@functools.lru_cache(maxsize=None)
def reference(shape, query_range=1.0, scale=SCALE, mask_spec=None, p=0.0, seed=None):
    """The inputs, the float64 chain on the CPU and the fp32 chain on the GPU (with the op's own keep mask when p > 0)."""
    Lq, Lk, B, H = shape
    *tensors, up = cases.inputs(Lq, Lk, B, H, 800 + Lq + Lk, query_range)
    mask = None if mask_spec is None else cases.padding_mask(B, Lk, *mask_spec)
    keep = None
    if p > 0.0:
        keep = torch.ops.cerberus_attn.attn_dropout_keep(seed_tensor(seed), B, H, Lq, Lk, p).cpu()
    fn = lambda q, k, v: cases.chain(q, k, v, H, scale, mask, keep, p)
    ref = cases.run(fn, tensors, up, "cpu", torch.float64)
    stock = cases.run(fn, tensors, up, DEV, torch.float32)
    return tensors, up, mask, ref, stock


def check(tag, got, stock, ref, names=NAMES):
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
def test_output_and_gradients_match_float64_within_the_stock_chains_error(shape):
    Lq, Lk, B, H = shape
    tensors, up, _, ref, stock = reference(shape)
    got = cases.run(fused(H), tensors, up, DEV, torch.float32)
    check("attention %s" % (shape,), got, stock, ref)
    # the second output of the raw op: the log-sum-exp of every row
    q, k, v = (t.to(DEV) for t in tensors)
    lse = torch.ops.cerberus_attn.attention(q, k, v, H, None, SCALE, 0.0, None)[1]
    assert lse.shape == (B, H, Lq)
    stats = torch.ops.cerberus_attn.attention(q, k, v, H, None, SCALE, 0.0, None)[2]
    assert stats.shape == (B, H, Lq, 2) and torch.allclose(lse, stats[..., 0] + torch.log(stats[..., 1]), rtol=1e-6, atol=1e-6)
    want = cases.lse_chain(tensors[0].double(), tensors[1].double(), H, SCALE).numpy()
    e, e_stock = rel_err(lse.double().cpu().numpy(), want), rel_err(cases.lse_chain(q, k, H, SCALE).double().cpu().numpy(), want)
    print("attention %s lse rel_err: fused %.3e stock %.3e" % (shape, e, e_stock))
    assert e <= cases.bound(e_stock)


def test_a_wholly_masked_first_key_tile_and_a_ragged_masked_tail():
    """Entry 0 ignores its first 40 keys (the whole first tile of 32 and a part of the second) and its last 61; entry 1 its first 32
    exactly and its last 1: the running maximum starts at -inf and must not poison what follows."""
    shape, spec = (100, 561, 2, 8), ((40, 32), (61, 1))
    tensors, up, mask, ref, stock = reference(shape, mask_spec=spec)
    assert bool(mask[:, :32].all()) and not bool(mask[:, 100:400].any())
    got = cases.run(fused(8, mask), tensors, up, DEV, torch.float32)
    check("masked %s" % (shape,), got, stock, ref)
    for g in got[2:]:                                   # an ignored key receives exactly nothing
        assert int(torch.count_nonzero(g[:40, 0])) == 0 and int(torch.count_nonzero(g[-61:, 0])) == 0
        assert int(torch.count_nonzero(g[:32, 1])) == 0 and int(torch.count_nonzero(g[-1:, 1])) == 0
    q, k, v = (t.to(DEV) for t in tensors)
    lse = torch.ops.cerberus_attn.attention(q, k, v, 8, mask.to(DEV), SCALE, 0.0, None)[1].double().cpu().numpy()
    want = cases.lse_chain(tensors[0].double(), tensors[1].double(), 8, SCALE, mask).numpy()
    assert rel_err(lse, want) <= cases.bound(rel_err(cases.lse_chain(q, k, 8, SCALE, mask).double().cpu().numpy(), want))


def test_an_entry_with_every_key_masked_gives_zeros_and_leaves_the_others_alone():
    """The deliberate difference from the stock chain (NaN there): zeros out, lse -inf, zero gradients; entry 0 keeps its bits."""
    Lq, Lk, B, H = 70, 45, 2, 3
    *tensors, up = cases.inputs(Lq, Lk, B, H, 900)
    none, one = cases.padding_mask(B, Lk, (3, 0), (0, 0)), cases.padding_mask(B, Lk, (3, Lk), (0, 0))
    results = []
    for mask in (none, one):
        leaves = [t.to(DEV).requires_grad_(True) for t in tensors]
        out, lse = ops_attn._Attention.apply(*leaves, H, mask.to(DEV), SCALE, 0.0, None)
        grads = torch.autograd.grad(out, leaves, up.to(DEV))
        results.append([out.detach(), lse.detach()] + list(grads))
    plain, masked = results
    for i, (a, b) in enumerate(zip(plain, masked)):
        if i == 1:                                      # lse is (B,H,Lq)
            assert same_bits(a[0], b[0]) and bool((b[1] == float("-inf")).all())
        else:
            assert same_bits(a[:, 0], b[:, 0]), i
            assert int(torch.count_nonzero(b[:, 1])) == 0 and bool(torch.isfinite(b).all()), i
            assert int(torch.count_nonzero(a[:, 1])) > 0, i


def test_queries_times_60_stay_finite_and_within_the_bound():
    """x 60 at scale 1: exp overflows fp32 unless the running maximum is subtracted, and the maximum moves from tile to tile."""
    shape = (100, 561, 2, 8)
    tensors, up, _, ref, stock = reference(shape, 60.0, 1.0)
    sim = torch.einsum("ibe,jbe->bij", tensors[0][:, :, :D].double(), tensors[1][:, :, :D].double())
    assert float(sim.max()) > 89.0
    got = cases.run(fused(8, scale=1.0), tensors, up, DEV, torch.float32)
    check("attention x60", got, stock, ref)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_matches_the_float64_chain_under_the_ops_own_keep_mask(p):
    shape, seed = (100, 561, 2, 8), 20240 + int(p * 10)
    tensors, up, _, ref, stock = reference(shape, p=p, seed=seed)
    got = cases.run(fused(8, None, p, seed_tensor(seed)), tensors, up, DEV, torch.float32)
    check("dropout %.1f %s" % (p, shape), got, stock, ref)
    spec = ((40, 32), (61, 1))
    tensors, up, mask, ref, stock = reference(shape, mask_spec=spec, p=p, seed=seed)
    got = cases.run(fused(8, mask, p, seed_tensor(seed)), tensors, up, DEV, torch.float32)
    check("dropout %.1f masked %s" % (p, shape), got, stock, ref)


def raw(tensors, up, H, mask, p, seed, need, shift=False):
    prep = _shifted if shift else (lambda t: t.clone())
    q, k, v, g = (prep(t.to(DEV)) for t in (*tensors, up))
    m = None if mask is None else mask.to(DEV)
    out, lse, stats = torch.ops.cerberus_attn.attention(q, k, v, H, m, SCALE, p, seed)
    grads = torch.ops.cerberus_attn.attention_backward(g, q, k, v, out, stats, H, m, SCALE, p, seed, need)
    return [out, lse, stats] + list(grads)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_two_runs_and_every_gradient_subset_give_the_same_bits(p):
    Lq, Lk, B, H = 130, 65, 2, 3
    *tensors, up = cases.inputs(Lq, Lk, B, H, 910)
    mask, seed = cases.padding_mask(B, Lk, (0, 33), (5, 0)), seed_tensor(77)
    full = raw(tensors, up, H, mask, p, seed, [True, True, True])
    for a, b in zip(full, raw(tensors, up, H, mask, p, seed, [True, True, True])):
        assert same_bits(a, b)
    assert all(int(torch.count_nonzero(g)) > 0 for g in full)
    for bits in range(7):
        need = [bool(bits & 1), bool(bits & 2), bool(bits & 4)]
        got = raw(tensors, up, H, mask, p, seed, need)[3:]
        for g, want, n in zip(got, full[3:], need):
            assert same_bits(g, want) if n else g.shape == (0,), (need,)


def _shifted(t):
    """``t``'s values in a view that starts one element into a larger buffer."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_misaligned_views_give_the_same_bits(p):
    Lq, Lk, B, H = 100, 100, 2, 8
    *tensors, up = cases.inputs(Lq, Lk, B, H, 920)
    mask, seed = cases.padding_mask(B, Lk, (0, 3), (2, 0)), seed_tensor(78)
    need = [True, True, True]
    for a, b in zip(raw(tensors, up, H, mask, p, seed, need), raw(tensors, up, H, mask, p, seed, need, shift=True)):
        assert same_bits(a, b)


def test_a_graph_captured_on_one_stream_replays_to_the_eager_bits():
    Lq, Lk, B, H, p = 100, 561, 2, 8, 0.1
    q, k, v, g = (t.to(DEV) for t in cases.inputs(Lq, Lk, B, H, 930))
    mask, seed = cases.padding_mask(B, Lk, (40, 32), (61, 1)).to(DEV), seed_tensor(79)

    def step():
        out, lse, stats = torch.ops.cerberus_attn.attention(q, k, v, H, mask, SCALE, p, seed)
        return [out, lse, stats] + list(torch.ops.cerberus_attn.attention_backward(g, q, k, v, out, stats, H, mask, SCALE, p, seed,
                                                                                   [True, True, True]))

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert same_bits(a, b)
    assert int(seed.item()) == 79
    # another seed in the same tensor: the replay reads it on the device
    seed.fill_(80)
    graph.replay()
    torch.cuda.synchronize()
    assert not same_bits(eager[0], captured[0])
    for a, b in zip(step(), captured):
        assert same_bits(a, b)


# ---- the keep mask ------------------------------------------------------------------------------------------------------------------
KEEP_SHAPE = (2, 3, 70, 130)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_mask_equals_the_python_restatement_and_has_the_stated_share(p):
    B, H, Lq, Lk = KEEP_SHAPE
    seed = 0x123456789ABCDE + int(p * 10)
    keep = torch.ops.cerberus_attn.attn_dropout_keep(seed_tensor(seed), B, H, Lq, Lk, p)
    assert keep.dtype == torch.bool and keep.shape == KEEP_SHAPE
    assert torch.equal(keep.cpu(), cases.keep_reference(seed, B, H, Lq, Lk, p))
    assert torch.equal(torch.ops.cerberus_attn.attn_dropout_keep(seed_tensor(-seed), B, H, Lq, Lk, p).cpu(),
                       cases.keep_reference(-seed, B, H, Lq, Lk, p))
    share = keep.double().mean().item()
    n = keep.numel()
    print("keep p=%.1f: kept share %.5f of %d" % (p, share, n))
    assert abs(share - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5
    planes = keep.double().flatten(2).mean(2).flatten().tolist()
    for s in planes:
        assert abs(s - (1 - p)) <= 5 * (p * (1 - p) / (Lq * Lk)) ** 0.5, planes


def test_two_seeds_give_different_masks_and_p_zero_keeps_everything():
    B, H, Lq, Lk = KEEP_SHAPE
    a = torch.ops.cerberus_attn.attn_dropout_keep(seed_tensor(1), B, H, Lq, Lk, 0.5)
    b = torch.ops.cerberus_attn.attn_dropout_keep(seed_tensor(2), B, H, Lq, Lk, 0.5)
    differ = (a != b).double().mean().item()
    assert abs(differ - 0.5) < 0.02                     # independent masks differ in half their entries
    assert not torch.equal(a[0, 0], a[0, 1]) and not torch.equal(a[0], a[1])
    assert bool(torch.ops.cerberus_attn.attn_dropout_keep(seed_tensor(1), B, H, Lq, Lk, 0.0).all())


def test_the_wrapper_draws_a_seed_on_the_device_when_none_is_given():
    q, k, v, _ = (t.to(DEV) for t in cases.inputs(100, 100, 2, 8, 940))
    a, b = ca.detr_attention(q, k, v, 8, dropout_p=0.5), ca.detr_attention(q, k, v, 8, dropout_p=0.5)
    assert not same_bits(a, b)
    s = seed_tensor(5)
    assert same_bits(ca.detr_attention(q, k, v, 8, dropout_p=0.5, seed=s), ca.detr_attention(q, k, v, 8, dropout_p=0.5, seed=s))
    assert same_bits(ca.detr_attention(q, k, v, 8), ca.detr_attention(q, k, v, 8, scale=SCALE))


# ---- memory -------------------------------------------------------------------------------------------------------------------------
def _peak(fn, tensors, up):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(*tensors)
    grads = torch.autograd.grad(out, tensors, up)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out, grads
    return peak


def test_nothing_of_the_probability_matrixs_size_is_allocated():
    Lq = Lk = 2048
    B, H = 1, 8
    matrix = 4 * B * H * Lq * Lk                                        # 134 MB
    q, k, v, up = (t.to(DEV) for t in cases.inputs(Lq, Lk, B, H, 950))
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    route = fused(H, None, 0.1, seed_tensor(3))
    _peak(route, (q, k, v), up)                                         # warm the allocator and the library
    got = _peak(route, (q, k, v), up)
    mha = torch.nn.MultiheadAttention(H * D, H, dropout=0.1).to(DEV).train()
    stock = _peak(lambda q, k, v: mha(q, k, value=v)[0], (q, k, v), up)
    print("attention forward + backward at L = 2048, H = 8: peak excess fused %d B (allowed %d B), nn.MultiheadAttention %d B" % (
        got, matrix // 4, stock))
    assert got < matrix // 4
    assert stock > matrix                                               # the measurement sees the matrix when there is one


def test_raw_ops_reject_what_the_modules_route_elsewhere():
    q, k = torch.zeros(5, 2, 64, device=DEV), torch.zeros(7, 2, 64, device=DEV)
    with pytest.raises(RuntimeError, match="cerberus_attn::attention: .*float32"):
        torch.ops.cerberus_attn.attention(q.half(), k.half(), k.half(), 2, None, 1.0, 0.0, None)
    with pytest.raises(RuntimeError, match="cerberus_attn::attention: needs a head width of 32, got 16"):
        torch.ops.cerberus_attn.attention(q, k, k, 4, None, 1.0, 0.0, None)
    with pytest.raises(RuntimeError, match="cerberus_attn::attention: v must be"):
        torch.ops.cerberus_attn.attention(q, k, k[:6], 2, None, 1.0, 0.0, None)
    with pytest.raises(RuntimeError, match="cerberus_attn::attention: key_padding_mask must be"):
        torch.ops.cerberus_attn.attention(q, k, k, 2, torch.zeros(2, 6, dtype=torch.bool, device=DEV), 1.0, 0.0, None)
    with pytest.raises(RuntimeError, match="cerberus_attn::attention: dropout_p > 0 needs a seed"):
        torch.ops.cerberus_attn.attention(q, k, k, 2, None, 1.0, 0.1, None)
    with pytest.raises(RuntimeError, match="cerberus_attn::attention_backward: stats must be"):
        torch.ops.cerberus_attn.attention_backward(q, q, k, k, q, torch.zeros(2, 2, 6, 2, device=DEV), 2, None, 1.0, 0.0, None, [True] * 3)
