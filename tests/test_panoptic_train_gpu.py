"""GPU tests of the panoptic training side (csrc/panoptic_train.hip): ``cerberus::panoptic_targets`` and
``cerberus::panoptic_loss`` with their wrappers.

Targets: every comparison is BIT FOR BIT -- against tests/golden/panoptic_train.npz (the reference's own generator on the CPU),
against the stock route on the same device, and for the 2048 x 2048 case against the closed-form integer model of
tests/panoptic_train_cases.py (one instance spans 4096 workgroups; sum y is 2^32 - 2^21 there and passes 2^32 at 2112 x 2048).

Loss: yardstick float64 on the CPU (``cases.loss64``).  Values: relative error <= 1e-5.  Gradients: ``l2_err`` and ``rel_err``
each at most 4 x max(e_stock, 2^-23), e_stock being the same error of the stock fp32 chain on the GPU in the same test (the
rule of tests/test_seg_loss_gpu.py).  Exact zeros are required where m == 0 in pixel mode, where d == 0 in the L1 term (every
fifth offset element is a planted tie) and everywhere when a mask is empty."""
import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import panoptic_train_cases as cases
import reduction_cases as rc
from cerberusnet_amd import ops
from cerberusnet_amd.utilities.panoptic_targets import PanopticTargetGenerator, gaussian_table, panoptic_targets
from conftest import l2_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_TOL = 1e-5
GRAD_FACTOR = 4.0
GRAD_FLOOR = 2.0 ** -23


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_bits(a, b):
    """Two device tensors hold the same bits (NaNs included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


KEYS = cases.ITEMS + ["center_points"]


# ---- targets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.TARGET_CASES))
@pytest.mark.parametrize("id_dtype", [torch.int64, torch.int32])
def test_targets_reproduce_the_reference_and_the_stock_route(golden, name, id_dtype):
    g = golden("panoptic_train")
    ids, sid, cat, crowd, count, _segs, kwargs = cases.target_case(name)
    args = [dev(ids).to(id_dtype)] + [dev(a) for a in (sid, cat, crowd, count)]
    out = panoptic_targets(*args, backend="hip", **kwargs)
    stock = panoptic_targets(*args, backend="torch", **kwargs)
    for item in cases.ITEMS:
        assert out[item].is_cuda and bits_equal(out[item].cpu().numpy(), g["tgt_%s_%s" % (name, item)]), (name, item)
    assert bits_equal(out["center_points"].cpu().numpy(), g["tgt_%s_points" % name]), name
    for key in KEYS:
        assert same_bits(out[key], stock[key]), (name, key)
    again = panoptic_targets(*args, backend="hip", **kwargs)
    assert all(same_bits(out[k], again[k]) for k in KEYS)                 # run to run


def test_targets_at_the_row_limit_and_past_it(golden):
    g = golden("panoptic_train")
    limit = ops.PANOPTIC_TARGETS_MAX_SEGMENTS
    n = g["tgt_vector_points"].shape[1]
    for S in (limit, limit + 1):            # the fused route, then the fallback
        ids, sid, cat, crowd, count, kwargs = cases.widened("vector", S)
        out = panoptic_targets(*[dev(a) for a in (ids, sid, cat, crowd, count)], backend="hip", **kwargs)
        for item in cases.ITEMS:
            assert bits_equal(out[item].cpu().numpy(), g["tgt_vector_%s" % item]), (S, item)
        pts = out["center_points"].cpu().numpy()
        assert pts.shape == (2, S, 2) and bits_equal(pts[:, -n:], g["tgt_vector_points"]) and np.isnan(pts[:, :-n]).all()
    with pytest.raises(RuntimeError, match="at most 256 table rows"):
        flags = torch.zeros((2, S), dtype=torch.int32, device=DEV)
        torch.ops.cerberus.panoptic_targets(dev(ids), dev(sid), dev(cat), flags, dev(count), gaussian_table(2, DEV), 255, 2, False, 0, 1.0, False)


@pytest.mark.parametrize("shape", cases.HUGE_SHAPES)
def test_targets_of_a_2048_square_against_the_integer_model(shape):
    ids, sid, cat, crowd, count, kwargs = cases.huge_case(shape)
    out = panoptic_targets(*[dev(a) for a in (ids, sid, cat, crowd, count)], backend="hip", **kwargs)
    centres, offset, center, semantic_mask = cases.huge_expected(shape, gaussian_table(8).numpy())
    assert bits_equal(out["center_points"].cpu().numpy()[0], centres)
    assert bits_equal(out["offset"].cpu().numpy(), offset)
    assert bits_equal(out["center"].cpu().numpy(), center)
    assert bits_equal(out["semantic_mask"].cpu().numpy(), semantic_mask)
    sem = out["semantic"].cpu().numpy()
    assert (sem == 12).sum() == 15 and (sem == 11).sum() == shape[0] * shape[1] - 15
    assert bool((out["foreground"] == 1).all()) and bool((out["center_mask"] == 1).all()) and bool((out["offset_mask"] == 1).all())


def test_targets_of_a_misaligned_id_map_give_the_same_bits():
    ids, sid, cat, crowd, count, _segs, kwargs = cases.target_case("vector")
    tables = [dev(a) for a in (sid, cat, crowd, count)]
    for dtype in (torch.int32, torch.int64):
        aligned = dev(ids).to(dtype)
        buf = torch.zeros(aligned.numel() + 1, dtype=dtype, device=DEV)
        shifted = buf[1:].view(aligned.shape)
        shifted.copy_(aligned)
        assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
        a = panoptic_targets(aligned, *tables, backend="hip", **kwargs)
        b = panoptic_targets(shifted, *tables, backend="hip", **kwargs)
        assert all(same_bits(a[k], b[k]) for k in KEYS)


def test_targets_in_a_captured_graph():
    ids, sid, cat, crowd, count, _segs, kwargs = cases.target_case("big")
    static = [dev(a) for a in (ids, sid, cat, crowd, count)]
    eager = panoptic_targets(*static, backend="hip", **kwargs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            panoptic_targets(*static, backend="hip", **kwargs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = panoptic_targets(*static, backend="hip", **kwargs)
    flipped = np.ascontiguousarray(ids[:, :, ::-1])
    want_flipped = panoptic_targets(dev(flipped), *static[1:], backend="hip", **kwargs)
    for maps, want in ((flipped, want_flipped), (ids, eager)):           # replayed twice, on two inputs
        static[0].copy_(dev(maps))
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(captured[k], want[k]) for k in KEYS)
    assert not same_bits(eager["offset"], want_flipped["offset"])


def test_generator_on_the_device(golden):
    g = golden("panoptic_train")
    ids, _sid, _cat, _crowd, _count, segs, kwargs = cases.target_case("big")
    gen = PanopticTargetGenerator(**kwargs)
    assert gen.backend == "hip" and gen.device.type == "cuda"
    out = gen(cases.colour(ids[0]), segs[0])
    for item in cases.ITEMS:
        assert out[item].is_cuda and bits_equal(out[item].cpu().numpy(), g["tgt_big_%s" % item]), item
    assert bits_equal(np.asarray(out["center_points"]), g["call_big_points"])


# ---- the loss -------------------------------------------------------------------------------------------------------------------
def _fused(arrays, with_c, with_o, masking, backend="hip"):
    """(value, grad_center, grad_offset) of the wrapper on device tensors (a list of six; a mask may be dropped)."""
    cp, ct, cm, op, ot, om = arrays
    p = {"center": cp.detach().clone().requires_grad_(True), "offset": op.detach().clone().requires_grad_(True)}
    t = {"center": ct, "offset": ot}
    if with_c:
        t["center_mask"] = cm
    if with_o:
        t["offset_mask"] = om
    v = ca.deeplab_panoptic_loss(p, t, cases.CENTER_WEIGHT, cases.OFFSET_WEIGHT, masking, backend=backend)
    gc, go = torch.autograd.grad(v, (p["center"], p["offset"]))
    return v.detach(), gc, go


def _check_grad(name, fused, stock, ref):
    for metric in (l2_err, rel_err):
        e, es = metric(fused, ref), metric(stock, ref)
        print("%s %s: fused %.3e stock fp32 %.3e" % (name, metric.__name__, e, es))
        assert e <= GRAD_FACTOR * max(es, GRAD_FLOOR), (name, metric.__name__, e, es)


def _against_float64(shape, with_c, with_o, masking):
    host = cases.loss_inputs(shape)
    arrays = [dev(a) for a in host]
    cp, ct, cm, op, ot, om = host
    ref, ref_c, ref_o = cases.loss64(cp, ct, cm if with_c else None, op, ot, om if with_o else None, cases.CENTER_WEIGHT,
                                     cases.OFFSET_WEIGHT, masking)
    v, gc, go = _fused(arrays, with_c, with_o, masking)
    vs, gcs, gos = _fused(arrays, with_c, with_o, masking, backend="torch")
    name = "panoptic loss %s masks %d%d %s" % (shape, with_c, with_o, masking)
    den = abs(ref) or 1.0                   # a one-pixel map whose only weight is 0: the value is 0
    print("%s value: fused rel %.3e stock fp32 rel %.3e" % (name, abs(v.item() - ref) / den, abs(vs.item() - ref) / den))
    assert v.shape == () and v.dtype == torch.float32 and abs(v.item() - ref) <= VALUE_TOL * abs(ref), (name, v.item(), ref)
    _check_grad(name + " centre", gc.cpu().numpy(), gcs.cpu().numpy(), ref_c)
    _check_grad(name + " offset", go.cpu().numpy(), gos.cpu().numpy(), ref_o)
    assert bool((go[arrays[3] == arrays[4]] == 0).all()) and int((arrays[3] == arrays[4]).sum()) >= op.size // 5      # sign(0) = 0
    if masking == "pixel":
        if with_c:
            assert bool((gc[:, 0][arrays[2] == 0] == 0).all())
        if with_o:
            assert bool((go[:, 0][arrays[5] == 0] == 0).all()) and bool((go[:, 1][arrays[5] == 0] == 0).all())
    # the raw op: the same bits, and the two scales
    loss, state = torch.ops.cerberus.panoptic_loss(arrays[0], arrays[1], arrays[2] if with_c else None, arrays[3], arrays[4],
                                                   arrays[5] if with_o else None, cases.CENTER_WEIGHT, cases.OFFSET_WEIGHT,
                                                   ops.PANOPTIC_LOSS_MODES[masking])
    assert torch.equal(loss, v) and state.shape == (2,)
    n = cp.size
    for i, (with_m, m, weight, count) in enumerate(((with_c, cm, cases.CENTER_WEIGHT, n), (with_o, om, cases.OFFSET_WEIGHT, 2 * n))):
        total = float(m.astype(np.float64).sum()) * count / n
        if with_m and total == 0:
            assert float(state[i]) == 0.0                                   # gated off
        else:
            want = weight / (total if (with_m and masking == "pixel") else count)
            assert abs(float(state[i]) - want) <= VALUE_TOL * want, (name, i)


@pytest.mark.parametrize("shape", cases.LOSS_SHAPES_SCALAR + cases.LOSS_SHAPES_VECTOR)
@pytest.mark.parametrize("with_c,with_o", cases.MASK_COMBOS)
@pytest.mark.parametrize("masking", ["reference", "pixel"])
def test_loss_against_float64(shape, with_c, with_o, masking):
    _against_float64(shape, with_c, with_o, masking)


@pytest.mark.parametrize("shape", cases.LOSS_TIER_SHAPES)
@pytest.mark.parametrize("masking,with_c,with_o", [("reference", True, False), ("pixel", True, True)])
def test_loss_past_one_finish_round(shape, masking, with_c, with_o):
    assert cases.loss_tiers(shape)
    _against_float64(shape, with_c, with_o, masking)


@pytest.mark.parametrize("masking", ["reference", "pixel"])
def test_empty_masks_give_exact_zeros(masking):
    host = list(cases.loss_inputs((2, 37, 53)))
    host[2], host[5] = np.zeros_like(host[2]), np.zeros_like(host[5])
    arrays = [dev(a) for a in host]
    v, gc, go = _fused(arrays, True, True, masking)
    assert v.item() == 0.0 and not gc.any() and not go.any()
    nan = [a.clone() for a in arrays]
    nan[0][0, 0, 3, 3] = float("nan")       # gated off: a NaN changes nothing, as in the reference, and gets the gradient 0.0f
    v, gc, go = _fused(nan, True, True, masking)
    assert v.item() == 0.0 and not gc.any() and not go.any()
    # one term gated off, the other one on
    v, gc, go = _fused(arrays, True, False, masking)
    ref, _, ref_o = cases.loss64(*host[:2], host[2], *host[3:5], None, cases.CENTER_WEIGHT, cases.OFFSET_WEIGHT, masking)
    assert abs(v.item() - ref) <= VALUE_TOL * ref and not gc.any() and l2_err(go.cpu().numpy(), ref_o) <= GRAD_FACTOR * GRAD_FLOOR


def test_nan_under_a_zero_weight():
    host = cases.loss_inputs((2, 37, 53))
    arrays = [dev(a) for a in host]
    clean, _, _ = _fused(arrays, True, True, "pixel")
    nan = [a.clone() for a in arrays]
    nan[0][:, 0][arrays[2] == 0] = float("nan")
    nan[3][:, 0][arrays[5] == 0] = float("nan")
    nan[3][:, 1][arrays[5] == 0] = float("inf")
    v, gc, go = _fused(nan, True, True, "pixel")
    assert torch.equal(v, clean) and not torch.isnan(gc).any() and not torch.isnan(go).any()
    assert bool((gc[:, 0][arrays[2] == 0] == 0).all()) and bool((go[:, 0][arrays[5] == 0] == 0).all())
    v, _, _ = _fused(nan, True, True, "reference")          # the reference's mean takes every element
    assert torch.isnan(v)


@pytest.mark.parametrize("shape", cases.LOSS_TIER_SHAPES)
def test_one_unmasked_pixel_in_each_marker_chunk(shape):
    """Pixel mode with ONE pixel of non-zero weight: the loss is that pixel's terms, whichever partial they land in."""
    host = cases.loss_inputs(shape)
    arrays = [dev(a) for a in host]
    cp, ct, _, op, ot, _ = host
    pixels = shape[0] * shape[1] * shape[2]
    nchunks = rc.chunks(pixels, ops.PANOPTIC_CHUNK_PIXELS)
    for k in rc.marker_chunks(nchunks):
        pixel = rc.marker_pixel(k, pixels, ops.PANOPTIC_CHUNK_PIXELS)
        flat_p, flat_t = op.reshape(shape[0], 2, -1), ot.reshape(shape[0], 2, -1)
        while (flat_p[0, :, pixel] == flat_t[0, :, pixel]).any():
            pixel -= 1                      # not a planted tie; the offsets inside a chunk leave room below
        assert pixel // ops.PANOPTIC_CHUNK_PIXELS == k
        mask = torch.zeros((pixels,), device=DEV)
        mask[pixel] = 0.5
        mask = mask.view(shape)
        v, gc, go = _fused([arrays[0], arrays[1], mask, arrays[3], arrays[4], mask], True, True, "pixel")
        b, r = divmod(pixel, shape[1] * shape[2])
        dc = float(cp.reshape(shape[0], -1)[b, r]) - float(ct.reshape(shape[0], -1)[b, r])
        do = op.reshape(shape[0], 2, -1)[b, :, r].astype(np.float64) - ot.reshape(shape[0], 2, -1)[b, :, r].astype(np.float64)
        want = cases.CENTER_WEIGHT * dc * dc + cases.OFFSET_WEIGHT * np.abs(do).sum() / 2
        assert abs(v.item() - want) <= VALUE_TOL * want, (k, pixel, v.item(), want)
        assert int((gc != 0).sum()) == 1 and int((go != 0).sum()) == 2, (k, pixel)
        got = gc.reshape(shape[0], -1)[b, r].item()
        assert abs(got - cases.CENTER_WEIGHT * 2 * dc) <= 4 * GRAD_FLOOR * abs(cases.CENTER_WEIGHT * 2 * dc), (k, got)
        assert np.array_equal(go.reshape(shape[0], 2, -1)[b, :, r].cpu().numpy(), (np.sign(do) * np.float32(cases.OFFSET_WEIGHT / 2)).astype(np.float32))


def test_loss_bits_run_to_run_misaligned_and_in_a_graph():
    for shape in ((2, 8, 64), (1, 257, 1024)):
        host = cases.loss_inputs(shape)
        arrays = [dev(a) for a in host]
        first = _fused(arrays, True, True, "pixel")
        assert all(torch.equal(a, b) for a, b in zip(first, _fused(arrays, True, True, "pixel")))
        shifted = []
        for a in arrays:
            buf = torch.zeros(a.numel() + 1, device=DEV)
            view = buf[1:].view(a.shape)
            view.copy_(a)
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            shifted.append(view)
        assert all(torch.equal(a, b) for a, b in zip(first, _fused(shifted, True, True, "pixel")))
    # a graph over forward and backward
    static = [a.clone() for a in arrays]
    step = lambda: _fused(static, True, True, "pixel")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    other = [dev(a) for a in cases.loss_inputs(shape, seed=5200)]
    want_other = _fused(other, True, True, "pixel")
    for src, want in ((other, want_other), (arrays, first)):
        with torch.no_grad():
            for s, a in zip(static, src):
                s.copy_(a)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured, want))
    assert not torch.equal(first[0], want_other[0])


def test_classes_end_to_end_and_what_takes_the_stock_chain():
    host = cases.loss_inputs((2, 37, 53))
    cp, ct, cm, op, ot, om = [dev(a) for a in host]
    targets = {"center": ct, "offset": ot, "center_mask": cm, "offset_mask": om}
    for masking in ("reference", "pixel"):
        res = []
        for backend in ("hip", "torch"):
            p = {"center": cp.clone().requires_grad_(True), "offset": op.clone().requires_grad_(True)}
            v = ca.DeeplabPanopticLoss(weight=0.5, masking=masking, backend=backend)(p, targets)
            v.backward()
            res.append((v.item(), p["center"].grad, p["offset"].grad))
        assert abs(res[0][0] - res[1][0]) <= 2 * VALUE_TOL * abs(res[1][0])
        assert l2_err(res[0][1].cpu().numpy(), res[1][1].cpu().numpy()) <= 1e-5 and l2_err(res[0][2].cpu().numpy(), res[1][2].cpu().numpy()) <= 1e-5
    preds = {"center": cp, "offset": op}
    fused = ca.deeplab_panoptic_loss(preds, targets)
    # 64-bit, 16-bit and CPU tensors: the stock chain
    v64 = ca.deeplab_panoptic_loss({k: v.double() for k, v in preds.items()}, {k: v.double() for k, v in targets.items()})
    assert v64.dtype == torch.float64 and abs(float(v64) - float(fused)) <= VALUE_TOL * float(fused)
    assert ca.deeplab_panoptic_loss({k: v.half() for k, v in preds.items()}, {k: v.half() for k, v in targets.items()}).dtype == torch.float16
    cpu = ca.deeplab_panoptic_loss({k: v.cpu() for k, v in preds.items()}, {k: v.cpu() for k, v in targets.items()})
    assert cpu.device.type == "cpu" and abs(float(cpu) - float(fused)) <= 2 * VALUE_TOL * float(fused)
    # a target that asks for a gradient: the stock chain, and it gets one
    tg = dict(targets, center=ct.clone().requires_grad_(True))
    assert float(torch.autograd.grad(ca.deeplab_panoptic_loss(preds, tg), tg["center"])[0].abs().sum()) > 0
    with pytest.raises(RuntimeError, match="no gradient for a target or a mask"):
        loss, _ = torch.ops.cerberus.panoptic_loss(cp.clone().requires_grad_(True), tg["center"], cm, op, ot, om, 1.0, 1.0, 0)
        torch.autograd.grad(loss, tg["center"])
    # what the raw op refuses
    op_ = torch.ops.cerberus.panoptic_loss
    with pytest.raises(RuntimeError, match="float32"):
        op_(cp.half(), ct, cm, op, ot, om, 1.0, 1.0, 0)
    with pytest.raises(RuntimeError, match="offset_mask must be"):
        op_(cp, ct, cm, op, ot, om[:, None], 1.0, 1.0, 0)
    with pytest.raises(RuntimeError, match="mode must be"):
        op_(cp, ct, cm, op, ot, om, 1.0, 1.0, 2)
    loss, state = op_(cp.clone().requires_grad_(True), ct, cm, op.clone().requires_grad_(True), ot, om, 1.0, 1.0, 0)
    with pytest.raises(RuntimeError, match="no double backward"):
        x = cp.clone().requires_grad_(True)
        gc, _ = torch.ops.cerberus.panoptic_loss_backward(x, ct, cm, op, ot, om, state, loss.detach(), 0)
        gc.sum().backward()
