"""CPU tests of the panoptic training side (cerberusnet_amd/utilities/panoptic_targets.py, loss_functions/panoptic_loss.py,
csrc/panoptic_train.hip): the stock routes against results of the reference's own code (tests/golden/panoptic_train.npz,
written by tools/gen_golden_panoptic_train.py), and the op / C-ABI layer as far as it goes without a GPU.

Targets are compared BIT FOR BIT (an integer model: integer sums, one float64 division per centre, one float64 subtraction
rounded to float32 per pixel, a table look-up for the heat map).  The loss: value within 1e-5 relative (the VALUE_TOL of
tests/test_depth_loss_gpu.py), gradient ``l2_err`` within 1e-5."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import panoptic_train_cases as cases
from cerberusnet_amd import _lib, build as cbuild, loss_functions as L, ops, utilities as U
from cerberusnet_amd.loss_functions import panoptic_loss as PL
from cerberusnet_amd.utilities.panoptic_targets import PanopticTargetGenerator, gaussian_table, panoptic_targets
from conftest import l2_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_TOL = 1e-5
GRAD_TOL = 1e-5


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def tensors(name):
    ids, sid, cat, crowd, count, _segs, kwargs = cases.target_case(name)
    return [torch.from_numpy(a) for a in (ids, sid, cat, crowd, count)], kwargs


# ---- targets ----------------------------------------------------------------------------------------------------------------
def test_golden_file_is_small_and_recorded_with_numpy_2(golden):
    g = golden("panoptic_train")
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "panoptic_train.npz")) < 300 * 1024
    assert str(g["numpy_version"]).startswith("2.")          # the offsets are float64 subtractions rounded once: numpy 2's rule
    big = g["tgt_big_center"][0, 0]
    assert big[0, :].max() > 0 and big[-1, :].max() > 0 and big[:, 0].max() > 0 and big[:, -1].max() > 0     # clipped on four borders
    assert np.isnan(g["tgt_big_points"][0, 4]).all() and np.isnan(g["tgt_big_points"][0, 0]).all()           # absent id; stuff
    assert set(np.unique(g["tgt_big_semantic_mask"])) == {1.0, 3.0} and (g["tgt_big_semantic_mask"] == 3).sum() == cases.SMALL_AREA - 1
    assert (g["tgt_big_s2_center"] == 0).mean() > 0.5        # sigma 2: most pixels lie outside every window


@pytest.mark.parametrize("name", list(cases.TARGET_CASES))
@pytest.mark.parametrize("id_dtype", [torch.int64, torch.int32])
def test_stock_route_reproduces_the_reference_bit_for_bit(golden, name, id_dtype):
    g = golden("panoptic_train")
    (ids, *tables), kwargs = tensors(name)
    out = panoptic_targets(ids.to(id_dtype), *tables, backend="torch", **kwargs)
    assert list(out) == cases.ITEMS + ["center_points"]
    for item in cases.ITEMS:
        assert bits_equal(out[item].numpy(), g["tgt_%s_%s" % (name, item)]), (name, item)
    assert bits_equal(out["center_points"].numpy(), g["tgt_%s_points" % name]), name
    # CPU tensors take the stock route whatever the backend
    hip = panoptic_targets(ids, *tables, backend="hip", **kwargs)
    assert all(torch.equal(hip[k], out[k]) for k in cases.ITEMS)


def test_more_rows_than_the_fused_limit_give_the_same_bits(golden):
    g = golden("panoptic_train")
    ids, sid, cat, crowd, count, kwargs = cases.widened("vector", ops.PANOPTIC_TARGETS_MAX_SEGMENTS + 1)
    out = panoptic_targets(*[torch.from_numpy(a) for a in (ids, sid, cat, crowd, count)], backend="torch", **kwargs)
    for item in cases.ITEMS:
        assert bits_equal(out[item].numpy(), g["tgt_vector_%s" % item]), item
    n = g["tgt_vector_points"].shape[1]
    assert bits_equal(out["center_points"].numpy()[:, -n:], g["tgt_vector_points"])
    assert np.isnan(out["center_points"].numpy()[:, :-n]).all()


def test_seg_count_defaults_to_every_row():
    (ids, sid, cat, crowd, count), kwargs = tensors("big")
    a = panoptic_targets(ids, sid, cat, crowd, None, backend="torch", **kwargs)
    b = panoptic_targets(ids, sid, cat, crowd, count, backend="torch", **kwargs)
    assert all(torch.equal(a[k], b[k]) for k in cases.ITEMS)


def test_generator_call_is_a_drop_in(golden):
    g = golden("panoptic_train")
    ids, _sid, _cat, _crowd, _count, segs, kwargs = cases.target_case("big")
    gen = PanopticTargetGenerator(backend="torch", **kwargs)
    assert gen.generated_items == cases.ITEMS and gen.device.type == "cpu"
    out = gen(cases.colour(ids[0]), segs[0])
    for item in cases.ITEMS:
        assert bits_equal(out[item].numpy(), g["tgt_big_%s" % item]), item
    assert isinstance(out["center_points"], list) and bits_equal(np.asarray(out["center_points"]), g["call_big_points"])
    # uint8 colours, a colour triple, and an image without segments
    rgb = np.zeros((4, 6, 3), dtype=np.uint8)
    rgb[1:3, 2:5] = (232, 3, 1)
    assert gen.rgb2id((232, 3, 1)) == 232 + 3 * 256 + 65536 and int(gen.rgb2id(rgb)[1, 2]) == 232 + 3 * 256 + 65536
    none = gen(rgb, [])
    assert none["center_points"] == [] and int((none["semantic"] != cases.IGNORE).sum()) == 0 and float(none["center"].max()) == 0
    one = gen(rgb, [{"id": 232 + 3 * 256 + 65536, "category_id": 11, "iscrowd": 0}])
    assert one["center_points"] == [[1.5, 3.0]] and float(one["center"][0, 0, 1, 3]) == 1.0
    names = ["ignore_label", "thing_list", "sigma", "ignore_stuff_in_offset", "small_instance_area", "small_instance_weight",
             "ignore_crowd_in_semantic", "backend", "device"]
    assert list(inspect.signature(PanopticTargetGenerator.__init__).parameters)[1:] == names


def test_gaussian_table_is_the_references_formula_rounded_once():
    for sigma in (1, 2, 8):
        size = 6 * sigma + 3
        x = np.arange(size, dtype=np.float64)
        want = np.exp(-((x[None] - 3 * sigma - 1) ** 2 + (x[:, None] - 3 * sigma - 1) ** 2) / (2 * sigma ** 2)).astype(np.float32)
        assert bits_equal(gaussian_table(sigma).numpy(), want)
    assert gaussian_table(8) is gaussian_table(8)            # made once


def test_target_arguments_are_rejected():
    (ids, sid, cat, crowd, count), kwargs = tensors("tiny")
    for sigma in (2.5, 0, -1, True):
        with pytest.raises(ValueError, match="sigma must be a positive integer"):
            panoptic_targets(ids, sid, cat, crowd, count, **dict(kwargs, sigma=sigma))
    with pytest.raises(ValueError, match="sigma must be a positive integer"):
        PanopticTargetGenerator(255, cases.THINGS, sigma=1.5)
    with pytest.raises(ValueError, match="backend"):
        panoptic_targets(ids, sid, cat, crowd, count, backend="numpy", **kwargs)
    with pytest.raises(ValueError, match="int32 or int64"):
        panoptic_targets(ids.float(), sid, cat, crowd, count, **kwargs)
    with pytest.raises(ValueError, match=r"\(B,S\)"):
        panoptic_targets(ids, sid[0], cat, crowd, count, **kwargs)
    with pytest.raises(ValueError, match="seg_count"):
        panoptic_targets(ids, sid, cat, crowd, count[None], **kwargs)
    assert panoptic_targets(ids, sid, cat, crowd, count, sigma=2.0, **{k: v for k, v in kwargs.items() if k != "sigma"})["center"].shape == (1, 1, 5, 7)


# ---- the loss -------------------------------------------------------------------------------------------------------------------
def _dicts(arrays, with_c, with_o, grad=True):
    cp, ct, cm, op, ot, om = (torch.from_numpy(a.copy()) for a in arrays)
    p = {"center": cp.requires_grad_(grad), "offset": op.requires_grad_(grad)}
    t = {"center": ct, "offset": ot}
    if with_c:
        t["center_mask"] = cm
    if with_o:
        t["offset_mask"] = om
    return p, t


@pytest.mark.parametrize("with_c,with_o", cases.MASK_COMBOS)
def test_stock_chain_reproduces_the_reference(golden, with_c, with_o):
    g = golden("panoptic_train")
    tag = "%d%d" % (with_c, with_o)
    p, t = _dicts(cases.loss_inputs(cases.GOLDEN_LOSS_SHAPE), with_c, with_o)
    crit = ca.DeeplabPanopticLoss(center_weight=cases.CENTER_WEIGHT, offset_weight=cases.OFFSET_WEIGHT, backend="torch")
    v = crit(p, t)
    gc, go = torch.autograd.grad(v, (p["center"], p["offset"]))
    want = float(g["loss_%s" % tag])
    print("reference %s: %.7f stock %.7f" % (tag, want, float(v.detach())))
    assert abs(float(v.detach()) - want) <= VALUE_TOL * abs(want)
    assert l2_err(gc.numpy(), g["loss_%s_gc" % tag]) <= GRAD_TOL and l2_err(go.numpy(), g["loss_%s_go" % tag]) <= GRAD_TOL


def test_stock_chain_with_empty_masks_reproduces_the_reference(golden):
    g = golden("panoptic_train")
    arrays = list(cases.loss_inputs(cases.GOLDEN_LOSS_SHAPE))
    for tag, empty in (("empty", (2, 5)), ("empty_center", (2,))):
        arr = [np.zeros_like(a) if i in empty else a for i, a in enumerate(arrays)]
        for masking in PL.MASKINGS:
            p, t = _dicts(arr, True, True)
            v = ca.deeplab_panoptic_loss(p, t, cases.CENTER_WEIGHT, cases.OFFSET_WEIGHT, masking, backend="torch")
            gc, go = torch.autograd.grad(v, (p["center"], p["offset"]))
            assert float(gc.abs().max()) == 0.0 and (tag == "empty_center" or float(go.abs().max()) == 0.0)
            if masking == "reference":
                want = float(g["loss_%s" % tag])
                got = float(v.detach())
                assert (got == 0.0) if want == 0.0 else (abs(got - want) <= VALUE_TOL * abs(want))
                assert l2_err(go.numpy(), g["loss_%s_go" % tag]) <= GRAD_TOL
            elif tag == "empty":
                assert float(v.detach()) == 0.0


def test_reference_masking_is_the_unmasked_mean_behind_a_gate(golden):
    g = golden("panoptic_train")
    assert len({float(g["loss_%d%d" % combo]) for combo in cases.MASK_COMBOS}) <= 2          # the masks change a rounding at most
    assert abs(float(g["loss_11"]) - float(g["loss_00"])) <= 1e-5 * float(g["loss_00"])


@pytest.mark.parametrize("with_c,with_o", cases.MASK_COMBOS)
@pytest.mark.parametrize("masking", ["reference", "pixel"])
def test_stock_chain_against_float64(with_c, with_o, masking):
    arrays = cases.loss_inputs((2, 37, 53))
    p, t = _dicts(arrays, with_c, with_o)
    v = ca.deeplab_panoptic_loss(p, t, cases.CENTER_WEIGHT, cases.OFFSET_WEIGHT, masking, backend="torch")
    gc, go = torch.autograd.grad(v, (p["center"], p["offset"]))
    cp, ct, cm, op, ot, om = arrays
    ref, rc_, ro = cases.loss64(cp, ct, cm if with_c else None, op, ot, om if with_o else None, cases.CENTER_WEIGHT,
                                cases.OFFSET_WEIGHT, masking)
    assert abs(float(v) - ref) <= VALUE_TOL * abs(ref)
    assert l2_err(gc.numpy(), rc_) <= GRAD_TOL and l2_err(go.numpy(), ro) <= GRAD_TOL
    if masking == "pixel" and with_o:
        assert float(go[:, 0][torch.from_numpy(om) == 0].abs().max()) == 0.0


def test_pixel_masking_skips_what_lies_under_a_zero_weight():
    arrays = [a.copy() for a in cases.loss_inputs((2, 5, 7))]
    clean = ca.deeplab_panoptic_loss(*_dicts(arrays, True, True, grad=False), masking="pixel", backend="torch")
    arrays[0][:, 0][arrays[2] == 0] = np.nan
    arrays[3][:, 1][arrays[5] == 0] = np.nan
    p, t = _dicts(arrays, True, True)
    v = ca.deeplab_panoptic_loss(p, t, masking="pixel", backend="torch")
    gc, go = torch.autograd.grad(v, (p["center"], p["offset"]))
    assert torch.equal(v.detach(), clean) and not torch.isnan(gc).any() and not torch.isnan(go).any()
    assert torch.isnan(ca.deeplab_panoptic_loss(*_dicts(arrays, True, True, grad=False), masking="reference", backend="torch"))


def test_loss_classes_and_arguments():
    crit = ca.DeeplabPanopticLoss()
    assert (crit.weight, crit.center_weight, crit.offset_weight, crit.masking, crit.backend) == (1.0, 200., .1, "reference", "hip")
    assert list(inspect.signature(ca.DeeplabPanopticLoss.__init__).parameters)[1:] == ["weight", "ignore_index", "masking", "backend", "kwargs"]
    assert list(inspect.signature(ca.deeplab_panoptic_loss).parameters)[:5] == ["predictions", "targets", "center_weight", "offset_weight", "masking"]
    p, t = _dicts(cases.loss_inputs((2, 5, 7)), True, True, grad=False)
    half = ca.DeeplabPanopticLoss(weight=0.5, center_weight=3.0, offset_weight=2.0)(p, t)
    full = ca.deeplab_panoptic_loss(p, t, 3.0, 2.0)
    assert torch.equal(half, 0.5 * full)                      # CPU tensors: the stock chain on either backend
    with pytest.raises(ValueError, match="masking"):
        ca.DeeplabPanopticLoss(masking="mean")
    with pytest.raises(ValueError, match="backend"):
        ca.deeplab_panoptic_loss(p, t, backend="numpy")


def test_tier_table_reaches_every_finish_step():
    reached = set().union(*[cases.loss_tiers(s) for s in cases.LOSS_TIER_SHAPES])
    assert [t for t in cases.LOSS_TIERS if t not in reached] == []
    assert cases.loss_tiers((1, 257, 1024)) == {"ploss_final second step, vector", "ploss_final third step, vector"}
    for shape in cases.LOSS_SHAPES_SCALAR + cases.LOSS_SHAPES_VECTOR:
        assert cases.loss_tiers(shape) == set()                # every thread of the finish reads at most one partial there
    assert all(s[1] * s[2] % 4 != 0 for s in cases.LOSS_SHAPES_SCALAR) and all(s[1] * s[2] % 4 == 0 for s in cases.LOSS_SHAPES_VECTOR)
    assert cases.LOSS_CHUNK == ops.PANOPTIC_CHUNK_PIXELS
    with open(os.path.join(REPO, "cerberusnet_amd", "csrc", "panoptic_train.hip")) as f:
        src = f.read()
    assert "constexpr int kChunk = kThreads * kQuad;" in src and "constexpr int kThreads = kReduceThreads;" in src
    assert "constexpr int kMaxSegments = %d;" % ops.PANOPTIC_TARGETS_MAX_SEGMENTS in src
    assert "for (int i = threadIdx.x; i < n; i += kThreads) a += p[i];" in src
    with open(os.path.join(REPO, "cerberusnet_amd", "csrc", "loss_reduce.h")) as f:
        assert "constexpr int kReduceThreads = %d;" % cases.FINISH_THREADS in f.read()


# ---- ops, bindings, the C ABI ------------------------------------------------------------------------------------------------------
def test_schemas():
    s = lambda name: str(getattr(torch.ops.cerberus, name).default._schema)
    assert s("panoptic_targets") == (
        "cerberus::panoptic_targets(Tensor ids, Tensor seg_ids, Tensor seg_category, Tensor seg_flags, Tensor seg_count, Tensor gauss, "
        "int ignore_label, int sigma, bool ignore_stuff_in_offset, int small_instance_area, float small_instance_weight, "
        "bool ignore_crowd_in_semantic) -> (Tensor semantic, Tensor foreground, Tensor center, Tensor offset, Tensor semantic_mask, "
        "Tensor center_mask, Tensor offset_mask, Tensor center_points)")
    assert s("panoptic_loss") == (
        "cerberus::panoptic_loss(Tensor center_pred, Tensor center_tgt, Tensor? center_mask, Tensor offset_pred, Tensor offset_tgt, "
        "Tensor? offset_mask, float center_weight, float offset_weight, int mode) -> (Tensor loss, Tensor state)")
    assert s("panoptic_loss_backward") == (
        "cerberus::panoptic_loss_backward(Tensor center_pred, Tensor center_tgt, Tensor? center_mask, Tensor offset_pred, "
        "Tensor offset_tgt, Tensor? offset_mask, Tensor state, Tensor grad_loss, int mode) -> (Tensor grad_center, Tensor grad_offset)")
    assert ops.PANOPTIC_LOSS_MODES == {"reference": 0, "pixel": 1}


def test_meta_shapes_and_cpu_rejection():
    m = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="meta")
    out = torch.ops.cerberus.panoptic_targets(m((2, 9, 11), torch.int32), m((2, 5), torch.int64), m((2, 5), torch.int64), m((2, 5), torch.int32),
                                              m((2,), torch.int64), m((51, 51), torch.float32), 255, 8, False, 0, 1.0, False)
    shapes = [(2, 9, 11), (2, 9, 11), (2, 1, 9, 11), (2, 2, 9, 11), (2, 9, 11), (2, 9, 11), (2, 9, 11), (2, 5, 2)]
    dtypes = [torch.int64, torch.int64] + [torch.float32] * 5 + [torch.float64]
    assert [tuple(o.shape) for o in out] == shapes and [o.dtype for o in out] == dtypes
    f = lambda shape: m(shape, torch.float32)
    loss, state = torch.ops.cerberus.panoptic_loss(f((2, 1, 9, 11)), f((2, 1, 9, 11)), None, f((2, 2, 9, 11)), f((2, 2, 9, 11)), f((2, 9, 11)),
                                                   200.0, 0.1, 1)
    assert loss.shape == () and state.shape == (2,)
    gc, go = torch.ops.cerberus.panoptic_loss_backward(f((2, 1, 9, 11)), f((2, 1, 9, 11)), None, f((2, 2, 9, 11)), f((2, 2, 9, 11)), None,
                                                       state, loss, 0)
    assert gc.shape == (2, 1, 9, 11) and go.shape == (2, 2, 9, 11)
    c = lambda shape: torch.zeros(shape)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.panoptic_loss(c((1, 1, 2, 2)), c((1, 1, 2, 2)), None, c((1, 2, 2, 2)), c((1, 2, 2, 2)), None, 1.0, 1.0, 0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.panoptic_loss_backward(c((1, 1, 2, 2)), c((1, 1, 2, 2)), None, c((1, 2, 2, 2)), c((1, 2, 2, 2)), None, c((2,)),
                                                  c(()), 0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.panoptic_targets(torch.zeros((1, 2, 2), dtype=torch.int64), torch.zeros((1, 1), dtype=torch.int64),
                                            torch.zeros((1, 1), dtype=torch.int64), torch.zeros((1, 1), dtype=torch.int32),
                                            torch.zeros((1,), dtype=torch.int64), torch.zeros((51, 51)), 255, 8, False, 0, 1.0, False)


def test_workspace_twins():
    lib = _lib.get()
    assert lib.cerberus_panoptic_targets_max_segments() == ops.PANOPTIC_TARGETS_MAX_SEGMENTS == 256
    for shape in [(1, 5, 7, 1), (2, 37, 53, 4), (2, 8, 64, 256), (4, 512, 1024, 60), (1, 2048, 2048, 2), (1, 5, 7, 257), (0, 5, 7, 1),
                  (1, 5, 7, 0), (65536, 1, 1, 1), (1, 46341, 46341, 1)]:
        assert ops._panoptic_targets_workspace_bytes(*shape) == lib.cerberus_panoptic_targets_workspace_bytes(*shape), shape
    assert ops._panoptic_targets_workspace_bytes(1, 5, 7, 1) == 44 + 144 and ops._panoptic_targets_workspace_bytes(1, 5, 7, 257) == 0
    for shape in [(1, 1, 1), (2, 37, 53), (1, 257, 1024), (1, 601, 1023), (4, 512, 1024), (0, 5, 7), (1, 32768, 32768)]:
        assert ops._panoptic_loss_workspace_bytes(*shape) == lib.cerberus_panoptic_loss_workspace_bytes(*shape), shape
    assert ops._panoptic_loss_workspace_bytes(1, 257, 1024) == 3 * (257 + 514) * 4 and ops._panoptic_loss_workspace_bytes(1, 32768, 32768) == 0


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _lib.get()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    tgt = lambda ptr, ws, ws_bytes, B, H, W, S, sigma, kind=1: lib.cerberus_panoptic_targets(
        ptr, kind, *[ptr] * 13, ws, ws_bytes, B, H, W, S, sigma, 255, 0, 0, 1.0, 0, None)
    invalid, dtype_err, unsupported, too_large = -1, -2, -5, -6       # CERB_EINVAL, CERB_EDTYPE, CERB_EUNSUPPORTED, CERB_ETOOLARGE
    assert tgt(p, p, 4096, 1, 2, 2, 257, 8) == unsupported and tgt(None, p, 4096, 1, 2, 2, 1, 8) == invalid
    assert tgt(p, p, 4096, 1, 2, 2, 1, 0) == invalid and tgt(p, p, 4096, 1, 0, 2, 1, 8) == invalid and tgt(p, p, 4096, 1, 2, 2, 1, 8, 2) == invalid
    assert tgt(p, p + 4, 4096, 1, 2, 2, 1, 8) == invalid and tgt(p, p, 8, 1, 2, 2, 1, 8) == invalid
    assert tgt(p, p, 4096, 65536, 2, 2, 1, 8) == too_large and tgt(p, p, 4096, 1, 46341, 46341, 1, 8) == too_large
    assert tgt(None, None, 0, 0, 2, 2, 1, 8) == 0                                                # B == 0: nothing to do
    fwd = lambda ptr, ws, ws_bytes, B, H, W, mode, dtype: lib.cerberus_panoptic_loss_forward(
        ptr, ptr, None, ptr, ptr, None, ptr, ptr, ws, ws_bytes, B, H, W, 200.0, 0.1, mode, dtype, None)
    bwd = lambda ptr, B, H, W, mode, dtype: lib.cerberus_panoptic_loss_backward(ptr, ptr, None, ptr, ptr, None, ptr, ptr, ptr, ptr, B, H, W,
                                                                               mode, dtype, None)
    assert fwd(None, p, 4096, 1, 2, 2, 0, 0) == invalid and fwd(p, p, 4096, 1, 2, 2, 2, 0) == invalid and fwd(p, p, 4, 1, 2, 2, 0, 0) == invalid
    assert fwd(p, p, 4096, 1, 2, 2, 0, 1) == unsupported and fwd(p, p, 4096, 1, 2, 2, 0, 9) == dtype_err
    assert fwd(None, None, 0, 0, 2, 2, 0, 0) == 0 and bwd(None, 0, 2, 2, 1, 0) == 0
    assert bwd(None, 1, 2, 2, 0, 0) == invalid and bwd(p, 1, 2, 2, 3, 0) == invalid and bwd(p, 1, 2, 2, 0, 2) == unsupported
    assert fwd(p, p, 4096, 1, 32768, 32768, 0, 0) == too_large


def test_header_binding_and_exports():
    with open(os.path.join(REPO, "include", "cerberus_hip.h")) as f:
        header = f.read()
    names = ["cerberus_panoptic_targets_max_segments", "cerberus_panoptic_targets_workspace_bytes", "cerberus_panoptic_targets",
             "cerberus_panoptic_loss_workspace_bytes", "cerberus_panoptic_loss_forward", "cerberus_panoptic_loss_backward"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in zip(names, (0, 4, 28, 3, 18, 16)):
        assert re.search(r"\b%s\(" % name, header) and hasattr(lib, name), name
        assert len(_lib.PROTOTYPES[name][1]) == nargs, name
        decl = re.search(r"^(?:int|int64_t) %s\(([^;]*)\);" % name, header, re.M).group(1)
        assert (0 if decl.strip() == "void" else decl.count(",") + 1) == nargs, name
    assert re.search(r"#define CERBERUS_HIP_ABI_VERSION 7\b", header) and _lib.ABI_VERSION == 7
    assert "panoptic_train.hip" in cbuild.SOURCES and "panoptic_train.hip" in cbuild.EXPERIMENT_SOURCES
    for mod in (L, ca):
        assert {"deeplab_panoptic_loss", "DeeplabPanopticLoss"} <= set(mod.__all__)
    for mod in (U, ca):
        assert {"panoptic_targets", "PanopticTargetGenerator"} <= set(mod.__all__)
    assert PL.__all__ == ["deeplab_panoptic_loss", "DeeplabPanopticLoss"]
    assert ca.DeeplabPanopticLoss is L.DeeplabPanopticLoss is PL.DeeplabPanopticLoss and ca.panoptic_targets is U.panoptic_targets
    assert U.PanopticTargetGenerator is PanopticTargetGenerator
