"""The DETR set loss without a GPU: the bundled host solver against brute force (and scipy), the stock-op route of the matcher and
the criterion against the float64 restatement of tests/detr_cases.py, the reference's output formats and names, and the C ABI's
argument checks and helpers."""
import os
import re

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import detr_cases as dcase
from cerberusnet_amd import _lib, build, ops_detr
from cerberusnet_amd.nnet_models.detr import box_ops
from cerberusnet_amd.nnet_models.detr.matcher import HungarianMatcher, _lsap_host, pad_targets
from cerberusnet_amd.synth import hash_uniform
from conftest import REPO

SIZES = [(r, c) for r in range(1, 8) for c in range(1, 8)]


# ---- 1. the host solver -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr,nc", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_lsap_host_equals_brute_force(nr, nc):
    assert (3, 5) in SIZES and (5, 3) in SIZES
    for k, cost in enumerate((hash_uniform((nr, nc), 100 * nr + nc, 0.0, 1.0).astype(np.float64),
                              np.floor(hash_uniform((nr, nc), 200 * nr + nc, 0.0, 4.0)).astype(np.float64),        # massive ties
                              np.outer(np.arange(1, nr + 1), np.arange(1, nc + 1)).astype(np.float64))):
        i, j = _lsap_host(cost)
        assert i.dtype == np.int64 and j.dtype == np.int64 and len(i) == len(j) == min(nr, nc)
        assert (np.diff(i) > 0).all() and len(set(j.tolist())) == len(j) and (j >= 0).all() and (j < nc).all()
        assert abs(cost[i, j].sum() - dcase.brute_force(cost)) <= 1e-12 * max(1.0, abs(cost[i, j].sum())), (k, nr, nc)


def test_lsap_host_edge_cases():
    i, j = _lsap_host(np.zeros((4, 0)))
    assert len(i) == 0 and len(j) == 0
    with pytest.raises(ValueError):
        _lsap_host(np.array([[1.0, np.nan]]))
    perm = np.array([3, 0, 4, 1, 2])
    cost = np.ones((5, 5))
    cost[np.arange(5), perm] = 0.0
    i, j = _lsap_host(cost)
    assert (i == np.arange(5)).all() and (j == perm).all()


def test_lsap_host_equals_scipy_total():
    scipy_optimize = pytest.importorskip("scipy.optimize")
    for k, shape in enumerate([(100, 37), (37, 100), (130, 126), (64, 64), (7, 3)]):
        for cost in (hash_uniform(shape, 300 + k, -5.0, 11.0).astype(np.float64), np.floor(hash_uniform(shape, 400 + k, 0.0, 4.0)).astype(np.float64)):
            i, j = _lsap_host(cost)
            a, b = scipy_optimize.linear_sum_assignment(cost)
            assert len(i) == len(a) and abs(cost[i, j].sum() - cost[a, b].sum()) <= 1e-12 * max(1.0, abs(cost[a, b].sum())), shape


# ---- 2. the stock-op route against the float64 restatement ------------------------------------------------------------------------
def _reference_targets(c):
    labels = [torch.from_numpy(c["tgt_labels"][b, :n]) for b, n in enumerate(c["counts"])]
    boxes = [torch.from_numpy(c["tgt_boxes"][b, :n]) for b, n in enumerate(c["counts"])]
    return {"labels": labels, "bboxes": boxes}


def _layers(c, requires_grad=False):
    B = c["B"]
    logits = torch.from_numpy(c["logits"]).requires_grad_(requires_grad)
    boxes = torch.from_numpy(c["boxes"]).requires_grad_(requires_grad)
    layers = [{"logits": logits[l * B:(l + 1) * B], "bboxes": boxes[l * B:(l + 1) * B]} for l in range(c["L"])]
    return logits, boxes, layers


def _match_of(indices, Q):
    m = np.full(Q, -1, dtype=np.int64)
    m[indices[0].numpy()] = indices[1].numpy()
    return m


@pytest.mark.parametrize("name", ["3x5_swapped", "7x7", "100x37", "batch_0_Tmax_1", "layers_3x2"])
def test_torch_matcher_is_optimal_for_the_float64_cost(name):
    c = dcase.case(name)
    matcher = HungarianMatcher(dcase.W_CLASS, dcase.W_BBOX, dcase.W_GIOU, backend="torch")
    cost64 = dcase.cost_matrix(c).numpy()
    _, _, layers = _layers(c)
    for l, outputs in enumerate(layers):
        indices = matcher(outputs, _reference_targets(c))
        assert len(indices) == c["B"]
        for b, (i, j) in enumerate(indices):
            n, T = l * c["B"] + b, c["counts"][b]
            assert i.dtype == torch.int64 and j.dtype == torch.int64 and i.device.type == "cpu"
            assert len(i) == len(j) == min(c["Q"], T) and bool((i[1:] > i[:-1]).all())
            dcase.check_matching(_match_of((i, j), c["Q"]), c["Q"], T)
            ri, rj = _lsap_host(cost64[n, :, :T])
            got, want = float(cost64[n][i.numpy(), j.numpy()].sum()), float(cost64[n, :, :T][ri, rj].sum())
            # the route solves its own float32 matrix: its total on the float64 matrix is within the float32 chain's error per pair
            assert abs(got - want) <= 1e-5 * max(1, len(i)), (name, n, got, want)


def test_matcher_output_format_with_an_empty_image_and_more_targets_than_queries():
    c = dcase.make_case(1, 3, 4, 5, (0, 6, 2), 6100)
    _, _, layers = _layers(c)
    for scipy_on in (True, False):
        matcher = HungarianMatcher(backend="torch")
        if not scipy_on:
            import cerberusnet_amd.nnet_models.detr.matcher as mod
            saved, mod._scipy_lsap = mod._scipy_lsap, None
        try:
            out = matcher(layers[0], _reference_targets(c))
        finally:
            if not scipy_on:
                mod._scipy_lsap = saved
        assert [len(i) for i, _ in out] == [0, 4, 2]
        assert all(i.dtype == torch.int64 and j.dtype == torch.int64 and i.dim() == 1 for i, j in out)
        assert out[1][0].tolist() == [0, 1, 2, 3] and len(set(out[1][1].tolist())) == 4 and max(out[1][1].tolist()) < 6
    assert matcher({"logits": layers[0]["logits"], "bboxes": layers[0]["bboxes"]},
                   {"labels": [torch.zeros(0, dtype=torch.int64)] * 3, "bboxes": [torch.zeros(0, 4)] * 3})[0][0].numel() == 0
    with pytest.raises(AssertionError):
        HungarianMatcher(0, 0, 0)


def test_pad_targets():
    c = dcase.make_case(1, 3, 4, 5, (0, 6, 2), 6100)
    t = _reference_targets(c)
    labels, boxes, count = pad_targets(t["labels"], t["bboxes"], "cpu")
    assert labels.dtype == torch.int64 and boxes.dtype == torch.float32 and count.dtype == torch.int32
    assert torch.equal(labels, torch.from_numpy(c["tgt_labels"])) and torch.equal(boxes, torch.from_numpy(c["tgt_boxes"]))
    assert count.tolist() == [0, 6, 2]
    labels, boxes, count = pad_targets([torch.zeros(0)] * 2, [torch.zeros(0, 4)] * 2, "cpu")
    assert labels.shape == (2, 0) and boxes.shape == (2, 0, 4) and count.tolist() == [0, 0]


def _weight_dict(L):
    d = {"loss_ce": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0}
    for i in range(L - 1):
        d.update({"loss_ce_%d" % i: 0.5 + i, "loss_bbox_%d" % i: 4.0 - i, "loss_giou_%d" % i: 1.5 + i})
    return d


def _criterion(c, backend, losses=("labels", "boxes", "cardinality")):
    return ca.DetrLoss(c["C1"] - 1, _weight_dict(c["L"]), dcase.EOS_COEF, list(losses), weight=0.7, backend=backend,
                       matcher_cfg={"cost_class": dcase.W_CLASS, "cost_bbox": dcase.W_BBOX, "cost_giou": dcase.W_GIOU})


@pytest.mark.parametrize("name", ["7x7", "batch_0_Tmax_1", "layers_3x2", "5x0"])
def test_torch_criterion_equals_the_float64_restatement(name):
    c = dcase.case(name)
    crit = _criterion(c, "torch")
    logits, boxes, layers = _layers(c, requires_grad=True)
    predictions = dict(layers[0], aux_outputs=layers[1:]) if c["L"] > 1 else dict(layers[0])
    total = crit(predictions, _reference_targets(c))
    gl, gb = torch.autograd.grad(total, [logits, boxes], allow_unused=True)
    # the restatement, at the assignment the route itself found
    match = np.stack([_match_of(ij, c["Q"]) for outputs in layers for ij in crit.matcher(outputs, _reference_targets(c))])
    wd = _weight_dict(c["L"])
    up = np.array([[wd["loss_ce" + s], wd["loss_bbox" + s], wd["loss_giou" + s], 0.0]
                   for s in [""] + ["_%d" % i for i in range(c["L"] - 1)]]) * 0.7
    losses, rl, rb = dcase.loss_and_grads(c, match, up, torch.float64)
    want = float((losses * torch.from_numpy(up)).sum())
    assert abs(float(total.detach()) - want) <= 2e-6 * max(1.0, abs(want)), (float(total.detach()), want)
    assert float((gl.double() - rl).abs().max()) <= 2e-6 * max(1.0, float(rl.abs().max()))
    if gb is not None:
        assert float((gb.double() - rb).abs().max()) <= 2e-6 * max(1.0, float(rb.abs().max()))


# ---- 3. the criterion's surface -----------------------------------------------------------------------------------------------------
def test_detr_loss_keys_weights_and_state_dict():
    c = dcase.case("layers_3x2")
    crit = _criterion(c, "hip")
    state = crit.state_dict()
    assert list(state) == ["empty_weight"] and state["empty_weight"].shape == (c["C1"],)
    assert float(state["empty_weight"][-1]) == pytest.approx(dcase.EOS_COEF) and bool((state["empty_weight"][:-1] == 1).all())
    assert isinstance(crit.matcher, HungarianMatcher) and crit.matcher.backend == "hip"
    assert (crit.matcher.cost_class, crit.matcher.cost_bbox, crit.matcher.cost_giou) == (dcase.W_CLASS, dcase.W_BBOX, dcase.W_GIOU)
    coef = crit._coefficients(3, "cpu")
    wd = _weight_dict(3)
    assert coef.tolist() == [[wd["loss_ce"], wd["loss_bbox"], wd["loss_giou"], 0.0],
                             [wd["loss_ce_0"], wd["loss_bbox_0"], wd["loss_giou_0"], 0.0],
                             [wd["loss_ce_1"], wd["loss_bbox_1"], wd["loss_giou_1"], 0.0]]
    # a loss that is not requested contributes nothing even where the weight_dict names it
    assert _criterion(c, "hip", losses=("labels",))._coefficients(1, "cpu").tolist() == [[1.0, 0.0, 0.0, 0.0]]
    # CPU tensors take the stock-op route under backend='hip' as well
    _, _, layers = _layers(c)
    predictions = dict(layers[0], aux_outputs=layers[1:])
    assert torch.equal(crit(predictions, _reference_targets(c)), _criterion(c, "torch")(predictions, _reference_targets(c)))
    import inspect
    assert list(inspect.signature(ca.DetrLoss.__init__).parameters)[1:6] == ["num_classes", "weight_dict", "eos_coef", "losses", "weight"]
    assert list(inspect.signature(HungarianMatcher.__init__).parameters)[1:4] == ["cost_class", "cost_bbox", "cost_giou"]
    from cerberusnet_amd import loss_functions
    assert loss_functions.DetrLoss is ca.DetrLoss and loss_functions.detr_set_loss is ca.detr_set_loss


def test_masks_raise():
    with pytest.raises(NotImplementedError):
        ca.DetrLoss(5, {}, 0.1, ["labels", "masks"], matcher_cfg={})
    with pytest.raises(ValueError):
        ca.DetrLoss(5, {}, 0.1, ["labels"], backend="triton", matcher_cfg={})


def test_box_ops():
    b = torch.from_numpy(dcase.make_boxes((6,), 7000))
    assert torch.allclose(box_ops.box_xyxy_to_cxcywh(box_ops.box_cxcywh_to_xyxy(b)), b, atol=1e-6)
    xy = box_ops.box_cxcywh_to_xyxy(b)
    iou, union = box_ops.box_iou(xy, xy)
    assert iou.shape == union.shape == (6, 6) and torch.allclose(iou.diag(), torch.ones(6), atol=1e-6)
    g = box_ops.generalized_box_iou(xy[:3], xy)
    want = dcase.giou_pairs(b[:3, None, :].double(), b[None, :, :].double())
    assert g.shape == (3, 6) and float((g.double() - want).abs().max()) < 1e-5 and bool((g >= -1).all()) and bool((g <= 1 + 1e-6).all())


# ---- 4. the C ABI without a GPU -----------------------------------------------------------------------------------------------------
def test_limit_and_workspace_helpers_agree_with_the_library():
    lib = _lib.get()
    for Q in (-1, 0, 1, 100, 128, 129, 130, 256, 257):
        for T in (-1, 0, 1, 64, 65, 126, 127, 128, 129):
            for C1 in (1, 2, 20, 256, 257):
                assert bool(lib.cerberus_detr_fused_ok(Q, T, C1)) == bool(ops_detr._detr_fused_ok(Q, T, C1)), (Q, T, C1)
    assert lib.cerberus_detr_fused_ok(130, 126, 20) == 1 and lib.cerberus_detr_fused_ok(256, 64, 20) == 1
    assert lib.cerberus_detr_fused_ok(131, 126, 20) == 0 and lib.cerberus_detr_fused_ok(256, 65, 20) == 0
    for N in (-1, 0, 1, 24, 1000):
        assert lib.cerberus_detr_workspace_bytes(N) == ops_detr._detr_workspace_bytes(N), N


def test_argument_rejection_without_gpu():
    lib = _lib.get()
    ok = (4, 2, 100, 20, 37)            # N, B, Q, C1, Tmax
    w = (1.0, 5.0, 2.0)

    def match_cost(N, B, Q, C1, T, dtype=0, ptr=None):
        return lib.cerberus_detr_match_cost(ptr, ptr, ptr, ptr, ptr, ptr, None, N, B, Q, C1, T, *w, dtype, None)

    def hungarian(N, B, Q, C1, T, dtype=0):
        return lib.cerberus_detr_hungarian_match(None, None, None, None, None, None, None, N, B, Q, C1, T, *w, dtype, None)

    def forward(N, B, Q, C1, T, dtype=0):
        return lib.cerberus_detr_set_loss_forward(*([None] * 11), 0, N, B, Q, C1, T, dtype, None)

    def backward(N, B, Q, C1, T, dtype=0):
        return lib.cerberus_detr_set_loss_backward(*([None] * 12), N, B, Q, C1, T, dtype, None)

    for fn in (match_cost, hungarian, forward, backward):
        assert fn(*ok) == -1                                 # null pointers
        assert fn(*ok, dtype=9) == -2 and fn(*ok, dtype=1) == -5
        assert fn(3, 2, 100, 20, 37) == -1                   # N % B != 0
        assert fn(4, 2, 257, 20, 37) == -5 and fn(4, 2, 100, 20, 129) == -5 and fn(4, 2, 256, 20, 65) == -5
        assert fn(4, 2, 100, 257, 37) == -5 and fn(4, 2, 100, 1, 37) == -1 and fn(4, 0, 100, 20, 37) == -1
        assert fn(0, 2, 100, 20, 37) == 0                    # N == 0: nothing to do, no launch
    assert lib.cerberus_detr_lsap(None, None, None, None, 4, 2, 100, 37, None) == -1
    assert lib.cerberus_detr_lsap(None, None, None, None, 3, 2, 100, 37, None) == -1
    assert lib.cerberus_detr_lsap(None, None, None, None, 4, 2, 257, 37, None) == -5
    assert lib.cerberus_detr_lsap(None, None, None, None, 0, 2, 100, 37, None) == 0


def test_the_source_is_built_and_the_header_matches_the_prototypes():
    assert "detr_loss.hip" in build.SOURCES and "detr_loss.hip" in build.EXPERIMENT_SOURCES
    text = open(os.path.join(REPO, "include", "cerberus_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(cerberus_detr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(n for n in _lib.PROTOTYPES if n.startswith("cerberus_detr_")) and len(declared) == 7
    for name in declared:                                     # the argument counts agree as well
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len([p for p in params.split(",") if p.strip()]) == len(_lib.PROTOTYPES[name][1]), name
    assert _lib.ABI_VERSION == 7


def test_ops_reject_what_the_fused_route_does_not_take():
    c = dcase.case("7x7")
    x = torch.from_numpy(c["logits"]).to("meta")
    assert not ops_detr.detr_fused_ok(torch.from_numpy(c["logits"]), torch.from_numpy(c["boxes"]), 7)      # CPU tensors
    assert ops_detr._detr_fused_ok(100, 60, 20) and not ops_detr._detr_fused_ok(300, 10, 20)
    assert x.shape == (1, 7, 5)
