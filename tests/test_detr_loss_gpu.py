"""The DETR set loss on the GPU: the three matching entry points, the assignment's optimality, the accuracy of the cost matrix and of
the loss terms and gradients against the float64 restatement of tests/detr_cases.py, padding, non-finite costs, misaligned inputs,
the modules and graph replay.

Bounds.  A device assignment and the host's are both optimal for the SAME float32 numbers (the matrix ``match_cost`` returns, taken to
float64 on the host), so their totals differ by summation order only: 1e-9 max(1, |total|).  Every accuracy bound is 4 x the error of
the stock float32 chain against the same float64 restatement on the same inputs (the margin covers operation order and expf); each
test prints the figures it compares before it asserts."""
import functools

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import detr_cases as dcase
from cerberusnet_amd import ops_detr
from cerberusnet_amd.nnet_models.detr.matcher import HungarianMatcher, _solve_host
from cerberusnet_amd.synth import hash_uniform
from op_cases import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = list(dcase.CASES)
WEIGHTS = (dcase.W_CLASS, dcase.W_BBOX, dcase.W_GIOU)
KEYS = ("logits", "boxes", "tgt_labels", "tgt_boxes", "tgt_count")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def inputs(c):
    return [dev(c[k]) for k in KEYS]


@functools.lru_cache(maxsize=None)
def device_results(name):
    """Everything the matching tests compare, computed once per case: the matrix, both assignments (twice), the status."""
    c = dcase.case(name)
    args = inputs(c)
    cost = ops_detr.match_cost(*args, *WEIGHTS)
    via_lsap = ops_detr.lsap(cost, args[4])
    fused, status = ops_detr.hungarian_match(*args, *WEIGHTS)
    again, status2 = ops_detr.hungarian_match(*args, *WEIGHTS)
    torch.cuda.synchronize()
    return {"c": c, "cost": cost.cpu(), "lsap": via_lsap.cpu(), "lsap2": ops_detr.lsap(cost, args[4]).cpu(), "fused": fused.cpu(),
            "again": again.cpu(), "status": status.cpu(), "status2": status2.cpu(), "cost2": ops_detr.match_cost(*args, *WEIGHTS).cpu()}


def host_total(cost64):
    i, j = _solve_host(cost64)
    return float(cost64[i, j].sum())


def assert_optimal(cost, match, counts, B, what):
    """Every image's assignment is valid and its float64 total on ``cost`` equals the host optimum of the same numbers."""
    cost = np.asarray(cost, dtype=np.float64)
    N, Q, _ = cost.shape
    for n in range(N):
        T = counts[n % B]
        dcase.check_matching(match[n], Q, T)
        got, want = dcase.total_of(cost[n, :, :T], match[n], T), (host_total(cost[n, :, :T]) if T else 0.0)
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (what, n, got, want)


# ---- 1. matching ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_assignment_is_valid_optimal_and_reproducible(name):
    r = device_results(name)
    c = r["c"]
    assert r["cost"].shape == (c["L"] * c["B"], c["Q"], c["Tmax"]) and r["fused"].dtype == torch.int32
    assert_optimal(r["cost"].numpy(), r["fused"].numpy(), c["counts"], c["B"], name)
    assert same_bits(r["fused"], r["lsap"]), "hungarian_match != lsap(match_cost)"
    assert same_bits(r["fused"], r["again"]) and same_bits(r["lsap"], r["lsap2"]) and same_bits(r["cost"], r["cost2"])
    assert same_bits(r["status"], r["status2"]) and not bool(r["status"].any())
    if name == "7x7":
        total = dcase.total_of(r["cost"][0].numpy(), r["fused"][0].numpy(), 7)
        assert abs(total - dcase.brute_force(r["cost"][0].numpy())) <= 1e-9 * max(1.0, abs(total))
    for n in range(c["L"] * c["B"]):                         # padding columns are zeroed
        assert not bool(r["cost"][n, :, c["counts"][n % c["B"]]:].any())


ADVERSARIAL = [(q, t) for q, t in ((1, 1), (3, 5), (7, 7), (100, 37), (130, 126), (256, 64), (64, 128))]


@pytest.mark.parametrize("Q,T", ADVERSARIAL, ids=["%dx%d" % s for s in ADVERSARIAL])
def test_lsap_on_adversarial_matrices(Q, T):
    """Long augmenting paths ((i+1)(j+1)), massive ties (integers 0..3), a unique optimum (a permutation matrix), and a batch whose
    counts stop short of Tmax."""
    i, j = np.arange(Q, dtype=np.float64)[:, None], np.arange(T, dtype=np.float64)[None, :]
    k = min(Q, T)
    unique = np.ones((Q, T))
    if Q <= T:                                               # every query its own target, every pair but these costs 1
        unique[np.arange(Q), np.argsort(hash_uniform((T,), 31 * Q + T))[:Q]] = 0.0
    else:
        unique[np.argsort(hash_uniform((Q,), 31 * Q + T))[:T], np.arange(T)] = 0.0
    stack = np.stack([(i + 1) * (j + 1), np.floor(hash_uniform((Q, T), 17 * Q + T, 0.0, 4.0)).astype(np.float64), unique]).astype(np.float32)
    counts = (T, T, T)
    match = ops_detr.lsap(dev(stack), dev(np.asarray(counts, dtype=np.int32)))
    match2 = ops_detr.lsap(dev(stack), dev(np.asarray(counts, dtype=np.int32)))
    assert same_bits(match, match2)
    m = match.cpu().numpy()
    assert_optimal(stack, m, counts, 3, (Q, T))
    q = np.nonzero(m[2] >= 0)[0]
    assert len(q) == k and (unique[q, m[2][q]] == 0.0).all(), "the unique optimum itself"
    if T > 1:                                                # shorter counts: columns at or past the count are never assigned
        short = (T - 1, 1, 0)
        ms = ops_detr.lsap(dev(stack), dev(np.asarray(short, dtype=np.int32))).cpu().numpy()
        assert_optimal(stack, ms, short, 3, (Q, T, "short"))


@pytest.mark.parametrize("name", [n for n in NAMES if n != "5x0"])
def test_match_cost_accuracy(name):
    r = device_results(name)
    ref = dcase.cost_matrix(r["c"])
    err = float((r["cost"].double() - ref).abs().max())
    stock = float((dcase.stock_cost(r["c"]).double() - ref).abs().max())
    print("match_cost %s: |C| <= %.3g, device error %.3g, stock float32 error %.3g" % (name, float(ref.abs().max()), err, stock))
    assert err <= 4 * stock, (name, err, stock)


@pytest.mark.parametrize("name", ["batch_0_Tmax_1", "layers_3x2", "100x37"])
def test_padding_slots_are_never_read_into_a_result(name):
    r = device_results(name)
    c = dict(r["c"])
    labels, tboxes = c["tgt_labels"].copy(), c["tgt_boxes"].copy()
    for b, n in enumerate(c["counts"]):
        labels[b, n:] = -1
        tboxes[b, n:] = np.nan
    c["tgt_labels"], c["tgt_boxes"] = labels, tboxes
    args = inputs(c)
    assert same_bits(ops_detr.match_cost(*args, *WEIGHTS).cpu(), r["cost"])
    match, status = ops_detr.hungarian_match(*args, *WEIGHTS)
    assert same_bits(match.cpu(), r["fused"]) and not bool(status.any())
    zero, poisoned = loss_on_device(r["c"], r["fused"]), loss_on_device(c, r["fused"])
    for a, b in zip(zero, poisoned):
        assert same_bits(a, b)


def test_a_nan_logit_row_sets_the_status_bit_and_the_matching_stays_valid():
    c = dict(dcase.case("layers_3x2"))
    logits = c["logits"].copy()
    logits[3, 4, 2] = np.nan                                  # image 3 = layer 1, batch row 1
    c["logits"] = logits
    args = inputs(c)
    match, status = ops_detr.hungarian_match(*args, *WEIGHTS)
    cost = ops_detr.match_cost(*args, *WEIGHTS)
    assert same_bits(match, ops_detr.lsap(cost, args[4]))
    assert status.cpu().tolist() == [0, 0, 0, ops_detr.STATUS_NON_FINITE, 0, 0]
    assert bool(torch.isfinite(cost).all()) and float(cost[3, 4, :3].min()) == 1e9 and not bool(cost[3, 4, 3:].any())
    m = match.cpu().numpy()
    for n in range(6):
        dcase.check_matching(m[n], c["Q"], c["counts"][n % 2])
    assert_optimal(cost.cpu().numpy(), m, c["counts"], 2, "nan row")


def test_a_label_outside_the_classes_sets_bit_1_and_counts_as_no_object():
    c = dict(dcase.case("layers_3x2"))
    labels = c["tgt_labels"].copy()
    labels[0, 1] = c["C1"] + 3                                # batch row 0 (5 targets): images 0, 2, 4
    c["tgt_labels"] = labels
    args = inputs(c)
    match, status = ops_detr.hungarian_match(*args, *WEIGHTS)
    cost = ops_detr.match_cost(*args, *WEIGHTS)
    assert status.cpu().tolist() == [ops_detr.STATUS_BAD_LABEL, 0] * 3 and same_bits(match, ops_detr.lsap(cost, args[4]))
    assert bool((cost[0::2, :, 1] == 1e9).all()) and bool((cost[1::2] < 1e3).all())
    m = match.cpu().numpy()
    assert_optimal(cost.cpu().numpy(), m, c["counts"], 2, "bad label")
    as_no_object = dict(c)
    as_no_object["tgt_labels"] = labels.copy()
    as_no_object["tgt_labels"][0, 1] = c["C1"] - 1
    up = dcase.upstream_of(c)
    got = loss_on_device(c, m)
    ref, stock = (dcase.loss_and_grads(as_no_object, m, up, dtype) for dtype in (torch.float64, torch.float32))
    for g, r, s in zip(got, ref, stock):
        err, base = float((g.double() - r).abs().max()), float((s.double() - r).abs().max())
        print("bad label: device error %.3g, stock float32 error %.3g" % (err, base))
        assert err <= 4 * base


# ---- 2. the loss --------------------------------------------------------------------------------------------------------------------
def loss_on_device(c, match, upstream=None, offset=False):
    """(losses, grad_logits, grad_boxes) on the CPU from the ops, at ``match``; ``offset``: boxes and tgt_boxes one element off."""
    x, p, tl, tb, tc = inputs(c)
    if offset:
        p, tb = shifted(p), shifted(tb)
    x, p = x.requires_grad_(True), p.requires_grad_(True)
    losses = ops_detr.set_loss(x, p, dev(np.asarray(match, dtype=np.int32)), tl, tb, tc, dev(c["weight"]), dev(c["num_boxes"]))
    up = dev(dcase.upstream_of(c) if upstream is None else upstream)
    gl, gb = torch.autograd.grad((losses * up).sum(), [x, p])
    return losses.detach().cpu(), gl.cpu(), gb.cpu()


def shifted(t):
    """A contiguous view of ``t``'s values whose storage starts one element past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == t.element_size() % 16 and buf.data_ptr() % 16 == 0
    return view


@pytest.mark.parametrize("name", NAMES)
def test_loss_terms_and_gradients_against_float64(name):
    r = device_results(name)
    c, match = r["c"], r["fused"].numpy()
    up = dcase.upstream_of(c)
    losses, gl, gb = loss_on_device(c, match)
    ref_l, ref_gl, ref_gb = dcase.loss_and_grads(c, match, up, torch.float64)
    stk_l, stk_gl, stk_gb = dcase.loss_and_grads(c, match, up, torch.float32)
    assert losses.shape == (c["L"], 4) and losses.dtype == torch.float32
    for k, term in enumerate(("loss_ce", "loss_bbox", "loss_giou", "cardinality_error")):
        err = float((losses[:, k].double() - ref_l[:, k]).abs().max())
        stock = float((stk_l[:, k].double() - ref_l[:, k]).abs().max())
        print("%s %s: value %.6g, device error %.3g, stock float32 error %.3g" % (name, term, float(ref_l[0, k]), err, stock))
        assert err <= 4 * stock, (name, term, err, stock)
    for what, got, ref, stk in (("grad_logits", gl, ref_gl, stk_gl), ("grad_boxes", gb, ref_gb, stk_gb)):
        err, stock = float((got.double() - ref).abs().max()), float((stk.double() - ref).abs().max())
        print("%s %s: max |g| %.3g, device error %.3g, stock float32 error %.3g" % (name, what, float(ref.abs().max()), err, stock))
        assert err <= 4 * stock, (name, what, err, stock)
    unmatched = torch.from_numpy(match < 0)
    assert not bool(gb[unmatched].any()), "unmatched queries get exact zeros"
    if sum(c["counts"]) == 0:
        assert float(losses[0, 1]) == 0.0 and float(losses[0, 2]) == 0.0 and not bool(gb.any())


def test_all_images_empty():
    c = dcase.make_case(2, 2, 6, 5, (0, 0), 8100)
    assert c["Tmax"] == 0
    x, p, tl, tb, tc = inputs(c)
    match, status = ops_detr.hungarian_match(x, p, tl, tb, tc, *WEIGHTS)
    assert bool((match == -1).all()) and not bool(status.any())
    losses, gl, gb = loss_on_device(c, match.cpu().numpy())
    assert float(losses[:, 1].abs().max()) == 0.0 and float(losses[:, 2].abs().max()) == 0.0 and not bool(gb.any())
    ref_l, ref_gl, _ = dcase.loss_and_grads(c, match.cpu().numpy(), dcase.upstream_of(c), torch.float64)
    assert float((losses.double() - ref_l).abs().max()) <= 1e-6 and float((gl.double() - ref_gl).abs().max()) <= 1e-7


@pytest.mark.parametrize("name", ["layers_3x2", "100x37"])
def test_misaligned_boxes_give_the_same_bits(name):
    r = device_results(name)
    c = r["c"]
    x, p, tl, tb, tc = inputs(c)
    ps, tbs = shifted(p), shifted(tb)
    assert same_bits(ops_detr.match_cost(x, ps, tl, tbs, tc, *WEIGHTS).cpu(), r["cost"])
    match, _ = ops_detr.hungarian_match(x, ps, tl, tbs, tc, *WEIGHTS)
    assert same_bits(match.cpu(), r["fused"])
    for a, b in zip(loss_on_device(c, r["fused"].numpy()), loss_on_device(c, r["fused"].numpy(), offset=True)):
        assert same_bits(a, b)


# ---- 3. the modules ---------------------------------------------------------------------------------------------------------------
def _targets(c, device):
    return {"labels": [torch.from_numpy(c["tgt_labels"][b, :n]).to(device) for b, n in enumerate(c["counts"])],
            "bboxes": [torch.from_numpy(c["tgt_boxes"][b, :n]).to(device) for b, n in enumerate(c["counts"])]}


def _predictions(c, device, dtype=torch.float32):
    B = c["B"]
    logits = torch.from_numpy(c["logits"]).to(device=device, dtype=dtype).requires_grad_(True)
    boxes = torch.from_numpy(c["boxes"]).to(device=device, dtype=dtype).requires_grad_(True)
    layers = [{"logits": logits[l * B:(l + 1) * B], "bboxes": boxes[l * B:(l + 1) * B]} for l in range(c["L"])]
    return logits, boxes, (dict(layers[0], aux_outputs=layers[1:]) if c["L"] > 1 else dict(layers[0]))


def _weight_dict(L):
    d = {"loss_ce": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0}
    for i in range(L - 1):
        d.update({"loss_ce_%d" % i: 0.5 + i, "loss_bbox_%d" % i: 4.0 - i, "loss_giou_%d" % i: 1.5 + i})
    return d


def _criterion(c, backend):
    return ca.DetrLoss(c["C1"] - 1, _weight_dict(c["L"]), dcase.EOS_COEF, ["labels", "boxes", "cardinality"], weight=0.7, backend=backend,
                       matcher_cfg={"cost_class": dcase.W_CLASS, "cost_bbox": dcase.W_BBOX, "cost_giou": dcase.W_GIOU}).to(DEV)


@pytest.mark.parametrize("name", ["layers_3x2", "batch_0_Tmax_1", "100x37"])
def test_matcher_forward_returns_the_reference_format(name):
    r = device_results(name)
    c = r["c"]
    _, _, predictions = _predictions(c, DEV)
    out = HungarianMatcher(*WEIGHTS)(predictions, _targets(c, DEV))
    assert len(out) == c["B"]
    for b, (i, j) in enumerate(out):
        assert i.dtype == torch.int64 and j.dtype == torch.int64 and i.device.type == "cpu" and j.device.type == "cpu"
        m = np.full(c["Q"], -1, dtype=np.int64)
        m[i.numpy()] = j.numpy()
        assert bool((i[1:] > i[:-1]).all()) and (m == r["fused"][b].numpy()).all()
    match, padded, status = HungarianMatcher(*WEIGHTS).match(predictions, _targets(c, DEV), predictions.get("aux_outputs"))
    assert same_bits(match.cpu(), r["fused"]) and status.shape == (c["L"] * c["B"],) and padded[2].tolist() == list(c["counts"])


@pytest.mark.parametrize("name", ["layers_3x2", "batch_0_Tmax_1", "100x37"])
def test_detr_loss_hip_equals_torch_backend(name):
    c = dcase.case(name)
    results = {}
    for backend in ("hip", "torch"):
        logits, boxes, predictions = _predictions(c, DEV)
        total = _criterion(c, backend)(predictions, _targets(c, DEV))
        results[backend] = (total.detach().cpu().double(),) + tuple(g.cpu().double() for g in torch.autograd.grad(total, [logits, boxes]))
    wd = _weight_dict(c["L"])
    up = np.array([[wd["loss_ce" + s], wd["loss_bbox" + s], wd["loss_giou" + s], 0.0] for s in [""] + ["_%d" % i for i in range(c["L"] - 1)]]) * 0.7
    ref_l, ref_gl, ref_gb = dcase.loss_and_grads(c, device_results(name)["fused"].numpy(), up, torch.float64)
    ref = ((ref_l * torch.from_numpy(up)).sum(), ref_gl, ref_gb)
    for what, hip, stock, want in zip(("total", "grad_logits", "grad_boxes"), results["hip"], results["torch"], ref):
        err, base = float((hip - want).abs().max()), float((stock - want).abs().max())
        print("DetrLoss %s %s: hip error %.3g, torch-backend error %.3g" % (name, what, err, base))
        assert err <= 4 * base, (name, what, err, base)


def test_16_bit_and_oversize_inputs_take_the_stock_route():
    c = dcase.case("layers_3x2")
    logits, boxes, predictions = _predictions(c, DEV, torch.bfloat16)
    total = _criterion(c, "hip")(predictions, _targets(c, DEV))
    assert bool(torch.isfinite(total))
    with pytest.raises(RuntimeError, match="float32"):
        ops_detr.hungarian_match(logits.detach(), boxes.detach(), *inputs(c)[2:], *WEIGHTS)
    big = dcase.make_case(1, 1, 300, 4, (2,), 8200)
    out = HungarianMatcher(*WEIGHTS)(_predictions(big, DEV)[2], _targets(big, DEV))
    assert len(out[0][0]) == 2
    with pytest.raises(RuntimeError, match="fused limits"):
        ops_detr.hungarian_match(*inputs(big), *WEIGHTS)
    with pytest.raises(RuntimeError, match="no multiple"):
        ops_detr.hungarian_match(*inputs(c)[:2], *[t[:1].repeat(4, *([1] * (t.dim() - 1))) for t in inputs(c)[2:]], *WEIGHTS)


def test_detr_set_loss_graphed_replay_is_bit_equal_to_eager():
    """Matching, loss and backward captured in ONE graph on a single stream, replayed after the inputs are overwritten in place, with
    an eager call in between: nothing synchronises, and the fixed-order reductions give the eager bits every time."""
    base = dcase.make_case(3, 2, 20, 9, (7, 4), 9000)
    weight, num_boxes = dev(base["weight"]), dev(base["num_boxes"])
    s_x = torch.zeros(base["logits"].shape, device=DEV, requires_grad=True)
    s_p = torch.zeros(base["boxes"].shape, device=DEV, requires_grad=True)
    s_tl, s_tb, s_tc = (torch.zeros_like(t) for t in inputs(base)[2:])

    def step(x, p, tl, tb, tc):
        terms = ca.detr_set_loss(x, p, tl, tb, tc, weight, num_boxes, *WEIGHTS)
        total = terms["loss_ce"] + 5 * terms["loss_bbox"] + 2 * terms["loss_giou_0"] + terms["loss_ce_1"]
        return (total,) + tuple(torch.autograd.grad(total, [x, p]))

    def load(c):
        with torch.no_grad():
            for dst, src in zip((s_x, s_p, s_tl, s_tb, s_tc), inputs(c)):
                dst.copy_(src)

    load(base)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(s_x, s_p, s_tl, s_tb, s_tc)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = step(s_x, s_p, s_tl, s_tb, s_tc)
    for i, counts in enumerate(((7, 4), (2, 7), (0, 7))):
        c = dcase.make_case(3, 2, 20, 9, counts, 9010 + 20 * i)
        assert c["Tmax"] == 7
        load(c)
        graph.replay()
        torch.cuda.synchronize()
        x, p, tl, tb, tc = inputs(c)
        eager = step(x.requires_grad_(True), p.requires_grad_(True), tl, tb, tc)          # the eager call in between
        for a, b in zip(g_out, eager):
            assert same_bits(a.detach(), b.detach()), i
        assert bool(torch.isfinite(g_out[0])) and float(g_out[1].abs().max()) > 0 and float(g_out[2].abs().max()) > 0
