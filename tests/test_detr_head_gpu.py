"""The DETR head on the GPU (nnet_models/detr): ``DetrSegmHead(backend='hip')`` -- stock ops around the fused
attention core of csrc/detr_attn.hip -- against the same module in float64 on the CPU.

The config (tests/attn_cases.py): d_model 64, 2 heads of width 32, feed-forward 64, 2 + 2 layers, 10 queries, a 2 x 24 x 9 x 13 feature
map: 117 pixels (encoder self-attention: 3 tiles of 32 + 21 keys, one workgroup of 128 queries), 10 queries (decoder self-attention:
less than a tile; cross-attention: 10 queries on 117 keys).

The bound.  ``backend='torch'`` runs on the GPU in the same test; its own error against float64 is ``e_stock``, and every output, the
input gradient and every parameter gradient of the fused route must have ``l2_err`` and ``rel_err`` of at most
``4 x max(e_stock, 2^-23)`` (tests/ocr_cases.bound).  A parameter gradient that is zero in exact arithmetic has no norm to divide by
(post-norm: the first decoder layer's self-attention sees values that are all zero, so its in_proj_weight receives nothing; float64
leaves rounding of 1e-9 of the largest gradient entry or less there): its largest entry must be at most 4 x max(the stock route's
largest entry, 2^-23 x the largest entry of any parameter gradient).

Measured on an MI355X (this file's own prints; fused / stock fp32 / bound, the entry of each kind nearest its bound): post-norm logits
5.0e-7 / 4.7e-7 / 1.9e-6, boxes 1.0e-7 / 1.0e-7 / 4.8e-7, input gradient 4.4e-7 / 4.8e-7 / 1.9e-6, parameter gradients 1.9e-7 / 1.0e-7 /
4.8e-7 (encoder.layers.0.norm2.weight); pre-norm logits 4.1e-7 / 4.4e-7 / 1.8e-6, auxiliary logits 5.0e-7 / 4.3e-7 / 1.7e-6, input
gradient 3.4e-7 / 3.0e-7 / 1.2e-6, parameter gradients 2.6e-7 / 8.6e-8 / 4.8e-7 (encoder.layers.1.self_attn.in_proj_bias); the zero
gradient (post-norm decoder.layers.0.self_attn.in_proj_weight) 2.1e-12 fused, 6.0e-13 stock, of a largest entry of 2.0.
Train mode under a fixed seed, two identical steps: in one session 1 of 76 tensors differed in bits, input_proj.weight's gradient, with
backend='hip' and with backend='torch' alike, in eval mode too (MIOpen's weight gradient of the 1x1 convolution; four pairs of
steps per backend, every pair); in another session no tensor differed with either backend.  q, k, v, out
and the four gradients of all six attention calls (117 x 117, 10 x 10 and 10 x 117 at B = 2, H = 2) have equal bits.
"""
import functools

import pytest
import torch

import attn_cases as cases
import cerberusnet_amd as ca
import detr_cases as dcase
from cerberusnet_amd import ops_attn
from conftest import l2_err, rel_err
from op_cases import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_head(head, x):
    """Every output, the input gradient and every parameter gradient of ``head_loss``, as float64 CPU tensors, by name."""
    x = x.clone().requires_grad_(True)
    out = head(x)
    cases.head_loss(out).backward()
    res = {"logits": out["logits"], "bboxes": out["bboxes"], "aux_logits": out["aux_outputs"][0]["logits"],
           "aux_bboxes": out["aux_outputs"][0]["bboxes"], "grad_input": x.grad}
    res.update({"grad " + n: p.grad for n, p in head.named_parameters()})
    return {k: v.detach().double().cpu() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def reference(pre):
    return run_head(cases.make_head(ca.DetrSegmHead, pre, backend="torch").double(), cases.features().double())


@pytest.mark.parametrize("pre", [False, True], ids=["post-norm", "pre-norm"])
def test_eval_head_matches_float64_within_the_stock_routes_error(pre):
    ref = reference(pre)
    x = cases.features().to(DEV)
    got = run_head(cases.make_head(ca.DetrSegmHead, pre, backend="hip").to(DEV), x)
    stock = run_head(cases.make_head(ca.DetrSegmHead, pre, backend="torch").to(DEV), x)
    assert list(got) == list(ref) == list(stock) and len(ref) > 60
    failed, worst = [], {}
    gmax = max(float(r.abs().max()) for n, r in ref.items() if n.startswith("grad "))
    for name, r in ref.items():
        g, s = got[name], stock[name]
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), name
        if float(r.abs().max()) <= 1e-9 * gmax:         # a gradient that is zero but for rounding: no norm to divide by
            e, e_stock = float(g.abs().max()), float(s.abs().max())
            print("head %s: zero in float64 (%.1e); fused %.3e stock fp32 %.3e of a largest gradient entry of %.3e" % (
                name, float(r.abs().max()), e, e_stock, gmax))
            if not e <= 4.0 * max(e_stock, cases.FLOOR * gmax):
                failed.append((name, "zero", e, e_stock))
            continue
        for metric in (l2_err, rel_err):
            e, e_stock = metric(g.numpy(), r.numpy()), metric(s.numpy(), r.numpy())
            kind = ("grad_param " if name.startswith("grad ") else name + " ") + metric.__name__
            if kind not in worst or e / cases.bound(e_stock) > worst[kind][0] / cases.bound(worst[kind][1]):
                worst[kind] = (e, e_stock, name)
            if not e <= cases.bound(e_stock):
                failed.append((name, metric.__name__, e, e_stock))
    for kind, (e, e_stock, name) in worst.items():
        print("head %s %s: fused %.3e stock fp32 %.3e (bound %.3e) [%s]" % ("pre-norm" if pre else "post-norm", kind, e, e_stock,
                                                                          cases.bound(e_stock), name))
    assert not failed, failed


def test_the_hip_backend_takes_the_fused_core_and_the_torch_backend_does_not(monkeypatch):
    seen = []
    real = ops_attn.detr_attention
    monkeypatch.setattr(ops_attn, "detr_attention", lambda *a, **k: (seen.append(tuple(a[0].shape)), real(*a, **k))[1])
    x = cases.features().to(DEV)
    with torch.no_grad():
        cases.make_head(ca.DetrSegmHead, backend="torch").to(DEV)(x)
        assert seen == []
        cases.make_head(ca.DetrSegmHead, backend="hip").to(DEV)(x)
        # 2 encoder layers on 117 pixels, then self- and cross-attention of 10 queries in each of 2 decoder layers
        assert seen == [(117, 2, 64)] * 2 + [(10, 2, 64)] * 4
        seen.clear()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            cases.make_head(ca.DetrSegmHead, backend="hip").to(DEV)(x)
        assert seen == []


def _train_step(head, x, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    head.zero_grad()
    xg = x.clone().requires_grad_(True)
    out = head(xg)
    cases.head_loss(out).backward()
    return [out["logits"].detach(), out["bboxes"].detach(), xg.grad] + [p.grad.clone() for p in head.parameters()]


STEP_NAMES = ["logits", "bboxes", "grad_input"]
# The one tensor of a step that the stock kernels do not reproduce bit for bit: the weight gradient of the head's 1x1 convolution
# (MIOpen).  It differs between two identical steps with backend='torch' as well, in train and in eval mode, and nothing else does.
STOCK_NOT_REPRODUCIBLE = {"input_proj.weight"}


def _differing(head, a, b):
    names = STEP_NAMES + [n for n, _ in head.named_parameters()]
    assert len(names) == len(a) == len(b)
    return [n for n, u, v in zip(names, a, b) if not same_bits(u, v)]


def test_train_mode_with_attention_dropout_live(monkeypatch):
    drawn = []
    real = ops_attn.draw_seed
    monkeypatch.setattr(ops_attn, "draw_seed", lambda device: (drawn.append(real(device)), drawn[-1])[1])
    head = cases.make_head(ca.DetrSegmHead, backend="hip").to(DEV).train()
    assert all(m.dropout == 0.1 for m in head.modules() if isinstance(m, torch.nn.MultiheadAttention))
    x = cases.features().to(DEV)
    first = _train_step(head, x)
    second = _train_step(head, x)
    for t in first + second:
        assert bool(torch.isfinite(t).all())
    seeds = [int(s.item()) for s in drawn]
    assert len(seeds) == 12 and len(set(seeds)) == 12                 # 6 attention calls per step, a seed of its own each
    assert not same_bits(first[0], second[0])
    # a fixed seed reproduces the bits: the six attention seeds, what every attention call reads and returns, forward and backward,
    # the outputs, the input gradient and every parameter gradient but STOCK_NOT_REPRODUCIBLE
    calls = []
    attention = ops_attn.detr_attention

    def recording(q, k, v, *args, **kwargs):
        out = attention(q, k, v, *args, **kwargs)
        rec = {"q": q.detach().clone(), "k": k.detach().clone(), "v": v.detach().clone(), "out": out.detach().clone()}
        for name, t in (("grad_q", q), ("grad_k", k), ("grad_v", v), ("grad_out", out)):
            if t.requires_grad:
                t.register_hook(lambda g, name=name, rec=rec: rec.__setitem__(name, g.detach().clone()))
        calls.append(rec)
        return out
    monkeypatch.setattr(ops_attn, "detr_attention", recording)
    drawn.clear()
    a, b = _train_step(head, x, seed=7), _train_step(head, x, seed=7)
    seeds = [int(s.item()) for s in drawn]
    assert seeds[:6] == seeds[6:] and len(set(seeds[:6])) == 6
    assert len(calls) == 12
    for i, (ra, rb) in enumerate(zip(calls[:6], calls[6:])):
        assert set(ra) == set(rb) == {"q", "k", "v", "out", "grad_q", "grad_k", "grad_v", "grad_out"}, i
        for key in ra:
            assert same_bits(ra[key], rb[key]), (i, key, tuple(ra["q"].shape), tuple(ra["k"].shape))
    differ = _differing(head, a, b)
    print("train mode, fixed seed, backend='hip': tensors that differ in bits between two steps: %s" % differ)
    assert set(differ) <= STOCK_NOT_REPRODUCIBLE, differ
    w = STEP_NAMES + [n for n, _ in head.named_parameters()]
    for n in STOCK_NOT_REPRODUCIBLE:
        u, v = a[w.index(n)], b[w.index(n)]
        assert float((u - v).abs().max()) <= 1e-5 * float(u.abs().max()), n
    # the control: the same two steps without the fused core
    stock = cases.make_head(ca.DetrSegmHead, backend="torch").to(DEV).train()
    control = _differing(stock, _train_step(stock, x, seed=7), _train_step(stock, x, seed=7))
    print("train mode, fixed seed, backend='torch': tensors that differ in bits between two steps: %s" % control)
    assert set(control) <= STOCK_NOT_REPRODUCIBLE, control
    assert not same_bits(a[0], _train_step(head, x, seed=8)[0])
    # eval mode draws nothing
    drawn.clear()
    with torch.no_grad():
        head.eval()(x)
    assert drawn == []


def test_the_fused_criterion_runs_on_the_heads_outputs():
    head = cases.make_head(ca.DetrSegmHead, backend="hip").to(DEV)
    out = head(cases.features().to(DEV))
    weights = {"loss_ce": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0, "loss_ce_0": 1.0, "loss_bbox_0": 5.0, "loss_giou_0": 2.0}
    crit = ca.DetrLoss(cases.HEAD["num_classes"], weights, 0.1, ["labels", "boxes", "cardinality"], backend="hip",
                       matcher_cfg={"cost_class": 1.0, "cost_bbox": 5.0, "cost_giou": 2.0}).to(DEV)
    targets = {"labels": [torch.tensor([1, 3, 0], device=DEV), torch.tensor([2], device=DEV)],
               "bboxes": [torch.from_numpy(dcase.make_boxes((3,), 11)).to(DEV), torch.from_numpy(dcase.make_boxes((1,), 12)).to(DEV)]}
    loss = crit(out, targets)
    loss = sum(loss.values()) if isinstance(loss, dict) else loss
    assert bool(torch.isfinite(loss))
    loss.backward()
    for name, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
