#!/usr/bin/env python3
"""Times the DETR set criterion, eager forward + backward on one GPU: the fused route (``DetrLoss(backend='hip')``: one
cerberus_detr::hungarian_match launch, one set_loss launch with its finish, one backward launch; csrc/detr_loss.hip) against the
reference's route written out here -- per decoder layer: the cost matrix in stock ops, ``.cpu()``, scipy's linear_sum_assignment per
image, index tensors from Python lists, cross_entropy / l1_loss / generalized_box_iou on the gathered pairs, ``num_boxes`` through
``.item()`` -- in the same process.  The comparison does not go through the package's own ``backend='torch'``.

    python tools/prof_detr_loss.py [--out profiles/detr_loss_fused.txt] [--passes 9]

Shape: the reference's DetrSegmHead, B = 4 images, Q = 100 queries, C1 = 20 classes (19 + no-object), 20..60 targets per image, with
L = 6 decoder layers (the main output and 5 auxiliary ones) and with L = 1.
Method (that of tools/prof_ocr_head.py): every call of a timed pass works on its own copy of the inputs (8 copies: the data is a few
hundred KiB, the cost is launches and host work, so nothing here is a cache effect), 3 warm-up passes, HIP events around a whole pass,
fused and stock passes alternating; the median over the passes with the smallest and the largest pass beside it.  Each L runs in a
child process under a time limit of its own; the first failure ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, Q, C1 = 4, 100, 20
COUNTS = (20, 33, 47, 60)
LAYERS = (6, 1)
COPIES = 8
LIMIT = 300
COST = {"cost_class": 1.0, "cost_bbox": 5.0, "cost_giou": 2.0}


def _time(forms, passes):
    """{label: (median, min, max) seconds per call}: forms = {label: [one closure per input copy]}, alternating pass by pass."""
    import torch
    for _ in range(3):
        for fns in forms.values():
            for fn in fns:
                fn()
    torch.cuda.synchronize()
    times = {label: [] for label in forms}
    for _ in range(passes):
        for label, fns in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for fn in fns:
                fn()
            b.record()
            torch.cuda.synchronize()
            times[label].append(a.elapsed_time(b) * 1e-3 / len(fns))
    return {label: (statistics.median(v), min(v), max(v)) for label, v in times.items()}


def _weight_dict(L):
    d = {"loss_ce": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0}
    for i in range(L - 1):
        d.update({"loss_ce_%d" % i: 1.0, "loss_bbox_%d" % i: 5.0, "loss_giou_%d" % i: 2.0})
    return d


def _inputs(L, seed, dev):
    import numpy as np
    import torch
    from cerberusnet_amd.synth import hash_uniform

    def boxes(shape, s):
        return np.concatenate([hash_uniform(shape + (2,), s, 0.1, 0.9), hash_uniform(shape + (2,), s + 1, 0.02, 0.32)], axis=-1)
    layers = [{"logits": torch.from_numpy(hash_uniform((B, Q, C1), seed + 10 * l, -3.0, 3.0)).to(dev).requires_grad_(True),
               "bboxes": torch.from_numpy(boxes((B, Q), seed + 10 * l + 1)).to(dev).requires_grad_(True)} for l in range(L)]
    targets = {"labels": [torch.from_numpy(np.floor(hash_uniform((n,), seed + 100 + b, 0.0, C1 - 1.0)).astype(np.int64).clip(0, C1 - 2)).to(dev)
                          for b, n in enumerate(COUNTS)],
               "bboxes": [torch.from_numpy(boxes((n,), seed + 200 + b)).to(dev) for b, n in enumerate(COUNTS)]}
    return layers, targets


def reference_route(solver):
    """The reference's DetrLoss.forward with its HungarianMatcher, restated in stock ops (what the reference executes per step)."""
    import torch
    import torch.nn.functional as F
    from cerberusnet_amd.nnet_models.detr.box_ops import box_cxcywh_to_xyxy, generalized_box_iou
    weight_cache = {}

    def matcher(outputs, targets):
        bs, nq = outputs["logits"].shape[:2]
        out_prob = outputs["logits"].flatten(0, 1).softmax(-1)
        out_bbox = outputs["bboxes"].flatten(0, 1)
        tgt_ids = torch.cat(targets["labels"]).type(torch.int64).to(out_prob.device)
        tgt_bbox = torch.cat(targets["bboxes"]).type(torch.float32).to(out_prob.device)
        cost = (COST["cost_bbox"] * torch.cdist(out_bbox, tgt_bbox, p=1) + COST["cost_class"] * -out_prob[:, tgt_ids]
                + COST["cost_giou"] * -generalized_box_iou(box_cxcywh_to_xyxy(out_bbox), box_cxcywh_to_xyxy(tgt_bbox)))
        cost = cost.view(bs, nq, -1).cpu()
        sizes = [len(v) for v in targets["bboxes"]]
        indices = [solver(c[i]) for i, c in enumerate(cost.split(sizes, -1))]
        return [(torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)) for i, j in indices]

    def terms(outputs, targets, indices, num_boxes, empty_weight):
        logits = outputs["logits"]
        batch_idx = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)])
        src_idx = torch.cat([src for (src, _) in indices])
        classes_o = torch.cat([t[J] for t, (_, J) in zip(targets["labels"], indices)])
        classes = torch.full(logits.shape[:2], C1 - 1, dtype=torch.int64, device=logits.device)
        classes[(batch_idx, src_idx)] = classes_o
        loss_ce = F.cross_entropy(logits.transpose(1, 2), classes, empty_weight)
        src_boxes = outputs["bboxes"][(batch_idx, src_idx)]
        tgt_boxes = torch.cat([t[i] for t, (_, i) in zip(targets["bboxes"], indices)], dim=0)
        loss_bbox = F.l1_loss(src_boxes, tgt_boxes, reduction="none").sum() / num_boxes
        loss_giou = (1 - torch.diag(generalized_box_iou(box_cxcywh_to_xyxy(src_boxes), box_cxcywh_to_xyxy(tgt_boxes)))).sum() / num_boxes
        return {"loss_ce": loss_ce, "loss_bbox": loss_bbox, "loss_giou": loss_giou}

    def forward(layers, targets, weight_dict):
        dev = layers[0]["logits"].device
        if dev not in weight_cache:
            w = torch.ones(C1, device=dev)
            w[-1] = 0.1
            weight_cache[dev] = w
        num_boxes = torch.as_tensor([sum(len(t) for t in targets["labels"])], dtype=torch.float, device=dev)
        num_boxes = torch.clamp(num_boxes, min=1).item()
        losses = {}
        for layer, outputs in enumerate(layers):
            indices = matcher({k: v.detach() for k, v in outputs.items()}, targets)
            for k, v in terms(outputs, targets, indices, num_boxes, weight_cache[dev]).items():
                losses[k if layer == 0 else "%s_%d" % (k, layer - 1)] = v
        return sum(losses[k] * weight_dict[k] for k in losses if k in weight_dict)
    return forward


def section(L, passes):
    import torch
    import cerberusnet_amd as ca
    try:
        from scipy.optimize import linear_sum_assignment
        solver, solver_name = (lambda c: linear_sum_assignment(c)), "scipy"
    except ImportError:
        from cerberusnet_amd.nnet_models.detr.matcher import _lsap_host
        solver, solver_name = (lambda c: _lsap_host(c.numpy())), "the package's numpy solver (scipy is not installed)"
    dev = torch.device("cuda", 0)
    weight_dict = _weight_dict(L)
    fused = ca.DetrLoss(C1 - 1, weight_dict, 0.1, ["labels", "boxes"], backend="hip", matcher_cfg=COST).to(dev)
    stock = reference_route(solver)
    sets = [_inputs(L, 1000 * (i + 1), dev) for i in range(COPIES)]

    def leaves(layers):
        return [t for o in layers for t in (o["logits"], o["bboxes"])]

    def run_fused(layers, targets):
        torch.autograd.grad(fused(dict(layers[0], aux_outputs=layers[1:]), targets), leaves(layers))

    def run_stock(layers, targets):
        torch.autograd.grad(stock(layers, targets, weight_dict), leaves(layers))
    a = float(fused(dict(sets[0][0][0], aux_outputs=sets[0][0][1:]), sets[0][1]))
    b = float(stock(sets[0][0], sets[0][1], weight_dict))
    res = _time({"fused": [lambda s=s: run_fused(*s) for s in sets], "stock": [lambda s=s: run_stock(*s) for s in sets]}, passes)
    rec = {"L": L, "solver": solver_name, "value_fused": a, "value_stock": b}
    for label, (med, lo, hi) in res.items():
        rec[label + "_us"] = [med * 1e6, lo * 1e6, hi * 1e6]
    print("ROW " + json.dumps(rec), flush=True)


def table(rows):
    out = ["DETR set criterion, eager forward + backward, fp32: fused (DetrLoss(backend='hip')) against the reference's route in stock ops",
           "with a host solver, in one process (us per call: median [smallest .. largest pass]; x = stock / fused)",
           "B = %d, Q = %d, C1 = %d, targets per image %s; host solver: %s" % (B, Q, C1, COUNTS, rows[0]["solver"] if rows else "-"), ""]
    for r in rows:
        s, f = r["stock_us"], r["fused_us"]
        out.append("  L = %d   stock %9.1f [%9.1f .. %9.1f]   fused %9.1f [%9.1f .. %9.1f]   x %6.2f   (loss: fused %.6f, stock %.6f)"
                   % (r["L"], s[0], s[1], s[2], f[0], f[1], f[2], s[0] / f[0], r["value_fused"], r["value_stock"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", type=int)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detr_loss_fused.txt"))
    ap.add_argument("--passes", type=int, default=9)
    args = ap.parse_args()
    if args.section is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_detr_loss: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.passes)
    rows = []
    for L in LAYERS:
        cmd = [sys.executable, os.path.abspath(__file__), "--section", str(L), "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_detr_loss: L = %d exceeded %d s; stopping" % (L, LIMIT))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_detr_loss: L = %d failed (%d); stopping" % (L, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
