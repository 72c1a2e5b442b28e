#!/usr/bin/env python3
"""Times the OHEM cross-entropy: the fused HIP op (cerberus::seg_ohem_cross_entropy) against the stock-op restatement on the
device (``backend='torch'``: softmax, gather, kthvalue, where, F.cross_entropy), the reference-style host route (logits to the
host, a numpy softmax, an argsort of every valid pixel, the target rewritten and copied back, F.cross_entropy on the device; for
the record) and the plain ``seg_cross_entropy`` of the same inputs, one process per shape on one GPU.

    python tools/prof_seg_ohem.py [--out profiles/seg_ohem_fused.txt] [--passes 7]

``SoftmaxCrossEntropyOHEMLoss(ignore_label=255, thresh=0.7, min_kept=100000, use_weight=False)`` on the confident logits of
tests/seg_ohem_cases.py at (4,19,512,1024) and (2,19,256,864), forward + backward per call.
Method (that of tools/prof_seg_loss.py): eager; every call of a timed pass works on its own copy of the inputs, 3 warm-up
passes, device events around a whole pass, the median over `passes` passes, the device forms alternating pass by pass.  The
host route is timed on one copy with the wall clock around a synchronised call, the median of 3.  By bytes the OHEM forward
should cost about (4 C + 28) / (4 C) of the plain one; the measured ratio is reported, not asserted.  Each shape runs in a child
process under a time limit of its own; the first failure ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from prof_photometric import _copies  # noqa: E402
from prof_seg_loss import _time_alternating  # noqa: E402

SHAPES = ((4, 19, 512, 1024), (2, 19, 256, 864))
LIMIT = 420
IGNORE, THRESH, MIN_KEPT = 255, 0.7, 100000


def host_route(x, t):
    """The reference's way, restated: everything between the logits and the rewritten target happens on the host."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    logits = x.detach().cpu().numpy()
    labels = t.cpu().numpy().reshape(-1)
    C = logits.shape[1]
    z = np.moveaxis(logits, 1, 0).reshape(C, -1)
    e = np.exp(z - z.max(axis=0, keepdims=True))
    e /= e.sum(axis=0, keepdims=True)
    where = np.flatnonzero(labels != IGNORE)
    if MIN_KEPT < where.size:
        pred = e[labels[where], where]
        kth = pred[np.argsort(pred)[MIN_KEPT - 1]]
        where = where[pred <= max(kth, THRESH)]
    new = np.full_like(labels, IGNORE)
    new[where] = labels[where]
    loss = F.cross_entropy(x, torch.from_numpy(new.reshape(t.shape)).to(x.device), ignore_index=IGNORE)
    torch.autograd.grad(loss, x)


def section(index, passes):
    import torch
    import cerberusnet_amd as ca
    import seg_ohem_cases as oc
    dev = torch.device("cuda", 0)
    shape = SHAPES[index]
    B, C, H, W = shape
    pixels = B * H * W
    n = _copies(4 * C * pixels)
    sets = [(torch.from_numpy(oc.inputs(shape, i)[0].copy()).to(dev).requires_grad_(True),
             torch.from_numpy(oc.inputs(shape, i)[1].copy()).to(dev)) for i in range(n)]
    kwargs = dict(ignore_label=IGNORE, thresh=THRESH, min_kept=MIN_KEPT, use_weight=False)
    fused, stock = ca.SoftmaxCrossEntropyOHEMLoss(backend="hip", **kwargs), ca.SoftmaxCrossEntropyOHEMLoss(backend="torch", **kwargs)
    forms = {"fused": lambda x, t: torch.autograd.grad(fused(x, t), x),
             "stock": lambda x, t: torch.autograd.grad(stock(x, t), x),
             "plain": lambda x, t: torch.autograd.grad(ca.seg_cross_entropy(x, t, None, IGNORE), x)}

    def fwd_only(fn):
        def call(x, t):
            with torch.no_grad():
                fn(x, t)
        return call
    forms_fwd = {"fused": fwd_only(fused), "stock": fwd_only(stock),
                 "plain": fwd_only(lambda x, t: ca.seg_cross_entropy(x, t, None, IGNORE))}
    stats = ca.seg_ohem_cross_entropy(sets[0][0], sets[0][1], None, IGNORE, THRESH, MIN_KEPT, return_stats=True)
    rec = {"shape": "x".join(map(str, shape)), "copies": n, "threshold": float(stats[1]), "num_valid": int(stats[2]),
           "num_kept": int(stats[3])}
    for what, group in (("fwd", forms_fwd), ("fwd_bwd", forms)):
        res = _time_alternating({label: [lambda fn=fn, x=x, t=t: fn(x, t) for x, t in sets] for label, fn in group.items()}, passes)
        for label, sec in res.items():
            rec["%s_%s_us" % (label, what)] = sec * 1e6
    host = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route(*sets[0])
        torch.cuda.synchronize()
        host.append(time.perf_counter() - t0)
    rec["host_fwd_bwd_us"] = statistics.median(host[1:]) * 1e6
    print("ROW " + json.dumps(rec), flush=True)


def table(rows):
    out = ["SoftmaxCrossEntropyOHEMLoss(ignore_label=255, thresh=0.7, min_kept=100000, use_weight=False), us per call, eager, "
           "median of the passes; plain = seg_cross_entropy of the same inputs; by bytes the OHEM forward is (4 C + 28) / (4 C) = "
           "1.37 of the plain one at C = 19",
           "  %-16s %6s %9s %9s | %9s %9s %9s %6s %6s | %9s %9s %9s %11s %6s" % (
               "shape", "copies", "valid", "kept", "fused fwd", "stock fwd", "plain fwd", "x stk", "/plain", "fused f+b", "stock f+b",
               "plain f+b", "host f+b", "x stk")]
    for r in rows:
        out.append("  %-16s %6d %9d %9d | %9.1f %9.1f %9.1f %6.2f %6.2f | %9.1f %9.1f %9.1f %11.1f %6.2f" % (
            r["shape"], r["copies"], r["num_valid"], r["num_kept"], r["fused_fwd_us"], r["stock_fwd_us"], r["plain_fwd_us"],
            r["stock_fwd_us"] / r["fused_fwd_us"], r["fused_fwd_us"] / r["plain_fwd_us"], r["fused_fwd_bwd_us"],
            r["stock_fwd_bwd_us"], r["plain_fwd_bwd_us"], r["host_fwd_bwd_us"], r["stock_fwd_bwd_us"] / r["fused_fwd_bwd_us"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", type=int)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "seg_ohem_fused.txt"))
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    if args.section is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_seg_ohem: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.passes)
    rows = []
    for index in range(len(SHAPES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", str(index), "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_seg_ohem: shape %s exceeded %d s; stopping" % (SHAPES[index], LIMIT))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_seg_ohem: shape %s failed (%d); stopping" % (SHAPES[index], res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
