#!/usr/bin/env python3
"""Times the segmentation loss: the stock-op chain (``backend='torch'``: ``unique`` for the dynamic weights, ``F.cross_entropy``,
the focal factor) against the fused HIP ops (``backend='hip'``: cerberus::class_histogram + cerberus::seg_cross_entropy), in
one process per section on one GPU.

    python tools/prof_seg_loss.py [--out profiles/seg_loss_fused.txt] [--passes 7]

For ``FocalLoss2D(gamma=2, ignore_index=-1, dynamic_weights=True, scale_factor=0.125)`` (the reference's Cityscapes
configuration) and plain cross-entropy (``SegCrossEntropy(ignore_index=-1)``) at (4,19,512,1024) and (2,19,1024,2048): forward
and forward + backward of both backends, the algorithmic bytes of the fused op (4 C + 12 per pixel forward: the logits, an
int64 label, lse; 8 C + 12 more for the backward: the logits again, the gradient, the label, lse) over its time as GB/s and
as a share of the 8 TB/s HBM peak, and the peak of ``torch.cuda.max_memory_allocated`` over one forward + backward above what
the inputs hold.
Method (that of tools/prof_photometric.py and prof_census.py): every call of a timed pass works on its own copy of the inputs,
the copies of one pass > 512 MiB in all (inputs come from HBM, not from the Infinity Cache), 3 warm-up passes, HIP events
around a whole pass, the median over `passes` passes, fused and stock passes alternating.  Each section runs in a child process
under a time limit of its own; the first failure ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from prof_photometric import _copies  # noqa: E402

SECTIONS = (("focal", 300), ("ce", 300))
SHAPES = ((4, 19, 512, 1024), (2, 19, 1024, 2048))
HBM_PEAK = 8.0e12


def _time_alternating(forms, passes):
    """median seconds per call of every form: forms = {label: [one closure per input copy]}; a pass calls each closure of
    one form once, and the forms take turns pass by pass"""
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
    return {label: statistics.median(v) for label, v in times.items()}


def section(name, passes):
    import torch
    import cerberusnet_amd as ca
    import seg_loss_cases as cases
    dev = torch.device("cuda", 0)
    cls, kwargs = ((ca.FocalLoss2D, dict(gamma=2.0, ignore_index=-1, dynamic_weights=True, scale_factor=0.125)) if name == "focal"
                   else (ca.SegCrossEntropy, dict(ignore_index=-1)))
    losses = {"fused": cls(backend="hip", **kwargs), "stock": cls(backend="torch", **kwargs)}
    for shape in SHAPES:
        B, C, H, W = shape
        pixels = B * H * W
        n = _copies(4 * C * pixels)
        sets = [(torch.from_numpy(cases.logits(shape, 10 + i)).to(dev).requires_grad_(True),
                 torch.from_numpy(cases.labels(shape, 40 + 2 * i, -1)).to(dev)) for i in range(n)]
        alg = ((4 * C + 12) * pixels, (12 * C + 24) * pixels)
        rec = {"section": name, "shape": "x".join(map(str, shape)), "copies": n, "cold": bool(n * alg[0] >= (512 << 20)),
               "alg_bytes_fwd": alg[0], "alg_bytes_fwd_bwd": alg[1]}

        def fwd(fn, x, t):
            with torch.no_grad():
                fn({"seg": x}, {"seg": t})

        def both(fn, x, t):
            torch.autograd.grad(fn({"seg": x}, {"seg": t}), x)
        for what, call in (("fwd", fwd), ("fwd_bwd", both)):
            res = _time_alternating({label: [lambda fn=fn, x=x, t=t: call(fn, x, t) for x, t in sets]
                                     for label, fn in losses.items()}, passes)
            for label, sec in res.items():
                rec["%s_%s_us" % (label, what)] = sec * 1e6
        for label, fn in losses.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            both(fn, *sets[0])
            torch.cuda.synchronize()
            rec[label + "_peak_mib"] = (torch.cuda.max_memory_allocated() - base) / float(1 << 20)
        print("ROW " + json.dumps(rec), flush=True)
        del sets
        torch.cuda.empty_cache()


def table(rows):
    titles = {"focal": "FocalLoss2D(gamma=2, ignore_index=-1, dynamic_weights=True, scale_factor=0.125)",
              "ce": "SegCrossEntropy(ignore_index=-1): plain cross-entropy"}
    out = []
    for name, _ in SECTIONS:
        out.append("%s (us per call; GB/s = algorithmic bytes of the fused op / its time, %% of the 8 TB/s HBM peak; cold = inputs "
                   "from HBM; peak MiB = max_memory_allocated of one forward + backward above the inputs)" % titles[name])
        out.append("  %-16s %6s %5s | %10s %10s %6s %7s %5s | %10s %10s %6s %7s %5s | %10s %10s" % (
            "shape", "copies", "cold", "stock fwd", "fused fwd", "x", "GB/s", "%", "stock f+b", "fused f+b", "x", "GB/s", "%",
            "stock MiB", "fused MiB"))
        for r in (r for r in rows if r["section"] == name):
            bw = [r["alg_bytes_fwd"] / (r["fused_fwd_us"] * 1e-6), r["alg_bytes_fwd_bwd"] / (r["fused_fwd_bwd_us"] * 1e-6)]
            out.append("  %-16s %6d %5s | %10.1f %10.1f %6.2f %7.0f %5.1f | %10.1f %10.1f %6.2f %7.0f %5.1f | %10.1f %10.1f" % (
                r["shape"], r["copies"], "yes" if r["cold"] else "no",
                r["stock_fwd_us"], r["fused_fwd_us"], r["stock_fwd_us"] / r["fused_fwd_us"], bw[0] / 1e9, 100 * bw[0] / HBM_PEAK,
                r["stock_fwd_bwd_us"], r["fused_fwd_bwd_us"], r["stock_fwd_bwd_us"] / r["fused_fwd_bwd_us"], bw[1] / 1e9,
                100 * bw[1] / HBM_PEAK, r["stock_peak_mib"], r["fused_peak_mib"]))
        out.append("")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "seg_loss_fused.txt"))
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    if args.section:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_seg_loss: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.passes)
    rows = []
    for name, limit in SECTIONS:
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_seg_loss: section %s exceeded %d s; stopping" % (name, limit))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_seg_loss: section %s failed (%d); stopping" % (name, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
