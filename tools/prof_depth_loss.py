#!/usr/bin/env python3
"""Times the supervised depth loss: the stock-op chain (``backend='torch'``: relu, sub, the mask product, abs, max, pow, add,
div, two compares, two casts, two products, add, mean) against the fused HIP op (``backend='hip'``: cerberus::inv_huber), in
one process per section on one GPU.

    python tools/prof_depth_loss.py [--out profiles/depth_loss_fused.txt] [--passes 7]

Section ``single``: ``InvHuberLoss`` at (2,1,256,864) (the output size of the reference's KITTI config), (4,1,512,1024) and
(2,1,1024,2048).  Section ``pyramid``: ``InvHuberLossPyr`` over 4 halving levels from (4,1,512,1024) against a (4,512,1024)
ground truth (the fused op gathers; the stock chain resizes with ``F.interpolate`` per level).  Forward and forward + backward
of both backends, the bytes the fused kernels load and store (16 per pixel forward: prediction and ground truth in each of
the two passes; 12 more for the backward: both again and the gradient) over its time as GB/s and as a share of the 8 TB/s HBM
peak, and the peak of ``torch.cuda.max_memory_allocated`` over one forward + backward above what the inputs hold.
Method (that of tools/prof_seg_loss.py): every call of a timed pass works on its own copy of the inputs, 3 warm-up passes, HIP
events around a whole pass, the median over `passes` passes, fused and stock passes alternating.  The maps are small (8 MB at
4 x 512 x 1024): 16 copies of a set stay below 512 MiB, so the column ``cold`` says whether a pass's inputs can have come
from HBM.  Each section runs in a child process under a time limit of its own; the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from prof_photometric import _copies  # noqa: E402
from prof_seg_loss import _time_alternating  # noqa: E402

SECTIONS = (("single", 300), ("pyramid", 300))
SHAPES = ((2, 1, 256, 864), (4, 1, 512, 1024), (2, 1, 1024, 2048))
PYRAMID = ((4, 1, 512, 1024), 4, (1.0, 0.5, 0.25, 0.125))
HBM_PEAK = 8.0e12


def _sets(shapes, gshape, n, dev):
    """n input sets: every set its own memory, the values of set 0 rolled by the set's index"""
    import torch
    import depth_loss_cases as cases
    base = [torch.from_numpy(cases.prediction(s, 10 + k)).to(dev) for k, s in enumerate(shapes)]
    gt = torch.from_numpy(cases.ground_truth(gshape, 40)).to(dev)
    return [([torch.roll(p, i, -1).requires_grad_(True) for p in base], torch.roll(gt, i, -1)) for i in range(n)]


def section(name, passes):
    import torch
    import cerberusnet_amd as ca
    dev = torch.device("cuda", 0)
    if name == "single":
        jobs = [((shape,), (shape[0],) + shape[2:], lambda backend: ca.InvHuberLoss(backend=backend), False) for shape in SHAPES]
    else:
        (B, _, H, W), levels, lvl_weights = PYRAMID
        shapes = tuple((B, 1, H >> k, W >> k) for k in range(levels))
        jobs = [(shapes, (B, H, W), lambda backend: ca.InvHuberLossPyr(list(lvl_weights), backend=backend), True)]
    for shapes, gshape, make, pyramid in jobs:
        losses = {"fused": make("hip"), "stock": make("torch")}
        pixels = sum(s[0] * s[2] * s[3] for s in shapes)
        n = _copies(8 * pixels)
        sets = _sets(shapes, gshape, n, dev)
        alg = (16 * pixels, 28 * pixels)
        rec = {"section": name, "shape": "x".join(map(str, shapes[0])) + (" +%d" % (len(shapes) - 1) if pyramid else ""),
               "copies": n, "cold": bool(n * 8 * pixels >= (512 << 20)), "alg_bytes_fwd": alg[0], "alg_bytes_fwd_bwd": alg[1]}

        def fwd(fn, preds, gt):
            with torch.no_grad():
                fn({"depth": preds if pyramid else preds[0]}, {"disparity": gt})

        def both(fn, preds, gt):
            torch.autograd.grad(fn({"depth": preds if pyramid else preds[0]}, {"disparity": gt}), preds)
        for what, call in (("fwd", fwd), ("fwd_bwd", both)):
            res = _time_alternating({label: [lambda fn=fn, p=p, g=g: call(fn, p, g) for p, g in sets]
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
    titles = {"single": "InvHuberLoss()", "pyramid": "InvHuberLossPyr([1, 0.5, 0.25, 0.125]): 4 halving levels, full-size ground truth"}
    out = []
    for name, _ in SECTIONS:
        out.append("%s (us per call; GB/s = bytes the fused kernels load and store / the fused time, %% of the 8 TB/s HBM peak; cold "
                   "= inputs from HBM; peak MiB = max_memory_allocated of one forward + backward above the inputs)" % titles[name])
        out.append("  %-18s %6s %5s | %10s %10s %6s %7s %5s | %10s %10s %6s %7s %5s | %10s %10s" % (
            "shape", "copies", "cold", "stock fwd", "fused fwd", "x", "GB/s", "%", "stock f+b", "fused f+b", "x", "GB/s", "%",
            "stock MiB", "fused MiB"))
        for r in (r for r in rows if r["section"] == name):
            bw = [r["alg_bytes_fwd"] / (r["fused_fwd_us"] * 1e-6), r["alg_bytes_fwd_bwd"] / (r["fused_fwd_bwd_us"] * 1e-6)]
            out.append("  %-18s %6d %5s | %10.1f %10.1f %6.2f %7.0f %5.1f | %10.1f %10.1f %6.2f %7.0f %5.1f | %10.1f %10.1f" % (
                r["shape"], r["copies"], "yes" if r["cold"] else "no",
                r["stock_fwd_us"], r["fused_fwd_us"], r["stock_fwd_us"] / r["fused_fwd_us"], bw[0] / 1e9, 100 * bw[0] / HBM_PEAK,
                r["stock_fwd_bwd_us"], r["fused_fwd_bwd_us"], r["stock_fwd_bwd_us"] / r["fused_fwd_bwd_us"], bw[1] / 1e9,
                100 * bw[1] / HBM_PEAK, r["stock_peak_mib"], r["fused_peak_mib"]))
        out.append("")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_loss_fused.txt"))
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    if args.section:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_depth_loss: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.passes)
    rows = []
    for name, limit in SECTIONS:
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_depth_loss: section %s exceeded %d s; stopping" % (name, limit))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_depth_loss: section %s failed (%d); stopping" % (name, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
