#!/usr/bin/env python3
"""Times the RMI loss: the stock-op chain (``backend='torch'``: one-hot, permuted logits, BCE, two poolings, the (N,C,9,P)
float64 stacks and their batched matmuls) against the fused route (``backend='hip'``: cerberus::rmi_moments, the 9 x 9 algebra
in torch float64 ops, cerberus::rmi_moments_backward), in one process per shape on one GPU.

    python tools/prof_rmi_loss.py [--out profiles/rmi_loss_fused.txt] [--passes 7]

``RMILossAux(num_classes=19)`` eager forward + backward on ``{'seg': logits}`` at (4,19,512,1024) and (2,19,256,864), then the
stages of the fused route one by one (the raw ops): the front end with its one-workgroup BCE sum (``do_rmi`` off), the means,
moments and fold (the forward op with ``do_rmi`` on minus the former), the backward launch; the rest of the fused total is the
9 x 9 algebra and autograd.  The front end's algorithmic bytes (4 C + 8 per pixel: the logits and an int64 label) over its time
are given as GB/s and as a share of the 8 TB/s HBM peak; the backward's are 8 C + 8 per pixel.
Method (that of tools/prof_seg_loss.py): every call of a timed pass works on its own copy of the inputs, the copies of one pass
> 512 MiB in all (inputs come from HBM, not from the Infinity Cache), 3 warm-up passes, HIP events around a whole pass, the
median over `passes` passes, fused and stock passes alternating.  Each shape runs in a child process under a time limit of its
own; the first failure ends the run."""
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

SHAPES = ((4, 19, 512, 1024), (2, 19, 256, 864))
LIMIT = 400
HBM_PEAK = 8.0e12


def section(index, passes):
    import torch
    import cerberusnet_amd as ca
    import rmi_cases as cases
    dev = torch.device("cuda", 0)
    shape = SHAPES[index]
    B, C, H, W = shape
    pixels = B * H * W
    n = _copies(4 * C * pixels)
    sets = [(torch.from_numpy(cases.logits(shape, 10 + i)).to(dev).requires_grad_(True),
             torch.from_numpy(cases.labels(shape, 40 + 2 * i)).to(dev)) for i in range(n)]
    losses = {"fused": ca.RMILossAux(num_classes=C, backend="hip"), "stock": ca.RMILossAux(num_classes=C, backend="torch")}
    rec = {"shape": "x".join(map(str, shape)), "copies": n, "front_bytes": (4 * C + 8) * pixels, "bwd_bytes": (8 * C + 8) * pixels}

    def both(fn, x, t):
        torch.autograd.grad(fn({"seg": x}, {"seg": t}), x)
    res = _time_alternating({label: [lambda fn=fn, x=x, t=t: both(fn, x, t) for x, t in sets] for label, fn in losses.items()},
                            passes)
    for label, sec in res.items():
        rec[label + "_fwd_bwd_us"] = sec * 1e6
    # the stages of the fused route, through the raw ops
    op = torch.ops.cerberus
    with torch.no_grad():
        saved = [op.rmi_moments(x, t, 3, 4, True) for x, t in sets]
        g = torch.full((), 0.5, device=dev)
        gm = [torch.randn_like(s[2]) * 1e-3 for s in saved]
        stages = _time_alternating({
            "front": [lambda x=x, t=t: op.rmi_moments(x, t, 3, 4, False) for x, t in sets],
            "forward": [lambda x=x, t=t: op.rmi_moments(x, t, 3, 4, True) for x, t in sets],
            "backward": [lambda x=x, t=t, s=s, m=m: op.rmi_moments_backward(x, t, s[4], s[5], s[6], s[7], g, m, m, 3, 4, True)
                         for (x, t), s, m in zip(sets, saved, gm)]}, passes)
    for label, sec in stages.items():
        rec[label + "_us"] = sec * 1e6
    del saved, gm
    for label, fn in losses.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        both(fn, *sets[0])
        torch.cuda.synchronize()
        rec[label + "_peak_mib"] = (torch.cuda.max_memory_allocated() - base) / float(1 << 20)
    print("ROW " + json.dumps(rec), flush=True)


def table(rows):
    out = ["RMILossAux(num_classes=19), eager forward + backward on {'seg': logits} (us per call, medians; peak MiB = "
           "max_memory_allocated of one forward + backward above the inputs)",
           "  %-16s %6s | %11s %11s %7s | %10s %10s" % ("shape", "copies", "stock f+b", "fused f+b", "x", "stock MiB", "fused MiB")]
    for r in rows:
        out.append("  %-16s %6d | %11.1f %11.1f %7.2f | %10.1f %10.1f" % (
            r["shape"], r["copies"], r["stock_fwd_bwd_us"], r["fused_fwd_bwd_us"], r["stock_fwd_bwd_us"] / r["fused_fwd_bwd_us"],
            r["stock_peak_mib"], r["fused_peak_mib"]))
    out += ["", "stages of the fused route (us; raw ops; GB/s = algorithmic bytes / time, % of the 8 TB/s HBM peak; algebra = the "
            "fused total minus the three stages: the 9 x 9 float64 torch ops and autograd)",
            "  %-16s | %10s %7s %5s | %16s | %10s %7s %5s | %10s" % ("shape", "front end", "GB/s", "%", "means + moments", "backward",
                                                                      "GB/s", "%", "algebra")]
    for r in rows:
        fb, bb = r["front_bytes"] / (r["front_us"] * 1e-6), r["bwd_bytes"] / (r["backward_us"] * 1e-6)
        out.append("  %-16s | %10.1f %7.0f %5.1f | %16.1f | %10.1f %7.0f %5.1f | %10.1f" % (
            r["shape"], r["front_us"], fb / 1e9, 100 * fb / HBM_PEAK, r["forward_us"] - r["front_us"], r["backward_us"], bb / 1e9,
            100 * bb / HBM_PEAK, r["fused_fwd_bwd_us"] - r["forward_us"] - r["backward_us"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", type=int)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rmi_loss_fused.txt"))
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    if args.section is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_rmi_loss: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.passes)
    rows = []
    for index, shape in enumerate(SHAPES):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", str(index), "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_rmi_loss: shape %s exceeded %d s; stopping" % (shape, LIMIT))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_rmi_loss: shape %s failed (%d); stopping" % (shape, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
