#!/usr/bin/env python3
"""Times the Panoptic-DeepLab head's own step: the fused route (cerberus_pdl::upcat_dwconv5x5 / dwconv5x5, csrc/pdl_head.hip)
against the stock chain (F.interpolate + torch.cat + F.conv2d with groups = C) in the same process, eager forward + backward (all
gradients), fp32, on one GPU.

    python tools/prof_pdl_head.py [--out profiles/pdl_head_fused.txt] [--passes 9]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/prof_pdl_head.py --kernels 0
    python tools/prof_pdl_head.py --stats DIR >> profiles/pdl_head_fused.txt

Shapes (4 pairs of 1024 x 512 on the W32 backbone): the last semantic decoder stage, low (4,256,64,128) with skip (4,32,128,256),
and a classifier's plain convolution on (4,256,128,256).
Method (that of tools/prof_ocr_head.py): every call of a timed pass works on its own copy of the inputs, the copies of one pass
> 512 MiB in all, 3 warm-up passes, HIP events around a whole pass, fused and stock passes alternating; the median over the passes
with the smallest and the largest pass beside it.  Each shape runs in a child process under a time limit of its own; the first
failure ends the run.  The forward alone is timed the same way.
``--kernels`` makes a few plain calls of the raw ops for a kernel-trace run of its own; ``--stats`` turns that run's kernel_trace
CSV into per-kernel device times and achieved bytes/s (the bytes the algorithm needs, from the shapes) against the 8 TB/s HBM peak."""
import argparse
import csv
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from prof_ocr_head import _time  # noqa: E402
from prof_photometric import _copies  # noqa: E402

# label, (B, Ca, Cb, h, w, H, W)
SHAPES = (("stage", (4, 256, 32, 64, 128, 128, 256)), ("plain", (4, 0, 256, 0, 0, 128, 256)))
LIMIT = 500
HBM_PEAK = 8.0e12


def _inputs(index, n, dev):
    """n sets of (low or None, skip, weight, grad_y), uniform in [-1, 1] from a seeded generator on the device."""
    import torch
    B, Ca, Cb, h, w, H, W = SHAPES[index][1]
    gen = torch.Generator(device=dev).manual_seed(1234 + index)
    rnd = lambda *s: torch.rand(s, device=dev, generator=gen) * 2 - 1
    return [[rnd(B, Ca, h, w) if Ca else None, rnd(B, Cb, H, W), rnd(Ca + Cb, 1, 5, 5) * 0.2, rnd(B, Ca + Cb, H, W)] for _ in range(n)]


def section(index, passes):
    import torch
    import pdl_cases as cases
    dev = torch.device("cuda", 0)
    label, (B, Ca, Cb, h, w, H, W) = SHAPES[index]
    n = _copies(4 * B * (2 * (Ca + Cb) + Cb) * H * W)
    sets = _inputs(index, n, dev)
    for s in sets:
        for t in s[:3]:
            if t is not None:
                t.requires_grad_(True)
    rec = {"label": label, "shape": "x".join(map(str, SHAPES[index][1])), "copies": n}
    # faster and different is not faster: the two routes on the first set
    low, skip, weight, gy = sets[0]
    leaves = [t for t in (low, skip, weight) if t is not None]
    ya, yb = cases.fused(low, skip, weight), cases.stock_chain(low, skip, weight)
    ga, gb = torch.autograd.grad(ya, leaves, gy), torch.autograd.grad(yb, leaves, gy)
    rec["max_rel_diff"] = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip([ya] + list(ga), [yb] + list(gb)))

    def fb(fn, s):
        leaves = [t for t in s[:3] if t is not None]
        torch.autograd.grad(fn(*s[:3]), leaves, s[3])

    def fwd(fn, s):
        with torch.no_grad():
            fn(*s[:3])
    routes = {"fused": cases.fused, "stock": cases.stock_chain}
    for what, run in (("fwdbwd", fb), ("fwd", fwd)):
        res = _time({name: [lambda fn=fn, s=s: run(fn, s) for s in sets] for name, fn in routes.items()}, passes)
        for name, (med, lo, hi) in res.items():
            rec["%s_%s_us" % (what, name)] = [med * 1e6, lo * 1e6, hi * 1e6]
    print("ROW " + json.dumps(rec), flush=True)


def kernels(index, reps=5):
    """Plain calls of the raw ops at both shapes (1 warm-up + ``reps``), for a kernel-trace run."""
    import torch
    import cerberusnet_amd  # noqa: F401  (registers the ops)
    dev = torch.device("cuda", 0)
    op = torch.ops.cerberus_pdl
    for i in range(len(SHAPES)):
        low, skip, weight, gy = _inputs(i, 1, dev)[0]
        for _ in range(reps + 1):
            if low is None:
                op.dwconv5x5(skip, weight)
                op.dwconv5x5_backward(gy, skip, weight, [True, True])
            else:
                op.upcat_dwconv5x5(low, skip, weight)
                op.upcat_dwconv5x5_backward(gy, low, skip, weight, [True, True, True])
    torch.cuda.synchronize()


def kernel_bytes():
    """{(kernel-name substring, workgroups) -> (what, bytes the algorithm needs)}: the two shapes differ in their plane count."""
    out = {}
    for label, (B, Ca, Cb, h, w, H, W) in SHAPES:
        C, hw = Ca + Cb, H * W
        src = 4 * B * (Ca * h * w + Cb * hw)
        tiles = -(-H // 32) * -(-W // 64)          # the trace reports grid.x or the whole grid, in work-items
        for planes in (B * C, B * C * tiles):
            out[("pdl_dwconv_kernel<0>", planes)] = ("%s forward: low + skip in, y out" % label, src + 4 * B * C * hw)
            out[("pdl_dwconv_kernel<2>", planes)] = ("%s backward: grad_y + low + skip in, input gradients out" % label, src + 8 * B * C * hw)
        if Ca:
            out[("pdl_grad_low_kernel", None)] = ("stage grad_low: upsampled gradient in, grad_low out", 4 * B * Ca * (hw + h * w))
    return out


def stats(directory):
    paths = [os.path.join(root, f) for root, _, files in os.walk(directory) for f in files if f.endswith("kernel_trace.csv")]
    if not paths:
        raise SystemExit("prof_pdl_head: no kernel_trace.csv under %s" % directory)
    groups = {}
    for r in csv.DictReader(open(sorted(paths)[0])):
        name = r.get("Kernel_Name", "")
        if "pdl_" not in name:
            continue
        planes = int(r.get("Grid_Size_X") or r["Grid_Size"]) // max(int(r.get("Workgroup_Size_X") or r["Workgroup_Size"]), 1)
        groups.setdefault((name, planes), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    table = kernel_bytes()
    out = ["", "per-kernel device times (rocprofv3 --kernel-trace, a run of its own: 1 warm-up + 5 calls of each raw op at both shapes; us;",
           "GB/s = the bytes the algorithm needs / median time, % of the 8 TB/s HBM peak; the first call of each kernel is left out)",
           "  %-26s %8s %5s %9s %9s %8s %6s  %s" % ("kernel", "groups", "calls", "med us", "min us", "GB/s", "%", "bytes counted")]
    for (name, planes), times in sorted(groups.items()):
        times = sorted(times[1:]) or times
        med, lo = times[len(times) // 2], times[0]
        short = "pdl_" + name.split("pdl_", 1)[1].split("(")[0]
        hit = [v for (key, p), v in table.items() if key in name and p in (None, planes)]
        if hit:
            what, nbytes = hit[0]
            rate = nbytes / (med * 1e-6)
            out.append("  %-26s %8d %5d %9.1f %9.1f %8.0f %6.1f  %s" % (short, planes, len(times), med, lo, rate / 1e9, 100 * rate / HBM_PEAK, what))
        else:
            out.append("  %-26s %8d %5d %9.1f %9.1f %8s %6s  (a small launch)" % (short, planes, len(times), med, lo, "-", "-"))
    print("\n".join(out))


def table(rows):
    out = ["Panoptic-DeepLab head's depthwise 5x5 step, eager, fp32: fused (cerberus_pdl::*) against the stock chain (interpolate + cat +",
           "conv2d, groups = C) in one process (us per call: median [smallest .. largest pass]; x = stock / fused;",
           "shape = B x Ca x Cb x h x w x H x W; max rel diff: the two routes' outputs and gradients on the first input set)", ""]
    for r in rows:
        out.append("  %s  %s  (%d input copies per pass, max rel diff %.2e)" % (r["label"], r["shape"], r["copies"], r["max_rel_diff"]))
        for what, text in (("fwdbwd", "fwd + bwd"), ("fwd", "fwd only")):
            s, f = r[what + "_stock_us"], r[what + "_fused_us"]
            out.append("    %-10s stock %9.1f [%9.1f .. %9.1f]   fused %9.1f [%9.1f .. %9.1f]   x %5.2f"
                       % (text, s[0], s[1], s[2], f[0], f[1], f[2], s[0] / f[0]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", type=int)
    ap.add_argument("--kernels", type=int)
    ap.add_argument("--stats")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pdl_head_fused.txt"))
    ap.add_argument("--passes", type=int, default=9)
    args = ap.parse_args()
    if args.stats is not None:
        return stats(args.stats)
    if args.section is not None or args.kernels is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_pdl_head: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.passes) if args.section is not None else kernels(args.kernels)
    rows = []
    for index, (label, shape) in enumerate(SHAPES):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", str(index), "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_pdl_head: shape %s exceeded %d s; stopping" % (shape, LIMIT))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_pdl_head: shape %s failed (%d); stopping" % (shape, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
