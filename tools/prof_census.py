#!/usr/bin/env python3
"""Times unFlowLoss's census (ternary) term: the stock-op chain ``TernaryLoss(...).mean()`` against the fused HIP op
(cerberus::census_loss), in one process per section on one GPU.

    python tools/prof_census.py [--out profiles/census_fused.txt] [--pairs 4] [--passes 7]

For the four loss scales at `pairs` image pairs and max_distance 1 (what unFlowLoss passes) and 3 (the 7 x 7 census of
UnFlow / ARFlow): forward and forward + backward of (a) the fused op and (b) the stock chain, and the peak of
``torch.cuda.max_memory_allocated`` over one forward + backward of each above what the inputs hold.  At 512 x 1024 the
photometric op's own forward + backward is timed in the same section, as a yardstick for a kernel of the same shape.
Method (that of tools/prof_photometric.py): every call of a timed pass works on its own copy of the inputs, the copies of
one pass > 512 MiB in all where memory allows (inputs come from HBM, not from the Infinity Cache; at the small scales 16
copies, which stay cache-resident: said in the table), 3 warm-up passes, HIP events around a whole pass, the median over
`passes` passes, (a) and (b) alternating.  Each section runs in a child process under a time limit of its own; the first
failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from prof_photometric import SCALES, _copies, _time  # noqa: E402

SECTIONS = (("d1", 240), ("d3", 300))


def section(name, pairs, passes):
    import torch
    import cerberusnet_amd as ca
    from cerberusnet_amd.synth import hash_uniform
    dev = torch.device("cuda", 0)
    d = int(name[1:])
    t = lambda shape, seed: torch.from_numpy(hash_uniform(shape, seed, 0.0, 1.0)).to(dev)
    stock = lambda a, b: ca.TernaryLoss(a, b, d).mean()
    fused = lambda a, b: torch.ops.cerberus.census_loss(a, b, d)
    for H, W in SCALES:
        shape = (pairs, 3, H, W)
        nbytes = 4 * pairs * 3 * H * W
        n = _copies(2 * nbytes)
        sets = [(t(shape, 10 + i), t(shape, 40 + i).requires_grad_(True)) for i in range(n)]
        alg = (2 * nbytes, 5 * nbytes)      # 2 image reads forward; 2 reads + 1 write more for the backward
        rec = {"d": d, "scale": "%dx%d" % (H, W), "copies": n, "cold": bool(n * alg[0] >= (512 << 20)),
               "alg_bytes_fwd": alg[0], "alg_bytes_fwd_bwd": alg[1]}
        forms = [("fused", fused), ("stock", stock)]
        if (H, W) == SCALES[0]:
            forms.append(("photometric", lambda a, b: ca.photometric_loss(a, b, 0.15, 0.85)))
        for label, fn in forms:
            def fwd(a, b, fn=fn):
                with torch.no_grad():
                    fn(a, b)

            def both(a, b, fn=fn):
                torch.autograd.grad(fn(a, b), b)
            rec[label + "_fwd_us"] = _time([lambda a=a, b=b: fwd(a, b) for a, b in sets], passes) * 1e6
            rec[label + "_fwd_bwd_us"] = _time([lambda a=a, b=b: both(a, b) for a, b in sets], passes) * 1e6
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            both(*sets[0])
            torch.cuda.synchronize()
            rec[label + "_peak_mib"] = (torch.cuda.max_memory_allocated() - base) / float(1 << 20)
        print("ROW " + json.dumps(rec), flush=True)
        del sets
        torch.cuda.empty_cache()


def table(rows):
    out = []
    for d in sorted({r["d"] for r in rows}):
        out.append("census, max_distance %d (us per call; GB/s = algorithmic bytes of the fused op / its time; cold = inputs from "
                   "HBM; peak MiB = max_memory_allocated of one forward + backward above the inputs)" % d)
        out.append("  %-10s %6s %5s | %10s %10s %7s %8s | %10s %10s %7s %8s | %10s %10s" % (
            "scale", "copies", "cold", "stock fwd", "fused fwd", "x", "GB/s", "stock f+b", "fused f+b", "x", "GB/s", "stock MiB",
            "fused MiB"))
        for r in (r for r in rows if r["d"] == d):
            out.append("  %-10s %6d %5s | %10.1f %10.1f %7.1f %8.0f | %10.1f %10.1f %7.1f %8.0f | %10.1f %10.1f" % (
                r["scale"], r["copies"], "yes" if r["cold"] else "no",
                r["stock_fwd_us"], r["fused_fwd_us"], r["stock_fwd_us"] / r["fused_fwd_us"], r["alg_bytes_fwd"] / r["fused_fwd_us"] / 1e3,
                r["stock_fwd_bwd_us"], r["fused_fwd_bwd_us"], r["stock_fwd_bwd_us"] / r["fused_fwd_bwd_us"],
                r["alg_bytes_fwd_bwd"] / r["fused_fwd_bwd_us"] / 1e3, r["stock_peak_mib"], r["fused_peak_mib"]))
        for r in (r for r in rows if r["d"] == d and "photometric_fwd_bwd_us" in r):
            out.append("  photometric_loss at %s in the same run: fwd %.1f us, fwd + bwd %.1f us; census fused fwd + bwd = %.2f x that" % (
                r["scale"], r["photometric_fwd_us"], r["photometric_fwd_bwd_us"], r["fused_fwd_bwd_us"] / r["photometric_fwd_bwd_us"]))
        out.append("")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "census_fused.txt"))
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    if args.section:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_census: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.pairs, args.passes)
    rows = []
    for name, limit in SECTIONS:
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--pairs", str(args.pairs), "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_census: section %s exceeded %d s; stopping" % (name, limit))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_census: section %s failed (%d); stopping" % (name, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
