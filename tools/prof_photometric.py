#!/usr/bin/env python3
"""Times unFlowLoss's photometric and smoothness terms: the stock-op chain against the fused HIP ops
(cerberus::photometric_loss / cerberus::edge_smoothness), in one process on one GPU.

    python tools/prof_photometric.py [--out profiles/photometric_fused.txt] [--pairs 4] [--passes 7]

For the four loss scales at `pairs` image pairs: forward and forward + backward of (a) the stock chain and (b) the fused
op; then one unFlowLoss forward + backward with fused off and on.  Method: every call of a timed pass works on its own
copy of the inputs, the copies of one pass > 512 MiB in all where memory allows (inputs come from HBM, not from the
Infinity Cache; at the small scales 16 copies, which stay cache-resident: said in the table), 3 warm-up passes, HIP events
around a whole pass, the median over `passes` passes, (a) and (b) alternating.  Achieved bytes/s of (b) against the
algorithmic bytes: 2 image reads forward; 2 reads + 1 write more for the backward.  Each section runs in a child process
under a time limit of its own; the first failure ends the run."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SECTIONS = (("photometric", 240), ("smoothness", 240), ("unflow", 240))
SCALES = ((512, 1024), (256, 512), (128, 256), (64, 128))


def _time(fns, passes):
    """median seconds per call: fns = one closure per input copy, a pass calls each once"""
    import torch
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for fn in fns:
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / len(fns))
    return statistics.median(times)


def _copies(set_bytes):
    return int(min(16, max(2, math.ceil((512 << 20) / set_bytes))))


def section(name, pairs, passes):
    import torch
    import cerberusnet_amd as ca
    from cerberusnet_amd.loss_functions import UnFlowLoss as U
    from cerberusnet_amd.synth import hash_uniform
    dev = torch.device("cuda", 0)
    t = lambda shape, seed, lo=-2.0, hi=2.0: torch.from_numpy(hash_uniform(shape, seed, lo, hi)).to(dev)
    rows = []
    if name in ("photometric", "smoothness"):
        stock_loss = U.unFlowLoss(backend="torch")
        for H, W in SCALES:
            if name == "photometric":
                shape = (pairs, 3, H, W)
                nbytes = 4 * pairs * 3 * H * W
                n = _copies(2 * nbytes)
                sets = [(t(shape, 10 + i), t(shape, 40 + i).requires_grad_(True)) for i in range(n)]
                stock = lambda o, r: stock_loss.loss_photometric(o, r)
                fused = lambda o, r: ca.photometric_loss(o, r, 0.15, 0.85)
                alg = (2 * nbytes, 5 * nbytes)
            else:
                fshape, ishape = (pairs, 2, H, W), (pairs, 3, H, W)
                fb, ib = 4 * pairs * 2 * H * W, 4 * pairs * 3 * H * W
                n = _copies(fb + ib)
                sets = [(t(ishape, 10 + i), t(fshape, 40 + i, -6.0, 6.0).requires_grad_(True)) for i in range(n)]
                stock = lambda img, f: U._edge_aware_smoothness(f, img, 0.2, 2)
                fused = lambda img, f: ca.edge_smoothness(f, img, 0.2, 2)
                alg = (fb + ib, 2 * (fb + ib) + fb)
            rec = {"section": name, "scale": "%dx%d" % (H, W), "copies": n,
                   "cold": bool(n * (alg[0]) >= (512 << 20)), "alg_bytes_fwd": alg[0], "alg_bytes_fwd_bwd": alg[1]}
            for label, fn in (("stock", stock), ("fused", fused)):
                def fwd(a, b, fn=fn):
                    with torch.no_grad():
                        fn(a, b)

                def both(a, b, fn=fn):
                    torch.autograd.grad(fn(a, b), b)
                rec[label + "_fwd_us"] = _time([lambda a=a, b=b: fwd(a, b) for a, b in sets], passes) * 1e6
                rec[label + "_fwd_bwd_us"] = _time([lambda a=a, b=b: both(a, b) for a, b in sets], passes) * 1e6
            rows.append(rec)
            del sets
            torch.cuda.empty_cache()
    else:
        import bench
        H, W = SCALES[0]
        img1, img2 = t((pairs, 3, H, W), 1), t((pairs, 3, H, W), 2)
        sizes = [(H, W), (H // 4, W // 4), (H // 8, W // 8), (H // 16, W // 16), (H // 32, W // 32)]
        mk = lambda s: [bench.Workload._flow(pairs, h, w, s + i, "smooth", dev).requires_grad_(True) for i, (h, w) in enumerate(sizes)]
        fw, bw = mk(80), mk(90)
        rec = {"section": name, "scale": "%dx%d, %d pairs, 4 scales x 2 directions" % (H, W, pairs)}
        for fused in (False, True):
            loss_fn = U.unFlowLoss(fused=fused)

            def step():
                loss = loss_fn({"flow": fw, "flow_b": bw}, {"l_img": img1, "l_seq": img2})
                torch.autograd.grad(loss, fw[:4] + bw[:4])
            rec["fused_us" if fused else "stock_us"] = _time([step] * 4, passes) * 1e6
        rows.append(rec)
    for r in rows:
        print("ROW " + json.dumps(r), flush=True)


def table(rows):
    out = []
    for name in ("photometric", "smoothness"):
        out.append("%s (us per call; GB/s = algorithmic bytes of the fused op / its time; cold = inputs from HBM)" % name)
        out.append("  %-10s %6s %5s | %10s %10s %7s %8s | %10s %10s %7s %8s" % (
            "scale", "copies", "cold", "stock fwd", "fused fwd", "x", "GB/s", "stock f+b", "fused f+b", "x", "GB/s"))
        for r in (r for r in rows if r["section"] == name):
            out.append("  %-10s %6d %5s | %10.1f %10.1f %7.1f %8.0f | %10.1f %10.1f %7.1f %8.0f" % (
                r["scale"], r["copies"], "yes" if r["cold"] else "no",
                r["stock_fwd_us"], r["fused_fwd_us"], r["stock_fwd_us"] / r["fused_fwd_us"], r["alg_bytes_fwd"] / r["fused_fwd_us"] / 1e3,
                r["stock_fwd_bwd_us"], r["fused_fwd_bwd_us"], r["stock_fwd_bwd_us"] / r["fused_fwd_bwd_us"],
                r["alg_bytes_fwd_bwd"] / r["fused_fwd_bwd_us"] / 1e3))
        out.append("")
    for r in (r for r in rows if r["section"] == "unflow"):
        out.append("unFlowLoss forward + backward (%s; warps and pyramid included; inputs replayed, cache-warm): fused=False %.1f us, "
                   "fused=True %.1f us (x %.2f)" % (r["scale"], r["stock_us"], r["fused_us"], r["stock_us"] / r["fused_us"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "photometric_fused.txt"))
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    if args.section:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_photometric: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.pairs, args.passes)
    rows = []
    for name, limit in SECTIONS:
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--pairs", str(args.pairs), "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_photometric: section %s exceeded %d s; stopping" % (name, limit))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_photometric: section %s failed (%d); stopping" % (name, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
