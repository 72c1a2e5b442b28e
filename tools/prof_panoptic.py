#!/usr/bin/env python3
"""Times the panoptic metric: the three fused ops of csrc/panoptic.hip against their stock-op chains, and a whole
``PanopticMetric.add_sample`` -- device work, the host copies and the host part -- with ``backend='hip'`` against
``backend='torch'``, on one GPU.

    python tools/prof_panoptic.py [--out profiles/panoptic_fused.txt] [--passes 7]

Section ``ops``: ``group_pixels`` alone at 1 x 512 x 1024 with K = 99 centres (against ``group_stock``: the (K, H*W, 2) difference,
its norm, the argmin); ``center_peaks`` with kernel 7 at 4 x 1 x 512 x 1024 (against threshold + max_pool2d + where);
``instance_overlap`` at 4 x 512 x 1024 with 101 ids and 20 classes (against three ``scatter_add_``).  Each op is reported against
the bytes it must move (inputs once, output once) and the 8 TB/s HBM peak.
Section ``metric``: ``PanopticMetric(19).add_sample`` at 4 x 19 x 512 x 1024 and 2 x 19 x 256 x 864 with some 60 peaks per heat
map, and the peak device memory of one call above what the inputs hold (``torch.cuda.max_memory_allocated``), both backends.
Method (that of tools/prof_metrics.py): within one process fused and stock passes alternate, every shape is warmed up by 3
passes, a pass is timed by device events around it and a synchronise, every call of a pass works on its own copy of the
inputs, the median over ``passes`` passes counts.  Each section runs in a child process under a time limit of its own; the
first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from prof_seg_loss import _time_alternating  # noqa: E402

SECTIONS = (("ops", 400), ("metric", 500))
METRIC_SHAPES = ((4, 19, 512, 1024), (2, 19, 256, 864))
HBM_PEAK = 8.0e12
PEAKS = 60


def ops_section(passes):
    import torch
    import cerberusnet_amd  # noqa: F401
    import panoptic_cases as cases
    from cerberusnet_amd.statistics.panoptic import overlap_stock
    from cerberusnet_amd.utilities import panoptic_post_processing as pp
    dev = torch.device("cuda", 0)
    ops = torch.ops.cerberus
    up = lambda a: torch.from_numpy(a).to(dev)

    def row(what, fused, stock, nbytes):
        res = _time_alternating({"fused": fused, "stock": stock}, passes)
        print("ROW " + json.dumps({"section": "ops", "what": what, "copies": len(fused), "alg_bytes": nbytes,
                                   "fused_us": res["fused"] * 1e6, "stock_us": res["stock"] * 1e6}), flush=True)
    n = 4
    H, W, K = 512, 1024, 99
    offs = [up(cases.offsets((1, H, W), 40 + i, "float")) for i in range(n)]
    ctrs = [up(cases.centers(K, H, W, 50 + i))[None] for i in range(n)]
    cnt = torch.full((1,), K, dtype=torch.int64, device=dev)
    row("group_pixels, 1x512x1024, K = 99", [lambda o=o, c=c: ops.group_pixels(o, c, cnt, None, -1) for o, c in zip(offs, ctrs)],
        [lambda o=o, c=c: pp.group_stock(o, c, cnt) for o, c in zip(offs, ctrs)], (8 + 8) * H * W)
    del offs, ctrs
    B = 4
    heats = [up(cases.heatmap((B, 1, H, W), 60 + i, step=1.0 / 4096)) for i in range(n)]
    row("center_peaks, 4x1x512x1024, kernel 7", [lambda h=h: ops.center_peaks(h, 0.1, 7) for h in heats],
        [lambda h=h: pp.peaks_stock(h, 0.1, 7) for h in heats], 8 * B * H * W)
    del heats
    maps = [[up(m) for m in cases.id_maps((B, H, W), 70 + i, 101, 20, spread=0)] for i in range(n)]
    row("instance_overlap, 4x512x1024, M = 101, C = 20", [lambda m=m: ops.instance_overlap(*m, 101, 20) for m in maps],
        [lambda m=m: overlap_stock(*m, 101, 20) for m in maps], 32 * B * H * W)


def metric_section(passes):
    import torch
    import cerberusnet_amd as ca
    dev = torch.device("cuda", 0)
    for shape in METRIC_SHAPES:
        B, C, H, W = shape
        gen = torch.Generator(device=dev).manual_seed(80)
        rnd = lambda *s: torch.rand(*s, device=dev, generator=gen)

        def heat():
            x = rnd(B, 1, H, W) * 0.09                                     # below the threshold everywhere ...
            at = torch.randint(0, H * W, (B, PEAKS), device=dev, generator=gen)
            x.view(B, -1).scatter_(1, at, 0.5 + 0.5 * rnd(B, PEAKS))       # ... but at some 60 peaks
            return x

        def one():
            pred = {"seg": rnd(B, C, H, W), "center": heat(), "offset": (rnd(B, 2, H, W) - 0.5) * 40}
            tgt = {"seg": torch.randint(0, C, (B, H, W), device=dev, generator=gen), "center": heat(),
                   "offset": (rnd(B, 2, H, W) - 0.5) * 40, "center_points": [[[H // 2, W // 2], [H // 3, W // 3]]] * B}
            return pred, tgt
        sets = [one() for _ in range(2)]
        metrics = {"fused": ca.PanopticMetric(C, backend="hip"), "stock": ca.PanopticMetric(C, backend="torch")}

        def sample(metric, p, tg):
            metric.add_sample(p, tg)
            if len(metric.metric_data["Batch_Loss"]) > 64:
                metric._reset_metric()
        res = _time_alternating({label: [lambda m=m, p=p, tg=tg: sample(m, p, tg) for p, tg in sets] for label, m in metrics.items()},
                                passes)
        memory = {}
        for label, m in metrics.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            sample(m, *sets[0])
            torch.cuda.synchronize()
            memory[label] = torch.cuda.max_memory_allocated() - base
        print("ROW " + json.dumps({"section": "metric", "shape": "x".join(map(str, shape)), "copies": len(sets),
                                   "fused_us": res["fused"] * 1e6, "stock_us": res["stock"] * 1e6, "fused_bytes": memory["fused"],
                                   "stock_bytes": memory["stock"]}), flush=True)
        del sets
        torch.cuda.empty_cache()


def table(rows):
    out = ["single ops: us per call (no copy); GB/s = the bytes the op must move (inputs once, output once) / the fused time, "
           "% of the 8 TB/s HBM peak", "",
           "  %-48s %6s | %12s %12s %7s | %7s %5s" % ("op", "copies", "stock", "fused", "x", "GB/s", "%")]
    for r in (r for r in rows if r["section"] == "ops"):
        bw = r["alg_bytes"] / (r["fused_us"] * 1e-6)
        out.append("  %-48s %6d | %12.1f %12.1f %7.2f | %7.0f %5.1f" % (r["what"], r["copies"], r["stock_us"], r["fused_us"],
                                                                      r["stock_us"] / r["fused_us"], bw / 1e9, 100 * bw / HBM_PEAK))
    out += ["", "PanopticMetric(19).add_sample: us per call (device work, host copies and the host part); peak device memory of one "
            "call above the inputs, MB", "",
            "  %-18s %6s | %12s %12s %7s | %10s %10s" % ("shape", "copies", "stock", "fused", "x", "stock MB", "fused MB")]
    for r in (r for r in rows if r["section"] == "metric"):
        out.append("  %-18s %6d | %12.1f %12.1f %7.2f | %10.1f %10.1f" % (r["shape"], r["copies"], r["stock_us"], r["fused_us"],
                                                                         r["stock_us"] / r["fused_us"], r["stock_bytes"] / 1e6,
                                                                         r["fused_bytes"] / 1e6))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "panoptic_fused.txt"))
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    if args.section:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_panoptic: no GPU (a timing needs one; there is no fallback)")
        return ops_section(args.passes) if args.section == "ops" else metric_section(args.passes)
    rows = []
    for name, limit in SECTIONS:
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_panoptic: section %s exceeded %d s; stopping" % (name, limit))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_panoptic: section %s failed (%d); stopping" % (name, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
        print("section %s: done" % name, flush=True)
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
