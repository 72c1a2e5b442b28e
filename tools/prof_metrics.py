#!/usr/bin/env python3
"""Times the training-metric loggers: a whole ``add_sample`` -- device work and the one device-to-host copy -- of the stock-op
chain (``backend='torch'``) against the fused HIP ops (``backend='hip'``, csrc/metrics.hip), in one process per section on one
GPU.

    python tools/prof_metrics.py [--out profiles/metrics_fused.txt] [--passes 7]

Section ``seg``: ``SegmentationMetric(19)`` at (4,19,512,1024).  Section ``depth``: ``DepthMetric`` at (2,1,256,864) (the output
size of the reference's KITTI config) and (4,1,512,1024).  Section ``flow``: ``OpticFlowMetric`` at (4,2,512,1024) flows with
(4,3,512,1024) images.  Besides the two ``add_sample`` times, the fused ops alone (no packing, no copy) are timed, and the bytes
they load -- logits and labels; prediction and ground truth; both flows and the mask, then image, source and flow -- over that
time are given as GB/s and as a share of the 8 TB/s HBM peak.
Method (that of tools/prof_seg_loss.py): every call of a timed pass works on its own copy of the inputs, 3 warm-up passes, HIP
events around a whole pass, the median over `passes` passes, fused and stock passes alternating.  An ``add_sample`` ends in a
host copy, so its time includes the launch latency of its whole chain: that is what the trainer waits for after every step.
Section ``kernels`` times single ops at the shapes above: ``seg_confusion`` on the section's labels, with EVERY label ignored
(no LDS add at all: what the kernel costs without its histogram) and with one label and one winning class everywhere (all 64
lanes of a wave add to the same bin: the most contended case) -- the difference is all that any further aggregation of the LDS
adds, across the wave for instance, could win; and ``flow_metric_sums`` and ``warp_sad`` apart, the latter also under a smooth
flow (the section ``flow``'s flows are independent per pixel over +-20 px, so its gathers are scattered over 40 rows).
Each section runs in a child process under a time limit of its own; the first failure ends the run."""
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

SECTIONS = (("seg", 300), ("depth", 300), ("flow", 300), ("kernels", 300))
SEG_SHAPE = (4, 19, 512, 1024)
DEPTH_SHAPES = ((2, 1, 256, 864), (4, 1, 512, 1024))
FLOW_SHAPE = (4, 512, 1024)
HBM_PEAK = 8.0e12


def kernels_section(passes):
    import torch
    import cerberusnet_amd  # noqa: F401
    import metrics_cases as cases
    dev = torch.device("cuda", 0)
    ops = torch.ops.cerberus
    up = lambda a: torch.from_numpy(a).to(dev)

    def row(what, fns, nbytes):
        sec = _time_alternating({"k": fns}, passes)["k"]
        print("ROW " + json.dumps({"section": "kernels", "what": what, "copies": len(fns), "alg_bytes": nbytes, "us": sec * 1e6}), flush=True)
    B, C, H, W = SEG_SHAPE
    n = _copies(4 * C * B * H * W)
    x, t = up(cases.logits(SEG_SHAPE, 10)), up(cases.labels(SEG_SHAPE, 15))
    xs = [torch.roll(x, i, -1) for i in range(n)]
    seg_bytes = (4 * C + 8) * B * H * W
    ts = [torch.roll(t, i, -1) for i in range(n)]
    row("seg_confusion, the section's labels (runs of 4, 15 % ignored)", [lambda a=a, b=b: ops.seg_confusion(a, b, 255) for a, b in zip(xs, ts)],
        seg_bytes)
    ignored = torch.full_like(t, 255)
    row("seg_confusion, every label ignored (no LDS add)", [lambda a=a: ops.seg_confusion(a, ignored, 255) for a in xs], seg_bytes)
    one = torch.full_like(t, 3)
    peaked = [a.clone() for a in xs]
    for a in peaked:
        a[:, 7] = 9.0
    del xs
    row("seg_confusion, one (label, class) pair everywhere (one bin)", [lambda a=a: ops.seg_confusion(a, one, 255) for a in peaked], seg_bytes)
    del peaked
    torch.cuda.empty_cache()
    B, H, W = FLOW_SHAPE
    n = _copies((20 + 24) * B * H * W)
    fp, fg, mask = (up(a) for a in cases.flow_inputs(FLOW_SHAPE, seed=30, check=False))
    img, seq, _ = (up(a) for a in cases.warp_inputs((B, 3, H, W), 35))
    sets = [[torch.roll(a, i, -1) for a in (fp, fg, mask, img, seq)] for i in range(n)]
    row("flow_metric_sums", [lambda s=s: ops.flow_metric_sums(s[0], s[1], s[2]) for s in sets], 20 * B * H * W)
    row("warp_sad, flows independent per pixel over +-20 px", [lambda s=s: ops.warp_sad(s[3], s[4], s[0]) for s in sets], 32 * B * H * W)
    ys, xs_ = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    smooth = torch.stack([6.0 * torch.sin(ys / 40.0) + 0.01 * xs_, 4.0 * torch.cos(xs_ / 60.0)], 0)[None].expand(B, 2, H, W).contiguous()
    smooths = [torch.roll(smooth, i, -1) for i in range(n)]
    row("warp_sad, a smooth flow (|flow| <= 16 px, slope <= 0.15)", [lambda s=s, f=f: ops.warp_sad(s[3], s[4], f) for s, f in zip(sets, smooths)],
        32 * B * H * W)


def section(name, passes):
    import torch
    import cerberusnet_amd as ca
    import metrics_cases as cases
    if name == "kernels":
        return kernels_section(passes)
    dev = torch.device("cuda", 0)
    ops = torch.ops.cerberus
    up = lambda a: torch.from_numpy(a).to(dev)
    jobs = []
    if name == "seg":
        B, C, H, W = SEG_SHAPE
        n = _copies(4 * C * B * H * W)
        x, t = up(cases.logits(SEG_SHAPE, 10)), up(cases.labels(SEG_SHAPE, 15))
        sets = [({"seg": torch.roll(x, i, -1)}, {"seg": torch.roll(t, i, -1)}) for i in range(n)]
        jobs.append(("x".join(map(str, SEG_SHAPE)), lambda backend: ca.SegmentationMetric(C, backend=backend), sets,
                     lambda p, tg: ops.seg_confusion(p["seg"], tg["seg"], 255), (4 * C + 8) * B * H * W))
    elif name == "depth":
        for shape in DEPTH_SHAPES:
            B, _, H, W = shape
            n = _copies(8 * B * H * W)
            p, g = (up(a) for a in cases.depth_inputs((B, H, W), seed=20, check=False))
            sets = [({"depth": torch.roll(p, i, -1)}, {"disparity": torch.roll(g, i, -1)}) for i in range(n)]
            jobs.append(("x".join(map(str, shape)), lambda backend: ca.DepthMetric(backend=backend), sets,
                         lambda pr, tg: ops.depth_metric_sums(pr["depth"], tg["disparity"], 0.0, 80.0), 8 * B * H * W))
    else:
        B, H, W = FLOW_SHAPE
        n = _copies((20 + 24) * B * H * W)
        fp, fg, mask = (up(a) for a in cases.flow_inputs(FLOW_SHAPE, seed=30, check=False))
        img, seq, _ = (up(a) for a in cases.warp_inputs((B, 3, H, W), 35))
        sets = [({"flow": torch.roll(fp, i, -1)}, {"flow": torch.roll(fg, i, -1), "flow_mask": torch.roll(mask, i, -1),
                                                   "l_img": torch.roll(img, i, -1), "l_seq": torch.roll(seq, i, -1)}) for i in range(n)]

        def fused_ops(p, tg):
            ops.flow_metric_sums(p["flow"], tg["flow"], tg["flow_mask"])
            ops.warp_sad(tg["l_img"], tg["l_seq"], p["flow"])
        jobs.append(("4x(2|3)x512x1024", lambda backend: ca.OpticFlowMetric(backend=backend), sets, fused_ops, (20 + 32) * B * H * W))
    for shape, make, sets, kernels, nbytes in jobs:
        metrics = {"fused": make("hip"), "stock": make("torch")}

        def sample(metric, p, tg):
            metric.add_sample(p, tg)
            if len(metric.metric_data["Batch_Loss"]) > 64:
                metric._reset_metric()
        res = _time_alternating({label: [lambda m=m, p=p, tg=tg: sample(m, p, tg) for p, tg in sets] for label, m in metrics.items()},
                                passes)
        alone = _time_alternating({"kernels": [lambda p=p, tg=tg: kernels(p, tg) for p, tg in sets]}, passes)
        rec = {"section": name, "shape": shape, "copies": len(sets), "alg_bytes": nbytes, "stock_us": res["stock"] * 1e6,
               "fused_us": res["fused"] * 1e6, "kernels_us": alone["kernels"] * 1e6}
        print("ROW " + json.dumps(rec), flush=True)
        del sets
        torch.cuda.empty_cache()


def table(rows):
    titles = {"seg": "SegmentationMetric(19).add_sample", "depth": "DepthMetric().add_sample", "flow": "OpticFlowMetric().add_sample"}
    out = ["add_sample: us per call, device work and the one host copy; kernels: the fused ops alone, no copy; GB/s = bytes the fused "
           "kernels load / the kernels' time, % of the 8 TB/s HBM peak", ""]
    for name, _ in SECTIONS[:3]:
        out.append(titles[name])
        out.append("  %-18s %6s | %12s %12s %6s | %10s %7s %5s" % ("shape", "copies", "stock", "fused", "x", "kernels", "GB/s", "%"))
        for r in (r for r in rows if r["section"] == name):
            bw = r["alg_bytes"] / (r["kernels_us"] * 1e-6)
            out.append("  %-18s %6d | %12.1f %12.1f %6.2f | %10.1f %7.0f %5.1f" % (
                r["shape"], r["copies"], r["stock_us"], r["fused_us"], r["stock_us"] / r["fused_us"], r["kernels_us"], bw / 1e9,
                100 * bw / HBM_PEAK))
        out.append("")
    out.append("single ops at the shapes above (us per call, no copy)")
    out.append("  %-62s %6s | %10s %7s %5s" % ("op", "copies", "us", "GB/s", "%"))
    for r in (r for r in rows if r["section"] == "kernels"):
        bw = r["alg_bytes"] / (r["us"] * 1e-6)
        out.append("  %-62s %6d | %10.1f %7.0f %5.1f" % (r["what"], r["copies"], r["us"], bw / 1e9, 100 * bw / HBM_PEAK))
    out.append("")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "metrics_fused.txt"))
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    if args.section:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_metrics: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.passes)
    rows = []
    for name, limit in SECTIONS:
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_metrics: section %s exceeded %d s; stopping" % (name, limit))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_metrics: section %s failed (%d); stopping" % (name, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
