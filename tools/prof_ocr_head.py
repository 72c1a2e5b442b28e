#!/usr/bin/env python3
"""Times the OCR segmentation head's two own steps and the whole ``OCR_block``: the fused route (``backend='hip'``:
cerberus_ocr::spatial_gather / object_attention, csrc/ocr_head.hip) against the stock chain (``backend='torch'``: softmax + matmul;
two matmuls, scale, softmax and the permuted copy) in the same process, eager forward + backward, on one GPU.

    python tools/prof_ocr_head.py [--out profiles/ocr_head_fused.txt] [--passes 9]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prof_ocr_head.py --kernels 0
    python tools/prof_ocr_head.py --stats DIR --shape 0 >> profiles/ocr_head_fused.txt

Shapes: the model's (1024 x 512 input, stride 4: (4, 512, 128, 256) features, 256 key channels, 19 classes) and (2, 512, 64, 216).
The whole block takes a (B, 480, H, W) input (the W32 backbone's concatenated features).
Method (that of tools/prof_seg_loss.py): every call of a timed pass works on its own copy of the inputs, the copies of one pass
> 512 MiB in all, 3 warm-up passes, HIP events around a whole pass, fused and stock passes alternating; the median over the
passes with the smallest and the largest pass beside it.  Each shape runs in a child process under a time limit of its own; the
first failure ends the run.
``--kernels`` makes a few plain calls of the four raw ops for a kernel-trace run of its own; ``--stats`` turns that run's
kernel_stats CSV into per-kernel device times and achieved bytes/s (the bytes the algorithm needs, from the shapes) against the
8 TB/s HBM peak."""
import argparse
import csv
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

# B, mid channels, H, W; key channels and classes are the model's
SHAPES = ((4, 512, 128, 256), (2, 512, 64, 216))
KEY, CLASSES, HIGH = 256, 19, 480
LIMIT = 500
HBM_PEAK = 8.0e12
CHUNK = 256


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


def _inputs(index, n, dev):
    import ocr_cases as cases
    B, C, H, W = SHAPES[index]
    gather = [[t.to(dev) for t in cases.gather_inputs(B, C, CLASSES, H, W, 10 + 5 * i)] for i in range(n)]
    attention = [[t.to(dev) for t in cases.attention_inputs(B, KEY, CLASSES, H, W, 100 + 5 * i)] for i in range(n)]
    return gather, attention


def section(index, passes):
    import torch
    import cerberusnet_amd as ca
    import ocr_cases as cases
    dev = torch.device("cuda", 0)
    B, C, H, W = SHAPES[index]
    n = _copies(4 * B * C * H * W)
    gather, attention = _inputs(index, n, dev)
    for group in gather + attention:
        for t in group[:-1]:
            t.requires_grad_(True)
    scale = KEY ** -0.5
    rec = {"shape": "x".join(map(str, SHAPES[index])), "copies": n}

    def fb(fn, inputs, up):
        torch.autograd.grad(fn(*inputs), inputs, up)
    steps = {
        "gather": ({"fused": lambda f, x: ca.spatial_gather(f, x, 1.0).unsqueeze(3), "stock": cases.gather_chain}, gather),
        "attention": ({"fused": lambda q, k, v: ca.object_attention(q, k, v, scale),
                       "stock": lambda q, k, v: cases.attention_chain(q, k, v, scale)}, attention),
    }
    for step, (fns, sets) in steps.items():
        res = _time({label: [lambda fn=fn, s=s: fb(fn, s[:-1], s[-1]) for s in sets] for label, fn in fns.items()}, passes)
        for label, (med, lo, hi) in res.items():
            rec["%s_%s_us" % (step, label)] = [med * 1e6, lo * 1e6, hi * 1e6]
    del gather, attention, steps
    torch.cuda.empty_cache()
    blocks = {label: ca.OCR_block(HIGH, mid_channels=C, key_channels=KEY, classes=CLASSES, backend=backend).to(dev).train()
              for label, backend in (("fused", "hip"), ("stock", "torch"))}
    blocks["stock"].load_state_dict(blocks["fused"].state_dict())
    xs = [cases.tensor((B, HIGH, H, W), 300 + i).to(dev).requires_grad_(True) for i in range(2)]

    def block_fb(block, x):
        torch.autograd.grad(cases.block_loss(*block(x)), [x] + list(block.parameters()))
    res = _time({label: [lambda b=b, x=x: block_fb(b, x) for x in xs] for label, b in blocks.items()}, passes)
    for label, (med, lo, hi) in res.items():
        rec["block_%s_us" % label] = [med * 1e6, lo * 1e6, hi * 1e6]
    print("ROW " + json.dumps(rec), flush=True)


def kernels(index, reps=5):
    """Plain calls of the four raw ops (1 warm-up + ``reps``), for a kernel-trace run."""
    import torch
    dev = torch.device("cuda", 0)
    gather, attention = _inputs(index, 1, dev)
    f, x, g = gather[0]
    q, k, v, up = attention[0]
    op = torch.ops.cerberus_ocr
    for _ in range(reps + 1):
        ctx, _ = op.spatial_gather(f, x, 1.0)
        op.spatial_gather_backward(f, x, ctx, g.squeeze(3), 1.0)
        _, attn = op.object_attention(q, k, v, KEY ** -0.5)
        op.object_attention_backward(up, q, k, v, attn, KEY ** -0.5)
    torch.cuda.synchronize()


def kernel_bytes(index):
    """{substring of the kernel's name: (what, the bytes the algorithm needs)} at one shape."""
    B, C, H, W = SHAPES[index]
    hw, R = H * W, CLASSES
    chunks = (hw + CHUNK - 1) // CHUNK
    return {
        "ocr_row_stats_kernel": ("row statistics (logits, once)", 4 * B * R * hw),
        "ocr_pool_kernel<true>": ("gather forward: features + logits + partials", 4 * B * (hw * (C + R) + chunks * C * R)),
        "ocr_gather_bwd_kernel": ("gather backward: features, logits in; both gradients out", 4 * B * hw * (2 * C + 2 * R)),
        "ocr_attn_fwd_kernel": ("attention forward: query in; context, attn out", 4 * B * hw * (2 * KEY + R)),
        "ocr_attn_bwd_kernel": ("attention backward: grad, attn in; grad_query, dsim out", 4 * B * hw * (2 * KEY + 2 * R)),
        "ocr_pool_kernel<false>": ("dkey / dvalue: a (B,Kc,HW) and a (B,R,HW) tensor + partials",
                                   4 * B * (hw * (KEY + R) + chunks * KEY * R)),
    }


def stats(directory, index):
    paths = [os.path.join(root, f) for root, _, files in os.walk(directory) for f in files if f.endswith("kernel_stats.csv")]
    if not paths:
        raise SystemExit("prof_ocr_head: no kernel_stats.csv under %s" % directory)
    rows = list(csv.DictReader(open(sorted(paths)[0])))
    out = ["", "per-kernel device times at %s, key %d, %d classes (rocprofv3 --kernel-trace --stats, a run of its own: 1 warm-up + 5 "
           "calls of each raw op; us; GB/s = the bytes the algorithm needs / average time, %% of the 8 TB/s HBM peak)"
           % ("x".join(map(str, SHAPES[index])), KEY, CLASSES),
           "  %-28s %5s %9s %9s %8s %6s  %s" % ("kernel", "calls", "avg us", "min us", "GB/s", "%", "bytes counted")]
    table = kernel_bytes(index)
    for r in rows:
        name = r.get("Name", "")
        if "ocr_" not in name:
            continue
        avg, lo, calls = float(r["AverageNs"]) * 1e-3, float(r["MinNs"]) * 1e-3, int(r["Calls"])
        short = name.split("ocr_", 1)[1].split("(")[0]
        hit = [v for key, v in table.items() if key in name]
        if hit:
            what, nbytes = hit[0]
            rate = nbytes / (avg * 1e-6)
            out.append("  %-28s %5d %9.1f %9.1f %8.0f %6.1f  %s" % ("ocr_" + short, calls, avg, lo, rate / 1e9, 100 * rate / HBM_PEAK, what))
        else:
            out.append("  %-28s %5d %9.1f %9.1f %8s %6s  (a small launch)" % ("ocr_" + short, calls, avg, lo, "-", "-"))
    print("\n".join(out))


def table(rows):
    out = ["OCR head, eager forward + backward, fp32: fused (backend='hip') against the stock chain (backend='torch') in one process",
           "(us per call: median [smallest .. largest pass]; x = stock / fused; key %d, %d classes; the block takes (B,%d,H,W))"
           % (KEY, CLASSES, HIGH), ""]
    for r in rows:
        out.append("  %s  (%d input copies per pass)" % (r["shape"], r["copies"]))
        for step in ("gather", "attention", "block"):
            s, f = r[step + "_stock_us"], r[step + "_fused_us"]
            out.append("    %-10s stock %9.1f [%9.1f .. %9.1f]   fused %9.1f [%9.1f .. %9.1f]   x %5.2f"
                       % (step, s[0], s[1], s[2], f[0], f[1], f[2], s[0] / f[0]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", type=int)
    ap.add_argument("--kernels", type=int)
    ap.add_argument("--stats")
    ap.add_argument("--shape", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ocr_head_fused.txt"))
    ap.add_argument("--passes", type=int, default=9)
    args = ap.parse_args()
    if args.stats is not None:
        return stats(args.stats, args.shape)
    if args.section is not None or args.kernels is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_ocr_head: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.passes) if args.section is not None else kernels(args.kernels)
    rows = []
    for index, shape in enumerate(SHAPES):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", str(index), "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_ocr_head: shape %s exceeded %d s; stopping" % (shape, LIMIT))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_ocr_head: shape %s failed (%d); stopping" % (shape, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
