#!/usr/bin/env python3
"""Time the panoptic training ops (csrc/panoptic_train.hip) against the stock device chains on one MI355X.

    python tools/prof_panoptic_train.py [--out profiles/panoptic_train_fused.txt]

Method: the fused op and the stock chain alternate in one process, device events around each pass, median of 7 after two
warm-up passes.  Shapes: 4 x 512 x 1024 and 2 x 256 x 864, about 60 segments per image (a 6 x 10 grid of blocks, things and
stuff alternating, every seventh thing a crowd).  Timed: the targets (and, on the wall clock, a host numpy generator in the
style of the reference -- one full-image mask pass per use and segment -- for the record), the loss forward, and the loss
forward plus backward.  GB/s is against the bytes each op MUST move: 48 per pixel for the targets (an int64 id in; two int64
maps, a heat map, two offsets and three masks out), 32 for the loss forward (eight fp32 maps in), 76 with the backward (the
same eight again, three gradient maps out).
"""
import argparse
import subprocess
import sys
import time
import os

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cerberusnet_amd as ca  # noqa: E402
from cerberusnet_amd.synth import hash_uniform  # noqa: E402
from cerberusnet_amd.utilities.panoptic_targets import gaussian_table, panoptic_targets  # noqa: E402

THINGS = [11, 12, 13, 14, 15, 16, 17, 18]
REPEATS, WARMUP = 7, 2


def scene(B, H, W, rows=6, cols=10):
    """(ids (B,H,W) int64, seg_ids, seg_category, seg_iscrowd (B,S)): a grid of blocks with ragged borders."""
    ys = (np.arange(H) * rows // H)[:, None]
    xs = (np.arange(W) * cols // W)[None, :]
    ids, tables = [], []
    for b in range(B):
        wobble = (hash_uniform((H, W), 40 + b, 0.0, 1.0) < 0.02).astype(np.int64)        # two percent of the pixels join the next block
        block = np.minimum(ys * cols + xs + wobble, rows * cols - 1)
        cat = np.where(np.arange(rows * cols) % 2 == 0, 11 + np.arange(rows * cols) % 8, np.arange(rows * cols) % 11)
        seg = 1000 * cat + np.arange(rows * cols) + 1
        crowd = ((np.arange(rows * cols) % 14) == 0).astype(np.int64)
        ids.append(seg[block])
        tables.append((seg, cat, crowd))
    stack = lambda i: np.stack([t[i] for t in tables]).astype(np.int64)
    return np.stack(ids).astype(np.int64), stack(0), stack(1), stack(2)


def host_generator(ids, seg, cat, crowd, sigma, gauss):
    """The reference's method on the host, for the record: per segment one full-image comparison per use."""
    H, W = ids.shape
    semantic = np.full((H, W), 255, dtype=np.uint8)
    foreground = np.zeros((H, W), dtype=np.uint8)
    center = np.zeros((H, W), dtype=np.float32)
    offset = np.zeros((2, H, W), dtype=np.float32)
    center_mask = np.zeros((H, W), dtype=np.uint8)
    offset_mask = np.zeros((H, W), dtype=np.uint8)
    yc = np.arange(H, dtype=np.float32)[:, None] * np.ones((1, W), dtype=np.float32)
    xc = np.ones((H, 1), dtype=np.float32) * np.arange(W, dtype=np.float32)[None, :]
    size, reach = gauss.shape[0], gauss.shape[0] // 2
    for s, c, cr in zip(seg, cat, crowd):
        semantic[ids == s] = c
        if c in THINGS:
            foreground[ids == s] = 1
        if not cr:
            center_mask[ids == s] = 1
            offset_mask[ids == s] = 1
        if c in THINGS:
            idx = np.where(ids == s)
            if len(idx[0]) == 0:
                continue
            cy, cx = np.mean(idx[0]), np.mean(idx[1])
            top, left = int(cy) - reach, int(cx) - reach
            a, b, l, r = max(top, 0), min(top + size, H), max(left, 0), min(left + size, W)
            center[a:b, l:r] = np.maximum(center[a:b, l:r], gauss[a - top:b - top, l - left:r - left])
            offset[0][idx] = cy - yc[idx]
            offset[1][idx] = cx - xc[idx]
    return semantic, foreground, center, offset, center_mask, offset_mask


def timed(fns):
    """Median milliseconds of each function: they alternate, device events around each pass."""
    times = [[] for _ in fns]
    for it in range(WARMUP + REPEATS):
        for i, fn in enumerate(fns):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            if it >= WARMUP:
                times[i].append(start.elapsed_time(stop))
    return [float(np.median(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    except OSError:
        commit = ""
    say("panoptic training ops on %s, torch %s, commit %s" % (torch.cuda.get_device_name(0), torch.__version__, commit or "(no git)"))
    say("median of %d after %d warm-up passes, fused and stock alternating; GB/s against the bytes the op must move" % (REPEATS, WARMUP))
    say("%-28s %-14s %10s %10s %8s %9s" % ("op", "shape", "fused ms", "stock ms", "ratio", "GB/s"))
    dev = "cuda:0"
    for B, H, W in ((4, 512, 1024), (2, 256, 864)):
        ids, seg, cat, crowd = scene(B, H, W)
        t = [torch.from_numpy(a).to(dev) for a in (ids, seg, cat, crowd)]
        kw = dict(ignore_label=255, thing_list=THINGS, sigma=8, small_instance_area=4096, small_instance_weight=3)
        fused = lambda: panoptic_targets(*t, backend="hip", **kw)
        stock = lambda: panoptic_targets(*t, backend="torch", **kw)
        a, b = fused(), stock()
        assert all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a), "fused and stock targets differ"
        pixels = B * H * W
        f, s = timed([fused, stock])
        say("%-28s %-14s %10.3f %10.3f %8.2f %9.1f" % ("targets (%d segments)" % seg.shape[1], "%dx%dx%d" % (B, H, W), f, s, s / f, 48 * pixels / f / 1e6))
        g = gaussian_table(8).numpy()
        t0 = time.perf_counter()
        for i in range(B):
            host_generator(ids[i], seg[i], cat[i], crowd[i], 8, g)
        say("%-28s %-14s %10s %10.3f   (wall clock, numpy on the host, not counting the upload)" % ("targets, host loop", "%dx%dx%d" % (B, H, W), "", 1e3 * (time.perf_counter() - t0)))
        tg = {k: v for k, v in a.items() if k in ("center", "offset", "center_mask", "offset_mask")}
        cp = torch.from_numpy(hash_uniform((B, 1, H, W), 7, 0.0, 1.0)).to(dev)
        op = torch.from_numpy(hash_uniform((B, 2, H, W), 8, -40.0, 40.0)).to(dev)
        for masking in ("reference", "pixel"):
            def forward(backend, grad):
                p = {"center": cp.requires_grad_(grad), "offset": op.requires_grad_(grad)}
                v = ca.deeplab_panoptic_loss(p, tg, 200.0, 0.1, masking, backend=backend)
                if grad:
                    torch.autograd.grad(v, (p["center"], p["offset"]))
            for grad, nbytes, label in ((False, 32, "forward"), (True, 76, "forward+backward")):
                f, s = timed([lambda: forward("hip", grad), lambda: forward("torch", grad)])
                say("%-28s %-14s %10.3f %10.3f %8.2f %9.1f" % ("loss %s, %s" % (label, masking), "%dx%dx%d" % (B, H, W), f, s, s / f, nbytes * pixels / f / 1e6))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
