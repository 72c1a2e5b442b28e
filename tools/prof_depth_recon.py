#!/usr/bin/env python3
"""Times the stereo reprojection warp of the depth reconstruction loss: the stock-op chain (BackprojectDepth -> Project3D ->
grid_sample, ``depth_losses._reproject_stock``) against the HIP op (cerberus::reproject_warp), on one GPU.

    python tools/prof_depth_recon.py [--out profiles/depth_recon.txt] [--items 4] [--passes 7]

For `items` 3-channel images at 512 x 1024 and 256 x 512: eager microseconds per call, forward and forward + backward to the
depth, of (a) the op and (b) the stock chain; ``flow_warp`` forward and forward + grad_flow on the same image shape in the
same run, as a kernel of the same traffic class (it reads a 2-channel flow where this op reads a 1-channel depth); and the
whole loss, ``DepthReconstructionLossV1`` with backend 'hip' against 'torch'.
Method (that of tools/prof_photometric.py): every call of a timed pass works on its own copy of the inputs, the copies of
one pass > 512 MiB in all where memory allows, 3 warm-up passes, HIP events around a whole pass, the median over `passes`
passes.  Algorithmic bytes of the op: image + depth read, image-sized output written forward; image + depth + grad_out read
and a depth-sized gradient written more for the backward.  The section runs in a child process under a time limit."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from prof_photometric import _copies, _time  # noqa: E402

SCALES = ((512, 1024), (256, 512))
LIMIT = 420


def section(items, passes):
    import torch
    import cerberusnet_amd as ca
    from cerberusnet_amd.loss_functions import depth_losses as D
    from cerberusnet_amd.synth import hash_uniform, stereo_camera, stereo_depth
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a).to(dev)
    for H, W in SCALES:
        shape = (items, 3, H, W)
        img_b, dep_b = 4 * items * 3 * H * W, 4 * items * H * W
        n = _copies(img_b + dep_b)
        mats = [t(m) for m in stereo_camera(items, H, W, "cityscapes")]
        sets = [(t(hash_uniform(shape, 10 + i, 0.0, 1.0)), t(stereo_depth(items, H, W, 40 + 2 * i)).requires_grad_(True))
                for i in range(n)]
        flows = [t(hash_uniform((items, 2, H, W), 80 + i, 1.0, 6.0)).requires_grad_(True) for i in range(n)]
        r_img = t(hash_uniform(shape, 9, 0.0, 1.0))
        alg = (2 * img_b + dep_b, 4 * img_b + 3 * dep_b)
        rec = {"scale": "%dx%d" % (H, W), "copies": n, "cold": bool(n * (img_b + dep_b) >= (512 << 20)),
               "alg_bytes_fwd": alg[0], "alg_bytes_fwd_bwd": alg[1]}
        forms = [("op", lambda img, d: ca.reproject_warp(img, d, *mats)),
                 ("stock", lambda img, d: D._reproject_stock(img, d, *mats, 1e-7))]
        for label, fn in forms:
            def fwd(a, b, fn=fn):
                with torch.no_grad():
                    fn(a, b)

            def both(a, b, fn=fn):
                torch.autograd.grad(fn(a, b).sum(), b)
            rec[label + "_fwd_us"] = _time([lambda a=a, b=b: fwd(a, b) for a, b in sets], passes) * 1e6
            rec[label + "_fwd_bwd_us"] = _time([lambda a=a, b=b: both(a, b) for a, b in sets], passes) * 1e6

        def warp_fwd(a, f):
            with torch.no_grad():
                ca.flow_warp(a, f, pad="border")
        rec["flow_warp_fwd_us"] = _time([lambda a=a, f=f: warp_fwd(a, f) for (a, _), f in zip(sets, flows)], passes) * 1e6
        rec["flow_warp_fwd_bwd_us"] = _time([lambda a=a, f=f: torch.autograd.grad(ca.flow_warp(a, f, pad="border").sum(), f)
                                             for (a, _), f in zip(sets, flows)], passes) * 1e6
        for backend in ("hip", "torch"):
            loss = ca.DepthReconstructionLossV1(items, H, W, pred_type="depth", backend=backend)
            cam = {"inv_K": mats[0], "K": mats[1], "baseline_T": mats[2]}
            rec["loss_%s_fwd_bwd_us" % backend] = _time(
                [lambda a=a, b=b: torch.autograd.grad(loss({"depth": b}, {"camera": cam, "l_img": a, "r_img": r_img}), b)
                 for a, b in sets], passes) * 1e6
        print("ROW " + json.dumps(rec), flush=True)
        del sets, flows
        torch.cuda.empty_cache()


def table(rows, items):
    out = ["reprojection warp, %d x 3 channels (us per call, eager; x = stock / op; GB/s = algorithmic bytes of the op / its time; "
           "cold = inputs from HBM)" % items,
           "  %-10s %6s %5s | %10s %10s %7s %8s | %10s %10s %7s %8s" % (
               "scale", "copies", "cold", "stock fwd", "op fwd", "x", "GB/s", "stock f+b", "op f+b", "x", "GB/s")]
    for r in rows:
        out.append("  %-10s %6d %5s | %10.1f %10.1f %7.1f %8.0f | %10.1f %10.1f %7.1f %8.0f" % (
            r["scale"], r["copies"], "yes" if r["cold"] else "no",
            r["stock_fwd_us"], r["op_fwd_us"], r["stock_fwd_us"] / r["op_fwd_us"], r["alg_bytes_fwd"] / r["op_fwd_us"] / 1e3,
            r["stock_fwd_bwd_us"], r["op_fwd_bwd_us"], r["stock_fwd_bwd_us"] / r["op_fwd_bwd_us"],
            r["alg_bytes_fwd_bwd"] / r["op_fwd_bwd_us"] / 1e3))
    for r in rows:
        out.append("  flow_warp (3 channels, no grad_image) at %s in the same run: fwd %.1f us, fwd + grad_flow %.1f us; the op's fwd "
                   "= %.2f x, fwd + bwd = %.2f x that" % (r["scale"], r["flow_warp_fwd_us"], r["flow_warp_fwd_bwd_us"],
                                                           r["op_fwd_us"] / r["flow_warp_fwd_us"],
                                                           r["op_fwd_bwd_us"] / r["flow_warp_fwd_bwd_us"]))
    for r in rows:
        out.append("  DepthReconstructionLossV1 fwd + bwd at %s: backend='torch' %.1f us, backend='hip' %.1f us (%.1f x)" % (
            r["scale"], r["loss_torch_fwd_bwd_us"], r["loss_hip_fwd_bwd_us"], r["loss_torch_fwd_bwd_us"] / r["loss_hip_fwd_bwd_us"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_recon.txt"))
    ap.add_argument("--items", type=int, default=4)
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    if args.section:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_depth_recon: no GPU (a timing needs one; there is no fallback)")
        return section(args.items, args.passes)
    cmd = [sys.executable, os.path.abspath(__file__), "--section", "--items", str(args.items), "--passes", str(args.passes)]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        raise SystemExit("prof_depth_recon: exceeded %d s; stopping" % LIMIT)
    if res.returncode != 0:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        raise SystemExit("prof_depth_recon: failed (%d); stopping" % res.returncode)
    rows = [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows, args.items)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
