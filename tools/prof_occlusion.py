#!/usr/bin/env python3
"""Times the occlusion ops (csrc/occlusion.hip) against this package's own stock-op formulations, on one GPU in one process
per section.

    python tools/prof_occlusion.py [--out profiles/occlusion_ops.txt] [--pairs 4] [--passes 7]

For the four loss scales at `pairs` flow pairs, on a smooth flow family (a smooth +-6 px field + +-0.25 px noise and a
roughly inverse one) and a noisy one (+-8 px white noise: no two neighbours land together, nearly every tap of the splat
misses the LDS window and goes to memory directly):
  backward     get_occu_mask_backward(flow21)            HIP: cerberus::corresponding_map + one comparison chain
               vs _occu_mask_backward_stock              (device-built mesh, ~45 launches, float scatter_add_)
  map          cerberus::corresponding_map alone vs _corresponding_map_stock on mesh + flow
  bidirection  cerberus::occlusion_mask_bidirection      vs _occu_mask_bidirection_stock (grid_sample + ~12 launches)
Method (that of tools/prof_photometric.py): every call of a timed pass works on its own copy of the inputs, 3 warm-up
passes, HIP events around a whole pass, the median over `passes` passes, op and stock chain in the same process one after
the other.  Each section runs in a child process under a time limit of its own; the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from prof_photometric import SCALES, _copies, _time  # noqa: E402

SECTIONS = (("smooth", 240), ("noisy", 240))


def _pair(torch, hash_uniform, B, H, W, family, seed):
    t = lambda shape, s, amp: torch.from_numpy(hash_uniform(shape, s, -amp, amp))
    if family == "noisy":
        return t((B, 2, H, W), seed, 8.0), t((B, 2, H, W), seed + 1, 8.0)
    up = lambda s, amp: torch.nn.functional.interpolate(t((B, 2, max(2, H // 8), max(2, W // 8)), s, amp), size=(H, W),
                                                        mode="bilinear", align_corners=True)
    f12 = up(seed, 6.0) + t((B, 2, H, W), seed + 1, 0.25)
    return f12, -f12 + up(seed + 2, 1.5) + t((B, 2, H, W), seed + 3, 0.25)


def section(name, pairs, passes):
    import torch
    import cerberusnet_amd as ca
    from cerberusnet_amd.loss_functions import UnFlowLoss as U
    from cerberusnet_amd.synth import hash_uniform
    dev = torch.device("cuda", 0)
    forms = {
        "backward": (lambda a, b: ca.get_occu_mask_backward(b), lambda a, b: U._occu_mask_backward_stock(b, 0.2)),
        "map": (lambda a, b: torch.ops.cerberus.corresponding_map(b, True),
                lambda a, b: U._corresponding_map_stock(U.mesh_grid(*b.shape[:1], *b.shape[2:], device=b.device).type_as(b) + b)),
        "bidirection": (lambda a, b: ca.get_occu_mask_bidirection(a, b), lambda a, b: U._occu_mask_bidirection_stock(a, b, 0.01, 0.5)),
    }
    with torch.no_grad():
        for H, W in SCALES:
            nbytes = 4 * pairs * 2 * H * W
            n = _copies(2 * nbytes)
            sets = [tuple(f.to(dev) for f in _pair(torch, hash_uniform, pairs, H, W, name, 100 + 10 * i)) for i in range(n)]
            rec = {"family": name, "scale": "%dx%d" % (H, W), "copies": n}
            for label, (op, stock) in forms.items():
                assert op(*sets[0]).shape == stock(*sets[0]).shape
                rec[label + "_op_us"] = _time([lambda a=a, b=b: op(a, b) for a, b in sets], passes) * 1e6
                rec[label + "_stock_us"] = _time([lambda a=a, b=b: stock(a, b) for a, b in sets], passes) * 1e6
            print("ROW " + json.dumps(rec), flush=True)
            del sets
            torch.cuda.empty_cache()


def table(rows):
    out = ["occlusion ops against this package's stock-op formulations (us per eager call, 4 flow pairs unless said; x = stock / op)",
           "  %-7s %-10s %6s | %10s %9s %6s | %10s %9s %6s | %10s %9s %6s" % (
               "flows", "scale", "copies", "stock back", "HIP back", "x", "stock map", "HIP map", "x", "stock bidi", "HIP bidi", "x")]
    for r in rows:
        cells = []
        for label in ("backward", "map", "bidirection"):
            s, o = r[label + "_stock_us"], r[label + "_op_us"]
            cells.append("%10.1f %9.1f %6.1f" % (s, o, s / o))
        out.append("  %-7s %-10s %6d | %s" % (r["family"], r["scale"], r["copies"], " | ".join(cells)))
    full = [r for r in rows if r["scale"] == "%dx%d" % SCALES[0]]
    for label in ("backward", "bidirection"):
        ok = all(r[label + "_op_us"] < r[label + "_stock_us"] for r in full)
        out.append("%s at %dx%d: the HIP op %s its stock chain on %s" % (
            label, SCALES[0][0], SCALES[0][1], "beats" if ok else "DOES NOT beat", " and ".join(r["family"] for r in full) + " flows"))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occlusion_ops.txt"))
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    if args.section:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_occlusion: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.pairs, args.passes)
    rows = []
    for name, limit in SECTIONS:
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--pairs", str(args.pairs), "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_occlusion: section %s exceeded %d s; stopping" % (name, limit))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_occlusion: section %s failed (%d); stopping" % (name, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
