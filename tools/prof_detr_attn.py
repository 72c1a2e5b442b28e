#!/usr/bin/env python3
"""Times the DETR head's attention: the fused core (cerberus_attn::attention, csrc/detr_attn.hip) against the reference's route
(``nn.MultiheadAttention`` as nnet_models/detr/transformer.py calls it, default ``need_weights=True``) and, for information, against
``F.scaled_dot_product_attention`` in fp32 on the same projected tensors; eager forward + backward in train mode (attention dropout
0.1), on one GPU.

    python tools/prof_detr_attn.py [--out profiles/detr_attn_fused.txt] [--passes 9]

Rows per shape:
    core       ``detr_attention(q, k, v)`` against SDPA on the same (L,B,E) tensors viewed as (B,H,L,D): no projections
    attention  one ``nn.MultiheadAttention`` module with its projections: ``attend(..., backend='hip')`` against the module call
    layer      one ``TransformerEncoderLayer`` (self-attention shapes only), ``backend='hip'`` against ``backend='torch'``
Shapes (Lq, Lk, B, H; D = 32): the encoder at (2048, 2048, 2, 8); the decoder's cross-attention at (100, 2048, 2, 8); the workload's
own encoder, (32768, 32768, 4, 8), fused only -- the stock route's probability tensor is computed in bytes and printed, never
attempted.
Method (that of tools/prof_ocr_head.py): every call of a timed pass works on its own copy of the inputs, the copies of one pass
> 512 MiB in all (at most 16), 3 warm-up passes, HIP events around a whole pass, the routes alternating; the median over the passes
with the smallest and the largest pass beside it.  Each shape runs in a child process under a time limit of its own; the first
failure ends the run.  TFLOP/s counts the algorithm's 14 Lq Lk D B H flops (two products forward, five backward) against the
157.3 TFLOP/s fp32 matrix peak; the backward's recomputation is not counted."""
import argparse
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

# Lq, Lk, B, H, with the stock routes or without
SHAPES = ((2048, 2048, 2, 8, True), (100, 2048, 2, 8, True), (32768, 32768, 4, 8, False))
D, P, FF = 32, 0.1, 2048
LIMIT = 500
PEAK = 157.3e12


def section(index, passes):
    import torch
    import torch.nn.functional as F
    import attn_cases as cases
    import cerberusnet_amd as ca
    from cerberusnet_amd.nnet_models.detr.transformer import attend
    dev = torch.device("cuda", 0)
    Lq, Lk, B, H, stock = SHAPES[index]
    E = H * D
    n = _copies(4 * E * B * (2 * Lq + 2 * Lk))
    sets = [[t.to(dev) for t in cases.inputs(Lq, Lk, B, H, 10 + 5 * i)] for i in range(n)]
    for s in sets:
        for t in s[:3]:
            t.requires_grad_(True)
    rec = {"shape": (Lq, Lk, B, H), "copies": n, "stock": stock, "matrix_bytes": 4 * B * H * Lq * Lk}

    def fb(fn, inputs, up, params=()):
        torch.autograd.grad(fn(*inputs), list(inputs) + list(params), up)

    def sdpa(q, k, v):
        heads = lambda t: t.view(t.shape[0], B * H, D).transpose(0, 1).view(B, H, t.shape[0], D)
        out = F.scaled_dot_product_attention(heads(q), heads(k), heads(v), dropout_p=P)
        return out.permute(2, 0, 1, 3).reshape(Lq, B, E)

    def put(step, forms):
        for label, (med, lo, hi) in _time(forms, passes).items():
            rec["%s_%s_us" % (step, label)] = [med * 1e6, lo * 1e6, hi * 1e6]

    core = {"fused": lambda q, k, v: ca.detr_attention(q, k, v, H, None, P)}
    if stock:
        core["sdpa"] = sdpa
    put("core", {label: [lambda fn=fn, s=s: fb(fn, s[:3], s[3]) for s in sets] for label, fn in core.items()})

    mha = torch.nn.MultiheadAttention(E, H, dropout=P).to(dev).train()
    module = {"fused": "hip", "stock": "torch"} if stock else {"fused": "hip"}
    put("attention", {label: [lambda b=backend, s=s: fb(lambda q, k, v: attend(mha, q, k, v, backend=b), s[:3], s[3], mha.parameters())
                              for s in sets] for label, backend in module.items()})
    if Lq == Lk:
        layers = {label: ca.TransformerEncoderLayer(E, H, FF, P, backend=backend).to(dev).train() for label, backend in module.items()}
        put("layer", {label: [lambda m=m, s=s: fb(lambda x, pos: m(x, pos=pos), s[:2], s[3], m.parameters()) for s in sets]
                      for label, m in layers.items()})
    print("ROW " + json.dumps(rec), flush=True)


def table(rows):
    out = ["DETR attention, eager forward + backward, fp32, train mode (attention dropout %.1f), D = %d" % (P, D),
           "(us per call: median [smallest .. largest pass]; x = other route / fused; TF = 14 Lq Lk D B H flops / median, % of the "
           "157.3 TFLOP/s fp32 matrix peak)",
           "  core       detr_attention(q, k, v) against F.scaled_dot_product_attention (fp32, for information) on the same tensors",
           "  attention  one nn.MultiheadAttention with its projections: the fused route against the module as the reference calls it",
           "  layer      one TransformerEncoderLayer (feed-forward %d): backend='hip' against backend='torch'" % FF, ""]
    for r in rows:
        Lq, Lk, B, H = r["shape"]
        flops = 14.0 * Lq * Lk * D * B * H
        out.append("  Lq %d  Lk %d  B %d  H %d  (%d input copies per pass)" % (Lq, Lk, B, H, r["copies"]))
        if not r["stock"]:
            out.append("    stock routes: does not fit: %.0f GB for ONE (B H, Lq, Lk) fp32 probability tensor; not attempted"
                       % (r["matrix_bytes"] / 1e9))
        for step, other in (("core", "sdpa"), ("attention", "stock"), ("layer", "stock")):
            f = r.get(step + "_fused_us")
            if f is None:
                continue
            line = "    %-10s fused %10.1f [%10.1f .. %10.1f]" % (step, f[0], f[1], f[2])
            if step == "core":
                rate = flops / (f[0] * 1e-6)
                line += "   %6.1f TF %5.1f %%" % (rate / 1e12, 100 * rate / PEAK)
            s = r.get("%s_%s_us" % (step, other))
            if s is not None:
                line += "   %-5s %10.1f [%10.1f .. %10.1f]   x %5.2f" % (other, s[0], s[1], s[2], s[0] / f[0])
            out.append(line)
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", type=int)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detr_attn_fused.txt"))
    ap.add_argument("--passes", type=int, default=9)
    args = ap.parse_args()
    if args.section is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prof_detr_attn: no GPU (a timing needs one; there is no fallback)")
        return section(args.section, args.passes)
    rows = []
    for index, shape in enumerate(SHAPES):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", str(index), "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            raise SystemExit("prof_detr_attn: shape %s exceeded %d s; stopping" % (shape, LIMIT))
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("prof_detr_attn: shape %s failed (%d); stopping" % (shape, res.returncode))
        rows += [json.loads(line[4:]) for line in res.stdout.splitlines() if line.startswith("ROW ")]
    text = table(rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
