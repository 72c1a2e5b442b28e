#!/usr/bin/env python3
"""A few plain launches of the warp ops per level (for rocprofv3 --kernel-trace --stats).

    prof_warp.py [levels] [pad] [mode] [dtype] [config]

levels: comma list (default 3); pad: zeros / border (default) / reflection; mode: bilinear (default) / nearest;
dtype: float32 (default) / float16 / bfloat16; config: 3 (1024 x 512 pyramid, default) / 5 (2048 x 1024)."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cerberusnet_amd  # noqa: F401
from cerberusnet_amd.ops import PAD_MODES, INTERP_MODES
from cerberusnet_amd.synth import hash_uniform, pyramid_shapes
from bench import Workload
ops = torch.ops.cerberus
arg = lambda k, d: sys.argv[k] if len(sys.argv) > k else d   # noqa: E731
levels = [int(v) for v in arg(1, "3").split(",")]
pad, mode = PAD_MODES[arg(2, "border")], INTERP_MODES[arg(3, "bilinear")]
dtype = getattr(torch, arg(4, "float32"))
shapes = pyramid_shapes(2048, 1024) if arg(5, "3") == "5" else pyramid_shapes()
for lvl in levels:
    C, H, W = shapes[lvl]
    B = 4
    img = torch.from_numpy(hash_uniform((B, C, H, W), 1)).cuda().to(dtype)
    go = torch.from_numpy(hash_uniform((B, C, H, W), 2)).cuda().to(dtype)
    fl = Workload._flow(B, H, W, 3, "smooth", "cuda").to(dtype)
    for _ in range(20):
        out, ctx = ops.flow_warp_ctx(img, fl, pad, mode)
        ops.flow_warp_backward_ctx(img, fl, ctx, go, pad, mode, True, True)
    torch.cuda.synchronize()
