#!/usr/bin/env python3
"""Headline benchmark: image-pairs/s of the correlation + flow-warp hot path,
forward + backward, on the HRNetV2-W32 feature pyramid of a 1024x512 frame pair.

    python bench.py --gpus N --steps K --warmup W

N > 1: one process per GPU over RCCL.  Under torchrun (RANK / WORLD_SIZE set) the process is
one rank; launched plainly, the parent starts `python -m torch.distributed.run` with N
children BEFORE it touches the GPU, relays rank 0's JSON line and exits with their code.
Every rank owns `--pairs` image pairs (weak scaling).  Default step by N:
  N = 1  --step ops   : the hot-path ops alone (below): the headline (roofline and cpu_baseline with --full)
  N > 1  --step model : one TRAINING step of the host model (HRNetV2-W32 backbone + PWC flow head, unFlowLoss,
                        backward, Adam) under DistributedDataParallel over RCCL: 122 MB of gradients all-reduced
                        inside every step -- the step data-parallel scaling is judged on; read it against
                        `extra.model_step` of the N = 1 --full line (the same step on one GPU)
`--step ops` at N > 1 reports the op-only rate of the N ranks (the ops have no parameters: no collective
belongs to them) with the model-sized exchange timed beside it as `gradient_exchange`; `--step head` is the
flow head alone under DDP.  Every N > 1 line carries `single_gpu_step` and `scaling_efficiency` = value /
(N x single_gpu_step) at its top level: the like-for-like ratio of the step `config.step` names.
`--device cpu` (gloo) is the dry run of the N > 1 route on a box without GPUs: the same launcher, rendezvous, DDP
wrap, timed region, no_sync pass and rank gather, on a small host model with the stock-PyTorch fallback ops.

One "step" = the hot path of one training iteration over a batch of `--pairs`
image pairs (default 4 per GPU, BASELINE config 4's per-GPU batch; the tensors
are BASELINE config 3's: W32 pyramid, 1024x512, d=4, fp32): for both flow
directions and all four pyramid levels, in the order PWCNetHead issues them
(reference pwcnet_sfd.py:171-197, cerberus.py:131,135):

    forward : [flow_warp(f2, flow)] -> correlation(f1, warped)          (L0 has no warp)
    backward: correlation_backward -> [flow_warp_backward]

Inputs are synthetic (portable hash generator), resident in HBM before the
timed region.  The timed region replays the whole step from a hipGraph
(captured through torch.cuda.CUDAGraph; --no-graph launches eagerly).
`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy.

A plain run sets up, warms up, times the K steps and prints the headline.  With
`--full` the JSON line also carries
  roofline     : achieved algorithmic GB/s of the dominant kernel, measured
                 live with HIP events on the launch stream, vs the 8 TB/s HBM peak
  cpu_baseline : the reference's pure-PyTorch CPU correlation (oracle port of
                 CorrelationTorch, correlation.py:4-21) fwd+bwd on the same
                 pyramid, timed on this box's host cores on a bounded sample
and the steady-state, after-idle and stock-PyTorch GPU passes and the extra
configurations (extra.*) of the op step.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
METRIC = "image-pairs/sec fwd+bwd @1024×512 d=4; correlation HBM GB/s vs roofline"
CORR_P = (4, 1, 4, 1, 1, 1)  # pad, k, d, s1, s2, corr_type_multiply (pwcnet_sfd.py:131-133)


def corr_bytes(C, B, H, W, e=4):
    """ALGORITHMIC bytes: fwd (2C+81)BHWe, bwd (4C+81)BHWe."""
    return (2 * C + 81) * B * H * W * e, (4 * C + 81) * B * H * W * e


def warp_bytes(C, B, H, W, e=4):
    return (2 * C + 2) * B * H * W * e, (3 * C + 4) * B * H * W * e


class Workload:
    """Device-resident tensors of one step + the op sequence."""

    @staticmethod
    def _flow(pairs, H, W, seed, kind, device):
        """Synthetic flow field in pixels.  'smooth' mimics what PWCNetHead feeds the warp:
        a coarse field upsampled bilinearly (pwcnet_sfd.py:176) -- here a random (H/8, W/8)
        field in [-6, 6) px, x8 bilinear, plus +-0.25 px of per-pixel residual.  'noise' is
        the adversarial case used by the parity tests: independent uniform [-6, 6) per pixel."""
        from cerberusnet_amd.synth import hash_uniform
        if kind == "noise":
            return torch.from_numpy(hash_uniform((pairs, 2, H, W), seed, -6.0, 6.0)).to(device)
        coarse = torch.from_numpy(hash_uniform((pairs, 2, max(2, H // 8), max(2, W // 8)), seed,
                                               -6.0, 6.0))
        up = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear",
                                             align_corners=True)
        up = up + torch.from_numpy(hash_uniform((pairs, 2, H, W), seed + 100, -0.25, 0.25))
        return up.contiguous().to(device)

    def __init__(self, pairs, width, height, device, flow_kind="smooth", fuse=False, chains=1,
                 dtype=torch.float32):
        from cerberusnet_amd.synth import hash_uniform, pyramid_shapes
        import cerberusnet_amd  # noqa: F401  registers torch.ops.cerberus.*
        self.levels = pyramid_shapes(width, height, 32)
        self.pairs = pairs
        self.dtype = dtype
        self.esize = torch.empty(0, dtype=dtype).element_size()
        self.stagger = True
        self.dirs = []
        if pairs % chains:
            raise SystemExit("--chains must divide --pairs")
        pairs = pairs // chains
        # `chains` > 1: every direction's batch is split into that many independent
        # sub-batches (the op is stateless and batch items never interact)
        for direction in range(2 * chains):
            lv = []
            for l, (C, H, W) in enumerate(self.levels):
                seed = 16 * direction + 4 * l
                t = lambda shape, s, lo=-1.0, hi=1.0: torch.from_numpy(
                    hash_uniform(shape, seed + s, lo, hi)).to(device=device, dtype=dtype)
                lv.append(dict(
                    f1=t((pairs, C, H, W), 0), f2=t((pairs, C, H, W), 1),
                    gout=t((pairs, 81, H, W), 2),
                    flow=(self._flow(pairs, H, W, seed + 3, flow_kind, device).to(dtype)
                          if l > 0 else None)))
            self.dirs.append(lv)
        if fuse:
            # both directions as ONE batched call per op (2*pairs items): what a caller does
            # that stacks (enc, enc_bw) and (enc_bw, enc) before entering the head
            fused = []
            for a, b in zip(*self.dirs):
                fused.append({k: (torch.cat([a[k], b[k]], 0) if a[k] is not None else None)
                              for k in ("f1", "f2", "gout", "flow")})
            self.dirs = [fused]
        # what the last step handed its caller, by (direction tag, level, what): see _record() and outputs()
        self.results = {}
        self.tags = {id(lv): ("both" if fuse else "d%d" % i) for i, lv in enumerate(self.dirs)}

    def _record(self, lv, l, **arrays):
        tag = self.tags.get(id(lv))
        if tag is not None:
            for what, t in arrays.items():
                self.results[(tag, l, what)] = t

    def outputs(self, results=None):
        """{name: tensor} of what one step hands its caller (`results`: a copy of self.results taken earlier): per
        flow direction d<i> and level L<l> the correlation output `corr`, the warped image `warped`, and the
        gradients `grad_f1`, `grad_f2`, `grad_flow` of the step's inputs.  A launch that carries both directions
        (stacked levels, --fuse-directions) is split back into them: direction 0 is the first half of its batch."""
        out = {}
        for (tag, l, what), t in sorted((self.results if results is None else results).items()):
            halves = t.shape[0] // 2
            parts = [("d0", t[:halves]), ("d1", t[halves:])] if tag == "both" else [(tag, t)]
            for d, part in parts:
                out["%s_L%d_%s" % (d, l, what)] = part
        return out

    def kernels(self):
        """(label, algorithmic bytes) of every launch of one direction (or of the fused call)."""
        out = []
        nb = self.dirs[0][0]["f1"].shape[0]
        for l, (C, H, W) in enumerate(self.levels):
            cf, cb = corr_bytes(C, nb, H, W, self.esize)
            out += [("corr_fwd_L%d" % l, cf), ("corr_bwd_L%d" % l, cb)]
            if l > 0:
                wf, wb = warp_bytes(C, nb, H, W, self.esize)
                out += [("warp_fwd_L%d" % l, wf), ("warp_bwd_L%d" % l, wb)]
        return out

    def _direction(self, lv, keep, skip=None, after_first=None):
        """`skip`: label of ONE launch to leave out (per-kernel in-step timing by difference); the tensors
        it would have produced are taken from an earlier full pass (`warped`, `ctx`) or replaced by a
        tensor of the same shape (the gradient fed to the warp backward)."""
        ops = torch.ops.cerberus
        # forward, coarse to fine
        for l, t in enumerate(lv):
            # training forward: the warp also saves its backward context (sample positions),
            # as autograd's save_for_backward does for grid_sample in the reference
            if l > 0:
                if skip != "warp_fwd_L%d" % l:
                    t["warped"], t["ctx"] = ops.flow_warp_ctx(t["f2"], t["flow"], 1, 0)
            else:
                t["warped"] = t["f2"]
            if skip != "corr_fwd_L%d" % l:
                t["out"] = ops.correlation(t["f1"], t["warped"], *CORR_P)
            if skip is None:
                self._record(lv, l, corr=t["out"], **({"warped": t["warped"]} if l > 0 else {}))
            if l == 0 and after_first is not None:
                after_first()          # (the other direction's stream forks here: see step())
        # backward, fine to coarse
        for l in reversed(range(len(lv))):
            t = lv[l]
            if skip != "corr_bwd_L%d" % l:
                g1, g2 = ops.correlation_backward(t["f1"], t["warped"], t["gout"], *CORR_P)
                keep.append(g1)
            else:
                g1, g2 = None, t["f1"]
            if l > 0:
                if skip != "warp_bwd_L%d" % l:
                    gi, gf = ops.flow_warp_backward_ctx(t["f2"], t["flow"], t["ctx"], g2, 1, 0, True, True)
                    keep += [gi, gf]
                    if skip is None:
                        self._record(lv, l, grad_f1=g1, grad_f2=gi, grad_flow=gf)
            else:
                keep.append(g2)
                if skip is None:
                    self._record(lv, l, grad_f1=g1, grad_f2=g2)

    def _levels_fwd(self, lv, levels):
        ops = torch.ops.cerberus
        for l in levels:
            t = lv[l]
            if l > 0:
                t["warped"], t["ctx"] = ops.flow_warp_ctx(t["f2"], t["flow"], 1, 0)
            else:
                t["warped"] = t["f2"]
            t["out"] = ops.correlation(t["f1"], t["warped"], *CORR_P)
            self._record(lv, l, corr=t["out"], **({"warped": t["warped"]} if l > 0 else {}))

    def _levels_bwd(self, lv, levels, keep):
        ops = torch.ops.cerberus
        for l in levels:
            t = lv[l]
            g1, g2 = ops.correlation_backward(t["f1"], t["warped"], t["gout"], *CORR_P)
            keep.append(g1)
            if l > 0:
                gi, gf = ops.flow_warp_backward_ctx(t["f2"], t["flow"], t["ctx"], g2, 1, 0, True, True)
                keep += [gi, gf]
                self._record(lv, l, grad_f1=g1, grad_f2=gi, grad_flow=gf)
            else:
                keep.append(g2)
                self._record(lv, l, grad_f1=g1, grad_f2=g2)

    def step_hybrid(self, streams, ncoarse=2):
        """the two flow directions STACKED into one batched call per op on the `ncoarse` coarsest levels
        (where a launch is priced by its latency, not its bytes: one launch instead of two), two streams above.  The
        level order is the head's (coarse to fine forward, fine to coarse backward), so the stacked launches sit at
        the two ends of the step."""
        if getattr(self, "stacked", None) is None:
            self.stacked = []
            for a, b in zip(*self.dirs):
                self.stacked.append({k: (torch.cat([a[k], b[k]], 0) if a[k] is not None else None)
                                     for k in ("f1", "f2", "gout", "flow")})
            self.tags[id(self.stacked)] = "both"
        keep = []
        main = torch.cuda.current_stream()
        n = len(self.levels)
        coarse, fine = list(range(ncoarse)), list(range(ncoarse, n))
        self._levels_fwd(self.stacked, coarse)
        side = streams[0]
        side.wait_stream(main)
        with torch.cuda.stream(side):
            self._levels_fwd(self.dirs[1], fine)
            self._levels_bwd(self.dirs[1], list(reversed(fine)), keep)
        self._levels_fwd(self.dirs[0], fine)
        self._levels_bwd(self.dirs[0], list(reversed(fine)), keep)
        main.wait_stream(side)
        self._levels_bwd(self.stacked, list(reversed(coarse)), keep)
        return keep

    def step_stacked(self, streams, stacked_levels):
        """Generalisation of step_hybrid (an experiment: --stack-levels 0,2): the levels in
        `stacked_levels` run as ONE batched call per op for both directions on the main stream, the others on two
        streams; the streams join in front of every stacked level and fork again behind it."""
        if getattr(self, "stacked", None) is None:
            self.stacked = []
            for a, b in zip(*self.dirs):
                self.stacked.append({k: (torch.cat([a[k], b[k]], 0) if a[k] is not None else None)
                                     for k in ("f1", "f2", "gout", "flow")})
            self.tags[id(self.stacked)] = "both"
        keep = []
        main, side = torch.cuda.current_stream(), streams[0]
        forked = [False]

        def level(l, fwd):
            if l in stacked_levels:
                if forked[0]:
                    main.wait_stream(side)
                    forked[0] = False
                (self._levels_fwd(self.stacked, [l]) if fwd else self._levels_bwd(self.stacked, [l], keep))
            else:
                if not forked[0]:
                    side.wait_stream(main)
                    forked[0] = True
                with torch.cuda.stream(side):
                    (self._levels_fwd(self.dirs[1], [l]) if fwd else self._levels_bwd(self.dirs[1], [l], keep))
                (self._levels_fwd(self.dirs[0], [l]) if fwd else self._levels_bwd(self.dirs[0], [l], keep))

        n = len(self.levels)
        for l in range(n):
            level(l, True)
        for l in reversed(range(n)):
            level(l, False)
        if forked[0]:
            main.wait_stream(side)
        return keep

    def serial_step(self, skip=None):
        """Both directions on the current stream; `skip` leaves one launch of direction 0 out."""
        keep = []
        for i, lv in enumerate(self.dirs):
            self._direction(lv, keep, skip if i == 0 else None)
        return keep

    def step(self, streams=None):
        """One step.  The two flow directions are independent (cerberus.py:131,135 run the
        same head on swapped inputs): with `streams` they are issued on two HIP streams
        (fork/join with events, capturable into one hipGraph) so that the latency-bound
        coarse-level kernels of one direction overlap the other's."""
        keep = []
        if not streams or len(self.dirs) == 1:
            for lv in self.dirs:
                self._direction(lv, keep)
            return keep
        main = torch.cuda.current_stream()

        def fork():
            for side, lv in zip(streams, self.dirs[1:]):
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    self._direction(lv, keep)

        if self.stagger:
            # the second direction starts ONE launch late: the two streams then pair DIFFERENT kernels (one
            # direction's store burst with the other's channel loop) instead of running the same kernel side
            # by side all the way: 0.353 -> 0.346 ms per step, alternating runs on one box
            self._direction(self.dirs[0], keep, after_first=fork)
        else:
            fork()
            self._direction(self.dirs[0], keep)
        for side in streams[:len(self.dirs) - 1]:
            main.wait_stream(side)
        return keep


L3_BYTES = 256 << 20   # MI355X Infinity Cache (MI355X_MICROARCH.md): FETCH_SIZE counts its hits, a replay of one launch sits in it


def _time_graph(fn_list, reps):
    """`reps` launches (cycling through fn_list) captured back to back in one hipGraph, replayed between
    HIP events on the launch stream: seconds per launch (mean of 12 timed replays after 6 untimed ones:
    the first replays after an idle gap run up to 30 % slow, tools/timing_spread.py)."""
    for fn in fn_list[:2]:
        fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn_list[0]()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [fn_list[i % len(fn_list)]() for i in range(reps)]
    for _ in range(6):
        graph.replay()
    torch.cuda.synchronize()
    samples = []
    for _ in range(12):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        samples.append(a.elapsed_time(b) * 1e-3 / reps)
    del keep, graph
    return float(np.mean(samples))


def per_kernel_times(wl, reps, cold=True):
    """Seconds per launch for every distinct kernel of the step (direction 0 tensors), two ways:
      hot  : the same launch replayed back to back on the same tensors -- its whole working set
             (<= 110 MB) stays in the 256 MiB Infinity Cache, so this is an on-die number;
      cold : the launches of one graph walk through enough independent copies of the tensors that
             more than 256 MiB (inputs alone) pass between two uses of a copy: every launch reads
             its inputs from HBM, as it does inside the step.  The roofline fractions use this one."""
    ops = torch.ops.cerberus
    lv = wl.dirs[0]
    # an eager pass first: the tensors a capture assigned (warped, ctx) belong to the graph's pool and hold nothing until
    # the graph has been replayed; the launches timed here must see a real context
    wl._direction(lv, [])
    torch.cuda.synchronize()
    kern = dict(wl.kernels())

    def calls_for(t, l):
        c = {"corr_fwd_L%d" % l: (lambda: ops.correlation(t["f1"], t["warped"], *CORR_P)),
             "corr_bwd_L%d" % l: (lambda: ops.correlation_backward(t["f1"], t["warped"], t["gout"], *CORR_P))}
        if l > 0:
            c["warp_fwd_L%d" % l] = (lambda: ops.flow_warp_ctx(t["f2"], t["flow"], 1, 0))
            c["warp_bwd_L%d" % l] = (lambda: ops.flow_warp_backward_ctx(t["f2"], t["flow"], t["ctx"], t["f1"],
                                                                         1, 0, True, True))
        return c

    hot, cold_t = {}, {}
    # the cold passes first (they allocate and free > 256 MiB of copies per level), the hot ones last, finest level
    # last: the pass then ends on ~50 ms of back-to-back launches with nothing but event waits in between
    for l, t in enumerate(lv):
        if not cold:
            continue
        # independent copies of this level's tensors: enough that the smallest kernel of the level
        # (the forward warp / correlation) still cycles through more than the Infinity Cache
        smallest = min(v for k, v in kern.items() if k.endswith("_L%d" % l))
        ncopy = int(min(48, L3_BYTES // smallest + 2))
        copies = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in t.items()} for _ in range(ncopy)]
        per_label = {}
        for cp in copies:
            for label, fn in calls_for(cp, l).items():
                per_label.setdefault(label, []).append(fn)
        for label, fns in per_label.items():
            cold_t[label] = _time_graph(fns, max(reps, len(fns)))
        del copies, per_label
        torch.cuda.empty_cache()
    for l, t in enumerate(lv):
        for label, fn in calls_for(t, l).items():
            hot[label] = _time_graph([fn], reps)
    return hot, cold_t


STEP_ORDER = None   # labels of the launches of one direction, in _direction()'s order (filled by step_order())


def step_order(nlevels):
    fwd, bwd = [], []
    for l in range(nlevels):
        if l > 0:
            fwd.append("warp_fwd_L%d" % l)
        fwd.append("corr_fwd_L%d" % l)
    for l in reversed(range(nlevels)):
        bwd.append("corr_bwd_L%d" % l)
        if l > 0:
            bwd.append("warp_bwd_L%d" % l)
    return fwd + bwd


def trace_child(args, device):
    """Hidden mode (--trace-child): replay the whole step on ONE stream a number of times and exit.
    The parent runs this under `rocprofv3 --kernel-trace` and reads the kernel durations."""
    dtype = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    wl = Workload(args.pairs, args.width, args.height, device, args.flow, False, 1, dtype)
    for _ in range(3):
        wl.serial_step()
    torch.cuda.synchronize()
    if args.no_graph:        # the counter passes: plain launches (counters are collected per dispatch, serialised)
        for _ in range(args.steps):
            wl.serial_step()
        torch.cuda.synchronize()
        return
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wl.serial_step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = wl.serial_step()  # noqa: F841
    for _ in range(args.steps):
        g.replay()
    torch.cuda.synchronize()


_PROFILER_PREFIXES = ("ROCP_", "ROCPROF", "ROCPROFILER_", "ROCTRACER_", "ROCTX_", "HSA_TOOLS_", "ROCPROFV3_",
                      "OMNIPERF_", "ROCPROFSYS_")


def _is_profiler_variable(name):
    return name.startswith(_PROFILER_PREFIXES) or name in ("LD_PRELOAD", "HSA_TOOLS_LIB")


def profiler_in_environment(environ=None):
    """True when this process was started by rocprofv3 / rocprof (tool library preloaded or registered)."""
    env = os.environ if environ is None else environ
    if any(env.get(k) for k in ("ROCP_TOOL_LIBRARIES", "ROCP_TOOL_LIB", "HSA_TOOLS_LIB", "ROCPROFILER_REGISTER_FORCE_LOAD")):
        return True
    if any(k.startswith(("ROCPROF_", "ROCPROFILER_", "ROCPROFV3_")) and env.get(k) for k in env):
        return True
    pre = env.get("LD_PRELOAD", "")
    return any(t in pre for t in ("rocprof", "roctracer", "rocprofiler", "roctx"))


def in_step_times(args, nlevels, replays=60):
    """Seconds per launch INSIDE the step, from the profiler: a child process replays the whole step on
    one stream (every kernel alone on the chip, caches in the state the step leaves them in) under
    `rocprofv3 --kernel-trace`; the hot-path kernels of its trace come in blocks of 2 x 14 in the step's
    launch order, which identifies the level of each.  Returns ({label: seconds}, info) or (None, reason)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found"
    # never start a profiler from inside a profiled process.  An outer rocprofv3 (or any
    # preloaded tool) has already initialised the GPU in THIS process, and its environment would make
    # the inner launcher initialise it before exec'ing the child -- the exec-after-GPU-init hop that
    # takes a box of this pool down.
    if profiler_in_environment():
        return None, "already under a profiler (preload / rocprofiler variables present): in-step pass skipped"
    order = step_order(nlevels)
    out = tempfile.mkdtemp(prefix="cerb_trace_", dir="/tmp")
    cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable,
           os.path.abspath(__file__), "--trace-child", "--steps", str(replays), "--pairs", str(args.pairs),
           "--width", str(args.width), "--height", str(args.height), "--dtype", args.dtype, "--flow", args.flow]
    if args.no_mfma:
        cmd.append("--no-mfma")
    try:
        env = {k: v for k, v in os.environ.items()
               if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GROUP_RANK",
                            "LOCAL_WORLD_SIZE", "ROLE_RANK", "ROLE_WORLD_SIZE", "TORCHELASTIC_RUN_ID")
               and not _is_profiler_variable(k)}
        env["TMPDIR"] = "/tmp"
        subprocess.run(cmd, cwd="/tmp", env=env, timeout=300, check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        paths = glob.glob(out + "/**/*kernel_trace.csv", recursive=True)
        if not paths:
            return None, "no kernel trace written"
        rows = []
        for r in csv.DictReader(open(paths[0])):
            n = r["Kernel_Name"]
            if any(k in n for k in ("corr_fwd", "corr_bwd", "warp_fwd", "warp_bwd")):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), n))
        rows.sort()
        per_step = 2 * len(order)
        if len(rows) < 10 * per_step or len(rows) % per_step:
            return None, "unexpected launch count %d in the trace" % len(rows)
        rows = rows[-(replays - 10) * per_step:]            # graph replays only, the first ten dropped
        acc = {k: [] for k in order}
        for i, (_, dur, name) in enumerate(rows):
            label = order[(i % per_step) % len(order)]
            if label.split("_L")[0] not in name.replace("corr_bwd_d4", "corr_bwd").replace("corr_fwd_d4", "corr_fwd"):
                return None, "trace order mismatch at %d: %s vs %s" % (i, label, name[:60])
            acc[label].append(dur * 1e-9)
        return ({k: float(np.mean(v)) for k, v in acc.items()},
                {"source": "rocprofv3 --kernel-trace of a child replaying the step on one stream",
                 "launches_per_label": len(acc[order[0]])})
    except Exception as exc:  # the headline must not depend on the profiler
        return None, repr(exc)[:200]
    finally:
        shutil.rmtree(out, ignore_errors=True)


def live_traffic(args, nlevels, steps=4):
    """HBM-side bytes per launch of every kernel of the step, measured by THIS run: two children replay the
    step eagerly on one stream under `rocprofv3 --kernel-trace --pmc FETCH_SIZE` and `--pmc WRITE_SIZE`
    (separate passes: the two do not fit one on gfx950; MI355X_MICROARCH.md, HBM / rocprofv3 PMC slots) and
    the dispatches are matched to the step's launch order as in in_step_times().  Corrections as that
    guide prescribes: read bytes = 2 x FETCH_SIZE KiB (gfx950 tallies the 128-byte requests of a wide
    coalesced stream at 64 bytes; factor 2.000 re-measured for 16- and 4-byte-per-lane streams,
    profiles/r04_fetch_size_calibration.json), write bytes = WRITE_SIZE KiB.  FETCH_SIZE counts Infinity-Cache
    hits as traffic.  Returns ({label: {"read_bytes", "write_bytes", "traffic_bytes"}}, info) or (None, reason)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found"
    if profiler_in_environment():
        return None, "already under a profiler"
    order = step_order(nlevels)
    per_step = 2 * len(order)
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GROUP_RANK",
                        "LOCAL_WORLD_SIZE", "ROLE_RANK", "ROLE_WORLD_SIZE", "TORCHELASTIC_RUN_ID")
           and not _is_profiler_variable(k)}
    env["TMPDIR"] = "/tmp"
    got = {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = tempfile.mkdtemp(prefix="cerb_pmc_", dir="/tmp")
            try:
                cmd = [prof, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out, "--", sys.executable,
                       os.path.abspath(__file__), "--trace-child", "--no-graph", "--steps", str(steps), "--pairs", str(args.pairs),
                       "--width", str(args.width), "--height", str(args.height), "--dtype", args.dtype, "--flow", args.flow]
                if args.no_mfma:
                    cmd.append("--no-mfma")
                subprocess.run(cmd, cwd="/tmp", env=env, timeout=300, check=True, stdout=subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL)
                paths = glob.glob(out + "/**/*counter_collection.csv", recursive=True)
                if not paths:
                    return None, "no counter file written (%s)" % counter
                rows = []
                for r in csv.DictReader(open(paths[0])):
                    n = r["Kernel_Name"]
                    if r["Counter_Name"] == counter and any(k in n for k in ("corr_fwd", "corr_bwd", "warp_fwd", "warp_bwd")):
                        rows.append((int(r["Dispatch_Id"]), float(r["Counter_Value"]), n))
                rows.sort()
                if len(rows) < steps * per_step or len(rows) % per_step:
                    return None, "unexpected dispatch count %d in the %s pass" % (len(rows), counter)
                rows = rows[-steps * per_step:]
                acc = {k: [] for k in order}
                for i, (_, val, name) in enumerate(rows):
                    label = order[(i % per_step) % len(order)]
                    if label.split("_L")[0] not in name.replace("corr_bwd_d4", "corr_bwd").replace("corr_fwd_d4", "corr_fwd"):
                        return None, "dispatch order mismatch at %d: %s vs %s" % (i, label, name[:60])
                    acc[label].append(val)
                got[counter] = {k: float(np.mean(v)) for k, v in acc.items()}
            finally:
                shutil.rmtree(out, ignore_errors=True)
        res = {}
        for k in order:
            rd, wr = 2.0 * got["FETCH_SIZE"][k] * 1024.0, got["WRITE_SIZE"][k] * 1024.0
            res[k] = {"read_bytes": int(round(rd)), "write_bytes": int(round(wr)), "traffic_bytes": int(round(rd + wr))}
        return res, {"source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (two passes) of children of this run replaying "
                               "the step eagerly on one stream; read = 2 x FETCH_SIZE KiB, write = WRITE_SIZE KiB; "
                               "Infinity-Cache hits count as traffic",
                     "launches_per_label": 2 * steps}
    except Exception as exc:  # the headline must not depend on the profiler
        return None, repr(exc)[:200]


def torch_gpu_reference(wl, budget_s=4.0):
    """the same step with the op swapped for stock PyTorch on the SAME
    device -- CorrelationTorch (correlation.py:4-21, the reference's own fallback) + autograd, and
    the reference's flow_warp composition (mesh + norm_grid + F.grid_sample) + autograd.  Context
    only (what a user gets without the HIP kernels); not the product and not the oracle."""
    import torch.nn.functional as F
    from cerberusnet_amd.correlation_package.correlation import CorrelationTorch
    from cerberusnet_amd.loss_functions.UnFlowLoss import mesh_grid, norm_grid
    corr = CorrelationTorch(4)

    def one_step():
        for lv in wl.dirs:
            for l, t in enumerate(lv):
                f1 = t["f1"].detach().requires_grad_(True)
                f2 = t["f2"].detach().requires_grad_(True)
                ins = [f1, f2]
                if l > 0:
                    flow = t["flow"].detach().requires_grad_(True)
                    b, _, h, w = f2.shape
                    grid = norm_grid(mesh_grid(b, h, w).type_as(f2) + flow)
                    warped = F.grid_sample(f2, grid, mode="bilinear", padding_mode="border",
                                           align_corners=False)
                    ins.append(flow)
                else:
                    warped = f2
                torch.autograd.grad(corr(f1, warped), ins, t["gout"])

    one_step()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        one_step()
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt > budget_s or n >= 50:
            break
    return {"value": round(wl.pairs * n / dt, 2), "unit": "image-pairs/s",
            "what": "same tensors and op sequence in stock PyTorch ops on this GPU (CorrelationTorch + "
                    "F.grid_sample + autograd, eager), %d steps in %.1f s" % (n, dt)}


def cpu_baseline(levels, budget_s=20.0):
    """Reference CPU path: the semantics of CorrelationTorch.forward
    (correlation.py:11-21; oracle port, bit-identical to the reference in the build container) on
    the config-1 tensor and the four config-3 level shapes, B = 1: forward, and forward +
    autograd backward; 3 warm-ups, then >= 10 timed iterations each (fewer only if the time budget
    runs out), min and median.  `value` = image pairs/s from the median fwd+bwd times (4 levels x 2
    flow directions = one pair; correlation only)."""
    from oracle import correlation_torch_ref
    from cerberusnet_amd.synth import hash_uniform
    shapes = [("config1_1x64x64x128", (64, 64, 128))] + [("L%d" % l, s) for l, s in enumerate(levels)]
    data = {}
    for i, (name, (C, H, W)) in enumerate(shapes):
        data[name] = (torch.from_numpy(hash_uniform((1, C, H, W), 4 * i)).requires_grad_(True),
                      torch.from_numpy(hash_uniform((1, C, H, W), 4 * i + 1)).requires_grad_(True),
                      torch.from_numpy(hash_uniform((1, 81, H, W), 4 * i + 2)))

    def fwd(name):
        x1, x2, _ = data[name]
        with torch.no_grad():
            return correlation_torch_ref(x1, x2, 4)

    def fwdbwd(name):
        x1, x2, go = data[name]
        torch.autograd.grad(correlation_torch_ref(x1, x2, 4), (x1, x2), go)

    # torch's default (one thread per host core) is far from optimal on these small maps (14x slower
    # on the 256-core GPU box): probe a few thread counts on one image pair and use the best
    default_threads = torch.get_num_threads()
    ncpu = os.cpu_count() or 1
    usable, usable_how = usable_cores()
    probe = {}
    for th in sorted({min(default_threads, 2 * usable), usable, 32, 16, 8}):
        if th > ncpu or th > 2 * usable:
            continue
        torch.set_num_threads(th)
        for name, _ in shapes[1:]:
            fwdbwd(name)
        t0 = time.perf_counter()
        for name, _ in shapes[1:]:
            fwdbwd(name)
        probe[th] = time.perf_counter() - t0
    threads = min(probe, key=probe.get)
    torch.set_num_threads(threads)
    t_start = time.perf_counter()
    table = {}
    for name, _ in shapes:
        row = {}
        for what, fn in (("fwd", fwd), ("fwd_bwd", fwdbwd)):
            for _ in range(3):
                fn(name)
            ts = []
            while len(ts) < 10 and (len(ts) < 3 or time.perf_counter() - t_start < budget_s):
                t0 = time.perf_counter()
                fn(name)
                ts.append(time.perf_counter() - t0)
            row[what + "_ms_min"] = round(1e3 * min(ts), 3)
            row[what + "_ms_median"] = round(1e3 * float(np.median(ts)), 3)
            row[what + "_iters"] = len(ts)
        table[name] = row
    # for the record: the config-1 forward with torch's default of one thread per visible core (skipped where the
    # visible cores exceed the ones this process may run on: see usable_cores())
    all_cores_ms = None
    if ncpu <= 32:
        torch.set_num_threads(ncpu)
        fwd(shapes[0][0])
        t0 = time.perf_counter()
        fwd(shapes[0][0])
        all_cores_ms = round(1e3 * (time.perf_counter() - t0), 3)
    # BASELINE.md section 4 as written: torch.set_num_threads(all host cores), forward + backward on the four levels.
    # "All host cores" = the cores this process may RUN on: the GPU boxes show 256 logical CPUs to os.cpu_count() and to
    # sched_getaffinity, but their cgroup grants 16 CPUs of time (cpu.max = 1600000 100000) -- 256 compute threads under
    # that quota are throttled to a crawl (rounds 5 / 6 measured 19.8 s for ONE config-1 forward, ~50 s per fwd + bwd of
    # any level; cpu.stat's nr_throttled counts it), which is a property of the container, not of the baseline.  The
    # pass runs in a CHILD process with a hard deadline (a torch CPU op cannot be interrupted from inside): the levels it
    # finished are measured, any rest is scaled from the probed-thread medians by the ratio seen on the finished ones.
    all_budget = max(6.0, budget_s)
    all_table, all_note = _cpu_all_cores_child(levels, all_budget, usable)
    done = [k for k, v in all_table.items() if v.get("iters")]
    ratio = (sum(all_table[k]["fwd_bwd_ms_median"] for k in done) / sum(table[k]["fwd_bwd_ms_median"] for k in done)) if done else None
    for l in range(len(levels)):
        k = "L%d" % l
        if k not in done:
            all_table[k] = ({"fwd_bwd_ms_median": round(table[k]["fwd_bwd_ms_median"] * ratio, 3), "iters": 0,
                             "extrapolated": "probed-thread median x %.2f (the all-cores / probed ratio of %s)" % (ratio, "+".join(done))}
                            if ratio else {"fwd_bwd_ms_median": None, "iters": 0})
    all_pair_s = (2 * sum(all_table["L%d" % l]["fwd_bwd_ms_median"] for l in range(len(levels))) * 1e-3) if ratio else None
    torch.set_num_threads(default_threads)
    pair_s = 2 * sum(table["L%d" % l]["fwd_bwd_ms_median"] for l in range(len(levels))) * 1e-3
    return {"value": round(1.0 / pair_s, 4), "unit": "image-pairs/s", "cores": threads, "kind": "port",
            "host_cores": ncpu, "per_shape_ms": table,
            "value_all_cores": round(1.0 / all_pair_s, 4) if all_pair_s else None, "cores_all": usable,
            "all_cores": {"per_shape_ms": all_table, "usable_cores": usable_how,
                          "what": "BASELINE.md section 4 as specified: torch.set_num_threads(%d) = every core this process may "
                                  "run on (%s), fwd + autograd bwd on the four level shapes (smallest first), 1 warm-up + up to 3 "
                                  "timed iterations per level in a child process stopped after %.0f s; %s; `value` / `cores` "
                                  "beside it is the best thread count of a probe" % (usable, usable_how, all_budget, all_note)},
            "config1_fwd_ms_with_all_%d_cores" % ncpu: all_cores_ms,
            "sample": "CorrelationTorch semantics on torch CPU, B=1: config-1 tensor + the 4 level shapes, "
                      "3 warm-ups + up to 10 timed iterations each of fwd and fwd+autograd bwd (min / median "
                      "in per_shape_ms); value = 1 / (2 directions x sum of the levels' median fwd+bwd); "
                      "%d threads = best of %s on a box with %d host cores, %.1f s in all"
                      % (threads, sorted(probe), ncpu, time.perf_counter() - t_start)}


def usable_cores():
    """(n, how): the CPUs this process may actually run on = min(visible CPUs, scheduler affinity, the cgroup's CPU-time
    quota).  os.cpu_count() alone reports the machine (256 on the GPU boxes), not the container's share (16 there)."""
    n = os.cpu_count() or 1
    how = ["os.cpu_count() = %d" % n]
    try:
        a = len(os.sched_getaffinity(0))
        how.append("affinity = %d" % a)
        n = min(n, a)
    except (AttributeError, OSError):
        pass
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:                       # cgroup v2
            q, per = f.read().split()[:2]
            if q != "max":
                quota = float(q) / float(per)
                how.append("cgroup cpu.max = %s %s" % (q, per))
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:      # cgroup v1
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = int(f.read())
            if q > 0:
                quota = q / per
                how.append("cgroup cfs quota = %d / %d" % (q, per))
        except (OSError, ValueError):
            pass
    if quota:
        n = min(n, max(1, int(-(-quota // 1))))
    return n, ", ".join(how)


def _cpu_all_cores_child(levels, budget_s, threads):
    """The all-host-cores pass of cpu_baseline() in a child process with a hard deadline (a torch CPU op cannot be
    interrupted from inside).  Returns ({level: {fwd_bwd_ms_median, iters}}, note)."""
    import subprocess
    code = ("import json, os, sys, time\n"
            "sys.path.insert(0, %r)\n"
            "import numpy as np, torch\n"
            "from oracle import correlation_torch_ref\n"
            "from cerberusnet_amd.synth import hash_uniform\n"
            "torch.set_num_threads(%d)\n"
            "for l, (C, H, W) in enumerate(%r):\n"
            "    x1 = torch.from_numpy(hash_uniform((1, C, H, W), 4 * (l + 1))).requires_grad_(True)\n"
            "    x2 = torch.from_numpy(hash_uniform((1, C, H, W), 4 * (l + 1) + 1)).requires_grad_(True)\n"
            "    go = torch.from_numpy(hash_uniform((1, 81, H, W), 4 * (l + 1) + 2))\n"
            "    for it in range(4):\n"
            "        t0 = time.perf_counter()\n"
            "        torch.autograd.grad(correlation_torch_ref(x1, x2, 4), (x1, x2), go)\n"
            "        print(json.dumps({'level': l, 'iter': it, 'ms': 1e3 * (time.perf_counter() - t0)}), flush=True)\n"
            % (REPO, threads, [list(s) for s in levels]))
    env = {k: v for k, v in os.environ.items() if not _is_profiler_variable(k) and k not in ("OMP_NUM_THREADS", "MKL_NUM_THREADS")}
    env["CUDA_VISIBLE_DEVICES"] = ""            # CPU work only: the child never touches the GPU
    env["HIP_VISIBLE_DEVICES"] = ""
    rows = {}
    t0 = time.perf_counter()
    try:
        proc = subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, env=env)
    except OSError as exc:
        return {}, "child not started: %r" % (exc,)
    import threading
    killer = threading.Timer(budget_s, proc.kill)
    killer.start()
    try:
        for line in proc.stdout:
            try:
                r = json.loads(line)
            except ValueError:
                continue
            rows.setdefault(r["level"], []).append(r["ms"])
        proc.wait()
    finally:
        killer.cancel()
    used = time.perf_counter() - t0
    table = {}
    for l, ms in rows.items():
        timed = ms[1:] if len(ms) > 1 else ms          # the first call of a level is its warm-up when more were finished
        table["L%d" % l] = {"fwd_bwd_ms_median": round(float(np.median(timed)), 3), "iters": len(timed),
                            "warmups": 1 if len(ms) > 1 else 0}
    note = ("%d of %d levels measured in %.1f s%s" % (len(table), len(levels), used,
            "" if proc.returncode == 0 else " (deadline reached: the child was stopped)"))
    return table, note


GRAD_BYTES = 137_100_000   # HRNetV2-W32 + FlowEstimatorLite: 34.27 M fp32 parameters


def spawn_ranks(n):
    """Plain `python bench.py --gpus N`: become the launcher.  Nothing here touches the GPU
    (device_count() does not initialise it); the ranks are children, never an exec of a process
    that has a GPU context."""
    import socket
    import subprocess
    have = n if "cpu" in [a for i, a in enumerate(sys.argv) if i and sys.argv[i - 1] == "--device"] else torch.cuda.device_count()
    if have < n:
        print(json.dumps({"metric": METRIC, "skipped": "--gpus %d but this box has %d GPU(s)" % (n, have),
                          "n_gpus": n}), flush=True)
        return 0
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def loss_side_times(pairs, width, height, device, reps=12):
    """The hot path's SECOND workload inside a training step: what unFlowLoss launches around the
    head -- the two target images resized to every flow scale (UnFlowLoss.py:279-280), the RGB warps of those images by
    every predicted flow, forward and grad_flow (UnFlowLoss.py:282-283: 8 + 8 launches per step) -- and the pass that
    turns the concatenation buffer's gradient into the correlation backward's gradOutput (pwcnet_sfd.py:181-187 seen
    from autograd).  Every launch timed on its own like `per_kernel_times`: hot (replayed on the same tensors) and cold
    (rotating copies, > 256 MiB apart); `frac` = algorithmic bytes / cold time / 8 TB/s.  `before` = the same call on
    the round-4 kernels (warp option warp_fewc = -1: channel-group kernels with context; one area_resize per scale)."""
    from cerberusnet_amd import _lib
    from cerberusnet_amd.synth import hash_uniform
    ops = torch.ops.cerberus
    B, H, W = pairs, height, width
    scales = [(H, W), (H // 2, W // 2), (H // 4, W // 4), (H // 8, W // 8)]        # the flow list of the host model's head at this frame size (w_wrp_scales [1, 1, 1, 1, 0])
    t = lambda shape, seed, lo=-1.0, hi=1.0: torch.from_numpy(hash_uniform(shape, seed, lo, hi)).to(device)
    out = {}

    def measure(label, make, nbytes, before=None):
        """make(i) -> a zero-argument launch on the i-th independent copy of the tensors"""
        ncopy = int(min(48, L3_BYTES // max(nbytes, 1) + 2))
        fns = [make(i) for i in range(ncopy)]
        hot = _time_graph([fns[0]], reps)
        cold = _time_graph(fns, max(reps, len(fns)))
        rec = {"us_hot": round(hot * 1e6, 2), "us_cold": round(cold * 1e6, 2), "algorithmic_bytes": nbytes,
               "GBps": round(nbytes / cold / 1e9, 1), "frac": round(nbytes / cold / 1e9 / HBM_PEAK_GBPS, 4)}
        if before is not None:
            bf = [before(i) for i in range(ncopy)]
            rec["before_us_hot"] = round(_time_graph([bf[0]], reps) * 1e6, 2)
            rec["before_us_cold"] = round(_time_graph(bf, max(reps, len(bf))) * 1e6, 2)
        del fns
        torch.cuda.empty_cache()
        out[label] = rec

    # ---- the loss pyramid of ONE image: source read once, three scales written (the identity scale is the image)
    flat = [v for s in scales for v in s]
    pyr_bytes = 4 * B * 3 * (H * W + sum(h * w for h, w in scales[1:]))
    imgs = {}

    def pyr_make(i):
        imgs[i] = t((B, 3, H, W), 500 + i, -2.0, 2.0)
        return lambda: ops.area_pyramid(imgs[i], flat)

    def pyr_before(i):
        return lambda: [ops.area_resize(imgs[i], h, w) for h, w in scales]
    measure("area_pyramid", pyr_make, pyr_bytes, pyr_before)
    imgs.clear()

    # ---- the RGB warps, scale by scale
    for si, (h, w) in enumerate(scales):
        fb, bb = warp_bytes(3, B, h, w)
        bb = (2 * 3 + 4) * B * h * w * 4            # grad_flow alone: gradOutput + image taps (3 each) + flow in, grad_flow out
        keep = {}

        def mk(i, h=h, w=w):
            if i not in keep:
                keep[i] = (t((B, 3, h, w), 600 + i, -2.0, 2.0), Workload._flow(B, h, w, 700 + i, "smooth", device),
                           t((B, 3, h, w), 800 + i))
            return keep[i]

        def fwd_make(i):
            img, flo, _ = mk(i)
            return lambda: ops.flow_warp(img, flo, 1, 0)

        def bwd_make(i):
            img, flo, go = mk(i)
            return lambda: ops.flow_warp_backward(img, flo, go, 1, 0, False, True)

        def old(fn_maker):
            def wrapped(i):
                inner = fn_maker(i)
                def call():
                    _lib.set_option("warp_fewc", -1)
                    try:
                        return inner()
                    finally:
                        _lib.set_option("warp_fewc", 0)
                return call
            return wrapped

        def fwd_before(i):
            img, flo, _ = mk(i)
            def call():
                _lib.set_option("warp_fewc", -1)
                try:
                    return ops.flow_warp_ctx(img, flo, 1, 0)      # round 4: the forward of a training warp always saved a context
                finally:
                    _lib.set_option("warp_fewc", 0)
            return call
        measure("rgb_warp_fwd_s%d" % si, fwd_make, fb, fwd_before)
        measure("rgb_warp_bwd_s%d" % si, bwd_make, bb, old(bwd_make))
        if si == 0:
            # the same launches under a uniform translation: the headline's synthetic "smooth" field has slopes of up to
            # 1.5 px per px (a gather instruction's 64 taps then spread over up to 13 image rows and the texture path walks
            # every cache line they touch); a real full-resolution flow is a x4 bilinear upsample with slopes ~0.1
            for i in list(keep):
                img, flo, go = keep[i]
                flo = torch.empty_like(flo)
                flo[:, 0] = 2.3
                flo[:, 1] = -1.7
                keep[i] = (img, flo, go)
            measure("rgb_warp_fwd_s0_translation", fwd_make, fb)
            measure("rgb_warp_bwd_s0_translation", bwd_make, bb)
        keep.clear()

    # ---- gradOutput of the level-3 correlation backward from the concatenation buffer's gradient
    C3, H3, W3 = 32, H // 4, W // 4            # the finest level of the W32 pyramid
    item = 81 * H3 * W3
    keep = {}

    def prep_tensors(i):
        if i not in keep:
            keep[i] = (t((B, C3, H3, W3), 900 + i), t((B, C3, H3, W3), 950 + i), t((B, 81 + 34, H3, W3), 1000 + i),
                       t((B, 81 + 34, H3, W3), 1050 + i))
        return keep[i]

    def prep_make(i):
        x1, x2, g, f = prep_tensors(i)
        return lambda: ops.correlation_backward_leaky(x1, x2, g, f, 0, *CORR_P, 0.1)

    def prep_before(i):
        x1, x2, g, f = prep_tensors(i)
        def call():
            gg = g[:, :81]
            gg = torch.where(f[:, :81] > 0, gg, gg * 0.1)
            return ops.correlation_backward(x1, x2, gg, *CORR_P)
        return call
    cb = corr_bytes(C3, B, H3, W3)[1] + 3 * B * item * 4      # the backward itself + one read of g, one of the stored volume, one write
    measure("corr_bwd_L3_from_concat_gradient", prep_make, cb, prep_before)
    keep.clear()
    tot = lambda key: round(2 * out["area_pyramid"][key] + 2 * sum(v[key] for k, v in out.items()
                                                                     if k.startswith("rgb_warp") and not k.endswith("translation")), 2)
    out["_per_step"] = {"us_cold": tot("us_cold"), "before_us_cold": tot("before_us_cold"),
                        "what": "2 pyramids + 8 forward + 8 grad_flow warps: the loss side of one training step at %d pairs" % B}
    return out


def head_step_mode(args, device, rank, world, dist):
    """--step head: what `--gpus N` scaling is judged on.  One step = zero_grad, PWCNetHead(1 -> 2),
    PWCNetHead(2 -> 1), loss, backward on `--pairs` image pairs per rank at the config-3 pyramid
    (reference loop: utilities/model_trainer.py:187-226; the head is called twice per step,
    cerberus.py:131,135).  N > 1: the head is wrapped by cerberusnet_amd.distributed.wrap_ddp
    (DistributedDataParallel over RCCL, 64 MB buckets, static graph): the all-reduce of its
    gradients overlaps the backward it belongs to.  Eager launches at every N (DDP's bucket hooks
    are not captured); at N = 1 the hipGraph replay of the same step is reported beside it."""
    from cerberusnet_amd.distributed import wrap_ddp
    from cerberusnet_amd.nnet_models import PWCNetHead
    from cerberusnet_amd.synth import fill_parameters, hash_uniform, pyramid_shapes
    levels = pyramid_shapes(args.width, args.height, 32)
    chans = [c for c, _, _ in reversed(levels)]          # high resolution first, as HRNet lists them
    head = PWCNetHead(chans, upsample=True,
                      correlation_args=dict(pad_size=4, kernel_size=1, max_displacement=4, stride1=1,
                                            stride2=1, corr_multiply=1),
                      flow_est_network=dict(type="FlowEstimatorLite", args={}),
                      context_network=dict(type="ContextNetwork", args={}),
                      **{"1x1_conv_out": 32}).to(device).train()
    fill_parameters(head, 7)                              # the same weights on every rank
    B = args.pairs
    pyr = lambda seed: [torch.from_numpy(hash_uniform((B, C, H, W), seed + i + 1000 * rank)).to(device)
                        for i, (C, H, W) in enumerate(levels)]
    p1, p2 = pyr(10), pyr(20)
    model = wrap_ddp(head, device) if world > 1 else head
    params = [p for p in head.parameters() if p.requires_grad]
    loss_fn = lambda flows: sum(f.abs().mean() for f in flows)

    if args.stack_directions:
        # PWCNetHead.forward_both: [f1; f2] against [f2; f1], one pass of the head on 2B items
        sa = [torch.cat([x, y], 0) for x, y in zip(p1, p2)]
        sb = [torch.cat([y, x], 0) for x, y in zip(p1, p2)]

    def step():
        for p in params:
            p.grad = None
        if args.stack_directions:
            flows = model((None, sa), (None, sb))
        else:
            flows = list(model((None, p1), (None, p2))) + list(model((None, p2), (None, p1)))
        loss_fn(list(flows)).backward()

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(max(3, args.warmup)):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if rank != 0:
        return
    nparam = sum(p.numel() for p in params)
    result = {
        "metric": METRIC, "value": round(B * world * args.steps / dt, 2), "unit": "image-pairs/s",
        "n_gpus": world, "steps": args.steps, "warmup": max(3, args.warmup),
        "ms_per_step": round(1e3 * dt / args.steps, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {
            "step": "head",
            "workload": "one training step of the flow head (PWCNetHead + FlowEstimatorLite + ContextNetwork, "
                        "%d parameters, random init) on the HRNetV2-W32 pyramid of %dx%d, %d image pairs per GPU: "
                        "both flow directions, loss, backward; the correlation / warp / flow-upsample ops are this "
                        "package's HIP kernels, the convolutions MIOpen's" % (nparam, args.width, args.height, B),
            "pairs_per_gpu": B, "levels_CHW": [list(x) for x in levels],
            "launch": "eager" + (", both directions stacked into one pass of the head (PWCNetHead.forward_both)"
                                 if args.stack_directions else ", the head called once per direction"),
            "sharding": ("DistributedDataParallel over RCCL (64 MB buckets, static graph): %.1f MB of gradients "
                         "all-reduced inside every step, overlapped with backward" % (4e-6 * nparam)
                         if world > 1 else "one rank"),
        },
        "roofline": None, "cpu_baseline": None,
        "note": "the op-only headline (python bench.py, no --step) carries roofline and cpu_baseline",
    }
    if world == 1:
        from cerberusnet_amd.graphs import GraphedFlowStep
        gstep = GraphedFlowStep(head, loss_fn, p1, p2)    # (the two-call form)
        for _ in range(5):
            gstep.graph.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            gstep.graph.replay()
        torch.cuda.synchronize()
        g = (time.perf_counter() - t0) / args.steps
        result["hipgraph_replay"] = {"ms_per_step": round(1e3 * g, 4), "pairs_per_s": round(B / g, 2),
                                     "what": "graph replay only: GraphedFlowStep.__call__ adds the copy of the inputs and, unless "
                                             "trust_captured_loss, the eager re-evaluation of the loss on the replayed flows"}
    print(json.dumps(result), flush=True)


def hot_kernel_times(wl, labels, reps=20):
    """Seconds per launch (hot: the same launch replayed on the same tensors, HIP events) of the named launches of
    direction 0."""
    ops = torch.ops.cerberus
    lv = wl.dirs[0]
    wl._direction(lv, [])
    torch.cuda.synchronize()
    out = {}
    for label in labels:
        kind, l = label.rsplit("_L", 1)
        t = lv[int(l)]
        fn = {"corr_fwd": (lambda t=t: ops.correlation(t["f1"], t["warped"], *CORR_P)),
              "corr_bwd": (lambda t=t: ops.correlation_backward(t["f1"], t["warped"], t["gout"], *CORR_P)),
              "warp_fwd": (lambda t=t: ops.flow_warp_ctx(t["f2"], t["flow"], 1, 0)),
              "warp_bwd": (lambda t=t: ops.flow_warp_backward_ctx(t["f2"], t["flow"], t["ctx"], t["f1"], 1, 0, True, True))}[kind]
        out[label] = _time_graph([fn], reps)
    return out


def f2_fused_times(pairs, width, height, device, reps=20):
    """SURVEY.md 8(f)-2 built (round 6): flow_warp + correlation + LeakyReLU as ONE forward kernel that never writes the warped
    features (cerberus::warp_correlation_leaky) against the two tuned launches, per level of the headline's pyramid; hot, HIP
    events.  `saved_bytes` = the warped tensor's write + read the fusion removes."""
    from cerberusnet_amd.synth import hash_uniform, pyramid_shapes
    ops = torch.ops.cerberus
    out = {}
    for l, (C, H, W) in enumerate(pyramid_shapes(width, height, 32)):
        if l == 0:
            continue                                     # (the coarsest level is not warped)
        f1 = torch.from_numpy(hash_uniform((pairs, C, H, W), 1)).to(device)
        f2 = torch.from_numpy(hash_uniform((pairs, C, H, W), 2)).to(device)
        fl = Workload._flow(pairs, H, W, 3, "smooth", device)
        t_f = _time_graph([lambda: ops.warp_correlation_leaky(f1, f2, fl, 1, 0.1)], reps)
        t_u = _time_graph([lambda: ops.correlation_leaky(f1, ops.flow_warp(f2, fl, 1, 0), *CORR_P, 0.1)], reps)
        nbytes = (2 * C + 2 + 81) * pairs * H * W * 4        # f1 + f2 + flow in, the cost volume out
        out["L%d" % l] = {"fused_us": round(t_f * 1e6, 2), "two_launches_us": round(t_u * 1e6, 2),
                          "algorithmic_bytes": nbytes, "fused_frac": round(nbytes / t_f / 1e9 / HBM_PEAK_GBPS, 4),
                          "saved_bytes": 2 * C * pairs * H * W * 4}
    out["what"] = ("cerberus::warp_correlation_leaky (warp_corr.hip: an 8 x 32 tile samples its 16 x 40 window -- 2.5 x the pixels "
                   "of the stand-alone warp -- into LDS and correlates from there) against flow_warp + correlation_leaky, "
                   "%d pairs, fp32, hot: the fusion loses, as DESIGN.md 3.5 priced it; opt-in (PWCNetHead(fuse_warp=True)) for "
                   "the memory it saves in training: no warped tensor, no warp context" % pairs)
    return out


def short_ops_rate(pairs, width, height, dtype, device, steps=60, warmup=10, flow_kind="smooth", probe=()):
    """A short timed pass of the op-only step on another configuration (value only: no per-kernel pass):
    same graph + two-stream launch as the headline.  Used for `extra.config5_f16` of the default line so
    that a driver-timed figure of BASELINE config 5 exists.  `probe`: launches to time on
    their own as well (hot, HIP events)."""
    wl = Workload(pairs, width, height, device, flow_kind, False, 1, dtype)
    streams = [torch.cuda.Stream()]
    for _ in range(3):
        wl.step(streams)
    torch.cuda.synchronize()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap):
        wl.step(streams)
    torch.cuda.current_stream().wait_stream(cap)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = wl.step(streams)  # noqa: F841
    for _ in range(warmup):
        graph.replay()
    torch.cuda.synchronize()
    # three timed passes of `steps` replays each, the MEDIAN pass reported (a 20 ms window is at the mercy of one host
    # hiccup: a default run once put the 896 x 448 pyramid at 10.9 k pairs/s with every kernel as fast as in the 12.6 k runs)
    passes = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            graph.replay()
        torch.cuda.synchronize()
        passes.append(time.perf_counter() - t0)
    dt = sorted(passes)[1]
    kern = dict(wl.kernels())
    corr_b = 2 * sum(v for k, v in kern.items() if k.startswith("corr"))
    out = {"value": round(pairs * steps / dt, 2), "unit": "image-pairs/s", "ms_per_step": round(1e3 * dt / steps, 5),
           "passes_ms_per_step": [round(1e3 * t / steps, 5) for t in passes],
           "steps": steps, "warmup": warmup, "pairs_per_gpu": pairs, "levels_CHW": [list(x) for x in wl.levels],
           "dtype": {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}[dtype],
           "algorithmic_bytes_per_step": 2 * sum(kern.values()),
           "step_algorithmic_GBps": round(2 * sum(kern.values()) * steps / dt / 1e9, 1),
           "corr_only_frac_of_hbm_peak_whole_step": round(corr_b * steps / dt / 1e9 / HBM_PEAK_GBPS, 4),
           "flow_field": flow_kind}
    del graph, held
    if probe:
        hot = hot_kernel_times(wl, probe)
        out["per_kernel_hot"] = {k: {"us": round(v * 1e6, 2), "frac": round(kern[k] / v / 1e9 / HBM_PEAK_GBPS, 4)}
                                 for k, v in hot.items()}
    del wl
    torch.cuda.empty_cache()
    return out


def model_step_mode(args, device, rank, world, dist, quiet=False):
    """--step model (the default when --gpus N > 1): one TRAINING step of the host model --
    HRNetV2-W32 backbone on both frames, PWCNetHead in both flow directions, unFlowLoss (L1 + SSIM +
    smoothness, consistency), backward, Adam -- on `--pairs` synthetic 1024x512 frame pairs per rank
    (reference loop: utilities/model_trainer.py:187-226; model: cerberus.py:103-146 without the segmentation
    and depth heads, which are outside this package's scope; optimiser: configs/HRNetV2_kt.json:104-111).
    N > 1: the model is wrapped by cerberusnet_amd.distributed.wrap_ddp (DistributedDataParallel over RCCL,
    64 MB buckets, static graph): 122 MB of fp32 gradients are all-reduced inside every step, overlapped with
    the backbone's backward -- the step the >= 6x DDP target is stated on.  BatchNorm stays per-replica
    (SURVEY.md section 5).  The correlation / warp / flow-upsample / area-resize ops are this package's HIP
    kernels; convolutions and batch norms are MIOpen's.  Returns the result dict (rank 0) or None."""
    from cerberusnet_amd.distributed import wrap_ddp
    from cerberusnet_amd.loss_functions import unFlowLoss
    from cerberusnet_amd.nnet_models import CerberusBase, cerberus_flow_config
    from cerberusnet_amd.nnet_models.hrnetv2 import W18, W32, W48
    from cerberusnet_amd.synth import fill_parameters, hash_uniform
    B, H, W = args.pairs, args.height, args.width
    on_gpu = device.type == "cuda"
    sync = torch.cuda.synchronize if on_gpu else (lambda: None)
    backend = getattr(args, "model_backend", "hip")          # "torch": the reference's own fallback ops (CorrelationTorch + grid_sample) on the GPU
    if not on_gpu:
        # --device cpu: the dry run of the N > 1 route (launcher, rendezvous, DDP, timed region, no_sync pass, gather) on a box
        # without GPUs.  The product has no CPU path: the hot-path ops are the reference's own stock-PyTorch fallback here.
        backend = "torch"
        args.channels_last = False
    arch = getattr(args, "arch", "w32")
    widths = {"w18": W18, "w32": W32, "w48": W48}[arch]
    if getattr(args, "miopen_find", False):
        # MIOpen's find mode (what torch.backends.cudnn.benchmark means on ROCm): every convolution shape is timed
        # once with a workspace it may use; without it PyTorch's immediate mode takes the solver of the find-db whose
        # workspace it then cannot provide and falls back to GEMM (round 4's stderr: "IsEnoughWorkspace ...
        # GemmBwdRest / GemmWrwUniversal" on every step)
        torch.backends.cudnn.benchmark = True
    model = CerberusBase(**cerberus_flow_config(widths=widths, correlation_backend=backend)).to(device).train()
    if getattr(args, "channels_last", True):
        model = model.to(memory_format=torch.channels_last)
    fill_parameters(model.backbone, 400)                  # the same weights on every rank
    fill_parameters(model.flow, 500)
    l_img = torch.from_numpy(hash_uniform((B, 3, H, W), 11 + 1000 * rank, -2.0, 2.0)).to(device)
    l_seq = torch.from_numpy(hash_uniform((B, 3, H, W), 12 + 1000 * rank, -2.0, 2.0)).to(device)
    # (CERB_FORCE_DIST=1 on one GPU: a one-rank RCCL group, the model really under DDP -- the self-test of this path)
    net = wrap_ddp(model, device, force=dist is not None, sync_bn=args.sync_bn) if dist is not None else model
    ddp = net is not model
    loss_fn = unFlowLoss(weights={"l1": 0.15, "ssim": 0.85}, consistency=True, backend=backend)
    if getattr(args, "channels_last", True):
        l_img, l_seq = l_img.contiguous(memory_format=torch.channels_last), l_seq.contiguous(memory_format=torch.channels_last)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-4, betas=(0.9, 0.99), weight_decay=1e-6)
    amp = args.dtype in ("f16", "bf16") and on_gpu
    adt = {"f16": torch.float16, "bf16": torch.bfloat16}.get(args.dtype)
    scaler = torch.amp.GradScaler(device.type, enabled=(args.dtype == "f16" and on_gpu))
    # test hook (tests/test_bench_cpu.py): "rank:step" -- that rank raises inside that timed step.  A failing rank must
    # take the whole job down with a non-zero exit code, never leave its peers waiting in a collective
    fail_rank, fail_step = (int(v) for v in os.environ.get("CERB_BENCH_FAIL_AT", "-1:-1").split(":"))
    nstep = [0]

    def step(timed=False):
        if timed:
            if rank == fail_rank and nstep[0] == fail_step:
                raise RuntimeError("CERB_BENCH_FAIL_AT: injected failure on rank %d in timed step %d" % (rank, fail_step))
            nstep[0] += 1
        opt.zero_grad(set_to_none=True)
        with torch.autocast(device.type, dtype=adt, enabled=amp):
            out = net(l_img=l_img, l_seq=l_seq, consistency=True)
            loss = loss_fn({k: [f.float() for f in v] for k, v in out.items()}, {"l_img": l_img, "l_seq": l_seq})
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        return loss

    def fence():
        sync()
        if dist is not None:
            dist.barrier()
            sync()

    warm = max(3, args.warmup) if on_gpu else max(1, args.warmup)
    for _ in range(warm):
        loss = step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step(timed=True)
    fence()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    # N > 1: the same step on every rank's own GPU WITHOUT the gradient exchange (DDP's no_sync), timed after the DDP
    # region: the per-GPU rate the scaling of `value` is to be read against, measured on this node in this run
    single = None
    if ddp:
        # every rank reaches the two collectives below whether or not its own pass failed (an exception on one rank
        # must not leave the others hanging in the timing all-reduce): the first carries an error flag, the second the time
        err, ds = None, 0.0
        try:
            with net.no_sync():
                for _ in range(2 if on_gpu else 1):
                    step()
                sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                sync()
                ds = time.perf_counter() - t0
        except Exception as exc:  # a side report: never fail the line on it
            err = exc
        t = torch.tensor([1.0 if err is not None else 0.0, ds], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        if float(t[0].item()) > 0:
            single = {"error": repr(err)[:200] if err is not None else "another rank failed in this pass"}
        else:
            ds = float(t[1].item())
            single = {"pairs_per_s_per_gpu": round(B * args.steps / ds, 2), "ms_per_step": round(1e3 * ds / args.steps, 4),
                      "what": "the same training step on every rank's GPU with the gradient all-reduce switched off "
                              "(DistributedDataParallel.no_sync), slowest rank, timed after the DDP region: "
                              "value / (n_gpus x this) is the scaling of the DDP step on this node"
                              + ("; NOT collective-free: --sync-bn keeps SyncBatchNorm's all-reduces in this pass too" if args.sync_bn else "")
                              + "; the optimizer steps on the rank's own (unreduced) gradients here: ranks diverge after this pass, which is why it runs last"}
    # the same step with the hot-path ops swapped for the reference's own stock-PyTorch fallback (CorrelationTorch +
    # grid_sample + F.interpolate: SURVEY 8(d) "the same model with the op swapped") and under bf16 autocast, in THIS process
    # (same model, MIOpen's solvers already chosen): a side table, one rank only
    table = None
    if getattr(args, "model_table", False) and world == 1 and not ddp:
        table = {}
        head = model.flow
        for tag, bk, dt_ in (("f32_hip", "hip", None), ("f32_torch", "torch", None), ("bf16_hip", "hip", torch.bfloat16),
                             ("bf16_torch", "torch", torch.bfloat16)):
            try:
                head.correlation_backend, loss_fn.backend = bk, bk
                amp, adt = dt_ is not None, dt_
                scaler = torch.amp.GradScaler("cuda", enabled=False)
                for _ in range(2):
                    step()
                sync()
                t0 = time.perf_counter()
                for _ in range(5):
                    step()
                sync()
                ms = (time.perf_counter() - t0) / 5 * 1e3
                table[tag] = {"ms_per_step": round(ms, 2), "pairs_per_s": round(B / ms * 1e3, 2)}
            except Exception as exc:
                table[tag] = {"error": repr(exc)[:160]}
        head.correlation_backend, loss_fn.backend = backend, backend
    if rank != 0:
        return None
    nparam = sum(p.numel() for p in params)
    result = {
        "metric": METRIC, "value": round(B * world * args.steps / dt, 2), "unit": "image-pairs/s",
        "n_gpus": world, "steps": args.steps, "warmup": warm,
        "ms_per_step": round(1e3 * dt / args.steps, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {
            "step": "model",
            "value_times": "`value` = image pairs per second of the whole DDP training step (all ranks); `single_gpu_step` = the "
                           "same step per GPU without the gradient exchange; `scaling_efficiency` = value / (n_gpus x single_gpu_step)",
            "workload": "one training step of the host model (HRNetV2-%s backbone + PWCNetHead / FlowEstimatorLite, "
                        "%d parameters, hash-filled; BASELINE configs 3 / 4 without the segmentation and depth heads) on "
                        "%d synthetic %dx%d frame pairs per %s: backbone on both frames, flow head in both directions, "
                        "unFlowLoss, backward, Adam%s" % (arch.upper(), nparam, B, W, H, "GPU" if on_gpu else "rank (CPU dry run)",
                                                          "; autocast " + args.dtype if amp else ""),
            "pairs_per_gpu": B, "frame": [H, W], "parameters": nparam, "gradient_bytes_per_step": 4 * nparam,
            "launch": "eager", "backend": backend, "miopen_find": bool(getattr(args, "miopen_find", False)),
            "channels_last": bool(getattr(args, "channels_last", True)),
            "device": device.type, "collective_backend": (dist.get_backend() if dist is not None else None),
            "sharding": ("image pairs sharded over ranks; DistributedDataParallel over %s (64 MB buckets, static graph): "
                         "%.1f MB of gradients all-reduced inside every step, overlapped with backward"
                         % ("RCCL" if on_gpu else "gloo (CPU dry run of the route)", 4e-6 * nparam)
                         if ddp else "one rank"),
            "hot_path_ops": ("cerberus:: HIP kernels (correlation_leaky_into, flow_warp, flow_upsample, area_resize)" if backend == "hip"
                             else "the reference's stock-PyTorch fallback (CorrelationTorch + grid_sample + F.interpolate)"),
            "loss_last_step": float(loss.item()),
        },
        "roofline": None, "cpu_baseline": None,
        "note": "the op-only headline (python bench.py --gpus 1, or --step ops at any N) carries roofline and cpu_baseline; "
                "to judge scaling compare `value` with n_gpus x `single_gpu_step` of this line (or with `extra.model_step` of "
                "the N = 1 line): the N = 1 default line times a different step (the ops alone)",
    }
    if single is not None:
        # top level: the like-for-like figures of THIS step, so that no reader divides by the
        # N = 1 default line (which times the ops alone)
        result["single_gpu_step"] = single
        if "pairs_per_s_per_gpu" in single:
            result["scaling_efficiency"] = round(result["value"] / (world * single["pairs_per_s_per_gpu"]), 4)
    if table is not None:
        result["backend_table"] = dict(table, what="5 steps each after 2 warm-up steps, same process and model: the hot-path ops as "
                                       "this package's HIP kernels (hip) or as the reference's stock-PyTorch fallback on the same GPU "
                                       "(torch: CorrelationTorch + grid_sample + F.interpolate), fp32 and bf16 autocast")
    if not quiet:
        print(json.dumps(result), flush=True)
    return result


DUMP_BYTES = 48 << 20      # --dump-outputs writes at most this many bytes of array data in all


def dump_indices(name, numel, count):
    """The flat indices of the elements --dump-outputs keeps of an array: `count` of its `numel` drawn without
    replacement by numpy's default_rng seeded with crc32(name), in increasing order -- the same in every run."""
    import zlib
    return np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(numel, count, replace=False))


def dump_outputs(outputs, path):
    """--dump-outputs: every tensor of `outputs` ({name: tensor}) as <path>/<name>.npy in float32.  A tensor larger
    than its even share of DUMP_BYTES is written as the 1-D sample dump_indices() picks of its flattened elements."""
    os.makedirs(path, exist_ok=True)
    share = DUMP_BYTES // 4 // max(1, len(outputs))
    for name, t in outputs.items():
        t = t.detach()
        if t.numel() > share:
            t = t.reshape(-1)[torch.from_numpy(dump_indices(name, t.numel(), share)).to(t.device)]
        np.save(os.path.join(path, name + ".npy"), t.float().cpu().numpy())


def _default_steps(args, steps, warmup):
    """--steps / --warmup not given: the defaults of the step being timed (one of them given: the other one keeps
    the op step's default)."""
    if args.steps is None and args.warmup is None:
        args.steps, args.warmup = steps, warmup
    args.steps = 200 if args.steps is None else args.steps
    args.warmup = 20 if args.warmup is None else args.warmup
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps (default 200 for the op step; --step model 20, --step head 30, --device cpu 3)")
    ap.add_argument("--warmup", type=int, default=None,
                    help="untimed steps right before the timed ones (default 20; --step model 3, --step head 5, "
                         "--device cpu 1)")
    ap.add_argument("--full", action="store_true",
                    help="the op step: after the headline also measure everything beside it -- the per-kernel, in-step "
                         "and counter passes and the roofline they feed, the steady-state and after-idle passes, the "
                         "stock-PyTorch GPU and CPU baselines and the extra configurations (extra.*).  Without it a run "
                         "sets up, warms up, times the K steps and prints the headline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="the op step: after the timed steps write what the last one computed -- per flow direction and "
                         "level the correlation output, the warped image and the gradients of f1, f2 and the flow -- as "
                         "DIR/<name>.npy in float32 (at most 48 MiB in all: larger arrays as a fixed, seeded sample of "
                         "their elements); the inputs are the same in every run with the same arguments")
    ap.add_argument("--pairs", type=int, default=4, help="image pairs per GPU per step")
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--dtype", choices=["f32", "f16", "bf16"], default="f32",
                    help="storage type of the feature maps (arithmetic is fp32 throughout); "
                         "BASELINE config 5 is --dtype f16 --width 2048 --height 1024")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--fuse-directions", action="store_true",
                    help="stack both flow directions into one batched call per op")
    ap.add_argument("--serial-directions", action="store_true",
                    help="issue both flow directions on one stream (default: two streams)")
    ap.add_argument("--no-stagger", action="store_true",
                    help="two streams: start both directions together (default: the second one forks after the first "
                         "direction's first launch, so that the streams pair different kernels)")
    ap.add_argument("--stack-coarse", type=int, default=1, metavar="N",
                    help="the two flow directions as ONE batched call per op on the N coarsest levels (where a launch is priced by "
                         "its latency), two streams above (VERDICT r4 #8; default 1: level 0 stacked, -6.7 us per step; 2 loses; "
                         "0 = rounds 1-4: every level on two streams)")
    ap.add_argument("--stack-levels", default=None, metavar="L,L",
                    help="experiment: exactly these levels as one batched call for both directions (joins / forks around them); "
                         "overrides --stack-coarse")
    ap.add_argument("--chains", type=int, default=1,
                    help="split each direction's batch into this many independent sub-batches, "
                         "one HIP stream each")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip torch_gpu_reference and cpu_baseline")
    ap.add_argument("--no-extra", action="store_true",
                    help="--full: skip the short side passes (extra.config5_f16, extra.bf16_1024x512, extra.flow_noise, "
                         "extra.ragged, extra.loss_side, extra.model_step)")
    ap.add_argument("--probe-steps", type=int, default=20)
    ap.add_argument("--flow", choices=["smooth", "noise"], default="smooth",
                    help="synthetic flow fields fed to the warp (see Workload._flow)")
    ap.add_argument("--with-exchange", action="store_true",
                    help="N > 1, --step ops: time `value` WITH the model-sized gradient all-reduce beside every step "
                         "(default: the op-only rate; the exchange is timed in a second pass and reported beside it)")
    ap.add_argument("--no-exchange", action="store_true", help="(the default now; accepted for old command lines)")
    ap.add_argument("--grad-mb", type=float, default=GRAD_BYTES / 1e6,
                    help="size of the gradient buffer exchanged per step (MB, fp32)")
    ap.add_argument("--bucket-mb", type=float, default=64.0)
    ap.add_argument("--no-mfma", action="store_true",
                    help="fp16 / bf16: keep the correlation on the vector kernels (option corr_no_mfma); "
                         "the fp32 path uses no MFMA either way")
    ap.add_argument("--step", choices=["ops", "head", "model"], default=None,
                    help="default: ops on one GPU, model when --gpus N > 1.  model: one training step of the host model "
                         "(HRNetV2-W32 + PWCNetHead, loss, backward, Adam) under DistributedDataParallel when N > 1 -- the "
                         "step whose 122 MB gradient all-reduce DDP scaling is judged on; "
                         "ops (the headline): the hot-path ops alone, both directions x 4 levels; "
                         "head: one training step of the whole flow head (PWCNetHead, FlowEstimatorLite) on the same "
                         "pyramid -- both directions, loss, backward -- under DistributedDataParallel when N > 1, so the "
                         "gradient all-reduce runs inside the step it can hide behind")
    ap.add_argument("--stack-directions", action="store_true",
                    help="--step head: run both flow directions as one stacked pass (PWCNetHead.forward_both)")
    ap.add_argument("--model-backend", choices=["hip", "torch"], default="hip",
                    help="--step model: the hot-path ops of the host model: this package's HIP kernels, or the reference's "
                         "own stock-PyTorch fallback (CorrelationTorch + grid_sample) on the same GPU")
    ap.add_argument("--miopen-find", action="store_true",
                    help="--step model: torch.backends.cudnn.benchmark = True (MIOpen find mode: ~4 minutes of solver "
                         "compilation on a fresh box, then 147.8 instead of 172.6 ms per fp32 step, 134.5 instead of 147.1 bf16)")
    ap.add_argument("--nchw", dest="channels_last", action="store_false",
                    help="--step model: NCHW weights and inputs (round 4's layout: MIOpen's immediate mode then falls back to "
                         "GEMM solvers with workspace warnings on every step and 16.6 ms per step go to layout transposes)")
    ap.add_argument("--model-table", action="store_true",
                    help="--step model at N = 1: after the timed region also time the step with the stock-PyTorch fallback ops and "
                         "under bf16 autocast (`backend_table`)")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-cold", action="store_true", help="--full: skip the cold (HBM-resident inputs) per-kernel pass")
    ap.add_argument("--sync-bn", action="store_true",
                    help="--step model, N > 1: SyncBatchNorm instead of per-replica BatchNorm statistics")
    ap.add_argument("--no-traffic", action="store_true",
                    help="--full: skip the two counter passes (FETCH_SIZE / WRITE_SIZE children) behind roofline.traffic; the committed "
                         "figure of profiles/ is reported instead, labelled as such")
    ap.add_argument("--probe-after", action="store_true",
                    help="--full: run the per-kernel passes after the timed region (the order of rounds 1-3) instead of before it")
    ap.add_argument("--bwd-variant", type=int, default=0, help="experiments: option corr_bwd_variant")
    ap.add_argument("--fwd-variant", type=int, default=0, help="experiments: option corr_fwd_variant")
    ap.add_argument("--bwd-cslice", type=int, default=0, help="experiments: option corr_bwd_cslice")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                    help="experiments: set a library tuning option (include/cerberus_hip.h), repeatable")
    ap.add_argument("--device", choices=["cuda", "cpu"], default="cuda",
                    help="cpu: dry run of the N > 1 route without GPUs (gloo; --step model only, the host model on the "
                         "reference's stock-PyTorch fallback ops: the product itself has no CPU path)")
    ap.add_argument("--arch", choices=["w18", "w32", "w48"], default="w32", help="--step model: HRNetV2 width")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world == 1 and "RANK" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.device == "cpu":
        # the N > 1 route on a box without GPUs: same launcher / rendezvous / DDP / timed region / gather, gloo instead of RCCL
        if (args.step or "model") != "model":
            raise SystemExit("--device cpu runs --step model only (the hot-path ops have no CPU implementation)")
        if args.dump_outputs:
            raise SystemExit("--dump-outputs writes the outputs of the op step (--step ops) only")
        args.step = "model"
        device = torch.device("cpu")
        dist = None
        if world > 1 or os.environ.get("CERB_FORCE_DIST") == "1":
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29511")
            dist.init_process_group("gloo", rank=rank, world_size=world)
        _default_steps(args, 3, 1)
        torch.set_num_threads(max(1, usable_cores()[0] // max(1, world)))      # not os.cpu_count(): see usable_cores()
        model_step_mode(args, device, rank, world, dist)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU path exists for the product)")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if args.no_mfma or args.bwd_variant or args.fwd_variant or args.bwd_cslice:
        from cerberusnet_amd import _lib as _cerb_lib
        _cerb_lib.set_option("corr_no_mfma", int(args.no_mfma))
        _cerb_lib.set_option("corr_bwd_variant", args.bwd_variant)
        _cerb_lib.set_option("corr_fwd_variant", args.fwd_variant)
        _cerb_lib.set_option("corr_bwd_cslice", args.bwd_cslice)
    for kv in args.option:
        from cerberusnet_amd import _lib as _cerb_lib
        name, _, val = kv.partition("=")
        _cerb_lib.set_option(name, int(val))
    dist = None
    if world > 1 or os.environ.get("CERB_FORCE_DIST") == "1":  # the latter: 1-rank RCCL self-test
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)  # RCCL

    if args.trace_child:
        _default_steps(args, 200, 20)
        trace_child(args, device)
        return
    if args.step is None:
        args.step = "model" if world > 1 else "ops"
    if args.dump_outputs and args.step != "ops":
        raise SystemExit("--dump-outputs writes the outputs of the op step (--step ops) only")
    if args.step == "model":
        _default_steps(args, 20, 3)      # the op step's defaults are sized for its 0.4 ms
        model_step_mode(args, device, rank, world, dist)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    if args.step == "head":
        if args.dtype != "f32":
            raise SystemExit("--step head runs in fp32")
        if world > 1 and dist is None:
            raise SystemExit("--step head with N > 1 needs torch.distributed")
        _default_steps(args, 30, 5)      # the op step's defaults are sized for its 0.4 ms
        head_step_mode(args, device, rank, world, dist)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    _default_steps(args, 200, 20)
    dtype = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    wl = Workload(args.pairs, args.width, args.height, device, args.flow, args.fuse_directions,
                  args.chains, dtype)
    wl.stagger = not args.no_stagger

    # ---- warm-up (eager), then capture the step into a hipGraph ----
    streams = None if args.serial_directions else [torch.cuda.Stream()
                                                   for _ in range(max(1, len(wl.dirs) - 1))]
    hybrid = bool(args.stack_coarse and streams and len(wl.dirs) == 2)
    step_fn = (lambda: wl.step_hybrid(streams, args.stack_coarse)) if hybrid else (lambda: wl.step(streams))
    if args.stack_levels is not None and streams and len(wl.dirs) == 2:
        stacked_set = {int(v) for v in args.stack_levels.split(",") if v != ""}
        step_fn = lambda: wl.step_stacked(streams, stacked_set)
    for _ in range(max(1, args.warmup if args.no_graph else 3)):
        step_fn()
    torch.cuda.synchronize()
    graph = None
    if not args.no_graph:
        cap = torch.cuda.Stream()
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap):
            step_fn()
        torch.cuda.current_stream().wait_stream(cap)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            held = step_fn()  # noqa: F841  keep outputs alive for the graph's pool
    run = graph.replay if graph is not None else step_fn
    # the tensors the captured step writes its results into (every replay rewrites them); eagerly, the last step's
    # own tensors, taken after the timed region
    step_results = dict(wl.results) if graph is not None else None

    # ---- per-kernel pass (rank 0 only): every launch of the step timed on its own ----
    # R back-to-back launches of ONE kernel are captured into a hipGraph (no host launch gaps between them) and
    # the replay is bracketed by HIP events on the launch stream; the in-step pass reads a profiler trace of a child.
    # Round 4: these passes run BEFORE the timed region instead of after it.  They are seconds of GPU work that
    # the line needs anyway, and with them in front the W warm-up steps and the K timed steps start on a chip
    # that is already at its working clock: with the driver's --steps 20 --warmup 5 (a 7 ms timed region) the
    # same build on the same box read 10.8 k pairs/s with the passes behind the timed region and 12.1 k at
    # --steps 200 -- the first replays after seconds of host-side set-up ran at the idle clock.  Run with --full only.
    probe = None
    if rank == 0 and args.full and not args.probe_after:
        instep, instep_info = ((None, "skipped") if (args.no_cold or args.fuse_directions or args.chains > 1 or world > 1)
                               else in_step_times(args, len(wl.levels)))
        live, live_info = ((None, "skipped") if instep is None or args.no_traffic else live_traffic(args, len(wl.levels)))
        hot, cold = per_kernel_times(wl, max(2, args.probe_steps), cold=not args.no_cold)
        probe = (hot, cold, instep, instep_info, live, live_info)
    # The step's steady-state time by HIP events over 60 back-to-back replays: a figure of its own (the rate a training
    # loop sees once it runs) AND the last pass before the warm-up + timed region, which therefore start on a chip that is
    # in its working state.  Measured (profiles/r04_replay_gaps.txt): after >= 10 ms of idle -- and the set-up, capture and
    # single-kernel probe passes above are full of such gaps -- this chip runs the next ~8 ms of work 5-12 % slow (0.39 ->
    # 0.36 -> 0.39 -> 0.365 ms per replay over 24 replays), a transient longer than the driver's whole 20-step timed region;
    # 40 replays, a synchronize and <= 3 ms of idle later it holds 0.34 ms from the first replay.  Nothing is skipped or
    # shortened inside the timed region; --probe-after restores the order of rounds 1-3.
    steady = None
    if dist is not None and world > 1:
        # only rank 0 runs the seconds-long probe passes above: the other ranks wait HERE, not inside the timed region's
        # first fence, so that every rank runs its steady-state pass right before the warm-up + timed steps
        dist.barrier()
    if graph is not None and not args.probe_after:
        for _ in range(20):
            graph.replay()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(60):
            graph.replay()
        ev1.record()
        torch.cuda.synchronize()
        steady = {"ms_per_step": round(ev0.elapsed_time(ev1) / 60, 5), "replays": 60,
                  "pairs_per_s_per_gpu": round(args.pairs * 60 / (ev0.elapsed_time(ev1) * 1e-3), 1),
                  "what": "HIP events around 60 back-to-back replays of the step graph after 20 untimed ones, on this rank; "
                          "run right before the W warm-up and K timed steps (the chip's post-idle transient, "
                          "profiles/r04_replay_gaps.txt, is over by then)"}
    steady_slowest = None
    if steady is not None and dist is not None and world > 1:
        t = torch.tensor([steady["pairs_per_s_per_gpu"]], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        steady_slowest = float(t.item())
    if graph is not None:
        for _ in range(args.warmup):
            graph.replay()

    # ---- the gradient exchange of data-parallel training (N > 1) ----
    exchange = None
    if dist is not None and world > 1:
        from cerberusnet_amd.distributed import GradientExchange
        exchange = GradientExchange(int(args.grad_mb * 1e6) // 4, device, args.bucket_mb)
        for _ in range(3):
            exchange.start()
            exchange.finish()
        torch.cuda.synchronize()

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    def timed(steps, with_exchange):
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            if with_exchange:
                exchange.start()      # last step's gradients travel beside this step's kernels
            run()
            if with_exchange:
                exchange.finish()
        fence()
        dt = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    use_exchange = exchange is not None and args.with_exchange and not args.no_exchange
    if graph is None:
        wl.results = {}      # eager: only what the timed steps record (the per-kernel pass records one direction)
    elapsed = timed(args.steps, use_exchange)
    if args.dump_outputs and rank == 0:
        dump_outputs(wl.outputs(step_results), args.dump_outputs)
    # Round-over-round comparability: rounds 1-3 timed the K steps right after seconds of
    # host-side set-up (the chip's post-idle transient inside the timed region); since round 4 the measurement passes and 80
    # replays of the steady-state pass come first.  The old-order figure is reproduced here, after the headline: 0.5 s of
    # idle, the same W warm-up replays, the same K timed steps.
    after_idle = None
    if graph is not None and args.full and not args.probe_after:
        time.sleep(0.5)
        for _ in range(args.warmup):
            graph.replay()
        after_idle = timed(args.steps, use_exchange)
    extra = {}
    if exchange is not None:
        # the other variant and the exchange alone (bus bandwidth), outside the headline region
        other = timed(args.steps, not use_exchange)
        fence()
        t0 = time.perf_counter()
        reps = 10
        for _ in range(reps):
            exchange.start()
            exchange.finish()
        fence()
        ar = (time.perf_counter() - t0) / reps
        t = torch.tensor([ar], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ar = float(t.item())
        pairs_total = args.pairs * world * args.steps
        extra = {
            "gradient_exchange": {
                "in_timed_loop": use_exchange, "bytes_per_step": exchange.nbytes,
                "buckets": len(exchange.buckets), "bucket_mb": args.bucket_mb,
                "collective": "RCCL all_reduce(AVG) per bucket on a side stream, overlapped with the step",
                "allreduce_ms": round(ar * 1e3, 4),
                "allreduce_busbw_GBps": round(GradientExchange.bus_bandwidth(exchange.nbytes, ar, world) / 1e9, 1),
                "pairs_per_s_with_exchange": round(pairs_total / (elapsed if use_exchange else other), 2),
                "pairs_per_s_without_exchange": round(pairs_total / (other if use_exchange else elapsed), 2),
            }}

    result = None
    if rank == 0:
        pairs_total = args.pairs * world * args.steps
        kern = dict(wl.kernels())
        ndir = len(wl.dirs)                                       # 2, or 1 when fused (2x batch)
        step_bytes = ndir * sum(kern.values())
        corr_step_bytes = ndir * sum(v for k, v in kern.items() if k.startswith("corr"))
        cfg = ("BASELINE config 3 tensors" if (args.width, args.height, args.dtype) == (1024, 512, "f32")
               else "BASELINE config 5 tensors" if (args.width, args.height, args.dtype) == (2048, 1024, "f16")
               else "custom tensors")
        result = {
            "metric": METRIC, "value": round(pairs_total / elapsed, 2), "unit": "image-pairs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 5), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {
                "step": "ops",
                "workload": "%s (HRNetV2-W32 pyramid of %dx%d, corr d=4 + flow-warp, %s), %d image "
                            "pairs per GPU per step (config 4's per-GPU batch), both flow "
                            "directions, fwd+bwd; flow fields fed to the warp: %s" % (cfg, args.width, args.height, args.dtype, args.pairs,
                            "smooth (an upsampled coarse field, as the flow head produces; the per-pixel uniform field of "
                            "SURVEY 8(d) is extra.flow_noise)" if args.flow == "smooth" else "per-pixel uniform [-6, 6) px (SURVEY 8(d))"),
                "value_times": "`value` = image pairs per second of the op-only step (all ranks)",
                "pairs_per_gpu": args.pairs, "levels_CHW": [list(s) for s in wl.levels],
                "flow_field": args.flow,
                "flow_field_note": "`smooth` (the headline) = what PWCNetHead feeds the warp: a coarse random field in [-6, 6) px "
                                   "upsampled x8 bilinearly (pwcnet_sfd.py:176) + 0.25 px of residual; SURVEY 8(d)'s per-pixel "
                                   "uniform [-6, 6) field (`noise`, what the parity tests use) is timed as extra.flow_noise",
                "stack_coarse": args.stack_coarse if hybrid else 0,
                "stack_levels": args.stack_levels,
                "launch": ("hipGraph replay" if graph is not None else "eager") +
                          (", directions fused into one batched call" if args.fuse_directions else
                           ", %d streams (one per flow direction%s%s)" % (
                               len(streams) + 1, " and sub-batch" if args.chains > 1 else "",
                               ("; the %d coarsest level(s) as one call for both directions (8 items) at the two ends of the step"
                                % args.stack_coarse) if hybrid else
                               ", the second forks after the first one's first launch" if wl.stagger else "")
                           if streams else ", 1 stream"),
                "sharding": ("image pairs sharded over ranks, no data-path collective in the ops; value = "
                             + ("the rate WITH the model-sized gradient all-reduce beside every step"
                                if use_exchange else "the op-only rate (the ops have no parameters)")
                             + "; see gradient_exchange") if world > 1 else
                            "one rank (image pairs are sharded over ranks when N > 1)",
                "algorithmic_bytes_per_step": step_bytes,
                "step_algorithmic_GBps_per_gpu": round(step_bytes * args.steps / elapsed / 1e9, 1),
                "corr_only_frac_of_hbm_peak_whole_step": round(
                    corr_step_bytes * args.steps / elapsed / 1e9 / HBM_PEAK_GBPS, 4),
            },
        }
        result.update(extra)
        if steady is not None and (args.full or world > 1):
            result["steady_state"] = steady
        if world > 1 and steady is not None:
            # the like-for-like ratio at the top level of every N > 1 line: the ops have no collective, so the single-GPU
            # figure is the slowest rank's own steady-state rate of the same step graph, measured in this run
            result["single_gpu_step"] = {"pairs_per_s_per_gpu": steady_slowest, "what": "slowest rank's steady-state rate of the "
                                         "same op-only step graph (HIP events over 60 replays, no other rank's work involved)"}
            result["scaling_efficiency"] = round(result["value"] / (world * steady_slowest), 4)
        # what preceded the timed region besides the W warm-up steps `warmup` reports
        result["pre_timed"] = {
            "probe_order": ("after" if args.probe_after else "before") if args.full else "not run (--full runs them)",
            "graph_replays_before_warmup": 0 if (args.probe_after or graph is None) else 80,
            "what": ("the per-kernel / in-step / counter passes (rank 0) and the 20 + 60 replays of the steady_state pass "
                     "(every rank) run BEFORE the W warm-up and K timed steps; rounds 1-3 ran the probes after the timed "
                     "region (--probe-after): compare those rounds with first_steps_after_idle") if args.full else
                    ("20 + 60 untimed replays of the step graph (every rank) run BEFORE the W warm-up and K timed steps, "
                     "so that these start on a chip in its working state")}
        if after_idle is not None:
            result["first_steps_after_idle"] = {
                "value": round(pairs_total / after_idle, 2), "unit": "image-pairs/s",
                "ms_per_step": round(1e3 * after_idle / args.steps, 5), "idle_s": 0.5,
                "steps": args.steps, "warmup": args.warmup,
                "what": "the same W warm-up + K timed replays started 0.5 s after the chip went idle: the order of rounds "
                        "1-3 (what --probe-after measures as `value`); the chip's post-idle transient lies inside it"}

    # ---- the roofline report from the per-kernel passes ----
    if rank == 0 and args.full:
        if probe is None:   # --probe-after: the round-3 order
            hot, cold = per_kernel_times(wl, max(2, args.probe_steps), cold=not args.no_cold)
            instep, instep_info = ((None, "skipped") if (args.no_cold or args.fuse_directions or args.chains > 1 or world > 1)
                                   else in_step_times(args, len(wl.levels)))
            live, live_info = ((None, "skipped") if instep is None or args.no_traffic else live_traffic(args, len(wl.levels)))
        else:
            hot, cold, instep, instep_info, live, live_info = probe
        # The roofline figures use the IN-STEP launch time (the profiler's kernel durations while the whole
        # step replays on one stream: caches in the state the step leaves them in); "us_hot" (one launch
        # replayed on the same tensors, HIP events: Infinity-Cache resident) and "us_cold" (inputs from
        # HBM, HIP events) bracket it and are reported beside it.  Without the in-step pass (--no-cold,
        # or no rocprofv3): cold if measured, else hot.
        per = instep if instep else (cold if cold else hot)
        kern = dict(wl.kernels())
        gbps = lambda k: kern[k] / per[k] / 1e9
        # dominant kernel = the longest single launch of the step, over ALL kernels; the longest
        # correlation launch is reported beside it (BASELINE's second metric is the
        # correlation's achieved HBM rate)
        dominant = max(per, key=lambda k: per[k])
        dom_corr = max((k for k in per if k.startswith("corr")), key=lambda k: per[k])
        corr_t = sum(v for k, v in per.items() if k.startswith("corr"))
        corr_b = sum(v for k, v in kern.items() if k.startswith("corr"))
        top = len(wl.levels) - 1
        fb_t = per["corr_fwd_L%d" % top] + per["corr_bwd_L%d" % top]
        fb_b = kern["corr_fwd_L%d" % top] + kern["corr_bwd_L%d" % top]
        # HBM-side bytes per launch: measured by this run (live_traffic: two counter passes of children); without
        # a profiler, the committed figure of profiles/ (tools/collect_profiles.sh), labelled as a constant
        traffic, traffic_src = None, None
        if live is not None:
            traffic = live[dominant]["traffic_bytes"]
            traffic_src = dict(live_info, measured_by_this_run=True,
                               ratio_to_algorithmic=round(traffic / kern[dominant], 3))
        cfg_key = (args.width, args.height, args.dtype)
        tnames = {(1024, 512, "f32"): ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json"),
                  (2048, 1024, "f16"): ("r06_config5_f16_pmc_traffic.json", "r05_config5_f16_pmc_traffic.json", "r04_config5_f16_pmc_traffic.json",
                                        "r03_config5_f16_pmc_traffic.json", "r02_config5_f16_pmc_traffic.json")}.get(cfg_key, ())
        for tname in tnames:
            tpath = os.path.join(REPO, "profiles", tname)
            if traffic is None and os.path.exists(tpath) and args.pairs == 4 and not args.fuse_directions:
                blob = json.load(open(tpath))
                traffic = blob.get(dominant, {}).get("traffic_bytes")
                traffic_src = {"file": "profiles/" + tname,
                               "commit": blob.get("_commit"), "kernels": blob.get("_kernels"),
                               "note": "constant from the committed PMC passes, not collected by this run"}
                break
        result["roofline"] = {
            "bound": "hbm", "achieved": round(gbps(dominant), 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": round(gbps(dominant) / HBM_PEAK_GBPS, 4), "traffic": traffic,
            "traffic_source": traffic_src, "kernel": dominant,
            "avg_us": round(per[dominant] * 1e6, 2), "algorithmic_bytes": kern[dominant],
            "timing": ("in-step: kernel durations from a rocprofv3 kernel trace of the whole step replayed on one stream "
                       "(a child process of this run), %d launches per kernel" % instep_info["launches_per_label"]
                       if instep else
                       "cold: every launch of the timed graph works on its own copy of the tensors, > 256 MiB "
                       "(the Infinity Cache) apart" if cold else
                       "hot: one launch replayed on the same tensors (Infinity-Cache resident)"),
            "in_step": instep_info if instep else {"unavailable": instep_info},
            "dominant_any": dominant,
            "dominant_corr": {"kernel": dom_corr, "avg_us": round(per[dom_corr] * 1e6, 2),
                              "GBps": round(gbps(dom_corr), 1),
                              "frac": round(gbps(dom_corr) / HBM_PEAK_GBPS, 4)},
            # the quantity the north star's 60 % is stated on: correlation fwd+bwd at the
            # finest level (1024x512: 32x128x256)
            "corr_fwd_bwd_L%d" % top: {"us": round(fb_t * 1e6, 2), "GBps": round(fb_b / fb_t / 1e9, 1),
                                        "frac": round(fb_b / fb_t / 1e9 / HBM_PEAK_GBPS, 4)},
            "corr_all_levels": {"GBps": round(corr_b / corr_t / 1e9, 1),
                                "frac": round(corr_b / corr_t / 1e9 / HBM_PEAK_GBPS, 4),
                                "us_per_direction": round(corr_t * 1e6, 2)},
            "per_kernel": {k: {"us": round(per[k] * 1e6, 2), "us_hot": round(hot[k] * 1e6, 2),
                               "us_cold": round(cold[k] * 1e6, 2) if cold else None,
                               "us_in_step": round(instep[k] * 1e6, 2) if instep else None,
                               "GBps": round(gbps(k), 1), "frac": round(gbps(k) / HBM_PEAK_GBPS, 4),
                               "traffic": live[k]["traffic_bytes"] if live else None,
                               "traffic_over_algorithmic": round(live[k]["traffic_bytes"] / kern[k], 3) if live else None}
                           for k in sorted(per)},
        }
        try:
            from cerberusnet_amd import _lib
            result["roofline"]["variants"] = [_lib.last_kernel(0), _lib.last_kernel(1)]
        except Exception:  # diagnostics only
            pass
        if not args.no_cpu_baseline and world == 1:
            try:
                result["torch_gpu_reference"] = torch_gpu_reference(wl)
            except Exception as exc:  # context only: never fail the bench line on it
                result["torch_gpu_reference"] = {"error": repr(exc)[:200]}
            result["cpu_baseline"] = cpu_baseline(wl.levels)
        elif not args.no_cpu_baseline:
            result["cpu_baseline"] = None
        if world == 1 and not args.no_extra and (args.width, args.height, args.dtype, args.pairs) == (1024, 512, "f32", 4) \
                and not (args.fuse_directions or args.serial_directions or args.chains > 1 or args.no_graph):
            extra_lines = {}
            try:    # BASELINE config 5 (AMP fp16 storage, 2048x1024 frames), value only
                extra_lines["config5_f16"] = dict(
                    short_ops_rate(4, 2048, 1024, torch.float16, device),
                    workload="BASELINE config 5 tensors (HRNetV2-W32 pyramid of 2048x1024, fp16 storage, fp32 "
                             "accumulation), 4 image pairs, both directions, fwd+bwd; same launch as the headline")
            except Exception as exc:  # never fail the headline on a side report
                extra_lines["config5_f16"] = {"error": repr(exc)[:200]}
            try:    # bf16 storage at the headline's own pyramid (AMP with bf16), value only
                extra_lines["bf16_1024x512"] = dict(
                    short_ops_rate(4, 1024, 512, torch.bfloat16, device),
                    workload="the headline's tensors in bf16 storage (fp32 accumulation), 4 image pairs, both directions, "
                             "fwd+bwd; same launch as the headline")
            except Exception as exc:
                extra_lines["bf16_1024x512"] = {"error": repr(exc)[:200]}
            try:    # the headline's schedule since round 5 stacks level 0 of both directions; the schedule of rounds 1-4 beside it
                sc = short_ops_rate(4, 1024, 512, torch.float32, device, steps=100, warmup=20)
                extra_lines["stack_coarse_0"] = dict(
                    value=sc["value"], unit=sc["unit"], ms_per_step=sc["ms_per_step"], steps=sc["steps"], warmup=sc["warmup"],
                    what="the headline's tensors with EVERY level on two streams (--stack-coarse 0: the schedule of rounds 1-4; "
                         "the headline runs level 0 of both directions as one stacked call since round 5)")
            except Exception as exc:
                extra_lines["stack_coarse_0"] = {"error": repr(exc)[:200]}
            try:    # SURVEY 8(d)'s flow field: independent uniform [-6, 6) px per pixel (the headline uses the smooth field)
                fn = short_ops_rate(4, 1024, 512, torch.float32, device, flow_kind="noise",
                                    probe=("warp_fwd_L3", "warp_bwd_L3", "warp_bwd_L2", "warp_bwd_L1"))
                extra_lines["flow_noise"] = dict(
                    value=fn["value"], unit=fn["unit"], ms_per_step=fn["ms_per_step"], steps=fn["steps"], warmup=fn["warmup"],
                    warp_bwd_L3_us=fn["per_kernel_hot"]["warp_bwd_L3"]["us"], per_kernel_hot=fn["per_kernel_hot"],
                    workload="the headline's tensors with the flow fields of SURVEY 8(d): per-pixel uniform in [-6, 6) px "
                             "(a warp backward tile then gathers from a region 2.2 x its size)")
            except Exception as exc:
                extra_lines["flow_noise"] = {"error": repr(exc)[:200]}
            try:    # frames off the tuned widths (the reference trains on random-scale crops and KITTI: datasets/__init__.py:33-112)
                rag = {}
                for (rw, rh) in ((896, 448), (1216, 352)):
                    r = short_ops_rate(4, rw, rh, torch.float32, device, steps=40, warmup=8,
                                       probe=[k % l for l in (1, 2, 3) for k in ("corr_fwd_L%d", "corr_bwd_L%d", "warp_fwd_L%d", "warp_bwd_L%d")]
                                       + ["corr_fwd_L0", "corr_bwd_L0"])
                    rag["%dx%d" % (rw, rh)] = {k: r[k] for k in ("value", "unit", "ms_per_step", "levels_CHW", "per_kernel_hot",
                                                                  "step_algorithmic_GBps")}
                rag["what"] = ("the W32 pyramids of 896x448 and 1216x352 frames (level widths 28..224 / 38..304: none of the widths "
                               "16 / 32 / 64 / 128 / 256 the tuned kernels were built on), 4 image pairs, same launch as the headline; "
                               "per_kernel_hot: one launch replayed on the same tensors (HIP events), frac = algorithmic bytes / time / 8 TB/s")
                extra_lines["ragged"] = rag
            except Exception as exc:
                extra_lines["ragged"] = {"error": repr(exc)[:200]}
            try:    # f2: the fused warp + correlation forward against the two tuned launches
                extra_lines["f2_fused"] = f2_fused_times(args.pairs, args.width, args.height, device)
            except Exception as exc:
                extra_lines["f2_fused"] = {"error": repr(exc)[:200]}
            try:    # the loss side of the training step: pyramid, RGB warps, gradOutput from the concat buffer's gradient
                extra_lines["loss_side"] = loss_side_times(args.pairs, args.width, args.height, device)
            except Exception as exc:
                extra_lines["loss_side"] = {"error": repr(exc)[:300]}
            try:    # the host model's training step on this GPU: the N = 1 point of the DDP scaling curve
                margs = argparse.Namespace(**vars(args))
                margs.steps, margs.warmup = 10, 3
                margs.model_table = True
                m = model_step_mode(margs, device, 0, 1, None, quiet=True)
                extra_lines["model_step"] = {k: m[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup")}
                extra_lines["model_step"]["backend_table"] = m.get("backend_table")
                extra_lines["model_step"]["settings"] = {k: m["config"][k] for k in ("channels_last", "miopen_find", "backend")}
                extra_lines["model_step"]["workload"] = m["config"]["workload"]
                extra_lines["model_step"]["note"] = ("what `bench.py --gpus N` (N > 1) times per rank under "
                                                     "DistributedDataParallel; compare N > 1 lines with this figure")
            except Exception as exc:
                extra_lines["model_step"] = {"error": repr(exc)[:200]}
            result["extra"] = extra_lines
    if rank == 0:
        print(json.dumps(result), flush=True)

    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
