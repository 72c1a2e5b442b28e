"""Misaligned pointers for the hot-path kernels (tests/test_alignment_gpu.py, tests/test_op_contract_gpu.py).

``embed(t, shift)`` puts ``t``'s values ``shift`` elements off a 16-byte boundary inside a larger buffer whose bands (the
elements in front of and behind the view) hold NaN for a tensor the kernels read and ``SENTINEL`` for one they write:
a read outside the tensor that reaches the arithmetic shows as a non-finite result, a store outside it as a changed band.

The tables name, per kernel route, the shape and options that take it, the kernel ``cerberus_last_kernel`` must report for the
16-byte-aligned call (so that a case is known to stand at the gate it is about), and ``gates``: the alignment in bytes each
pointer must have for that route, read off the dispatch code (the audit table of DESIGN.md 3.23).  A shift that is no
multiple of a shifted pointer's gate must take another kernel; any other shift must take the same one and give the same bits.
``renames`` is False for the register-staged kernels, which report one name for their vector and their scalar form.

Shapes are the smallest the existing route tests use for the same kernels; nothing exceeds 64 x 256 pixels."""
import torch

SENTINEL = 7.5
GUARD = 64
INT_FILL = -777                     # the bands of an integer tensor (no NaN there): no valid label, id or count

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# bound of the ops' own tests against the oracle on the (rounded) inputs: tests/test_corr_gpu.py, tests/test_warp_gpu.py
BOUND = {F32: 1e-5, F16: 2e-3, BF16: 1.6e-2}
# shifts in elements: every misalignment an element-aligned pointer can have relative to 16 bytes, and one whole 16 bytes
SHIFTS = {F32: (1, 2, 4), F16: (1, 2, 4, 8), BF16: (1, 2, 4, 8)}


def embed(t, shift, guard=GUARD, written=False):
    """A contiguous view holding ``t``'s values that starts ``guard + shift`` elements into a fresh 1-D buffer and has ``guard``
    elements behind it.  ``written``: the buffer (the view included) is filled with ``SENTINEL`` -- the call must overwrite
    the view and nothing else; otherwise the bands hold NaN (``INT_FILL`` for an integer tensor)."""
    assert t.is_contiguous() and guard * t.element_size() % 16 == 0
    if written:
        fill = SENTINEL
    else:
        fill = float("nan") if t.is_floating_point() else INT_FILL
    buf = torch.full((guard + shift + t.numel() + guard,), fill, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[guard + shift:guard + shift + t.numel()].view(t.shape)
    if not written:
        view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == shift * t.element_size() % 16
    return view


def bands(view):
    """The elements in front of and behind an ``embed`` view, as one tensor."""
    buf = view._base
    assert buf is not None and buf.dim() == 1
    lo = view.storage_offset()
    return torch.cat([buf[:lo], buf[lo + view.numel():]])


def bands_untouched(view):
    b = bands(view)
    return b.numel() >= 2 * GUARD and bool((b == SENTINEL).all())


def misaligned(nbytes, gate):
    """A pointer ``nbytes`` off a 16-byte boundary fails a gate that asks for ``gate`` bytes."""
    return nbytes % gate != 0


# (aligned call's kernel, misaligned call's kernel) pairs the suite already pins as bit-identical: the LDS-DMA kernels and
# the register-staged ones of the same tile (tests/test_corr_gpu.py:
# test_dma_kernels_are_bit_identical_to_the_register_staged_ones,
# test_channel_group_dma_forward_is_bit_identical_to_the_staged_variant)
PINNED = {
    ("corr_fwd_d4_dma_4x64", "corr_fwd_d4_4x64_cc4"),
    ("corr_fwd_d4_dma_2x64_s2", "corr_fwd_d4_2x64_s2"),
    ("corr_fwd_d4_dma_1x64_s4", "corr_fwd_d4_1x64_s4"),
    ("corr_fwd_d4_dma_1x32_s8", "corr_fwd_d4_1x32_s8"),
    ("corr_fwd_d4_dma_1x16_s16", "corr_fwd_d4_1x16_s16"),
    ("corr_bwd_d4_dma_8x64", "corr_bwd_d4_8x64"),
    ("corr_bwd_d4_dma_16x32", "corr_bwd_d4_16x32"),
    # test_mfma_forward_column_walk_equals_the_register_staged_form_bit_for_bit
    ("corr_fwd_d4_mfma_walk_4x32", "corr_fwd_d4_mfma_4x64"),
    ("corr_fwd_d4_mfma_walk_4x32_c64", "corr_fwd_d4_mfma_4x32"),
    ("corr_fwd_d4_mfma_tr_4x64", "corr_fwd_d4_mfma_4x64"),
}


def case(name, dtypes, shape, options, kernel, gates, renames=True, pinned=(), pinned_bytes=()):
    """``pinned``: pointers whose failed gate must lead to the aligned kernel's ``PINNED`` partner (at a shift of
    ``pinned_bytes``; empty: at any) -- the bit comparison then runs for certain, where a fallback to some other tile would
    reduce the check to the bound without a word."""
    return dict(name=name, dtypes=dtypes, shape=shape, options=options, kernel=kernel, gates=gates, renames=renames,
                pinned=pinned, pinned_bytes=pinned_bytes)


def per_dtype(cases):
    return [(c, dt) for c in cases for dt in c["dtypes"]]


def ids(pairs):
    return ["%s-%s" % (c["name"], str(dt).split(".")[1]) for c, dt in pairs]


HALF = (F16, BF16)
V16 = {"in1": 16, "in2": 16, "out": 16}              # fp32: `vec` / `half` of corr_d4_forward
V8 = {"in1": 8, "in2": 8, "out": 8}                  # 16-bit storage: the same flags
WALK = {"in1": 16, "in2": 16, "out": 8}              # + the 16-byte cells of the column walk and its `tr` form (fwd_pick)
TO_STAGED = dict(pinned=("in1", "in2"), pinned_bytes=(8,))    # an input at 8 mod 16: the register-staged matrix-core form

CORR_FORWARD = [
    # (the cost estimate and the fallback's "smallest split with >= 256 workgroups" chain both end at the 1 x 16 tile here;
    #  a forced LDS-DMA variant falls back through the same chain, not to its own tile)
    case("dma_tile", (F32,), (2, 32, 13, 72), {}, "corr_fwd_d4_dma_1x16_s16", V16, pinned=("in1", "in2", "out")),
    case("coarse_16", (F32,), (2, 128, 8, 16), {"corr_fwd_variant": 15}, "corr_fwd_d4_coarse_16", V16),
    case("coarse_32", (F32,), (2, 128, 7, 32), {"corr_fwd_variant": 15}, "corr_fwd_d4_coarse_32", V16),
    case("coarse_64", (F32,), (1, 64, 5, 64), {"corr_fwd_variant": 15}, "corr_fwd_d4_coarse_64", V16),
    case("coarse_half", (F32,), (1, 128, 5, 34), {"corr_fwd_variant": 15}, "corr_fwd_d4_coarse_half64", V16),
    case("register_staged", (F32,), (2, 32, 13, 72), {"corr_fwd_variant": 7}, "corr_fwd_d4_4x64_cc4", V16, renames=False),
    case("mfma_walk", HALF, (1, 20, 13, 72), {}, "corr_fwd_d4_mfma_walk_4x32", WALK, **TO_STAGED),
    case("mfma_walk_c64", HALF, (2, 64, 9, 72), {}, "corr_fwd_d4_mfma_walk_4x32_c64", WALK, **TO_STAGED),
    case("mfma_tr", HALF, (1, 20, 13, 72), {"corr_fwd_variant": 26}, "corr_fwd_d4_mfma_tr_4x64", WALK, **TO_STAGED),
    case("mfma_4x64", HALF, (2, 32, 9, 68), {}, "corr_fwd_d4_mfma_4x64", V8),          # W % 8 == 4: no walk
    case("mfma_4x16", HALF, (2, 128, 9, 36), {}, "corr_fwd_d4_mfma_4x16", V8),
    case("valu_c16", HALF, (1, 16, 9, 64), {"corr_fwd_variant": 7}, "corr_fwd_d4_4x64_cc4", V8),
]

B16 = {"in1": 16, "in2": 16, "gout": 16, "gin1": 16, "gin2": 16}
B8 = {"in1": 8, "in2": 8, "gout": 8, "gin1": 8, "gin2": 8}
CORR_BACKWARD = [
    case("strip_128", (F32,), (1, 32, 12, 128), {"corr_bwd_variant": 12}, "corr_bwd_d4_strip_w128", B16),
    case("strip_64", (F32,), (2, 32, 8, 64), {"corr_bwd_variant": 12}, "corr_bwd_d4_strip_w64", B16),
    case("coarse_32", (F32,), (2, 128, 7, 32), {"corr_bwd_variant": 14}, "corr_bwd_d4_coarse_32", B16),
    case("rows_cb8", (F32,), (2, 32, 13, 72), {"corr_bwd_variant": 8}, "corr_bwd_d4_rows_4x64_cb8", B16),
    case("dma_8x64", (F32,), (2, 32, 13, 72), {"corr_bwd_variant": 4}, "corr_bwd_d4_dma_8x64", B16),
    case("dma_16x32", (F32,), (2, 24, 21, 32), {"corr_bwd_variant": 5}, "corr_bwd_d4_dma_16x32", B16,
         pinned=("in1", "in2", "gout", "gin1", "gin2")),
    case("g3_8x64", (F32,), (2, 32, 13, 72), {"corr_bwd_variant": 3}, "corr_bwd_d4_g3_8x64", B16, renames=False),
    case("mfma_seg", HALF, (2, 32, 9, 68), {}, "corr_bwd_d4_mfma_seg_4x64", B8),
    case("mfma_row", HALF, (2, 32, 9, 68), {"corr_bwd_variant": 11}, "corr_bwd_d4_mfma_4x64", B8),
]

# flow_warp has no kernel report: `gates` is what the dispatch of warp.hip tests for the route the options force.  A shift
# that fails one of them changes the route (bound only); any other shift leaves it and must give the same bits.
# `flow`: the flow's dtype beside a 16-bit image (None: the image's)
def warp_case(name, dtypes, shape, options, gates, flow=None, deterministic=True):
    return dict(name=name, dtypes=dtypes, shape=shape, options=options, gates=gates, flow=flow, deterministic=deterministic)


WARP_FORWARD = [
    warp_case("fewc", (F32,), (2, 3, 9, 72), {}, {}),                                          # C <= 4: a lane per pixel
    warp_case("staged", (F32,), (2, 19, 13, 72), {}, {"image": 16}),
    warp_case("direct", (F32,), (2, 19, 13, 72), {"warp_staged": 2}, {}),
    # (warp16_forward asks 8 bytes of the flow whatever its type: a 16-bit flow, read as dwords, would do with 4 -- a 4-byte
    #  shift costs it the route, not the result)
    warp_case("warp16", HALF, (2, 16, 13, 72), {"warp_staged": 8}, {"image": 16, "flow": 8, "out": 8}),
    warp_case("warp16_f32flow", HALF, (2, 16, 13, 72), {"warp_staged": 8}, {"image": 16, "flow": 8, "out": 8}, flow=F32),
]

WARP_BACKWARD = [
    warp_case("tile_wide", (F32,), (2, 12, 13, 72), {}, {"gimage": 16}),                       # + the plain flow role
    warp_case("tile_pair16", HALF, (2, 12, 13, 72), {}, {"gout": 4, "gimage": 16}),
    warp_case("flow_staged", (F32,), (2, 12, 13, 72), {"warp_staged": 8}, {"image": 16, "gimage": 16}),
    warp_case("flow16", HALF, (2, 12, 13, 72), {"warp_staged": 8}, {"image": 16, "gout": 4, "gflow": 8, "gimage": 16}),
    warp_case("flow16_f32flow", HALF, (2, 12, 13, 72), {"warp_staged": 8}, {"image": 16, "gout": 4, "gflow": 8, "gimage": 16},
              flow=F32),
    # ATen's method: global float atomics for grad_image, whose order is not fixed -- held to the bound alone
    warp_case("scatter", (F32,), (2, 12, 13, 72), {"warp_force_scatter": 1}, {}, deterministic=False),
]
