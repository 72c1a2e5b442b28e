"""Cases, float64 references and a route model of the resampling kernels (csrc/upsample.hip), shared by
tests/test_resample_cpu.py and tests/test_resample_gpu.py.  Nothing here needs a GPU.

The route model mirrors the index arithmetic of ``upsample_fwd_kernel`` / ``upsample_bwd_kernel`` in numpy ``float32``,
rounding where the kernel rounds (contraction off: ``r * dst`` is rounded once, the weight is derived from the rounded
coordinate), and says which of the backward kernel's data paths a launch takes.  test_resample_cpu.py holds the case table
to it: every route and every loop flag is reached by some case, so the GPU tests cannot silently test less than they
claim."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from cerberusnet_amd.synth import hash_uniform

F32 = np.float32

# Copied from csrc/upsample.hip (not parsed from it: a change there must be made here by hand, with the cases re-read):
K_MAX_CAND = 16       # kUpMaxCand, upsample.hip:85  -- candidate outputs per axis kept in registers
K_MAX_ROWS = 10       # kUpMaxRows, upsample.hip:83  -- matching output rows staged in LDS
K_MAX_W = 1024        # kUpMaxW,    upsample.hip:85  -- widest output row the LDS copy takes
K_THREADS = 256       # workgroup size, the stride of the x / ox / LDS-copy loops, upsample.hip:55, :124, :139, :178
K_MAX_BLOCKS = 65536  # launch(), upsample.hip:229   -- grid-stride beyond this many rows

ROUTES = frozenset(["staged_fast", "staged_serial", "direct_fast", "direct_serial", "staged_overflow"])


# ---- the kernel's index arithmetic ----------------------------------------------------------------------------------
def ratio(n_in, n_out):
    """upsample.hip:37"""
    return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0.0)


def tap_of(dst, r, n_in):
    """upsample.hip:30 for an int array ``dst``: (i0, i1, l0, l1), the weights float32."""
    dst = np.asarray(dst)
    src = F32(r) * dst.astype(F32)                              # one rounding
    i0 = np.minimum(src.astype(np.int64), n_in - 1)             # (int) truncates; src >= 0
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(F32)
    return i0, i1, F32(1.0) - l1, l1


def first_dst(i, r, n_out):
    """upsample.hip:67"""
    i = np.asarray(i)
    if r <= 0:
        return np.zeros(i.shape, np.int64)
    return np.maximum(0, np.floor((i - 1).astype(F32) / F32(r)).astype(np.int64) - 1)


def last_dst(i, r, n_out):
    """upsample.hip:71"""
    i = np.asarray(i)
    if r <= 0:
        return np.full(i.shape, n_out - 1, np.int64)
    return np.minimum(n_out - 1, np.ceil((i + 1).astype(F32) / F32(r)).astype(np.int64) + 1)


def weights_1d(n_in, factor):
    """One axis as a dense (n_in * factor, n_in) matrix: the float32 weights of ``tap_of`` exactly, held in float64 (a
    clamped tap, i0 == i1, carries l0 + l1), and the boolean pattern of its taps, zero-weight taps included."""
    n_out = n_in * factor
    dst = np.arange(n_out)
    i0, i1, l0, l1 = tap_of(dst, ratio(n_in, n_out), n_in)
    A = np.zeros((n_out, n_in))
    np.add.at(A, (dst, i0), l0.astype(np.float64))
    np.add.at(A, (dst, i1), l1.astype(np.float64))
    taps = np.zeros((n_out, n_in), bool)
    taps[dst, i0] = True
    taps[dst, i1] = True
    return A, taps


def weight_matrix(H, W, factor):
    """The (oH * oW) x (H * W) matrix of one plane's forward WITHOUT the factor, and its tap pattern."""
    (Ay, ty), (Ax, tx) = weights_1d(H, factor), weights_1d(W, factor)
    return np.kron(Ay, Ax), np.kron(ty, tx)


def support(H, W, factor):
    """``f(oy, ox)`` -> the set of input elements (y, x) with a tap on output element (oy, ox), zero-weight taps
    included: what a non-finite gradient at (oy, ox) may reach in the backward, and nothing else."""
    ry, rx = ratio(H, H * factor), ratio(W, W * factor)

    def of(oy, ox):
        y0, y1, _, _ = tap_of(np.array([oy]), ry, H)
        x0, x1, _, _ = tap_of(np.array([ox]), rx, W)
        return {(int(y), int(x)) for y in (y0[0], y1[0]) for x in (x0[0], x1[0])}
    return of


def _axis(n_in, factor):
    """Per input index of one axis: the window [lo, hi] the backward scans, and the outputs whose taps touch it."""
    n_out = n_in * factor
    r = ratio(n_in, n_out)
    idx = np.arange(n_in)
    lo, hi = first_dst(idx, r, n_out), last_dst(idx, r, n_out)
    _, taps = weights_1d(n_in, factor)
    return lo, hi, taps


def windows_cover_taps(n_in, factor):
    """True when, for every input index of an axis, each output with a tap on it lies inside [first_dst, last_dst]: the
    'conservative by one' bounds of the backward really are conservative."""
    lo, hi, taps = _axis(n_in, factor)
    dst = np.arange(n_in * factor)[:, None]
    return bool(np.all(~taps | ((dst >= lo[None, :]) & (dst <= hi[None, :]))))


BwdRoutes = collections.namedtuple("BwdRoutes", "routes x_second_trip copy_multi_trip grid_stride")
FwdFlags = collections.namedtuple("FwdFlags", "ox_second_trip grid_stride")


def bwd_routes(H, W, factor, aligned, planes=1):
    """The data paths one ``upsample_bwd_kernel`` launch takes over all its input rows and columns (upsample.hip:109-220).
    ``aligned``: the gradient's address is a multiple of four elements (16 bytes in fp32, 8 in the 16-bit types)."""
    oH, oW = H * factor, W * factor
    stage_ok = oW >= 3 * W and oW % 4 == 0 and oW <= K_MAX_W and bool(aligned)
    x_lo, x_hi, _ = _axis(W, factor)
    col = {"fast" if f else "serial" for f in (x_hi - x_lo < K_MAX_CAND)}
    y_lo, y_hi, ytaps = _axis(H, factor)
    routes, multi = set(), False
    for y in range(H):
        nrow = int(ytaps[y_lo[y]:y_hi[y] + 1, y].sum())          # the kernel stops counting at kUpMaxRows + 1
        if stage_ok and nrow <= K_MAX_ROWS:
            routes |= {"staged_" + c for c in col}
            multi = multi or nrow * (oW // 4) > K_THREADS
        else:
            if stage_ok:
                routes.add("staged_overflow")
            routes |= {"direct_" + c for c in col}
    return BwdRoutes(frozenset(routes), W > K_THREADS, multi, planes * H > K_MAX_BLOCKS)


def fwd_flags(H, W, factor, planes=1):
    """upsample.hip:49, :55"""
    return FwdFlags(W * factor > K_THREADS, planes * H * factor > K_MAX_BLOCKS)


# ---- the case table: (B, C, H, W, factor) ---------------------------------------------------------------------------
CASES = [
    (2, 2, 9, 256, 4),       # 1: staged, oW == kUpMaxW exactly (the x4 upsample of the model's finest flow), multi-trip copy
    (1, 2, 5, 257, 4),       # 2: oW > kUpMaxW: direct at factor 4, x makes a second trip
    (1, 2, 6, 340, 3),       # 3: staged with W > 256 at a factor that is no power of two
    (1, 2, 7, 33, 3),        # oW % 4 != 0: direct
    (1, 2, 12, 20, 6),       # staged-eligible, but interior rows match 12-13 > kUpMaxRows output rows: the overflow fallback
                             # (direct, serial candidates); the first and the last row match 7: staged, serial candidates
    (1, 2, 10, 24, 8),       # the same at factor 8 (17-18 rows inside, 9 at the ends), with a multi-trip copy
    (1, 2, 10, 25, 7),       # oW % 4 != 0 at factor 7: direct with serial candidates in every row
    (1, 2, 1, 40, 8),        # H = 1, ry = 0: eight matching rows of weight one, staged with serial candidates
    (1, 2, 5, 300, 2),       # factor 2 (oW < 3 W: direct), x second trip
    (1, 2, 6, 10, 1),        # factor 1
] + [(1, 2, 1, 1, f) for f in (1, 3, 4, 8)] \
  + [(2, 3, 1, 9, f) for f in (1, 3, 4, 8)] \
  + [(1, 2, 9, 1, f) for f in (1, 3, 4, 8)] + [   # degenerate axes: ratio 0
    (3, 2, 17, 5, 5),        # factor 5
    (8, 2, 4099, 2, 2),      # grid stride both ways, direct
    (8, 2, 4099, 2, 4),      # grid stride both ways, staged: 48 workgroups walk a second row
]
MISALIGNED_CASES = [CASES[0], CASES[2], (1, 2, 5, 300, 2)]    # staged -> direct (x 2), and one that is direct either way
MATRIX_CASES = [(1, 2, 7, 33, 3), (3, 2, 17, 5, 5), (1, 2, 1, 40, 8), (1, 2, 9, 1, 4)]   # small enough for a dense matrix


def case_id(case):
    return "%dx%dx%dx%d_x%d" % case


def out_shape(case):
    B, C, H, W, k = case
    return (B, C, H * k, W * k)


def inputs(case):
    """(x in [-8, 8), grad_out in [-1, 1)) as numpy float32"""
    return hash_uniform(case[:4], 1810, -8.0, 8.0), hash_uniform(out_shape(case), 1820)


def stock(x, factor):
    """The op sequence flow_upsample replaces (pwcnet_sfd.py:176, :199-201), on x's device in x's dtype."""
    return F.interpolate(x * factor, scale_factor=factor, mode="bilinear", align_corners=True)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(x, grad_out, out64, grad_in64): the float64 CPU forward and its autograd gradient.  Shared, never written to."""
    x, go = inputs(case)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    out = stock(x64, case[4])
    gin, = torch.autograd.grad(out, x64, torch.from_numpy(go).double())
    arrays = (x, go, out.detach().numpy(), gin.numpy())
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- area ------------------------------------------------------------------------------------------------------------
# (source shape, [fractional down-size, integer down-size, up-size]); every window has fewer than 100 elements
AREA_CASES = [((2, 3, 37, 53), [(16, 24), (37, 1), (50, 70)]),
              ((1, 2, 74, 106), [(30, 40), (37, 53), (100, 130)]),
              ((1, 1, 5, 260), [(3, 100), (1, 130), (8, 300)])]


def area_input(shape):
    return hash_uniform(shape, 1830, -2.0, 2.0)


def area_reference(x, size):
    """F.interpolate(mode='area') in float64 on the CPU"""
    return F.interpolate(torch.as_tensor(x).double(), size, mode="area")


def area_mirror(x, size):
    """area_resize_kernel's arithmetic (upsample.hip:246-262) in numpy: ATen's window bounds, a float32 sum in row-major
    order, then / kh / kw."""
    x = np.asarray(x, F32)
    B, C, H, W = x.shape
    oH, oW = size
    out = np.empty((B, C, oH, oW), F32)
    for oy in range(oH):
        y0, y1 = oy * H // oH, ((oy + 1) * H + oH - 1) // oH
        for ox in range(oW):
            x0, x1 = ox * W // oW, ((ox + 1) * W + oW - 1) // oW
            s = np.zeros((B, C), F32)
            for y in range(y0, y1):
                for xx in range(x0, x1):
                    s = s + x[:, :, y, xx]
            out[:, :, oy, ox] = s / F32(y1 - y0) / F32(x1 - x0)
    return out
