"""CPU tests of tests/resample_cases.py: the case table reaches every route of ``upsample_bwd_kernel`` and every loop
flag of both kernels (so that tests/test_resample_gpu.py tests what it claims), and the numpy mirror of the kernels' tap
arithmetic reproduces the float64 reference within the error of an fp32 source coordinate."""
import numpy as np
import pytest
import torch

import resample_cases as rc
from resample_cases import CASES, MATRIX_CASES, MISALIGNED_CASES, ROUTES, case_id


def _planes(case):
    return case[0] * case[1]


def _bwd(case, aligned):
    B, C, H, W, k = case
    return rc.bwd_routes(H, W, k, aligned, planes=B * C)


def _is_staged(r):
    return bool(r.routes & {"staged_fast", "staged_serial"})


# ---- route coverage --------------------------------------------------------------------------------------------------
def test_the_case_table_reaches_every_backward_route():
    reached = {}
    for case in CASES:
        for route in _bwd(case, True).routes:
            reached.setdefault(route, []).append(case_id(case))
    missing = sorted(ROUTES - set(reached))
    assert not missing, "no case of resample_cases.CASES reaches the route(s) %s" % ", ".join(missing)
    assert set(reached) == ROUTES, sorted(set(reached) - ROUTES)
    # what each case is in the table for: (routes it must reach, routes it may reach)
    direct, staged = {"direct_fast", "direct_serial"}, {"staged_fast", "staged_serial"}
    expect = {(2, 2, 9, 256, 4): ({"staged_fast"}, {"staged_fast"}), (1, 2, 5, 257, 4): ({"direct_fast"}, {"direct_fast"}),
              (1, 2, 6, 340, 3): ({"staged_fast"}, {"staged_fast"}), (1, 2, 7, 33, 3): ({"direct_fast"}, {"direct_fast"}),
              (1, 2, 12, 20, 6): ({"staged_overflow", "staged_serial", "direct_serial"}, ROUTES),
              (1, 2, 10, 24, 8): ({"staged_overflow", "direct_serial"}, ROUTES),
              (1, 2, 10, 25, 7): ({"direct_serial"}, direct), (1, 2, 1, 40, 8): ({"staged_serial"}, staged),
              (1, 2, 5, 300, 2): ({"direct_fast"}, {"direct_fast"}), (8, 2, 4099, 2, 2): ({"direct_fast"}, {"direct_fast"}),
              (8, 2, 4099, 2, 4): ({"staged_fast"}, {"staged_fast"})}
    for case, (must, may) in expect.items():
        got = _bwd(case, True).routes
        assert case in CASES, "case %s, in the table for the route(s) %s, is gone" % (case, ", ".join(sorted(must)))
        assert must <= got <= may, "case %s reaches %s, not %s" % (case, sorted(got), sorted(must))


def test_every_loop_flag_is_raised_on_the_staged_and_on_the_direct_route():
    """x_second_trip and grid_stride exist on both routes (the second row of a workgroup is where the staged route reuses
    its LDS); copy_multi_trip and the oW == kUpMaxW boundary exist on the staged route only."""
    aligned = [_bwd(c, True) for c in CASES]
    for flag in ("x_second_trip", "grid_stride"):
        assert any(getattr(r, flag) and _is_staged(r) for r in aligned), "no staged case raises %s" % flag
        assert any(getattr(r, flag) and not _is_staged(r) for r in aligned), "no direct case raises %s" % flag
    assert any(r.copy_multi_trip for r in aligned), "no case makes a second trip of the LDS copy"
    assert any(not r.copy_multi_trip and _is_staged(r) for r in aligned), "no staged case with a single-trip copy"
    assert any(c[3] * c[4] == rc.K_MAX_W and _is_staged(_bwd(c, True)) for c in CASES), "no case at oW == kUpMaxW"
    assert any(c[3] * c[4] > rc.K_MAX_W and c[4] >= 3 for c in CASES), "no case beyond kUpMaxW at a factor >= 3"
    # a gradient that is not aligned takes the direct code whatever the shape
    for case in CASES:
        r = _bwd(case, False)
        assert r.routes <= {"direct_fast", "direct_serial"}, (case, sorted(r.routes))
    # the misaligned GPU test changes the route of two of its cases and leaves the third alone
    changed = [_is_staged(_bwd(c, True)) for c in MISALIGNED_CASES]
    assert changed.count(True) >= 2 and changed.count(False) >= 1, changed
    assert any(_bwd(c, False).x_second_trip for c in MISALIGNED_CASES)


def test_every_forward_flag_is_raised():
    flags = [rc.fwd_flags(c[2], c[3], c[4], planes=_planes(c)) for c in CASES]
    for name in rc.FwdFlags._fields:
        assert any(getattr(f, name) for f in flags), "no case raises the forward's %s" % name
        assert any(not getattr(f, name) for f in flags), "every case raises the forward's %s" % name


def test_the_factors_and_degenerate_axes_of_the_table():
    assert {c[4] for c in CASES} >= {1, 2, 3, 4, 5, 6, 8}
    for f in (1, 3, 4, 8):
        assert {(1, 1), (1, 9), (9, 1)} <= {(c[2], c[3]) for c in CASES if c[4] == f}, f
    for case in CASES:          # the largest tensor of a case (its float64 reference output) stays small
        assert np.prod(rc.out_shape(case)) * 8 <= 17 << 20, case


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_backward_windows_contain_every_tap(case):
    """first_dst / last_dst are 'conservative by one': an output with a tap on an input index outside that index's window
    would be a term the gather never adds."""
    _, _, H, W, k = case
    assert rc.windows_cover_taps(H, k) and rc.windows_cover_taps(W, k)


# ---- the mirror against float64 --------------------------------------------------------------------------------------
U = 2.0 ** -24                  # unit roundoff of float32


def _coordinate_error(n_in):
    """|fl(fl(r) * dst) - r * dst| for the exact ratio r = (in - 1) / (out - 1): two roundings, each at most U relative, of a
    coordinate that is at most in - 1 (at most one ulp of the largest source coordinate)."""
    return (2 * U + U * U) * (n_in - 1)


@pytest.mark.parametrize("case", MATRIX_CASES, ids=case_id)
def test_mirrored_taps_reproduce_the_float64_reference(case):
    B, C, H, W, k = case
    x, go, ref_out, ref_gin = rc.reference(case)
    M, taps = rc.weight_matrix(H, W, k)
    out = (M @ x.reshape(B * C, H * W).astype(np.float64).T).T.reshape(ref_out.shape) * k
    gin = (M.T @ go.reshape(B * C, -1).astype(np.float64).T).T.reshape(ref_gin.shape) * k
    # Per axis the weights are a continuous (Lipschitz 1) function of the source coordinate -- also where a coordinate that
    # lands a last bit below an integer moves the tap index -- so a coordinate error d moves a weight by at most d; l0 =
    # fl(1 - l1) adds U / 2.  Forward: interpolation is Lipschitz in the coordinate with the input's range as constant, per
    # axis; the two l0 roundings scale the largest input.  The (1 + 2^-10) covers the second-order terms.
    dx, dy = _coordinate_error(W), _coordinate_error(H)
    slack = 1 + 2.0 ** -10
    x_range, x_max = float(x.max()) - float(x.min()), float(np.abs(x).max())
    bound_fwd = k * ((dx + dy) * x_range + U * x_max) * slack
    # Backward: an input element sums at most ny * nx outputs (those within one source pixel of it on each axis, all of them
    # on an axis of one input element), each product of two weights off by at most dx + dy + U.
    n_axis = lambda n_in: n_in * k if n_in == 1 else int(np.floor(2 * (n_in * k - 1) / (n_in - 1))) + 2
    bound_bwd = k * n_axis(H) * n_axis(W) * (dx + dy + U) * float(np.abs(go).max()) * slack
    err_fwd, err_bwd = float(np.abs(out - ref_out).max()), float(np.abs(gin - ref_gin).max())
    print("%s: forward %.3e (bound %.3e), backward %.3e (bound %.3e)" % (case_id(case), err_fwd, bound_fwd, err_bwd, bound_bwd))
    assert err_fwd <= bound_fwd
    assert err_bwd <= bound_bwd
    assert taps.sum(1).max() <= 4 and taps.sum(0).max() <= n_axis(H) * n_axis(W)
    # rows of weights sum to one (to the two l0 roundings): the op reproduces a constant field
    assert np.abs(M.sum(1) - 1).max() <= 2 * U


@pytest.mark.parametrize("case", MATRIX_CASES, ids=case_id)
def test_support_is_the_tap_pattern_of_the_matrix(case):
    _, _, H, W, k = case
    M, taps = rc.weight_matrix(H, W, k)
    assert not (M != 0)[~taps].any()                    # a weight only where there is a tap
    of = rc.support(H, W, k)
    oW = W * k
    for o in range(M.shape[0]):
        want = {(int(i) // W, int(i) % W) for i in np.flatnonzero(taps[o])}
        assert of(o // oW, o % oW) == want, (o // oW, o % oW)


# ---- area ------------------------------------------------------------------------------------------------------------
def _largest_window(n_in, n_out):
    return max(((o + 1) * n_in + n_out - 1) // n_out - o * n_in // n_out for o in range(n_out))


@pytest.mark.parametrize("shape,sizes", rc.AREA_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_area_targets_are_what_the_gpu_test_says_and_torch_sums_them_serially(shape, sizes):
    """A fractional down-size, an integer down-size and an up-size per source, no window of a hundred elements or more; and
    on these torch's fp32 CPU kernel IS the kernel's arithmetic (serial fp32 sum, / kh / kw), which is what lets the GPU test
    ask for equal bits."""
    _, _, H, W = shape
    frac, integer, up = sizes
    assert frac[0] < H and frac[1] < W and (H % frac[0] or W % frac[1])
    assert H % integer[0] == 0 and W % integer[1] == 0 and integer != (H, W) and integer != (1, 1)
    assert up[0] > H and up[1] > W
    x = rc.area_input(shape)
    for oh, ow in sizes:
        n = _largest_window(H, oh) * _largest_window(W, ow)
        assert n < 100, (oh, ow, n)
        ref32 = torch.nn.functional.interpolate(torch.from_numpy(x), (oh, ow), mode="area").numpy()
        assert np.array_equal(rc.area_mirror(x, (oh, ow)), ref32), (oh, ow)
        # and float64 agrees to the rounding of a sum of n terms of magnitude <= 2: n * U * 2 each way, plus two divisions
        assert np.abs(ref32 - rc.area_reference(x, (oh, ow)).numpy()).max() <= (n + 2) * U * 2.0
