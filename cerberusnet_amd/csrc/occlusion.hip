// occlusion.hip -- unFlowLoss's occlusion masks as two forward-only ops, fp32.
//
// Reference (nnet_training/loss_functions/UnFlowLoss.py):
//   get_corresponding_map(data)           :34-81    bilinear forward splat of ones: ~40 small launches and a float
//                                                   scatter_add_ (atomics: not reproducible run to run)
//   get_occu_mask_backward(flow21, theta) :108-117  mesh + flow -> that map -> clamp(0, 1) < theta
//   get_occu_mask_bidirection(f12, f21)   :96-106   flow_warp(f21, f12, pad='zeros') + ~10 elementwise launches
// Masks are constants of the loss: neither op has a backward.
//
// ---- corresponding_map ----------------------------------------------------------------------------------------------
// Every source pixel adds to the four taps floor / floor + 1 of its target position (x, y) the weight
// (1 - |x - xt|) (1 - |y - yt|), formed in fp32 in the reference's order.  A tap is judged on the unclamped integer:
// it counts iff 0 <= xt < W and 0 <= yt < H (:53-60, :75).  With `is_flow` the position is pixel + flow, formed here in
// fp32 (one rounding, as `mesh.type_as(flow) + flow` in the reference); otherwise `data` holds absolute coordinates.
//
// Accumulator format.  A weight lies in [0, 1]; it is added as the 64-bit unsigned integer rint(w * 2^33): a STATIC
// scale, no block maximum.  w * 2^33 is an exact fp32 product (a power of two) and an integer for every w >= 2^-10, so
// the rounding moves a tap by at most 2^-34 and ordinary weights not at all.  Integer adds commute: the sum has the same
// bits whatever order the workgroups and their atomics arrive in, eager or replayed from a graph.
// Range: one source adds at most 2^33 to a cell, a map has H * W < 2^30 sources (api.hip rejects 2 H W >= 2^31), so a
// cell that receives EVERY source holds less than 2^30 * 2^33 = 2^63 < 2^64: no wrap.  H, W <= 2^24 (rejected above
// that), so floor(x) + 1 is exact in fp32 wherever a tap can count.
//
// Launches: a zero-fill kernel over the (B, H, W) u64 workspace (a kernel, not hipMemsetAsync: captured in a graph, the
// memset left stale sums in the workspace from the second replay on -- tests/test_occlusion_gpu.py caught it), the
// splat, a conversion pass u64 -> double * 2^-33 -> float.
// Splat: a workgroup owns a 16 x 64 tile of SOURCE pixels and a 33 x 81 window of u64 cells in LDS, placed where the
// tile's first pixel lands (window origin = that target - 8).  Under a smooth flow nearly every tap of the tile falls into
// the window and is a ds_add_u64; the window's non-zero cells then go to the workspace with one global 64-bit integer
// atomic each, row by row (~1.1 per source pixel instead of 4).  A tap outside the window (noisy or diverging flow) goes
// to the workspace directly: the same integer, so the result does not depend on which way a tap took.
//
// Non-finite positions.  In the reference +-Inf adds nothing (all four taps are invalid) and NaN is undefined (.long() of
// NaN as a scatter index).  Here both add nothing: the range test `floor(x) >= -1 && floor(x) <= W - 1` is false for NaN
// and +-Inf, and is made in fp32 BEFORE any conversion to an integer, so a position of any magnitude is dropped without
// index arithmetic; every other pixel's value is unaffected.  Nothing is read or written outside the map.
//
// ---- occlusion_mask_bidirection -------------------------------------------------------------------------------------
// One launch, one thread per pixel: the two planes of flow21 are sampled where flow_warp(., flow12, pad='zeros') samples
// them -- source_coord, Bilinear (weights, flags, summation order, clamped offsets) and tap_ptr of warp_common.h, so the
// sampled values w are the bits flow_warp returns, quirk Q2 (normalised by W - 1, sampled with align_corners=False)
// included -- then, each step rounded on its own as the reference's separate launches do (contraction is off),
//     |f12 + w|^2 > scale (|f12|^2 + |w|^2) + bias   ->  1.0, else 0.0.
// An IEEE comparison: a NaN anywhere in a pixel's terms gives 0 there.  The warped flow is never written.
#include "warp_common.h"

#pragma clang fp contract(off)

namespace cerb {
namespace {

using u64 = unsigned long long;

constexpr int kTW = 64;        // source tile: one column per lane ...
constexpr int kTH = 16;        // ... and 4 consecutive rows per thread, 4 waves
constexpr int kRows = 4;
constexpr int kThreads = 256;
constexpr int kPad = 8;                      // the window reaches 8 cells beyond the shifted tile on every side
constexpr int kWinW = kTW + 2 * kPad + 1;    // + 1: the floor + 1 taps
constexpr int kWinH = kTH + 2 * kPad + 1;
constexpr int kWinCells = kWinW * kWinH;     // 2673 u64 = 21384 B
constexpr float kFixScale = 8589934592.f;    // 2^33
constexpr double kFixInv = 1.0 / 8589934592.0;

inline int tiles(int n, int t) { return (n + t - 1) / t; }

__global__ __launch_bounds__(kThreads) void splat_kernel(const float *__restrict__ data, u64 *__restrict__ acc, int H, int W,
                                                         int tiles_x, int tiles_y, int is_flow) {
    __shared__ u64 win[kWinCells];
    __shared__ int origin[2];
    const int blk = blockIdx.x;
    const int tx = blk % tiles_x, ty = (blk / tiles_x) % tiles_y;
    const int64_t b = blk / (tiles_x * tiles_y);
    const int x0 = tx * kTW, y0 = ty * kTH;
    const int64_t plane = static_cast<int64_t>(H) * W;
    const float *px = data + b * 2 * plane, *py = px + plane;
    u64 *out = acc + b * plane;

    for (int i = threadIdx.x; i < kWinCells; i += kThreads) win[i] = 0;
    if (threadIdx.x == 0) {
        // the window follows the tile's first pixel (always inside the map).  tap_index saturates at +-2^24 and maps
        // NaN to 0: any origin is a valid one, a poor one only sends more taps the direct way
        const int64_t o = static_cast<int64_t>(y0) * W + x0;
        const float ax = is_flow ? static_cast<float>(x0) + px[o] : px[o];
        const float ay = is_flow ? static_cast<float>(y0) + py[o] : py[o];
        origin[0] = tap_index(floorf(ax)) - kPad;
        origin[1] = tap_index(floorf(ay)) - kPad;
    }
    __syncthreads();
    const int wx0 = origin[0], wy0 = origin[1];

    // one tap (xt, yt), known to be inside the map
    auto add = [&](int xt, int yt, float w) {
        const u64 q = static_cast<u64>(rintf(w * kFixScale));     // w in [0, 1]: at most 2^33
        if (q == 0) return;
        const int c = xt - wx0, r = yt - wy0;              // |wx0| <= 2^24 + 8, 0 <= xt < W: no overflow
        if (static_cast<unsigned>(c) < static_cast<unsigned>(kWinW) && static_cast<unsigned>(r) < static_cast<unsigned>(kWinH))
            atomicAdd(&win[r * kWinW + c], q);
        else
            atomicAdd(out + static_cast<int64_t>(yt) * W + xt, q);
    };

    const int lx = threadIdx.x & 63, ly = (threadIdx.x >> 6) * kRows;
    const int gx = x0 + lx;
    if (gx < W) {
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const int gy = y0 + ly + k;
            if (gy >= H) break;
            const int64_t o = static_cast<int64_t>(gy) * W + gx;
            const float x = is_flow ? static_cast<float>(gx) + px[o] : px[o];
            const float y = is_flow ? static_cast<float>(gy) + py[o] : py[o];
            const float x1 = floorf(x), y1 = floorf(y);
            // no tap of this source is inside the map (NaN and +-Inf fail every comparison): nothing to add
            if (!(x1 >= -1.f && x1 <= static_cast<float>(W - 1) && y1 >= -1.f && y1 <= static_cast<float>(H - 1))) continue;
            const int ix = static_cast<int>(x1), iy = static_cast<int>(y1);      // in [-1, W - 1] x [-1, H - 1]
            const float xc = x1 + 1.f, yc = y1 + 1.f;
            const float wxf = 1.f - fabsf(x - x1), wxc = 1.f - fabsf(x - xc);
            const float wyf = 1.f - fabsf(y - y1), wyc = 1.f - fabsf(y - yc);
            const bool okxf = ix >= 0, okxc = ix + 1 < W, okyf = iy >= 0, okyc = iy + 1 < H;
            if (okxc && okyc) add(ix + 1, iy + 1, wxc * wyc);
            if (okxc && okyf) add(ix + 1, iy, wxc * wyf);
            if (okxf && okyc) add(ix, iy + 1, wxf * wyc);
            if (okxf && okyf) add(ix, iy, wxf * wyf);
        }
    }
    __syncthreads();
    // a non-zero cell was written by a tap inside the map: its coordinates need no further test
    for (int i = threadIdx.x; i < kWinCells; i += kThreads) {
        const u64 v = win[i];
        if (v != 0) {
            const int r = i / kWinW, c = i - r * kWinW;
            atomicAdd(out + static_cast<int64_t>(wy0 + r) * W + (wx0 + c), v);
        }
    }
}

__global__ __launch_bounds__(kThreads) void splat_zero_kernel(u64 *__restrict__ acc, int64_t n) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i < n) acc[i] = 0;
}

__global__ __launch_bounds__(kThreads) void splat_convert_kernel(const u64 *__restrict__ acc, float *__restrict__ map, int64_t n) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i < n) map[i] = static_cast<float>(static_cast<double>(acc[i]) * kFixInv);
}

__global__ __launch_bounds__(kThreads) void occ_bidirection_kernel(const float *__restrict__ flow12, const float *__restrict__ flow21,
                                                                   float *__restrict__ mask, int64_t n, int H, int W, float scale,
                                                                   float bias) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t plane = static_cast<int64_t>(H) * W;
    const int64_t b = i / plane, p = i - b * plane;
    const int y = static_cast<int>(p / W), x = static_cast<int>(p - static_cast<int64_t>(y) * W);
    const float *fl = flow12 + b * 2 * plane + p;
    const float fx = fl[0], fy = fl[plane];
    // flow_warp's bilinear sample (warp_common.h: Bilinear), pad = zeros, on the two channels of flow21
    const Bilinear<float> t(source_coord<float>(x, fx, W, CERB_PAD_ZEROS).pos, source_coord<float>(y, fy, H, CERB_PAD_ZEROS).pos);
    int64_t onw, one, osw, ose;
    t.clamped_offsets(H, W, onw, one, osw, ose);
    bool nw, ne, sw, se;
    t.inside(H, W, nw, ne, sw, se);
    const float *img = flow21 + b * 2 * plane;
    float w[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float *ch = img + c * plane;
        w[c] = t.blend(ld(tap_ptr(ch + onw, nw)), ld(tap_ptr(ch + one, ne)), ld(tap_ptr(ch + osw, sw)), ld(tap_ptr(ch + ose, se)));
    }
    // :101-105, one rounding per stock launch
    const float dx = fx + w[0], dy = fy + w[1];
    const float lhs = dx * dx + dy * dy;
    const float mag = (fx * fx + fy * fy) + (w[0] * w[0] + w[1] * w[1]);
    const float th = scale * mag + bias;
    mask[i] = lhs > th ? 1.f : 0.f;
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------------------------------
int64_t corresponding_map_workspace_bytes(int B, int H, int W) {
    return static_cast<int64_t>(B) * H * W * static_cast<int64_t>(sizeof(u64));
}

int corresponding_map(const void *data, void *map, void *workspace, int B, int H, int W, int is_flow, hipStream_t s) {
    const int64_t n = static_cast<int64_t>(B) * H * W;
    u64 *acc = static_cast<u64 *>(workspace);
    const int nlin = static_cast<int>((n + kThreads - 1) / kThreads);
    splat_zero_kernel<<<nlin, kThreads, 0, s>>>(acc, n);
    int rc = launch_status();
    if (rc) return rc;
    const int tx = tiles(W, kTW), ty = tiles(H, kTH);
    const int nblocks = static_cast<int>(static_cast<int64_t>(tx) * ty * B);
    splat_kernel<<<nblocks, kThreads, 0, s>>>(static_cast<const float *>(data), acc, H, W, tx, ty, is_flow ? 1 : 0);
    rc = launch_status();
    if (rc) return rc;
    splat_convert_kernel<<<nlin, kThreads, 0, s>>>(acc, static_cast<float *>(map), n);
    return launch_status();
}

int occlusion_mask_bidirection(const void *flow12, const void *flow21, void *mask, int B, int H, int W, float scale, float bias,
                               hipStream_t s) {
    const int64_t n = static_cast<int64_t>(B) * H * W;
    occ_bidirection_kernel<<<static_cast<int>((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(
        static_cast<const float *>(flow12), static_cast<const float *>(flow21), static_cast<float *>(mask), n, H, W, scale, bias);
    return launch_status();
}

}  // namespace cerb
