// reproject.hip -- the stereo reprojection warp of the depth reconstruction loss, fp32, forward and backward to the depth
// (DESIGN.md 3.14).
//
// Reference (nnet_training/loss_functions/depth_losses.py):
//   BackprojectDepth.forward            :136-141   inv_K[:, :3, :3] @ (x, y, 1), * depth, cat ones          (bmm, mul, cat)
//   Project3D.forward                   :154-165   (K @ T)[:, :3, :] @ points, / (z + eps), / (W - 1), (. - 0.5) * 2
//   DepthReconstructionLossV1.forward   :198       F.grid_sample(l_img, pix_coords, padding_mode="border")
// About 20 stock launches over an N = H * W point cloud; here one launch each way.  Neither the point cloud nor the sample
// positions are ever written.  The image is a target (no gradient); the only gradient goes to the depth through the
// positions.
//
// Position of pixel (x, y) of item b, each stock launch's step rounded on its own (contraction is off) in the reference's
// order; inside the two matrix products the terms are accumulated with fused multiply-adds, as bmm does (dot3):
//     u   = inv_K3[b] . (x, y, 1)                      the unit-depth camera ray
//     cam = depth * u
//     p   = proj[b] . (cam, 1)                         proj = (K @ T)[:, :3, :], (B,3,4)
//     px  = p.x / (p.z + eps),  py = p.y / (p.z + eps)
//     g   = (px / (W - 1) - 0.5) * 2                   quirk Q2: normalised by W - 1 ...
//     s   = ((g + 1) * W - 1) / 2                      ... un-normalised with align_corners=False (ATen's fused multiply-add)
//     s   = clip(s, 0, W - 1)                          padding_mode="border"
// then flow_warp's bilinear taps, weights and summation order (warp_common.h: tap_index, tap_ptr, clip_kills_grad).
//
// Backward: one thread per pixel recomputes the position and gathers -- no atomics, no workspace, every element of
// grad_depth written exactly once:
//     grad_depth = sum_c grad_out[c] * (dv_c/dsx * dsx/ddepth + dv_c/dsy * dsy/ddepth)
//     ds/dp      = (size / 2) * 2 / (size - 1), in autograd's order; 0 where the clip holds the position (ATen's rule)
//     dpx/ddepth = (a.x * (p.z + eps) - p.x * a.z) / (p.z + eps)^2,   a = proj[:, :3] . u
//
// Layout: a wavefront owns 64 consecutive pixels of ONE image row, so the item b is wave-uniform and the 21 matrix
// elements are uniform loads; depth, grad_out and the result are read / written by 64 lanes on 64 consecutive floats.
// Stereo positions are smooth horizontal shifts: neighbouring lanes read neighbouring texels.  Channels are walked one at a
// time, the four taps of a channel issued together (8 waves per SIMD hide the rest); nothing is indexed dynamically (no
// scratch).
//
// Non-finite depth or positions.  A NaN position stays NaN through the clip (both comparisons are false), as in
// source_coord: tap_index maps it to tap 0, the weights are NaN and so is that pixel's result -- flow_warp's rule.  +-Inf
// positions (p.z + eps == 0 with p.x != 0) are clipped to the border like any other.  Every offset is formed from taps
// known to be inside the image; other pixels are not touched.
#include "warp_common.h"

#pragma clang fp contract(off)

namespace cerb {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kPix;

struct Ray {
    float ux, uy, uz;    // inv_K3 . (x, y, 1)
    float px, py, pz;    // proj . (depth * u, 1)
    float d;             // p.z + eps
};

// The first two terms of a row's dot product as a matrix product forms them: the runtime's bmm accumulates along k with fused
// multiply-adds, on the GPU and on the CPU alike (the stock fp32 chain's results are reproduced to the bit of its error
// against float64 by this order, and missed by up to 8 x on a 3 x 3 image by separately rounded products: the ray's x
// component cancels to a few per cent of its terms near the principal point).  Explicit: everything else here stays
// uncontracted, one rounding per stock launch.
__device__ __forceinline__ float dot3(const float *__restrict__ row, float a, float b) { return fma(row[1], b, row[0] * a); }

// m: inv_K3 row-major (9 floats), q: proj row-major (12 floats); both wave-uniform
__device__ __forceinline__ Ray project(const float *__restrict__ m, const float *__restrict__ q, float x, float y, float depth,
                                       float eps) {
    Ray r;
    r.ux = dot3(m, x, y) + m[2];
    r.uy = dot3(m + 3, x, y) + m[5];
    r.uz = dot3(m + 6, x, y) + m[8];
    const float cx = depth * r.ux, cy = depth * r.uy, cz = depth * r.uz;
    r.px = fma(q[2], cz, dot3(q, cx, cy)) + q[3];
    r.py = fma(q[6], cz, dot3(q + 4, cx, cy)) + q[7];
    r.pz = fma(q[10], cz, dot3(q + 8, cx, cy)) + q[11];
    r.d = r.pz + eps;
    return r;
}

// source_coord for a position that is already a pixel coordinate: the reference's normalisation (Project3D :162-164), ATen's
// un-normalisation (see unnormalized_coord) and the border clip with its gradient multiplier and NaN rule
__device__ __forceinline__ Coord<float> sample_coord(float pix, int size) {
    const float u = pix / static_cast<float>(size - 1);
    const float g = (u - 0.5f) * 2.0f;
    float p = fma(g + 1.0f, static_cast<float>(size), -1.0f) / 2.0f;
    float m = static_cast<float>(size) / 2.0f;
    const float hi = static_cast<float>(size - 1);
    if (clip_kills_grad(p, size)) m = 0.f;
    p = p <= 0.f ? 0.f : (p >= hi ? hi : p);
    return {p, m};
}

struct Taps {
    float ax, bx, ay, by;                // x1 - sx, sx - x0, y1 - sy, sy - y0
    int64_t onw, one, osw, ose;          // offsets inside a plane, clamped into it
    bool nw, ne, sw, se;                 // the tap is inside the image
};

__device__ __forceinline__ Taps make_taps(float sx, float sy, int H, int W) {
    Taps t;
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float x1f = x0f + 1.f, y1f = y0f + 1.f;
    t.ax = x1f - sx; t.bx = sx - x0f;
    t.ay = y1f - sy; t.by = sy - y0f;
    const int x0 = tap_index(x0f), y0 = tap_index(y0f);
    const bool okx0 = x0 >= 0 && x0 < W, okx1 = x0 + 1 >= 0 && x0 + 1 < W;
    const bool oky0 = y0 >= 0 && y0 < H, oky1 = y0 + 1 >= 0 && y0 + 1 < H;
    // an offset is formed only from coordinates inside the image; absent taps read a block of zeros (tap_ptr)
    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x0 + 1, 0), W - 1);
    const int64_t r0 = static_cast<int64_t>(min(max(y0, 0), H - 1)) * W, r1 = static_cast<int64_t>(min(max(y0 + 1, 0), H - 1)) * W;
    t.onw = r0 + cx0; t.one = r0 + cx1; t.osw = r1 + cx0; t.ose = r1 + cx1;
    t.nw = oky0 && okx0; t.ne = oky0 && okx1; t.sw = oky1 && okx0; t.se = oky1 && okx1;
    return t;
}

// the work item of a wavefront: (item b, row y, 64-pixel segment); false when there is none
__device__ __forceinline__ bool wave_item(int items, int segs, int H, int &b, int &y, int &x) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kPix), lane = threadIdx.x & (kPix - 1);
    const int item = xcd_chunk(blockIdx.x, gridDim.x) * kWaves + wave;      // wave-uniform
    if (item >= items) return false;
    const int sg = item % segs, row = item / segs;
    y = row % H; b = row / H;
    x = sg * kPix + lane;
    return true;
}

__global__ __launch_bounds__(kThreads) void reproject_warp_fwd_kernel(const float *__restrict__ image, const float *__restrict__ depth,
                                                                      const float *__restrict__ inv_k, const float *__restrict__ proj,
                                                                      float *__restrict__ out, int items, int segs, int C, int H, int W,
                                                                      float eps) {
    int b, y, x;
    if (!wave_item(items, segs, H, b, y, x) || x >= W) return;
    const int64_t plane = static_cast<int64_t>(H) * W;
    const int64_t p = static_cast<int64_t>(y) * W + x;
    const Ray r = project(inv_k + b * 9, proj + b * 12, static_cast<float>(x), static_cast<float>(y), depth[b * plane + p], eps);
    const Coord<float> cx = sample_coord(r.px / r.d, W);
    const Coord<float> cy = sample_coord(r.py / r.d, H);
    const Taps t = make_taps(cx.pos, cy.pos, H, W);
    const float wnw = t.ax * t.ay, wne = t.bx * t.ay, wsw = t.ax * t.by, wse = t.bx * t.by;
    const float *img = image + static_cast<int64_t>(b) * C * plane;
    float *dst = out + static_cast<int64_t>(b) * C * plane + p;
    for (int c = 0; c < C; ++c) {
        const float *ch = img + c * plane;
        const float vnw = ld(tap_ptr(ch + t.onw, t.nw)), vne = ld(tap_ptr(ch + t.one, t.ne));
        const float vsw = ld(tap_ptr(ch + t.osw, t.sw)), vse = ld(tap_ptr(ch + t.ose, t.se));
        float acc = vnw * wnw;     // absent taps contribute exact zeros
        acc += vne * wne;
        acc += vsw * wsw;
        acc += vse * wse;
        dst[c * plane] = acc;
    }
}

__global__ __launch_bounds__(kThreads) void reproject_warp_bwd_kernel(const float *__restrict__ image, const float *__restrict__ depth,
                                                                      const float *__restrict__ inv_k, const float *__restrict__ proj,
                                                                      const float *__restrict__ gout, float *__restrict__ gdepth,
                                                                      int items, int segs, int C, int H, int W, float eps) {
    int b, y, x;
    if (!wave_item(items, segs, H, b, y, x) || x >= W) return;
    const int64_t plane = static_cast<int64_t>(H) * W;
    const int64_t p = static_cast<int64_t>(y) * W + x;
    const float *q = proj + b * 12;
    const Ray r = project(inv_k + b * 9, q, static_cast<float>(x), static_cast<float>(y), depth[b * plane + p], eps);
    const Coord<float> cx = sample_coord(r.px / r.d, W);
    const Coord<float> cy = sample_coord(r.py / r.d, H);
    const Taps t = make_taps(cx.pos, cy.pos, H, W);
    const float *img = image + static_cast<int64_t>(b) * C * plane;
    const float *go = gout + static_cast<int64_t>(b) * C * plane + p;
    float gix = 0.f, giy = 0.f;       // sum_c grad_out[c] * dv_c/dsx, .. dsy
    for (int c = 0; c < C; ++c) {
        const float *ch = img + c * plane;
        const float g = go[c * plane];
        const float vnw = ld(tap_ptr(ch + t.onw, t.nw)), vne = ld(tap_ptr(ch + t.one, t.ne));
        const float vsw = ld(tap_ptr(ch + t.osw, t.sw)), vse = ld(tap_ptr(ch + t.ose, t.se));
        flow_grad_terms<float>(vnw, vne, vsw, vse, t.ax, t.bx, t.ay, t.by, g, gix, giy);
    }
    // autograd's order: grad_grid = mult * sum; through (. - 0.5) * 2: * 2; through / (size - 1)
    const float gpx = cx.mult * gix * 2.0f / static_cast<float>(W - 1);
    const float gpy = cy.mult * giy * 2.0f / static_cast<float>(H - 1);
    // a = proj[:, :3] . u: dp/ddepth
    const float ax = fma(q[2], r.uz, dot3(q, r.ux, r.uy));
    const float ay = fma(q[6], r.uz, dot3(q + 4, r.ux, r.uy));
    const float az = fma(q[10], r.uz, dot3(q + 8, r.ux, r.uy));
    const float dd = r.d * r.d;
    const float dpx = (ax * r.d - r.px * az) / dd;
    const float dpy = (ay * r.d - r.py * az) / dd;
    gdepth[b * plane + p] = gpx * dpx + gpy * dpy;
}

inline int64_t work_items(int B, int H, int W, int &segs) {
    segs = (W + kPix - 1) / kPix;
    return static_cast<int64_t>(B) * H * segs;
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------------------------------
int reproject_warp_forward(const void *image, const void *depth, const void *inv_k, const void *proj, void *out, int B, int C, int H,
                           int W, float eps, hipStream_t s) {
    int segs;
    const int items = static_cast<int>(work_items(B, H, W, segs));
    reproject_warp_fwd_kernel<<<(items + kWaves - 1) / kWaves, kThreads, 0, s>>>(
        static_cast<const float *>(image), static_cast<const float *>(depth), static_cast<const float *>(inv_k),
        static_cast<const float *>(proj), static_cast<float *>(out), items, segs, C, H, W, eps);
    return launch_status();
}

int reproject_warp_backward(const void *image, const void *depth, const void *inv_k, const void *proj, const void *grad_out,
                            void *grad_depth, int B, int C, int H, int W, float eps, hipStream_t s) {
    int segs;
    const int items = static_cast<int>(work_items(B, H, W, segs));
    reproject_warp_bwd_kernel<<<(items + kWaves - 1) / kWaves, kThreads, 0, s>>>(
        static_cast<const float *>(image), static_cast<const float *>(depth), static_cast<const float *>(inv_k),
        static_cast<const float *>(proj), static_cast<const float *>(grad_out), static_cast<float *>(grad_depth), items, segs, C, H,
        W, eps);
    return launch_status();
}

}  // namespace cerb
