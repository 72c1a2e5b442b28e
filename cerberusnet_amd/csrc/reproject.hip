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
// then flow_warp's bilinear taps, weights and summation order (warp_common.h: Bilinear, tap_ptr, flow_grad_terms,
// clip_kills_grad).
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
    const Bilinear<float> t(cx.pos, cy.pos);
    int64_t onw, one, osw, ose;
    t.clamped_offsets(H, W, onw, one, osw, ose);
    bool nw, ne, sw, se;
    t.inside(H, W, nw, ne, sw, se);
    const float *img = image + static_cast<int64_t>(b) * C * plane;
    float *dst = out + static_cast<int64_t>(b) * C * plane + p;
    for (int c = 0; c < C; ++c) {
        const float *ch = img + c * plane;
        dst[c * plane] = t.blend(ld(tap_ptr(ch + onw, nw)), ld(tap_ptr(ch + one, ne)), ld(tap_ptr(ch + osw, sw)), ld(tap_ptr(ch + ose, se)));
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
    const Bilinear<float> t(cx.pos, cy.pos);
    int64_t onw, one, osw, ose;
    t.clamped_offsets(H, W, onw, one, osw, ose);
    bool nw, ne, sw, se;
    t.inside(H, W, nw, ne, sw, se);
    const float *img = image + static_cast<int64_t>(b) * C * plane;
    const float *go = gout + static_cast<int64_t>(b) * C * plane + p;
    float gix = 0.f, giy = 0.f;       // sum_c grad_out[c] * dv_c/dsx, .. dsy
    for (int c = 0; c < C; ++c) {
        const float *ch = img + c * plane;
        const float g = go[c * plane];
        const float vnw = ld(tap_ptr(ch + onw, nw)), vne = ld(tap_ptr(ch + one, ne));
        const float vsw = ld(tap_ptr(ch + osw, sw)), vse = ld(tap_ptr(ch + ose, se));
        flow_grad_terms<float>(vnw, vne, vsw, vse, t.ax(), t.bx(), t.ay(), t.by(), g, gix, giy);
    }
    // autograd's order of THIS chain: grad_grid = mult * sum; through (. - 0.5) * 2: * 2; then through / (size - 1).  Not
    // flow_grad_out: norm_grid divides before it doubles, Project3D doubles last, and the roundings differ.
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
