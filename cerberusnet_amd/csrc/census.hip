// census.hip -- unFlowLoss's census ("ternary") term as ONE differentiable scalar op, fp32, 3 channels.
//
// Reference (nnet_training/loss_functions/UnFlowLoss.py:119-156, TernaryLoss, and :237-239 with the all-ones mask): a
// grayscale conversion, an identity-kernel conv2d that turns one gray plane into K = (2d+1)^2 planes, ~10 elementwise
// launches over those planes per image, a channel mean, a mask multiply and a whole-tensor mean; autograd keeps every
// intermediate.  Here, per call: one tile kernel + the shared single-workgroup sum forward, one tile kernel backward.
//
//   gray = 255 (0.2989 R + 0.5870 G + 0.1140 B),   x_o(q) = gray(q + o) - gray(q),   t = x / sqrt(0.81 + x^2)
//   dist(q) = (1 / K) sum_o D_o / (0.1 + D_o),  D_o = (t_o(im)(q) - t_o(im_warp)(q))^2,   loss = sum_{q interior} dist(q) / (B H W)
//
// Both kernels stage the GRAY value of a 16 x 64 tile + a halo of d of both images in LDS (two planes, not six) and walk
// the window from there.  The centre offset contributes exactly 0 (x = 0) and is skipped.
//
// Arithmetic.  Where a warped image is close to its target, t(im) - t(im_warp) is a difference of two nearly equal numbers,
// and on saturated windows (|x| >> 1, t = +-1 - O(1 / x^2)) an fp32 chain keeps only 2 or 3 digits of it.  So the gray
// planes are kept in fp64 (the differences x and x(im) - x(im_warp) are then exact up to one fp32 rounding), and for
// x_a x_b > 0 the difference is taken in its factored form
//     t(x_a) - t(x_b) = 0.81 (x_a - x_b) (x_a + x_b) / (s_a s_b (x_a s_b + x_b s_a)),   s = sqrt(0.81 + x^2),
// which has no cancellation; for x_a x_b <= 0 the plain form (x_a s_b - x_b s_a) / (s_a s_b) has none either.  Everything
// after the differences is fp32.
//
// Backward.  With n'(x) = 0.81 / (0.81 + x^2)^1.5, h'(e) = 0.2 e / (0.1 + e^2)^2 and
// g(q, o) = mask(q) h'(e_o(q)) n'(x_o(im_warp)(q)) / K, the gradient of the mean with respect to gray_warp(p) is
// (sum_o mask(p - o) g(p - o, o) - sum_o g(p, o)) / (B H W).  The term of centre p and offset -o uses the same pair of
// pixels as the term of centre p - o and offset o with x negated: t and e change sign, h' is odd, n' is even, so
// -g(p, -o) = +G(p, p - o) with  G(p, r) = h'(e) n'(x_w) / K,  x = gray(p) - gray(r),  e = t(x_w) - t(x_i).
// Hence  d / d gray_warp(p) = sum_{r in window(p), r != p} (mask(p) + mask(r)) G(p, r) / (B H W):  K - 1 terms per
// pixel, the same halo of d as the forward, every output element written once, no atomics.  a - b and b - a are exact
// negations in floating point, so this is the stated sum term by term, not an approximation of it.
#include "common.h"
#include "loss_reduce.h"

namespace cerb {
namespace {

constexpr int kTW = 64;        // tile: one column per lane ...
constexpr int kTH = 16;        // ... and 4 consecutive rows per thread, 4 waves
constexpr int kRows = 4;
constexpr int kThreads = kReduceThreads;
constexpr double kCoefR = 0.2989, kCoefG = 0.5870, kCoefB = 0.1140;

// the reference's order: the three products added left to right, then * 255
__device__ __forceinline__ double gray_at(const float *__restrict__ img, int hw, int o) {
    return (img[o] * kCoefR + img[hw + o] * kCoefG + img[2 * hw + o] * kCoefB) * 255.0;
}

// e = t(x_a) - t(x_b), t(x) = x / sqrt(0.81 + x^2), from x_a, x_b and dx = x_a - x_b (formed in fp64, rounded once);
// *sb_out = sqrt(0.81 + x_b^2)
__device__ __forceinline__ float ternary_diff(float xa, float xb, float dx, float *sb_out) {
    const float sa = sqrtf(0.81f + xa * xa), sb = sqrtf(0.81f + xb * xb);
    *sb_out = sb;
    const float cross = xa * sb + xb * sa;
    // a NaN fails the comparison and takes the plain form, which hands it on
    const float num = xa * xb > 0.f ? 0.81f * dx * (xa + xb) / cross : xa * sb - xb * sa;
    return num / (sa * sb);
}

// gray tile of both images + halo D -> LDS.  Outside the image the reference's conv2d pads with zero intensity; such a
// value only meets pixels within D of the border, which the valid mask removes (they are skipped here, not multiplied).
template <int D>
__device__ __forceinline__ void stage_gray(double *sa, double *sb, const float *__restrict__ a, const float *__restrict__ b, int H,
                                           int W, int y0, int x0) {
    constexpr int SH = kTH + 2 * D, SW = kTW + 2 * D;
    const int hw = H * W;
    for (int i = threadIdx.x; i < SH * SW; i += kThreads) {
        const int r = i / SW, c = i - r * SW;
        const int gy = y0 - D + r, gx = x0 - D + c;
        double u = 0.0, v = 0.0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int o = gy * W + gx;
            u = gray_at(a, hw, o);
            v = gray_at(b, hw, o);
        }
        sa[i] = u;
        sb[i] = v;
    }
}

template <int D>
struct Window {
    static constexpr int P = 2 * D + 1, K = P * P;
    static constexpr int SH = kTH + 2 * D, SW = kTW + 2 * D;   // LDS rows x pitch: a wave reads 64 consecutive words
    static constexpr int kLds = 2 * SH * SW;                   // doubles: 19008 / 21760 / 24640 B for D = 1 / 2 / 3
};

// ---- forward --------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kThreads) void census_fwd_kernel(const float *__restrict__ im, const float *__restrict__ im_warp,
                                                              float *__restrict__ partials, int H, int W, int tiles_x, int tiles_y) {
    using Win = Window<D>;
    constexpr int SW = Win::SW;
    __shared__ double lds[Win::kLds];
    __shared__ float red[4];
    double *sa = lds, *sb = lds + Win::SH * SW;
    const int blk = blockIdx.x;
    const int tx = blk % tiles_x, ty = (blk / tiles_x) % tiles_y;
    const int64_t b = blk / (tiles_x * tiles_y);
    const int x0 = tx * kTW, y0 = ty * kTH;
    const int64_t item = b * 3 * H * W;
    stage_gray<D>(sa, sb, im + item, im_warp + item, H, W, y0, x0);
    __syncthreads();

    const int lx = threadIdx.x & 63, ly = (threadIdx.x >> 6) * kRows;
    const int gx = x0 + lx;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int r = ly + k, gy = y0 + r;
        // the valid mask as a select: a masked pixel adds nothing, an interior one everything (a NaN included)
        if (gy >= D && gy < H - D && gx >= D && gx < W - D) {
            const int c = (r + D) * SW + lx + D;
            const double ca = sa[c], cb = sb[c];
            float sum = 0.f;
#pragma unroll
            for (int j = -D; j <= D; ++j)
#pragma unroll
                for (int i = -D; i <= D; ++i) {
                    if (j == 0 && i == 0) continue;
                    const double xa = sa[c + j * SW + i] - ca, xb = sb[c + j * SW + i] - cb;
                    float unused;
                    const float e = ternary_diff(static_cast<float>(xa), static_cast<float>(xb), static_cast<float>(xa - xb), &unused);
                    const float dd = e * e;
                    sum += dd / (0.1f + dd);
                }
            acc += sum / static_cast<float>(Win::K);
        }
    }
    const float total = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blk] = total;
}

// ---- backward -------------------------------------------------------------------------------------------------------
// grad_warp = grad_loss[0] * d loss / d im_warp, all three channels of every pixel written once
template <int D>
__global__ __launch_bounds__(kThreads) void census_bwd_kernel(const float *__restrict__ im, const float *__restrict__ im_warp,
                                                              const float *__restrict__ grad_loss, float *__restrict__ grad_warp, int H,
                                                              int W, int tiles_x, int tiles_y, float count) {
    using Win = Window<D>;
    constexpr int SW = Win::SW;
    __shared__ double lds[Win::kLds];
    double *si = lds, *sw = lds + Win::SH * SW;
    const int blk = blockIdx.x;
    const int tx = blk % tiles_x, ty = (blk / tiles_x) % tiles_y;
    const int64_t b = blk / (tiles_x * tiles_y);
    const int x0 = tx * kTW, y0 = ty * kTH;
    const int64_t item = b * 3 * H * W;
    const int hw = H * W;
    // the upstream gradient is read here, from device memory: no host synchronisation.  `scale` multiplies the finished
    // sum once, and scaling a float by a power of two is exact: the gradient is exactly linear in it.
    const float scale = grad_loss[0] / count;
    stage_gray<D>(si, sw, im + item, im_warp + item, H, W, y0, x0);
    __syncthreads();

    const int lx = threadIdx.x & 63, ly = (threadIdx.x >> 6) * kRows;
    const int gx = x0 + lx;
    if (gx >= W) return;
    float *pg = grad_warp + item;
    bool col_in[Win::P];           // is column gx + i inside the valid mask
#pragma unroll
    for (int i = -D; i <= D; ++i) col_in[i + D] = gx + i >= D && gx + i < W - D;
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int r = ly + k, gy = y0 + r;
        if (gy >= H) break;
        const int c = (r + D) * SW + lx + D;
        const double ci = si[c], cw = sw[c];
        const bool row_p = gy >= D && gy < H - D;
        const float mp = (row_p && col_in[D]) ? 1.f : 0.f;
        float sum = 0.f;
#pragma unroll
        for (int j = -D; j <= D; ++j) {
            const bool row_r = gy + j >= D && gy + j < H - D;
#pragma unroll
            for (int i = -D; i <= D; ++i) {
                if (j == 0 && i == 0) continue;
                const float wgt = mp + ((row_r && col_in[i + D]) ? 1.f : 0.f);     // mask(p) + mask(r): 0, 1 or 2
                if (wgt != 0.f) {
                    const double xi = ci - si[c + j * SW + i], xw = cw - sw[c + j * SW + i];
                    float sq;                                                       // sqrt(0.81 + x_w^2)
                    const float e = ternary_diff(static_cast<float>(xi), static_cast<float>(xw), static_cast<float>(xi - xw), &sq);
                    const float q = 0.1f + e * e;
                    sum -= wgt * ((0.2f * e) * 0.81f / ((q * q) * (sq * sq * sq)));  // h'(e_w - e_i) n'(x_w), e = -(e_w - e_i)
                }
            }
        }
        const float t = sum / static_cast<float>(Win::K);
        const int o = gy * W + gx;
        pg[o] = scale * (t * static_cast<float>(255.0 * kCoefR));
        pg[hw + o] = scale * (t * static_cast<float>(255.0 * kCoefG));
        pg[2 * hw + o] = scale * (t * static_cast<float>(255.0 * kCoefB));
    }
}

inline int tiles(int n, int t) { return (n + t - 1) / t; }

template <int D>
int forward_d(const float *im, const float *im_warp, float *loss, float *partials, int B, int H, int W, hipStream_t s) {
    const int tx = tiles(W, kTW), ty = tiles(H, kTH);
    const int nblocks = static_cast<int>(static_cast<int64_t>(tx) * ty * B);
    census_fwd_kernel<D><<<nblocks, kThreads, 0, s>>>(im, im_warp, partials, H, W, tx, ty);
    const int rc = launch_status();
    if (rc) return rc;
    // the mean runs over every pixel of the (B,1,H,W) map, the masked border included
    const float count = static_cast<float>(static_cast<double>(B) * H * W);
    final_sum_kernel<<<1, kThreads, 0, s>>>(partials, nullptr, nblocks, count, 1.0f, 1.0f, loss);
    return launch_status();
}

template <int D>
int backward_d(const float *im, const float *im_warp, const float *grad_loss, float *grad_warp, int B, int H, int W, hipStream_t s) {
    const int tx = tiles(W, kTW), ty = tiles(H, kTH);
    const int nblocks = static_cast<int>(static_cast<int64_t>(tx) * ty * B);
    const float count = static_cast<float>(static_cast<double>(B) * H * W);
    census_bwd_kernel<D><<<nblocks, kThreads, 0, s>>>(im, im_warp, grad_loss, grad_warp, H, W, tx, ty, count);
    return launch_status();
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------------------------------
int64_t census_workspace_bytes(int B, int H, int W) {
    return static_cast<int64_t>(tiles(W, kTW)) * tiles(H, kTH) * B * 4;
}

int census_forward(const void *im, const void *im_warp, void *loss, void *workspace, int B, int H, int W, int max_distance,
                   hipStream_t s) {
    const float *a = static_cast<const float *>(im), *b = static_cast<const float *>(im_warp);
    float *out = static_cast<float *>(loss), *ws = static_cast<float *>(workspace);
    switch (max_distance) {
    case 1: return forward_d<1>(a, b, out, ws, B, H, W, s);
    case 2: return forward_d<2>(a, b, out, ws, B, H, W, s);
    case 3: return forward_d<3>(a, b, out, ws, B, H, W, s);
    default: return CERB_EINVAL;
    }
}

int census_backward(const void *im, const void *im_warp, const void *grad_loss, void *grad_warp, int B, int H, int W,
                    int max_distance, hipStream_t s) {
    const float *a = static_cast<const float *>(im), *b = static_cast<const float *>(im_warp);
    const float *g = static_cast<const float *>(grad_loss);
    float *out = static_cast<float *>(grad_warp);
    switch (max_distance) {
    case 1: return backward_d<1>(a, b, g, out, B, H, W, s);
    case 2: return backward_d<2>(a, b, g, out, B, H, W, s);
    case 3: return backward_d<3>(a, b, g, out, B, H, W, s);
    default: return CERB_EINVAL;
    }
}

}  // namespace cerb
