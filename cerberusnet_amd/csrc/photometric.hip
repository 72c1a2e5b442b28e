// photometric.hip -- what unFlowLoss does AFTER each warp, fused: the photometric (L1 + SSIM) term and the
// edge-aware smoothness term as differentiable SCALAR ops.
//
// Reference (nnet_training/loss_functions/): loss_functions.py:47-77 (SSIM on 3 x 3 windows behind
// ReflectionPad2d(1), clamp((1 - SSIM) / 2, 0, 1)), UnFlowLoss.py:162-187 (edge-aware smoothness) and :236-255
// (loss_photometric with its all-ones mask) -- there 2 pads, 5 average pools, ~20 elementwise launches and two
// whole-tensor mean()s per call, and twice that again in autograd.  Here, per call: one tile kernel + one
// single-workgroup kernel forward, one tile kernel backward.
//
// Reductions: every workgroup writes ONE partial (its lanes folded by a fixed butterfly, its waves added in wave
// order) to a caller-owned workspace; a second launch of one workgroup adds the partials in a fixed order (thread t
// takes partials t, t + 256, ... in index order, then the 256 sums fold in a fixed tree).  No floating-point
// atomics: the result is bit-reproducible for a given shape, also inside a replayed graph.
//
// Arithmetic: the window moments are formed as the stock chain defines them (mean of 9 taps), but the variances and
// the covariance as means of DEVIATIONS from the window means, not as E[x^2] - mu^2: same value, without the
// cancellation that costs the stock fp32 chain 3 digits on smooth images.  The backward keeps to that: the gradient
// of pixel q is  sum_p m(p, q) [A'(p) + 2 (x_q - mu_x(p)) B(p) + (y_q - mu_y(p)) C(p)] / 9  over the window centres
// p whose reflected window holds q (m = how often), with A' = dV/dmu_x at fixed variance / covariance, B = dV/dvar_x,
// C = dV/dcov -- algebraically (sum A + 2 x_q sum B + y_q sum C) / 9 with A = A' - 2 mu_x B - mu_y C.
#include "common.h"
#include "loss_reduce.h"

namespace cerb {
namespace {

constexpr int kTW = 64;        // tile: one column per lane ...
constexpr int kTH = 16;        // ... and 4 consecutive rows per thread, 4 waves
constexpr int kRows = 4;
constexpr int kThreads = kReduceThreads;
constexpr float kC1 = 1e-4f;   // 0.01 ** 2
constexpr float kC2 = 9e-4f;   // 0.03 ** 2
constexpr float kNinth = 1.0f / 9.0f;

// ReflectionPad2d(1): -1 -> 1, n -> n - 2.  Positions further out (the backward's second halo ring, the part of a
// ragged tile beyond the image) only feed window centres that lie outside the image, whose terms are never used:
// they are clamped to a valid address.
__device__ __forceinline__ int reflect1(int p, int n) {
    p = p < 0 ? -p : p;
    p = p >= n ? 2 * n - 2 - p : p;
    return min(max(p, 0), n - 1);
}

// torch.clamp(v, 0, 1): a NaN stays a NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// tile of both images + HALO ring -> LDS, reflection applied while staging
template <int HALO>
__device__ __forceinline__ void stage_tiles(float *sx, float *sy, const float *__restrict__ x, const float *__restrict__ y,
                                            int H, int W, int y0, int x0) {
    constexpr int SH = kTH + 2 * HALO, SW = kTW + 2 * HALO;
    for (int i = threadIdx.x; i < SH * SW; i += kThreads) {
        const int r = i / SW, c = i - r * SW;
        const int o = reflect1(y0 - HALO + r, H) * W + reflect1(x0 - HALO + c, W);
        sx[i] = x[o];
        sy[i] = y[o];
    }
}

struct Moments { float mx, my, vx, vy, cov; };

// the 3 x 3 window whose top-left tap is sx[0] / sy[0] of an LDS image of pitch `pitch`
__device__ __forceinline__ Moments window_moments(const float *sx, const float *sy, int pitch) {
    float x[9], y[9];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            x[j * 3 + i] = sx[j * pitch + i];
            y[j * 3 + i] = sy[j * pitch + i];
        }
    Moments m;
    // the means in fp64, rounded once: SSIM's mean term is ill-conditioned where a window's mean is near zero (its
    // gradient grows like 1 / mean), and there the rounding of an fp32 sum of nine O(1) taps is what limits the result
    double ax = 0.0, ay = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        ax += static_cast<double>(x[k]);
        ay += static_cast<double>(y[k]);
    }
    m.mx = static_cast<float>(ax * (1.0 / 9.0));
    m.my = static_cast<float>(ay * (1.0 / 9.0));
    float vx = 0.f, vy = 0.f, cov = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float dx = x[k] - m.mx, dy = y[k] - m.my;
        vx += dx * dx;
        vy += dy * dy;
        cov += dx * dy;
    }
    m.vx = vx * kNinth; m.vy = vy * kNinth; m.cov = cov * kNinth;
    return m;
}

struct Ssim { float n1, n2, d1, d2, s, arg; };
__device__ __forceinline__ Ssim ssim_of(const Moments &m) {
    Ssim r;
    r.n1 = 2.0f * m.mx * m.my + kC1;
    r.n2 = 2.0f * m.cov + kC2;
    r.d1 = m.mx * m.mx + m.my * m.my + kC1;
    r.d2 = m.vx + m.vy + kC2;
    r.s = (r.n1 * r.n2) / (r.d1 * r.d2);
    r.arg = (1.0f - r.s) * 0.5f;
    return r;
}

// ---- photometric forward ------------------------------------------------------------------------------------------
constexpr int kFP = kTW + 2;                       // LDS row pitch, forward (66 floats): a wave reads 64 consecutive words
constexpr int kFwdLds = 2 * (kTH + 2) * kFP;       // 2376 floats = 9504 B

__global__ __launch_bounds__(kThreads) void photometric_fwd_kernel(const float *__restrict__ orig, const float *__restrict__ recons,
                                                                   float *__restrict__ partials, int H, int W, int tiles_x,
                                                                   int tiles_y, float l1_w, float ssim_w) {
    __shared__ float lds[kFwdLds];
    __shared__ float red[4];
    float *sx = lds, *sy = lds + (kTH + 2) * kFP;  // x = im_recons, y = im_orig (the argument order of the SSIM call)
    const int blk = blockIdx.x;
    const int tx = blk % tiles_x, ty = (blk / tiles_x) % tiles_y;
    const int64_t plane = blk / (tiles_x * tiles_y);
    const int x0 = tx * kTW, y0 = ty * kTH;
    const float *px = recons + plane * H * W, *py = orig + plane * H * W;
    stage_tiles<1>(sx, sy, px, py, H, W, y0, x0);
    __syncthreads();

    const int lx = threadIdx.x & 63, ly = (threadIdx.x >> 6) * kRows;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int r = ly + k;
        if (y0 + r < H && x0 + lx < W) {           // a pixel outside the image adds nothing (select, not multiply)
            const int o = r * kFP + lx;            // top-left tap of the window centred on LDS (r + 1, lx + 1)
            float v = 0.f;
            if (l1_w != 0.f) v = l1_w * fabsf(sy[o + kFP + 1] - sx[o + kFP + 1]);
            if (ssim_w != 0.f) v += ssim_w * clamp01(ssim_of(window_moments(sx + o, sy + o, kFP)).arg);
            acc += v;
        }
    }
    const float total = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blk] = total;
}

// ---- photometric backward -----------------------------------------------------------------------------------------
constexpr int kBP = kTW + 4;                       // input pitch (2-pixel halo): 68
constexpr int kBIn = (kTH + 4) * kBP;              // 1360 floats per image
constexpr int kDP = kTW + 2;                       // pitch of the per-centre terms (1-pixel halo): 66
constexpr int kBD = (kTH + 2) * kDP;               // 1188 centres
constexpr int kBwdLds = 2 * kBIn + 5 * kBD;        // 8660 floats = 34640 B

__global__ __launch_bounds__(kThreads) void photometric_bwd_kernel(const float *__restrict__ orig, const float *__restrict__ recons,
                                                                   const float *__restrict__ grad_loss, float *__restrict__ grad_recons,
                                                                   int H, int W, int tiles_x, int tiles_y, float l1_w, float ssim_w,
                                                                   float count) {
    __shared__ float lds[kBwdLds];
    float *sx = lds, *sy = lds + kBIn;
    float *sA = lds + 2 * kBIn, *sB = sA + kBD, *sC = sB + kBD, *sMx = sC + kBD, *sMy = sMx + kBD;
    const int blk = blockIdx.x;
    const int tx = blk % tiles_x, ty = (blk / tiles_x) % tiles_y;
    const int64_t plane = blk / (tiles_x * tiles_y);
    const int x0 = tx * kTW, y0 = ty * kTH;
    const float *px = recons + plane * H * W, *py = orig + plane * H * W;
    float *pg = grad_recons + plane * H * W;
    // the upstream gradient is read here, from device memory: no host synchronisation.  Scaling a float by a power of
    // two is exact, and `scale` multiplies the finished sum once: the gradient is exactly linear in it.
    const float scale = grad_loss[0] / count;
    stage_tiles<2>(sx, sy, px, py, H, W, y0, x0);
    __syncthreads();

    // the per-centre terms on the tile + 1 ring; a centre outside the image has no window: zeros
    if (ssim_w != 0.f) {
        for (int i = threadIdx.x; i < kBD; i += kThreads) {
            const int r = i / kDP, c = i - r * kDP;
            const int gy = y0 - 1 + r, gx = x0 - 1 + c;
            float a = 0.f, b = 0.f, cc = 0.f, mx = 0.f, my = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const Moments m = window_moments(sx + r * kBP + c, sy + r * kBP + c, kBP);
                const Ssim s = ssim_of(m);
                // clamp's gradient passes where its argument lies in [0, 1], bounds included (ATen)
                const float g = (s.arg >= 0.f && s.arg <= 1.f) ? -0.5f * ssim_w : 0.f;
                const float inv = 1.0f / (s.d1 * s.d2);
                // dS/dmu_x at fixed variance / covariance = 2 (n2 / d2) (mu_y d1 - mu_x n1) / d1^2, with the bracket in its
                // factored form (mu_y - mu_x) (mu_y (mu_y + mu_x) + C1): no cancellation where the two means are close
                a = g * (s.n2 * inv) * (2.0f * ((m.my - m.mx) * (m.my * (m.my + m.mx) + kC1)) / s.d1);
                b = g * (-s.s / s.d2);
                cc = g * (2.0f * s.n1 * inv);
                mx = m.mx; my = m.my;
            }
            sA[i] = a; sB[i] = b; sC[i] = cc; sMx[i] = mx; sMy[i] = my;
        }
        __syncthreads();
    }

    const int lx = threadIdx.x & 63, ly = (threadIdx.x >> 6) * kRows;
    const int gx = x0 + lx;
    if (gx >= W) return;
    // how often the window of the centre one column to the left / right holds this column: twice where the
    // reflection folds the padding column back onto it (column 1 from the centre on column 0, W - 2 from W - 1)
    const float wxm = gx == 1 ? 2.f : 1.f, wxp = gx == W - 2 ? 2.f : 1.f;
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int r = ly + k, gy = y0 + r;
        if (gy >= H) break;
        const float xq = sx[(r + 2) * kBP + lx + 2], yq = sy[(r + 2) * kBP + lx + 2];
        float t = 0.f;
        if (ssim_w != 0.f) {
            const float wym = gy == 1 ? 2.f : 1.f, wyp = gy == H - 2 ? 2.f : 1.f;
            float rows[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                float cols[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int o = (r + j) * kDP + lx + i;     // centre (gy - 1 + j, gx - 1 + i)
                    cols[i] = sA[o] + 2.0f * (xq - sMx[o]) * sB[o] + (yq - sMy[o]) * sC[o];
                }
                rows[j] = wxm * cols[0] + cols[1] + wxp * cols[2];
            }
            t = (wym * rows[0] + rows[1] + wyp * rows[2]) * kNinth;
        }
        if (l1_w != 0.f) {
            const float d = xq - yq;                          // d |y - x| / dx = sign(x - y), 0 at equality
            t += d > 0.f ? l1_w : (d < 0.f ? -l1_w : (d == d ? 0.f : d));
        }
        pg[gy * W + gx] = scale * t;
    }
}

// ---- edge-aware smoothness ----------------------------------------------------------------------------------------
constexpr int kSW = 64, kSH = 4;   // one pixel per thread, a 64 x 4 tile per workgroup; neighbours come from the cache

// exp(-alpha * mean_c |image[.., p + 1] - image[.., p]|) along one axis (`step` = 1 or W)
__device__ __forceinline__ float edge_weight(const float *__restrict__ img, int C, int plane_sz, int o, int step, float alpha) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += fabsf(img[c * plane_sz + o + step] - img[c * plane_sz + o]);
    return expf(-(s / static_cast<float>(C)) * alpha);
}

__device__ __forceinline__ float sign_of(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : (d == d ? 0.f : d)); }

// element e of the DEGREE-th difference along one axis, from f[e], f[e + step], (f[e + 2 step])
template <int DEGREE>
__device__ __forceinline__ float diff_at(const float *__restrict__ f, int o, int step) {
    if (DEGREE == 1) return f[o + step] - f[o];
    return (f[o + 2 * step] - f[o + step]) - (f[o + step] - f[o]);
}

template <int DEGREE>
__global__ __launch_bounds__(kThreads) void smooth_fwd_kernel(const float *__restrict__ flow, const float *__restrict__ image,
                                                              float *__restrict__ partials, int nblocks, int Cf, int Ci, int H,
                                                              int W, int tiles_x, int tiles_y, float alpha) {
    __shared__ float red[4];
    const int blk = blockIdx.x;
    const int tx = blk % tiles_x, ty = (blk / tiles_x) % tiles_y;
    const int64_t b = blk / (tiles_x * tiles_y);
    const int x = tx * kSW + (threadIdx.x & 63), y = ty * kSH + (threadIdx.x >> 6);
    const int hw = H * W;
    const float *f = flow + b * Cf * hw, *img = image + b * Ci * hw;
    float ax = 0.f, ay = 0.f;
    if (x < W && y < H) {
        const int o = y * W + x;
        // element x of the x term: degree 1 weighs |f[x+1] - f[x]| / 2 by the edge between x and x + 1, degree 2 weighs
        // the second difference at x .. x + 2 by the edge between x + 1 and x + 2 (the reference's wx[..., 1:])
        if (x + DEGREE < W) {
            const float w = edge_weight(img, Ci, hw, o + (DEGREE - 1), 1, alpha);
            for (int c = 0; c < Cf; ++c) {
                const float v = w * fabsf(diff_at<DEGREE>(f + c * hw, o, 1));
                ax += DEGREE == 1 ? v / 2.0f : v;
            }
        }
        if (y + DEGREE < H) {
            const float w = edge_weight(img, Ci, hw, o + (DEGREE - 1) * W, W, alpha);
            for (int c = 0; c < Cf; ++c) {
                const float v = w * fabsf(diff_at<DEGREE>(f + c * hw, o, W));
                ay += DEGREE == 1 ? v / 2.0f : v;
            }
        }
    }
    const float sx = block_sum(ax, red);
    __syncthreads();
    const float sy = block_sum(ay, red);
    if (threadIdx.x == 0) {
        partials[blk] = sx;
        partials[nblocks + blk] = sy;
    }
}

// d term / d f[p] along one axis: a gather over the (at most DEGREE + 1) differences that hold f[p].
// p = position along the axis, n = its extent, o = offset of f[p], step = 1 or W; w[DEGREE - k] = weight of element p - k.
template <int DEGREE>
__device__ __forceinline__ float smooth_axis_grad(const float *__restrict__ f, const float *w, int p, int n, int o, int step) {
    float t = 0.f;
    if (DEGREE == 1) {
        if (p + 1 < n) t -= w[1] * sign_of(diff_at<1>(f, o, step));            // element p: -f[p]
        if (p >= 1) t += w[0] * sign_of(diff_at<1>(f, o - step, step));        // element p - 1: +f[p]
    } else {
        if (p + 2 < n) t += w[2] * sign_of(diff_at<2>(f, o, step));                             // element p: +f[p]
        if (p >= 1 && p + 1 < n) t -= 2.0f * (w[1] * sign_of(diff_at<2>(f, o - step, step)));   // element p - 1: -2 f[p]
        if (p >= 2) t += w[0] * sign_of(diff_at<2>(f, o - 2 * step, step));                     // element p - 2: +f[p]
    }
    return t;
}

template <int DEGREE>
__global__ __launch_bounds__(kThreads) void smooth_bwd_kernel(const float *__restrict__ flow, const float *__restrict__ image,
                                                              const float *__restrict__ grad_loss, float *__restrict__ grad_flow,
                                                              int Cf, int Ci, int H, int W, int tiles_x, int tiles_y, float alpha,
                                                              float coef_x, float coef_y) {
    const int blk = blockIdx.x;
    const int tx = blk % tiles_x, ty = (blk / tiles_x) % tiles_y;
    const int64_t b = blk / (tiles_x * tiles_y);
    const int x = tx * kSW + (threadIdx.x & 63), y = ty * kSH + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int hw = H * W, o = y * W + x;
    const float *f = flow + b * Cf * hw, *img = image + b * Ci * hw;
    float *g = grad_flow + b * Cf * hw;
    const float gl = grad_loss[0];
    const float gx = gl * coef_x, gy = gl * coef_y;     // coef = 1 / (2 * count) (and the / 2 of degree 1): host constants
    // the weights of the elements p - DEGREE .. p that exist (index DEGREE = element p), shared by the flow's channels
    float wx[DEGREE + 1], wy[DEGREE + 1];
#pragma unroll
    for (int k = 0; k <= DEGREE; ++k) {
        const int ex = x - DEGREE + k, ey = y - DEGREE + k;
        wx[k] = (ex >= 0 && ex + DEGREE < W) ? edge_weight(img, Ci, hw, y * W + ex + (DEGREE - 1), 1, alpha) : 0.f;
        wy[k] = (ey >= 0 && ey + DEGREE < H) ? edge_weight(img, Ci, hw, (ey + DEGREE - 1) * W + x, W, alpha) : 0.f;
    }
    for (int c = 0; c < Cf; ++c) {
        const float *fc = f + c * hw;
        const float tx_ = smooth_axis_grad<DEGREE>(fc, wx, x, W, o, 1);
        const float ty_ = smooth_axis_grad<DEGREE>(fc, wy, y, H, o, W);
        g[c * hw + o] = gx * tx_ + gy * ty_;
    }
}

inline int tiles(int n, int t) { return (n + t - 1) / t; }

}  // namespace

// ---- host side ----------------------------------------------------------------------------------------------------
int64_t photometric_workspace_bytes(int B, int C, int H, int W) {
    return static_cast<int64_t>(tiles(W, kTW)) * tiles(H, kTH) * B * C * 4;
}

int photometric_forward(const void *orig, const void *recons, void *loss, void *workspace, int B, int C, int H, int W, float l1_w,
                        float ssim_w, hipStream_t s) {
    const int tx = tiles(W, kTW), ty = tiles(H, kTH);
    const int nblocks = static_cast<int>(static_cast<int64_t>(tx) * ty * B * C);
    float *partials = static_cast<float *>(workspace);
    photometric_fwd_kernel<<<nblocks, kThreads, 0, s>>>(static_cast<const float *>(orig), static_cast<const float *>(recons), partials,
                                                        H, W, tx, ty, l1_w, ssim_w);
    int rc = launch_status();
    if (rc) return rc;
    const float count = static_cast<float>(static_cast<double>(B) * C * H * W);
    final_sum_kernel<<<1, kThreads, 0, s>>>(partials, nullptr, nblocks, count, 1.0f, 1.0f, static_cast<float *>(loss));
    return launch_status();
}

int photometric_backward(const void *orig, const void *recons, const void *grad_loss, void *grad_recons, int B, int C, int H, int W,
                         float l1_w, float ssim_w, hipStream_t s) {
    const int tx = tiles(W, kTW), ty = tiles(H, kTH);
    const int nblocks = static_cast<int>(static_cast<int64_t>(tx) * ty * B * C);
    const float count = static_cast<float>(static_cast<double>(B) * C * H * W);
    photometric_bwd_kernel<<<nblocks, kThreads, 0, s>>>(static_cast<const float *>(orig), static_cast<const float *>(recons),
                                                        static_cast<const float *>(grad_loss), static_cast<float *>(grad_recons), H, W,
                                                        tx, ty, l1_w, ssim_w, count);
    return launch_status();
}

int64_t smoothness_workspace_bytes(int B, int H, int W) {
    return static_cast<int64_t>(tiles(W, kSW)) * tiles(H, kSH) * B * 2 * 4;
}

int smoothness_forward(const void *flow, const void *image, void *loss, void *workspace, int B, int Cf, int Ci, int H, int W,
                       float alpha, int degree, hipStream_t s) {
    const int tx = tiles(W, kSW), ty = tiles(H, kSH);
    const int nblocks = static_cast<int>(static_cast<int64_t>(tx) * ty * B);
    float *partials = static_cast<float *>(workspace);
    const float *f = static_cast<const float *>(flow), *img = static_cast<const float *>(image);
    if (degree == 1)
        smooth_fwd_kernel<1><<<nblocks, kThreads, 0, s>>>(f, img, partials, nblocks, Cf, Ci, H, W, tx, ty, alpha);
    else
        smooth_fwd_kernel<2><<<nblocks, kThreads, 0, s>>>(f, img, partials, nblocks, Cf, Ci, H, W, tx, ty, alpha);
    int rc = launch_status();
    if (rc) return rc;
    // the x and the y term are means over different element counts, then averaged
    const float nx = static_cast<float>(static_cast<double>(B) * Cf * H * (W - degree));
    const float ny = static_cast<float>(static_cast<double>(B) * Cf * (H - degree) * W);
    final_sum_kernel<<<1, kThreads, 0, s>>>(partials, partials + nblocks, nblocks, nx, ny, 0.5f, static_cast<float *>(loss));
    return launch_status();
}

int smoothness_backward(const void *flow, const void *image, const void *grad_loss, void *grad_flow, int B, int Cf, int Ci, int H,
                        int W, float alpha, int degree, hipStream_t s) {
    const int tx = tiles(W, kSW), ty = tiles(H, kSH);
    const int nblocks = static_cast<int>(static_cast<int64_t>(tx) * ty * B);
    const double term = degree == 1 ? 0.5 : 1.0;
    const float cx = static_cast<float>(0.5 * term / (static_cast<double>(B) * Cf * H * (W - degree)));
    const float cy = static_cast<float>(0.5 * term / (static_cast<double>(B) * Cf * (H - degree) * W));
    const float *f = static_cast<const float *>(flow), *img = static_cast<const float *>(image);
    const float *gl = static_cast<const float *>(grad_loss);
    float *g = static_cast<float *>(grad_flow);
    if (degree == 1)
        smooth_bwd_kernel<1><<<nblocks, kThreads, 0, s>>>(f, img, gl, g, Cf, Ci, H, W, tx, ty, alpha, cx, cy);
    else
        smooth_bwd_kernel<2><<<nblocks, kThreads, 0, s>>>(f, img, gl, g, Cf, Ci, H, W, tx, ty, alpha, cx, cy);
    return launch_status();
}

}  // namespace cerb
