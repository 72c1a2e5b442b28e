// rmi_loss.hip -- the heavy part of the region mutual information loss (RMILoss, reference nnet_training/loss_functions/rmi.py:
// 33-207) for radius 3 and average pooling, fp32 logits (N,C,H,W), int64 labels (N,H,W).
//
//   valid = 0 <= label < C;  o_c = valid and label == c;  s = sigmoid(x)
//   bce   = sum_{valid pixels, all classes} (max(x,0) - x o + log1p(exp(-|x|))) / (n_valid + 1)
//   prob  = valid ? s + 1e-6 : 1e-6
//   la, pr = avg_pool2d(o / prob, p, p, p / 2): (N,C,h,w), disjoint windows that start at p j - p / 2, divisor p p everywhere
//   L_k, Pr_k (k = (a,b), a,b < 3) = the 9 shifted (h-2) x (w-2) slices minus their own means, in float64
//   la_cov = L L^T, pr_cov = Pr Pr^T, la_pr_cov = L Pr^T: (N,C,9,9) float64
// The 9 x 9 algebra on the three matrices (inverse, Cholesky, log) is left to the caller, who hands back
// G_pr = dloss/dpr_cov and G_lp = dloss/dla_pr_cov; the backward here turns them into grad_logits in one launch.
//
// Front end and backward share one layout: the image is cut into the pooling's windows, EXTENDED past the last pooled row /
// column ((H - 1 + pad) / p + 1 of them) so that a trailing row or column that lies in no window still has an owner; a lane
// owns one such cell and its p x p pixels for a group of 8 class planes, adjacent lanes own adjacent cells: a wave's loads and
// stores cover whole rows of the logits.  The labels of the cell are classified once into LDS (class, -1 ignored, -2 outside
// the image).  Two routes with the same arithmetic in the same order (contraction into fma is off in this file):
//   pair   : p in {4, 8}, W even, 8-byte aligned logits / gradient, 16-byte aligned labels: a window starts at an even x, so a
//            lane takes its row as aligned pairs -- 8-byte loads of the logits, 16-byte loads of the labels
//   scalar : guarded 4-byte loads, any p in 1..8 and any W
// A row of a window is summed pair by pair from the left, the rows from the top.
//
// Every sum has a fixed order and no floating-point atomics: the BCE terms are added in fp32 per lane, in float64 from the lane
// upward (butterfly, 4 waves in wave order, per-workgroup partials, one workgroup adds the partials); the means and the centred
// products are float64 throughout (one lane per matrix entry walks its chunk of positions in order, the chunks are added in
// index order).  The same bits on every run.
//
// Labels never form an address.  An ignored pixel is skipped by selection: a NaN logit there changes nothing and its
// gradient is 0.0f.
#include "common.h"
#include "loss_reduce.h"

#pragma clang fp contract(off)

namespace cerb {
namespace {

constexpr int kThreads = kReduceThreads;
constexpr int kClassGroup = 8;        // class planes per workgroup of the front end and the backward
constexpr int kMaxPool = 8;
constexpr int kR = 3, kD = kR * kR;   // radius, and the dimension of a point
constexpr int kEntries = 3 * kD * kD; // la_cov, pr_cov, la_pr_cov
constexpr int kPosChunk = 1024;       // positions per workgroup of the moment kernel
constexpr float kClipMin = 1e-6f;

struct Geom {
    int N, C, H, W, p, pad;
    int h, w;        // the pooled maps
    int he, we;      // the cells: pooled windows and the rest of the image behind them
    int nh, nw, P;   // the positions of a 3 x 3 slice
    int nblk, ncg;   // front end / backward: workgroups per image and class group, class groups
    int nchunks;     // moment kernel: workgroups per (n, c)
};

inline Geom make_geom(int N, int C, int H, int W, int p) {
    Geom g;
    g.N = N; g.C = C; g.H = H; g.W = W; g.p = p; g.pad = p / 2;
    g.h = (H + 2 * g.pad - p) / p + 1;
    g.w = (W + 2 * g.pad - p) / p + 1;
    g.he = (H - 1 + g.pad) / p + 1;
    g.we = (W - 1 + g.pad) / p + 1;
    g.nh = g.h - kR + 1;
    g.nw = g.w - kR + 1;
    g.P = g.nh > 0 && g.nw > 0 ? g.nh * g.nw : 0;
    g.nblk = (g.he * g.we + kThreads - 1) / kThreads;
    g.ncg = (C + kClassGroup - 1) / kClassGroup;
    g.nchunks = (g.P + kPosChunk - 1) / kPosChunk;
    return g;
}

// loss_reduce.h's block_sum behind a barrier of its own: consecutive calls here share one red[4], which may still be read from
// the call before
__device__ __forceinline__ double block_sum_reusing(double v, double *red) {
    __syncthreads();
    return block_sum(v, red);
}

// ---- what the front end and the backward share -------------------------------------------------------------------
// the labels of this lane's cell, classified: class, -1 ignored, -2 outside the image.  codes[k * kThreads + lane], k = dy p + dx;
// written and read by the same lane only.  Returns the number of valid pixels.
template <bool kPair>
__device__ __forceinline__ int classify_cell(const int64_t *__restrict__ t, short *codes, const Geom &g, bool live, int y0, int x0) {
    int count = 0;
    for (int dy = 0; dy < g.p; ++dy) {
        const int y = y0 + dy;
        const bool row_in = live && y >= 0 && y < g.H;
        for (int dx = 0; dx < g.p; dx += 2) {
            const int x = x0 + dx;
            short c0 = -2, c1 = -2;
            if constexpr (kPair) {           // x is even and W is even: a pair is inside or outside as a whole
                if (row_in && x >= 0 && x < g.W) {
                    const longlong2 v = *reinterpret_cast<const longlong2 *>(t + static_cast<int64_t>(y) * g.W + x);
                    c0 = static_cast<uint64_t>(v.x) < static_cast<uint64_t>(g.C) ? static_cast<short>(v.x) : -1;
                    c1 = static_cast<uint64_t>(v.y) < static_cast<uint64_t>(g.C) ? static_cast<short>(v.y) : -1;
                }
            } else {
                if (row_in && x >= 0 && x < g.W) {
                    const int64_t v = t[static_cast<int64_t>(y) * g.W + x];
                    c0 = static_cast<uint64_t>(v) < static_cast<uint64_t>(g.C) ? static_cast<short>(v) : -1;
                }
                if (row_in && dx + 1 < g.p && x + 1 >= 0 && x + 1 < g.W) {
                    const int64_t v = t[static_cast<int64_t>(y) * g.W + x + 1];
                    c1 = static_cast<uint64_t>(v) < static_cast<uint64_t>(g.C) ? static_cast<short>(v) : -1;
                }
            }
            const int k = dy * g.p + dx;
            codes[k * kThreads + threadIdx.x] = c0;
            if (dx + 1 < g.p) codes[(k + 1) * kThreads + threadIdx.x] = c1;
            count += (c0 >= 0) + (c1 >= 0);
        }
    }
    return count;
}

// two neighbouring logits of a row; a pixel outside the image (code -2) is not loaded
template <bool kPair>
__device__ __forceinline__ void load2(const float *__restrict__ row, int x, short c0, short c1, float &v0, float &v1) {
    v0 = v1 = 0.f;
    if constexpr (kPair) {
        if (c0 != -2) {
            const float2 v = *reinterpret_cast<const float2 *>(row + x);
            v0 = v.x;
            v1 = v.y;
        }
    } else {
        if (c0 != -2) v0 = row[x];
        if (c1 != -2) v1 = row[x + 1];
    }
}

// sigmoid and the BCE term of one element from one exp: e = exp(-|x|)
__device__ __forceinline__ void sigmoid_bce(float x, bool hit, float &s, float &bce) {
    const float e = expf(-fabsf(x));
    const float r = 1.f / (1.f + e);
    s = x >= 0.f ? r : e * r;
    bce = (fmaxf(x, 0.f) - (hit ? x : 0.f)) + log1pf(e);
}

// ---- forward, front end ---------------------------------------------------------------------------------------------
// grid (nblk, ncg, N).  pbce / pcnt: one partial per workgroup, index (n ncg + group) nblk + block; the valid pixels are
// counted by class group 0 only.
template <bool kPair>
__global__ __launch_bounds__(kThreads) void rmi_front_kernel(const float *__restrict__ x, const int64_t *__restrict__ t,
                                                             float *__restrict__ la, float *__restrict__ pr, double *__restrict__ pbce,
                                                             double *__restrict__ pcnt, Geom g, int do_rmi) {
    __shared__ short codes[kMaxPool * kMaxPool * kThreads];
    __shared__ double red[4];
    const int cell = blockIdx.x * kThreads + threadIdx.x, n = blockIdx.z;
    const bool live = cell < g.he * g.we;
    const int i = cell / g.we, j = cell - i * g.we;
    const int y0 = i * g.p - g.pad, x0 = j * g.p - g.pad;
    const int64_t HW = static_cast<int64_t>(g.H) * g.W;
    const int count = classify_cell<kPair>(t + n * HW, codes, g, live, y0, x0);
    const bool pooled = do_rmi && live && i < g.h && j < g.w;
    const float div = static_cast<float>(g.p * g.p);
    const int c_end = min(g.C, (static_cast<int>(blockIdx.y) + 1) * kClassGroup);
    float bacc = 0.f;
    for (int c = blockIdx.y * kClassGroup; c < c_end; ++c) {
        const float *plane = x + (static_cast<int64_t>(n) * g.C + c) * HW;
        float cell_pr = 0.f;
        int hits = 0;
        if (live) {
            for (int dy = 0; dy < g.p; ++dy) {
                const float *row = plane + static_cast<int64_t>(y0 + dy) * g.W;       // formed, not read, outside the image
                float row_pr = 0.f;
                for (int dx = 0; dx < g.p; dx += 2) {
                    const int k = dy * g.p + dx;
                    const short c0 = codes[k * kThreads + threadIdx.x];
                    const short c1 = dx + 1 < g.p ? codes[(k + 1) * kThreads + threadIdx.x] : static_cast<short>(-2);
                    float v0, v1, s0, s1, b0, b1;
                    load2<kPair>(row, x0 + dx, c0, c1, v0, v1);
                    sigmoid_bce(v0, c0 == c, s0, b0);
                    sigmoid_bce(v1, c1 == c, s1, b1);
                    // probability: sigmoid * valid + 1e-6 inside the image, 0 (the pooling's padding) outside
                    const float p0 = c0 >= 0 ? s0 + kClipMin : (c0 == -1 ? kClipMin : 0.f);
                    const float p1 = c1 >= 0 ? s1 + kClipMin : (c1 == -1 ? kClipMin : 0.f);
                    const float pair = p0 + p1;
                    row_pr = dx == 0 ? pair : row_pr + pair;
                    bacc += c0 >= 0 ? b0 : 0.f;
                    bacc += c1 >= 0 ? b1 : 0.f;
                    hits += (c0 == c) + (c1 == c);
                }
                cell_pr = dy == 0 ? row_pr : cell_pr + row_pr;
            }
        }
        if (pooled) {
            const int64_t o = ((static_cast<int64_t>(n) * g.C + c) * g.h + i) * g.w + j;
            pr[o] = cell_pr / div;
            la[o] = static_cast<float>(hits) / div;
        }
    }
    const double tb = block_sum_reusing(static_cast<double>(bacc), red);
    const double tc = block_sum_reusing(static_cast<double>(count), red);
    if (threadIdx.x == 0) {
        const int64_t part = (static_cast<int64_t>(n) * g.ncg + blockIdx.y) * g.nblk + blockIdx.x;
        pbce[part] = tb;
        pcnt[part] = blockIdx.y == 0 ? tc : 0.0;
    }
}

// one workgroup adds the partials in a fixed order.  bce[0], state = [bce, n_valid, 1 / (n_valid + 1), 0]
__global__ __launch_bounds__(kThreads) void rmi_bce_final_kernel(const double *__restrict__ pbce, const double *__restrict__ pcnt,
                                                                 int64_t n, float *__restrict__ bce, float *__restrict__ state) {
    __shared__ double red[2][kThreads];
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) {
        a += pbce[i];
        b += pcnt[i];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    tree_sum(red);
    if (threadIdx.x == 0) {
        const double num = red[0][0], valid = red[1][0];
        const float v = static_cast<float>(num / (valid + 1.0));
        bce[0] = v;
        state[0] = v;
        state[1] = static_cast<float>(valid);
        state[2] = static_cast<float>(1.0 / (valid + 1.0));
        state[3] = 0.f;
    }
}

// ---- forward, moments ---------------------------------------------------------------------------------------------------
// the means of the 9 shifted slices of both maps: one workgroup per (n, c); means[(nc) 18 + m 9 + k], m = 0 label, 1 probability.
// An element (i, j) of a map lies in slice (a, b) at position (i - a, j - b) where that is one.
__global__ __launch_bounds__(kThreads) void rmi_mean_kernel(const float *__restrict__ la, const float *__restrict__ pr,
                                                            double *__restrict__ means, Geom g) {
    __shared__ double red[4];
    const int64_t base = static_cast<int64_t>(blockIdx.x) * g.h * g.w;
    double sl[kD], sp[kD];
#pragma unroll
    for (int k = 0; k < kD; ++k) sl[k] = sp[k] = 0.0;
    const int count = g.h * g.w;
    for (int e = threadIdx.x; e < count; e += kThreads) {
        const int i = e / g.w, j = e - i * g.w;
        const double vl = la[base + e], vp = pr[base + e];
#pragma unroll
        for (int a = 0; a < kR; ++a)
#pragma unroll
            for (int b = 0; b < kR; ++b) {
                const bool in = i - a >= 0 && i - a < g.nh && j - b >= 0 && j - b < g.nw;
                sl[a * kR + b] += in ? vl : 0.0;
                sp[a * kR + b] += in ? vp : 0.0;
            }
    }
    const double count_pos = static_cast<double>(g.P);
#pragma unroll
    for (int k = 0; k < kD; ++k) {
        const double tl = block_sum_reusing(sl[k], red), tp = block_sum_reusing(sp[k], red);
        if (threadIdx.x == 0) {
            means[static_cast<int64_t>(blockIdx.x) * 2 * kD + k] = tl / count_pos;
            means[static_cast<int64_t>(blockIdx.x) * 2 * kD + kD + k] = tp / count_pos;
        }
    }
}

// the centred products: workgroup (nc, chunk) = blockIdx.x, lane e < 243 owns entry (m, k, q) and walks the chunk's positions in
// order.  m = 0: la_cov, 1: pr_cov, 2: la_pr_cov.  The maps are small and stay in the caches: every lane of a wave reads one of
// at most 9 neighbouring addresses per map.  part[(nc nchunks + chunk) 243 + e]
__global__ __launch_bounds__(kThreads) void rmi_moment_kernel(const float *__restrict__ la, const float *__restrict__ pr,
                                                              const double *__restrict__ means, double *__restrict__ part, Geom g) {
    const int e = threadIdx.x;
    if (e >= kEntries) return;
    const int nc = blockIdx.x / g.nchunks, chunk = blockIdx.x - nc * g.nchunks;
    const int m = e / (kD * kD), k = (e / kD) % kD, q = e % kD;
    const int64_t base = static_cast<int64_t>(nc) * g.h * g.w;
    const float *A = (m == 1 ? pr : la) + base + (k / kR) * g.w + (k % kR);
    const float *B = (m == 0 ? la : pr) + base + (q / kR) * g.w + (q % kR);
    const double ma = means[static_cast<int64_t>(nc) * 2 * kD + (m == 1 ? kD : 0) + k];
    const double mb = means[static_cast<int64_t>(nc) * 2 * kD + (m == 0 ? 0 : kD) + q];
    const int p0 = chunk * kPosChunk, p1 = min(g.P, p0 + kPosChunk);
    int pi = p0 / g.nw, pj = p0 - pi * g.nw;
    int off = pi * g.w + pj;
    double acc = 0.0;
#pragma unroll 8
    for (int pos = p0; pos < p1; ++pos) {
        acc += (static_cast<double>(A[off]) - ma) * (static_cast<double>(B[off]) - mb);
        ++off;
        if (++pj == g.nw) {
            pj = 0;
            off += g.w - g.nw;
        }
    }
    part[static_cast<int64_t>(blockIdx.x) * kEntries + e] = acc;
}

// the chunks of one (n, c) in index order; cov = [la_cov, pr_cov, la_pr_cov], each (N C, 9, 9)
__global__ __launch_bounds__(kThreads) void rmi_moment_fold_kernel(const double *__restrict__ part, double *__restrict__ la_cov,
                                                                   double *__restrict__ pr_cov, double *__restrict__ lp_cov, Geom g) {
    const int e = threadIdx.x;
    if (e >= kEntries) return;
    const double *src = part + static_cast<int64_t>(blockIdx.x) * g.nchunks * kEntries + e;
    double acc = 0.0;
    for (int c = 0; c < g.nchunks; ++c) acc += src[static_cast<int64_t>(c) * kEntries];
    const int m = e / (kD * kD), r = e % (kD * kD);
    (m == 0 ? la_cov : m == 1 ? pr_cov : lp_cov)[static_cast<int64_t>(blockIdx.x) * kD * kD + r] = acc;
}

// ---- backward -------------------------------------------------------------------------------------------------------
// grid (nblk, ncg, N), the front end's layout.  Per class a lane gathers its cell's share of dloss/d(pooled probability)
//   g_pool[i, j] = sum_{k = (a,b), (i-a, j-b) a position} sum_q (G_pr + G_pr^T)[k,q] Pr[q, pos] + G_lp[q,k] L[q, pos]
// from the 5 x 5 neighbourhood of both maps (float64; the matrices and means are read with wave-uniform addresses), then
//   grad_x = valid ? s (1 - s) g_pool / p^2 + g_bce / (n_valid + 1) (s - o) : 0
// for its pixels.  The centred rows sum to zero, so the mean subtraction adds no term.  Every element is written once.
template <bool kPair>
__global__ __launch_bounds__(kThreads) void rmi_bwd_kernel(const float *__restrict__ x, const int64_t *__restrict__ t,
                                                           const float *__restrict__ state, const float *__restrict__ la,
                                                           const float *__restrict__ pr, const double *__restrict__ means,
                                                           const float *__restrict__ g_bce, const double *__restrict__ G_pr,
                                                           const double *__restrict__ G_lp, float *__restrict__ gx, Geom g, int do_rmi) {
    __shared__ short codes[kMaxPool * kMaxPool * kThreads];
    const int cell = blockIdx.x * kThreads + threadIdx.x, n = blockIdx.z;
    const bool live = cell < g.he * g.we;
    const int i = cell / g.we, j = cell - i * g.we;
    const int y0 = i * g.p - g.pad, x0 = j * g.p - g.pad;
    const int64_t HW = static_cast<int64_t>(g.H) * g.W;
    classify_cell<kPair>(t + n * HW, codes, g, live, y0, x0);
    if (!live) return;
    const bool pooled = do_rmi && i < g.h && j < g.w;
    const float cb = g_bce[0] * state[2];
    const double div = static_cast<double>(g.p * g.p);
    const int c_end = min(g.C, (static_cast<int>(blockIdx.y) + 1) * kClassGroup);
    for (int c = blockIdx.y * kClassGroup; c < c_end; ++c) {
        const int64_t nc = static_cast<int64_t>(n) * g.C + c;
        double gp = 0.0;
        if (pooled) {
            const float *ml = la + nc * g.h * g.w, *mp = pr + nc * g.h * g.w;
            float nl[25], np[25];
#pragma unroll
            for (int u = 0; u < 5; ++u)
#pragma unroll
                for (int v = 0; v < 5; ++v) {
                    const int yy = i - 2 + u, xx = j - 2 + v;
                    const bool in = yy >= 0 && yy < g.h && xx >= 0 && xx < g.w;
                    nl[u * 5 + v] = in ? ml[yy * g.w + xx] : 0.f;
                    np[u * 5 + v] = in ? mp[yy * g.w + xx] : 0.f;
                }
            const double *gpr = G_pr + nc * kD * kD, *glp = G_lp + nc * kD * kD, *mean = means + nc * 2 * kD;
#pragma unroll
            for (int a = 0; a < kR; ++a)
#pragma unroll
                for (int b = 0; b < kR; ++b) {
                    const int k = a * kR + b;
                    const bool pos = i - a >= 0 && i - a < g.nh && j - b >= 0 && j - b < g.nw;
                    double acc = 0.0;
#pragma unroll
                    for (int qa = 0; qa < kR; ++qa)
#pragma unroll
                        for (int qb = 0; qb < kR; ++qb) {
                            const int q = qa * kR + qb, idx = (2 - a + qa) * 5 + (2 - b + qb);
                            acc += (gpr[k * kD + q] + gpr[q * kD + k]) * (static_cast<double>(np[idx]) - mean[kD + q]);
                            acc += glp[q * kD + k] * (static_cast<double>(nl[idx]) - mean[q]);
                        }
                    gp += pos ? acc : 0.0;
                }
        }
        const float gcell = static_cast<float>(gp / div);
        const float *plane = x + nc * HW;
        float *gplane = gx + nc * HW;
        for (int dy = 0; dy < g.p; ++dy) {
            const int64_t ro = static_cast<int64_t>(y0 + dy) * g.W;
            for (int dx = 0; dx < g.p; dx += 2) {
                const int k = dy * g.p + dx;
                const short c0 = codes[k * kThreads + threadIdx.x];
                const short c1 = dx + 1 < g.p ? codes[(k + 1) * kThreads + threadIdx.x] : static_cast<short>(-2);
                float v0, v1, s0, s1, b0, b1;
                load2<kPair>(plane + ro, x0 + dx, c0, c1, v0, v1);
                sigmoid_bce(v0, false, s0, b0);
                sigmoid_bce(v1, false, s1, b1);
                const float r0 = c0 >= 0 ? (s0 * (1.f - s0)) * gcell + cb * (s0 - (c0 == c ? 1.f : 0.f)) : 0.f;
                const float r1 = c1 >= 0 ? (s1 * (1.f - s1)) * gcell + cb * (s1 - (c1 == c ? 1.f : 0.f)) : 0.f;
                if constexpr (kPair) {
                    if (c0 != -2) *reinterpret_cast<float2 *>(gplane + ro + x0 + dx) = make_float2(r0, r1);
                } else {
                    if (c0 != -2) gplane[ro + x0 + dx] = r0;
                    if (c1 != -2) gplane[ro + x0 + dx + 1] = r1;
                }
            }
        }
    }
}

inline bool pair_route(const Geom &g, const void *x, const void *t, const void *gx) {
    return (g.p == 4 || g.p == 8) && g.W % 2 == 0 && (reinterpret_cast<uintptr_t>(x) & 7) == 0 &&
           (reinterpret_cast<uintptr_t>(gx) & 7) == 0 && (reinterpret_cast<uintptr_t>(t) & 15) == 0;
}

inline int64_t bce_parts(const Geom &g) { return static_cast<int64_t>(g.N) * g.ncg * g.nblk; }

}  // namespace

// ---- host side ------------------------------------------------------------------------------------------------------
int rmi_max_pool() { return kMaxPool; }

bool rmi_pooled_size(int H, int W, int pool, int *h, int *w) {
    const Geom g = make_geom(1, 1, H, W, pool);
    *h = g.h;
    *w = g.w;
    return g.h >= kR && g.w >= kR;
}

int64_t rmi_moment_workgroups(int B, int C, int H, int W, int pool) {
    return static_cast<int64_t>(B) * C * make_geom(B, C, H, W, pool).nchunks;
}

// float64: a BCE and a count partial per front-end workgroup, then 243 partial products per moment workgroup
int64_t rmi_workspace_bytes(int B, int C, int H, int W, int pool) {
    const Geom g = make_geom(B, C, H, W, pool);
    return 8 * (2 * bce_parts(g) + static_cast<int64_t>(B) * C * g.nchunks * kEntries);
}

int rmi_forward(const void *logits, const void *target, void *bce, void *state, void *la_map, void *pr_map, void *means, void *la_cov,
                void *pr_cov, void *la_pr_cov, void *workspace, int B, int C, int H, int W, int pool, int do_rmi, hipStream_t s) {
    const Geom g = make_geom(B, C, H, W, pool);
    const float *x = static_cast<const float *>(logits);
    const int64_t *t = static_cast<const int64_t *>(target);
    float *la = static_cast<float *>(la_map), *pr = static_cast<float *>(pr_map);
    double *pbce = static_cast<double *>(workspace), *pcnt = pbce + bce_parts(g), *part = pcnt + bce_parts(g);
    const dim3 grid(g.nblk, g.ncg, g.N);
    if (pair_route(g, x, t, nullptr))
        rmi_front_kernel<true><<<grid, kThreads, 0, s>>>(x, t, la, pr, pbce, pcnt, g, do_rmi);
    else
        rmi_front_kernel<false><<<grid, kThreads, 0, s>>>(x, t, la, pr, pbce, pcnt, g, do_rmi);
    int rc = launch_status();
    if (rc) return rc;
    rmi_bce_final_kernel<<<1, kThreads, 0, s>>>(pbce, pcnt, bce_parts(g), static_cast<float *>(bce), static_cast<float *>(state));
    rc = launch_status();
    if (rc || !do_rmi) return rc;
    double *mean = static_cast<double *>(means);
    rmi_mean_kernel<<<B * C, kThreads, 0, s>>>(la, pr, mean, g);
    rc = launch_status();
    if (rc) return rc;
    rmi_moment_kernel<<<B * C * g.nchunks, kThreads, 0, s>>>(la, pr, mean, part, g);
    rc = launch_status();
    if (rc) return rc;
    rmi_moment_fold_kernel<<<B * C, kThreads, 0, s>>>(part, static_cast<double *>(la_cov), static_cast<double *>(pr_cov),
                                                     static_cast<double *>(la_pr_cov), g);
    return launch_status();
}

int rmi_backward(const void *logits, const void *target, const void *state, const void *la_map, const void *pr_map, const void *means,
                 const void *grad_bce, const void *grad_pr_cov, const void *grad_la_pr_cov, void *grad_logits, int B, int C, int H,
                 int W, int pool, int do_rmi, hipStream_t s) {
    const Geom g = make_geom(B, C, H, W, pool);
    const float *x = static_cast<const float *>(logits);
    const int64_t *t = static_cast<const int64_t *>(target);
    float *gx = static_cast<float *>(grad_logits);
    const dim3 grid(g.nblk, g.ncg, g.N);
    const auto kern = pair_route(g, x, t, gx) ? rmi_bwd_kernel<true> : rmi_bwd_kernel<false>;
    kern<<<grid, kThreads, 0, s>>>(x, t, static_cast<const float *>(state), static_cast<const float *>(la_map),
                                   static_cast<const float *>(pr_map), static_cast<const double *>(means),
                                   static_cast<const float *>(grad_bce), static_cast<const double *>(grad_pr_cov),
                                   static_cast<const double *>(grad_la_pr_cov), gx, g, do_rmi);
    return launch_status();
}

}  // namespace cerb
