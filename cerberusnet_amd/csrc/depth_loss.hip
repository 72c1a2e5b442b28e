// depth_loss.hip -- the supervised depth loss InvHuberLoss (berHu) as ONE differentiable scalar op, fp32.
//
// Reference (nnet_training/loss_functions/depth_losses.py:64-88, without `weight`): relu, sub, the mask as a product, abs,
// max, pow, add, div, two compares, two casts, two products, add, mean -- about 18 launches over a (B,h,w) map forward and as
// many backward.  Here: two passes over prediction and ground truth and a one-workgroup finish forward, one launch backward.
//
//   valid = g > 0                  d = max(p, 0) - g            err = valid ? |d| : 0
//   m = max over all pixels of err        c = 0.2 m              N = B h w (ALL pixels, as the reference's mean)
//   term = err > c ? (d d + c c) / (2 c) : err                  loss = sum(term) / N
//   S    = sum over {err > c} of (1/2 - d d / (2 c c))          ties = #{err == m}
//   dloss/dp = [valid and p > 0] ((err > c ? d / c : sign(d)) + [err == m] 0.2 S / ties sign(d)) / N
// The cutoff c depends on the data and carries a gradient: the second summand is what autograd sends through err.max() into
// the pixel(s) that hold the maximum (split evenly over ties, as Tensor.max()'s backward does).
//
// The ground truth may be finer than the prediction by integer ratios (a pyramid level): pixel (y, x) then reads
// gt[b, y * (H / h), x * (W / w)], which is the pixel F.interpolate(mode='nearest') picks -- no resized map is written.
//
// Forward: (1) a max pass of at most 1024 workgroups, each walking its 1024-pixel chunks and leaving ONE partial maximum (the
// bit pattern of a non-negative float orders as an unsigned integer, and a NaN sorts above infinity, so an integer max
// propagates NaN as torch.max does and does not depend on any order); (2) a sum pass, one chunk per workgroup, that folds the
// partial maxima itself (4 KB, from L2) and leaves a partial of sum(term), of S and of ties; (3) one workgroup that adds the
// partials in a fixed order and leaves the loss and state = [c, 0.2 S / ties, 1 / N, m] for the backward.  No atomics of any
// kind, nothing to zero, no workgroup waits for another one, no host round trip: the same bits on every run and in a
// replayed graph.
//
// Two routes, as in seg_loss.hip.  Both give a workgroup the SAME 1024 consecutive pixels, run the same per-pixel arithmetic
// (contraction into fma is off in this file) and fold them in the same order -- four consecutive pixels left to right, the 64
// groups of a wave by a butterfly, the 4 waves in wave order: a call on misaligned pointers gives the bits of the aligned one.
//   vector : h*w % 4 == 0, 16-byte aligned pointers, no gather: a lane owns 4 consecutive pixels, one 16-byte load each of
//            prediction and ground truth
//   scalar : everything else, every gather included: a lane owns one pixel at a time, four times; the per-pixel terms go
//            through LDS to the lane that folds them
//
// Corners are decided by selection, never by a product with a mask: an invalid pixel (g <= 0 or g NaN) adds nothing whatever
// its prediction holds (NaN, 1e30) and gets the gradient 0.0f; a NaN at a valid pixel makes the loss NaN; c == 0 (no valid
// pixel, or every valid pixel exact) gives the loss 0.0f and a gradient of zeros, where the reference divides by 2 c and
// returns NaN; p <= 0 gets the gradient 0 (relu'(0) = 0) and sign(0) = 0.
#include "common.h"
#include "loss_reduce.h"

#pragma clang fp contract(off)

namespace cerb {
namespace {

constexpr int kThreads = kReduceThreads;
constexpr int kQuad = 4;                      // consecutive pixels folded first (the vector route's pixels per lane)
constexpr int kChunk = kThreads * kQuad;      // pixels per workgroup and step, both routes
constexpr int kMaxParts = kThreads * kQuad;   // partial maxima: one 16-byte load per lane of the sum pass folds them all

// where the pixels of a call lie: N = B*hw pixels of the prediction; ry, rx = the ground truth's integer ratios
struct Geom {
    int N, hw, w;
    int ry, rx;
    int64_t HW;     // pixels of one ground-truth item
    int W;
};

// the ground truth of prediction pixel p under a gather (any ratio >= 1; 64-bit: B*H*W may pass 2^31)
__device__ __forceinline__ float gather_gt(const float *__restrict__ gt, const Geom &q, int p) {
    const int b = p / q.hw, r = p - b * q.hw;
    const int y = r / q.w, x = r - y * q.w;
    return gt[static_cast<int64_t>(b) * q.HW + static_cast<int64_t>(y) * q.ry * q.W + static_cast<int64_t>(x) * q.rx];
}

// ---- per-pixel arithmetic, shared by every kernel and both routes ---------------------------------------------------
struct Pixel {
    float d;        // max(p, 0) - g; NaN for a NaN p
    float err;      // |d| at a valid pixel, else 0; non-negative or a positive NaN
    bool valid;
};

__device__ __forceinline__ Pixel pixel(float p, float g) {
    Pixel px;
    px.valid = g > 0.f;                              // false for a NaN g
    px.d = (p <= 0.f ? 0.f : p) - g;                 // relu that keeps a NaN, as torch.relu
    px.err = px.valid ? fabsf(px.d) : 0.f;           // a select: what an invalid pixel holds never counts
    return px;
}

__device__ __forceinline__ float sign_of(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// what a pixel adds to sum(term), to S and to ties
__device__ __forceinline__ void pixel_terms(const Pixel &px, float c, float m, float &term, float &s, unsigned &tie) {
    const bool quad = px.err > c;                    // false for a NaN err or a NaN c: the NaN err itself is added
    const float dd = px.d * px.d;
    term = quad ? (dd + c * c) / (2.f * c) : px.err;
    s = quad ? 0.5f - dd / ((2.f * c) * c) : 0.f;
    tie = px.err == m ? 1u : 0u;
}

__device__ __forceinline__ float pixel_grad(float p, float g, float c, float m, float share, float coef) {
    const Pixel px = pixel(p, g);
    const float sg = sign_of(px.d);
    const float slope = px.err > c ? px.d / c : sg;
    const float through_max = px.err == m ? share * sg : 0.f;
    const float v = coef * (slope + through_max);
    return (px.valid && p > 0.f && c != 0.f) ? v : 0.f;          // a select: a NaN coefficient still leaves 0.0f
}

// ---- folds of non-negative floats as unsigned integers -----------------------------------------------------------------
__device__ __forceinline__ unsigned err_bits(float err) { return __float_as_uint(err); }   // err >= 0 or a positive NaN

// the maximum of the max pass's partials, in every thread
__device__ __forceinline__ unsigned fold_parts(const unsigned *__restrict__ pmax, int nparts, unsigned *red) {
    unsigned v = 0u;
    const int i0 = threadIdx.x * kQuad;
    if (i0 + kQuad <= nparts) {
        const uint4 q = *reinterpret_cast<const uint4 *>(pmax + i0);
        v = max(max(q.x, q.y), max(q.z, q.w));
    } else {
        for (int i = i0; i < nparts; ++i) v = max(v, pmax[i]);
    }
    return block_max(v, red);
}

// ---- forward, pass 1: the maximum ------------------------------------------------------------------------------------
template <bool kVec, bool kGather>
__global__ __launch_bounds__(kThreads) void inv_huber_max_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                                 unsigned *__restrict__ pmax, Geom q, int nchunks) {
    __shared__ unsigned red[4];
    unsigned v = 0u;
    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int base = ch * kChunk;
        if constexpr (kVec) {
            const int p0 = base + threadIdx.x * kQuad;
            if (p0 < q.N) {      // N % 4 == 0 on this route: a lane's 4 pixels are all inside
                const float4 a = *reinterpret_cast<const float4 *>(pred + p0), b = *reinterpret_cast<const float4 *>(gt + p0);
                v = max(v, max(max(err_bits(pixel(a.x, b.x).err), err_bits(pixel(a.y, b.y).err)),
                               max(err_bits(pixel(a.z, b.z).err), err_bits(pixel(a.w, b.w).err))));
            }
        } else {
#pragma unroll
            for (int j = 0; j < kQuad; ++j) {
                const int p = base + j * kThreads + threadIdx.x;
                if (p < q.N) v = max(v, err_bits(pixel(pred[p], kGather ? gather_gt(gt, q, p) : gt[p]).err));
            }
        }
    }
    const unsigned t = block_max(v, red);
    if (threadIdx.x == 0) pmax[blockIdx.x] = t;
}

// ---- forward, pass 2: the sums ---------------------------------------------------------------------------------------
template <bool kVec, bool kGather>
__global__ __launch_bounds__(kThreads) void inv_huber_sum_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                                 const unsigned *__restrict__ pmax, int nparts,
                                                                 float *__restrict__ psum, float *__restrict__ ps,
                                                                 unsigned *__restrict__ pties, Geom q) {
    __shared__ unsigned red_m[4], red_t[4];
    __shared__ float red_a[4], red_s[4];
    __shared__ float stage[kVec ? 2 : 2 * kChunk];
    const float m = __uint_as_float(fold_parts(pmax, nparts, red_m));
    const float c = 0.2f * m;
    const int base = blockIdx.x * kChunk;
    float t4[kQuad], s4[kQuad];
    unsigned ties = 0u;
    if constexpr (kVec) {
        const int p0 = base + threadIdx.x * kQuad;
#pragma unroll
        for (int k = 0; k < kQuad; ++k) t4[k] = s4[k] = 0.f;
        if (p0 < q.N) {
            const float4 a = *reinterpret_cast<const float4 *>(pred + p0), b = *reinterpret_cast<const float4 *>(gt + p0);
            const float pp[kQuad] = {a.x, a.y, a.z, a.w}, gg[kQuad] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int k = 0; k < kQuad; ++k) {
                unsigned tie;
                pixel_terms(pixel(pp[k], gg[k]), c, m, t4[k], s4[k], tie);
                ties += tie;
            }
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < kQuad; ++j) {
            const int i = j * kThreads + threadIdx.x, p = base + i;
            float term = 0.f, s = 0.f;
            if (p < q.N) {
                unsigned tie;
                pixel_terms(pixel(pred[p], kGather ? gather_gt(gt, q, p) : gt[p]), c, m, term, s, tie);
                ties += tie;                         // an integer count: any order
            }
            stage[i] = term;
            stage[kChunk + i] = s;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            t4[k] = stage[threadIdx.x * kQuad + k];
            s4[k] = stage[kChunk + threadIdx.x * kQuad + k];
        }
    }
    const float a = quad_sum(t4), s = quad_sum(s4);
    const float ta = block_sum(a, red_a), ts = block_sum(s, red_s);
    const unsigned tt = block_sum(ties, red_t);
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = ta;
        ps[blockIdx.x] = ts;
        pties[blockIdx.x] = tt;
    }
}

// ---- forward, the finish: one workgroup, fixed order ----------------------------------------------------------------------
// loss[0] and state = [c, 0.2 S / ties, 1 / N, m]
__global__ __launch_bounds__(kThreads) void inv_huber_final_kernel(const unsigned *__restrict__ pmax, int nparts,
                                                                   const float *__restrict__ psum, const float *__restrict__ ps,
                                                                   const unsigned *__restrict__ pties, int n, int N,
                                                                   float *__restrict__ loss, float *__restrict__ state) {
    __shared__ unsigned red_m[4];
    __shared__ float red[2][kThreads];
    __shared__ unsigned red_t[kThreads];
    const float m = __uint_as_float(fold_parts(pmax, nparts, red_m));
    float a = 0.f, b = 0.f;
    unsigned t = 0u;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        a += psum[i];
        b += ps[i];
        t += pties[i];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    red_t[threadIdx.x] = t;
    tree_sum(red, red_t);
    if (threadIdx.x == 0) {
        const float c = 0.2f * m, count = static_cast<float>(N);
        const bool flat = c == 0.f;                  // no valid pixel, or every valid pixel exact: the limit, not 0 / 0
        loss[0] = flat ? 0.f : red[0][0] / count;
        state[0] = c;
        state[1] = flat ? 0.f : (0.2f * red[1][0]) / static_cast<float>(red_t[0]);
        state[2] = 1.f / count;
        state[3] = m;
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------
template <bool kVec, bool kGather>
__global__ __launch_bounds__(kThreads) void inv_huber_bwd_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                                 const float *__restrict__ state, const float *__restrict__ grad_loss,
                                                                 float *__restrict__ gp, Geom q) {
    // read here, from device memory: no host synchronisation.  Scaling by a power of two is exact in both products: the
    // gradient is exactly linear in such an upstream gradient.
    const float c = state[0], share = state[1], m = state[3];
    const float coef = grad_loss[0] * state[2];
    const int base = blockIdx.x * kChunk;
    if constexpr (kVec) {
        const int p0 = base + threadIdx.x * kQuad;
        if (p0 >= q.N) return;
        const float4 a = *reinterpret_cast<const float4 *>(pred + p0), b = *reinterpret_cast<const float4 *>(gt + p0);
        *reinterpret_cast<float4 *>(gp + p0) = make_float4(pixel_grad(a.x, b.x, c, m, share, coef), pixel_grad(a.y, b.y, c, m, share, coef),
                                                           pixel_grad(a.z, b.z, c, m, share, coef), pixel_grad(a.w, b.w, c, m, share, coef));
    } else {
#pragma unroll
        for (int j = 0; j < kQuad; ++j) {
            const int p = base + j * kThreads + threadIdx.x;
            if (p >= q.N) return;
            gp[p] = pixel_grad(pred[p], kGather ? gather_gt(gt, q, p) : gt[p], c, m, share, coef);
        }
    }
}

inline int chunks(int64_t n) { return static_cast<int>((n + kChunk - 1) / kChunk); }

inline bool aligned16(const void *a, const void *b, const void *c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

inline Geom geom(int B, int h, int w, int H, int W) {
    Geom q;
    q.hw = h * w;
    q.N = B * q.hw;
    q.w = w;
    q.ry = H / h;
    q.rx = W / w;
    q.HW = static_cast<int64_t>(H) * W;
    q.W = W;
    return q;
}

// 0: vector, 1: scalar, 2: scalar with the pyramid gather
inline int route(const Geom &q, int h, int H, int W, const void *a, const void *b, const void *c = nullptr) {
    if (h != H || q.w != W) return 2;
    return (q.hw % kQuad == 0 && aligned16(a, b, c)) ? 0 : 1;
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------------------------------
int64_t inv_huber_workspace_bytes(int B, int h, int w) {
    // the partial maxima, then a partial of sum(term), of S and of ties per 1024 pixels
    return (kMaxParts + 3 * static_cast<int64_t>(chunks(static_cast<int64_t>(B) * h * w))) * 4;
}

int inv_huber_forward(const void *pred, const void *gt, void *loss, void *state, void *workspace, int B, int h, int w, int H, int W,
                      hipStream_t s) {
    const float *p = static_cast<const float *>(pred), *g = static_cast<const float *>(gt);
    const Geom q = geom(B, h, w, H, W);
    const int nblocks = chunks(q.N), nparts = std::min(nblocks, kMaxParts);
    unsigned *pmax = static_cast<unsigned *>(workspace);
    float *psum = reinterpret_cast<float *>(pmax + kMaxParts), *ps = psum + nblocks;
    unsigned *pties = reinterpret_cast<unsigned *>(ps + nblocks);
    const int r = route(q, h, H, W, p, g);
    if (r == 0)
        inv_huber_max_kernel<true, false><<<nparts, kThreads, 0, s>>>(p, g, pmax, q, nblocks);
    else if (r == 1)
        inv_huber_max_kernel<false, false><<<nparts, kThreads, 0, s>>>(p, g, pmax, q, nblocks);
    else
        inv_huber_max_kernel<false, true><<<nparts, kThreads, 0, s>>>(p, g, pmax, q, nblocks);
    int rc = launch_status();
    if (rc) return rc;
    if (r == 0)
        inv_huber_sum_kernel<true, false><<<nblocks, kThreads, 0, s>>>(p, g, pmax, nparts, psum, ps, pties, q);
    else if (r == 1)
        inv_huber_sum_kernel<false, false><<<nblocks, kThreads, 0, s>>>(p, g, pmax, nparts, psum, ps, pties, q);
    else
        inv_huber_sum_kernel<false, true><<<nblocks, kThreads, 0, s>>>(p, g, pmax, nparts, psum, ps, pties, q);
    rc = launch_status();
    if (rc) return rc;
    inv_huber_final_kernel<<<1, kThreads, 0, s>>>(pmax, nparts, psum, ps, pties, nblocks, q.N, static_cast<float *>(loss),
                                                  static_cast<float *>(state));
    return launch_status();
}

int inv_huber_backward(const void *pred, const void *gt, const void *state, const void *grad_loss, void *grad_pred, int B, int h, int w,
                       int H, int W, hipStream_t s) {
    const float *p = static_cast<const float *>(pred), *g = static_cast<const float *>(gt);
    const float *st = static_cast<const float *>(state), *gl = static_cast<const float *>(grad_loss);
    float *gp = static_cast<float *>(grad_pred);
    const Geom q = geom(B, h, w, H, W);
    const int nblocks = chunks(q.N);
    const int r = route(q, h, H, W, p, g, gp);
    if (r == 0)
        inv_huber_bwd_kernel<true, false><<<nblocks, kThreads, 0, s>>>(p, g, st, gl, gp, q);
    else if (r == 1)
        inv_huber_bwd_kernel<false, false><<<nblocks, kThreads, 0, s>>>(p, g, st, gl, gp, q);
    else
        inv_huber_bwd_kernel<false, true><<<nblocks, kThreads, 0, s>>>(p, g, st, gl, gp, q);
    return launch_status();
}

}  // namespace cerb
