// metrics.hip -- the per-image statistics of the training metrics, forward only, fp32 inputs: what the
// reference's metric loggers (nnet_training/statistics/semantic.py, depth.py, optical_flow.py) compute from the model's outputs
// after every step, as a single read of those outputs and a handful of numbers per image.
//
//   seg_confusion     : logits (B,C,H,W), labels (B,H,W) int64 -> (B,C,C) int64, [b, t, p] = the pixels of image b with label t
//                       and argmax_c logits = p (semantic.py:41-48, :190-194: argmax, two casts, a boolean-mask index, bincount)
//   depth_metric_sums : pred, gt (B,h,w) -> five float64 sums and four int64 counts per image (depth.py:35-78: ~40 launches)
//   flow_metric_sums  : flow_pred, flow_gt (B,2,H,W), mask (B,H,W) -> two float64 sums and one int64 count per image
//                       (optical_flow.py:28-37, :53-63)
//   warp_sad          : image, source (B,C,H,W), flow (B,2,H,W) -> sum |image - flow_warp(source, flow)| per image, float64; the
//                       warped image is never stored (optical_flow.py:68-70)
//
// One shape for all four: a workgroup of 256 lanes owns 1024 consecutive pixels of ONE image (grid.y = the image), a lane owns
// 4 consecutive pixels of them.  Two routes, chosen from the shape and the pointers:
//   vector : H*W % 4 == 0 and 16-byte aligned pointers: one 16-byte load per lane and plane (two for int64 labels)
//   scalar : everything else: the same 4 pixels by four guarded 4-byte loads
// Only the loads differ: the per-pixel arithmetic (contraction into fma is off in this file), the lane's left-to-right fold
// of its 4 pixels, the butterfly over a wave and the wave-order fold of the 4 waves are one piece of code, so a call on
// misaligned pointers gives the bits of the aligned one.
//
// Floating-point terms are computed in fp32 exactly as the reference's element-wise ops and ACCUMULATED in float64 from the
// lane upward.  A workgroup leaves one partial per sum and count in the workspace; a second launch of one workgroup per image
// adds them in a fixed order.  No floating-point atomics, nothing to zero, no host round trip: the same bits on every run and
// in a replayed graph.  The confusion matrix is integers: 32-bit LDS bins per workgroup (C*C <= 4096 of them), equal (t,p) pairs
// of a lane's 4 pixels combined before the LDS add, one 64-bit global add per non-empty bin into a matrix that the launch
// function zeroes on the stream with a kernel node of its own -- any order gives the same matrix.
//
// Corners are decided by selection, never by a product with a mask: an invalid depth pixel or an ignored label adds nothing
// whatever the prediction holds there.  Labels never form an address unless they lie in [0, C).
#include "warp_common.h"
#include "loss_reduce.h"

#pragma clang fp contract(off)

namespace cerb {
namespace {

constexpr int kThreads = kReduceThreads;
constexpr int kQuad = 4;                      // consecutive pixels per lane
constexpr int kChunk = kThreads * kQuad;      // pixels per workgroup and step
constexpr int kConfMaxClasses = 64;           // C*C 32-bit LDS bins: 16 KiB
constexpr int kConfGroupsPerImage = 256;      // workgroups per image of seg_confusion; each walks its chunks by a stride

// ---- a lane's 4 consecutive pixels of one plane --------------------------------------------------------------------------
// p0 = the first pixel's index in the plane, hw = pixels of the plane; pixels at or past hw read as `fill`
template <bool kVec>
__device__ __forceinline__ void load_quad(const float *__restrict__ plane, int p0, int hw, float fill, float (&v)[kQuad]) {
    if constexpr (kVec) {      // hw % 4 == 0 on this route: all inside or all outside
        if (p0 < hw) {
            const float4 q = *reinterpret_cast<const float4 *>(plane + p0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = v[1] = v[2] = v[3] = fill;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kQuad; ++k) v[k] = p0 + k < hw ? plane[p0 + k] : fill;
    }
}

template <bool kVec>
__device__ __forceinline__ void load_quad_labels(const int64_t *__restrict__ t, int p0, int hw, int64_t fill, int64_t (&v)[kQuad]) {
    if constexpr (kVec) {
        if (p0 < hw) {
            const longlong2 a = *reinterpret_cast<const longlong2 *>(t + p0), b = *reinterpret_cast<const longlong2 *>(t + p0 + 2);
            v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
        } else {
            v[0] = v[1] = v[2] = v[3] = fill;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kQuad; ++k) v[k] = p0 + k < hw ? t[p0 + k] : fill;
    }
}

// ---- float64 folds in a fixed order (loss_reduce.h) ------------------------------------------------------------------------
// the workgroup's partials of NS sums and NC counts, left at slot `slot` of the workspace by thread 0: block_sum's pieces,
// with one barrier for all of them
template <int NS, int NC>
__device__ __forceinline__ void leave_partials(const double (&s)[NS], const unsigned *c, double *__restrict__ psum,
                                               unsigned *__restrict__ pcnt, int64_t slot) {
    __shared__ double red_s[NS][4];
    __shared__ unsigned red_c[NC > 0 ? NC : 1][4];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const double v = wave_sum(s[i]);
        if ((threadIdx.x & 63) == 0) red_s[i][wave] = v;
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const unsigned v = wave_sum(c[i]);
        if ((threadIdx.x & 63) == 0) red_c[i][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) psum[slot * NS + i] = waves_fold<FoldSum>(red_s[i]);
#pragma unroll
        for (int i = 0; i < NC; ++i) pcnt[slot * NC + i] = waves_fold<FoldSum>(red_c[i]);
    }
}

// ---- the second launch: one workgroup per image, fixed order -----------------------------------------------------------------
// sums[b][NS] and counts[b][NC] from the n partials of image b
template <int NS, int NC>
__global__ __launch_bounds__(kThreads) void metric_finish_kernel(const double *__restrict__ psum, const unsigned *__restrict__ pcnt, int n,
                                                                 double *__restrict__ sums, long long *__restrict__ counts) {
    __shared__ double red_s[NS][kThreads];
    __shared__ long long red_c[NC > 0 ? NC : 1][kThreads];
    const int64_t first = static_cast<int64_t>(blockIdx.x) * n;
    double s[NS];
    long long c[NC > 0 ? NC : 1];
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NC; ++i) c[i] = 0;
    for (int j = threadIdx.x; j < n; j += kThreads) {
#pragma unroll
        for (int i = 0; i < NS; ++i) s[i] += psum[(first + j) * NS + i];
#pragma unroll
        for (int i = 0; i < NC; ++i) c[i] += pcnt[(first + j) * NC + i];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) red_s[i][threadIdx.x] = s[i];
#pragma unroll
    for (int i = 0; i < NC; ++i) red_c[i][threadIdx.x] = c[i];
    if constexpr (NC > 0)
        tree_sum(red_s, red_c);
    else
        tree_sum(red_s);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) sums[static_cast<int64_t>(blockIdx.x) * NS + i] = red_s[i][0];
#pragma unroll
        for (int i = 0; i < NC; ++i) counts[static_cast<int64_t>(blockIdx.x) * NC + i] = red_c[i][0];
    }
}

// ---- (a) the confusion matrix ------------------------------------------------------------------------------------------------
// torch.argmax's rule, streamed: the first maximal class wins; a NaN counts as the maximum and the first NaN wins
__device__ __forceinline__ void argmax_step(float v, int c, float &best, int &idx) {
    const bool take = v > best || (v != v && best == best);
    best = take ? v : best;
    idx = take ? c : idx;
}

__global__ __launch_bounds__(kThreads) void seg_confusion_zero_kernel(unsigned long long *__restrict__ conf, int64_t n) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) conf[i] = 0ull;
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void seg_confusion_kernel(const float *__restrict__ x, const int64_t *__restrict__ t,
                                                                 unsigned long long *__restrict__ conf, int C, int hw, int nchunks,
                                                                 int64_t ignore) {
    __shared__ unsigned int bins[kConfMaxClasses * kConfMaxClasses];
    const int nbins = C * C, b = blockIdx.y;
    for (int i = threadIdx.x; i < nbins; i += kThreads) bins[i] = 0u;
    __syncthreads();
    const float *xb = x + static_cast<int64_t>(b) * C * hw;
    const int64_t *tb = t + static_cast<int64_t>(b) * hw;
    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int p0 = ch * kChunk + threadIdx.x * kQuad;
        if (p0 >= hw) continue;
        int64_t lab[kQuad];
        load_quad_labels<kVec>(tb, p0, hw, ignore, lab);
        float best[kQuad];
        int idx[kQuad] = {0, 0, 0, 0};
        load_quad<kVec>(xb, p0, hw, 0.f, best);
#pragma unroll 4
        for (int c = 1; c < C; ++c) {
            float v[kQuad];
            load_quad<kVec>(xb + static_cast<int64_t>(c) * hw, p0, hw, 0.f, v);
#pragma unroll
            for (int k = 0; k < kQuad; ++k) argmax_step(v[k], c, best[k], idx[k]);
        }
        // the bin of each pixel, -1 where it does not count: ignored, out of range, or past the end of the image
        int bin[kQuad];
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            const bool in = lab[k] != ignore && static_cast<uint64_t>(lab[k]) < static_cast<uint64_t>(C) && p0 + k < hw;
            bin[k] = in ? static_cast<int>(lab[k]) * C + idx[k] : -1;
        }
        // neighbouring pixels mostly share a bin: equal bins of the lane's 4 pixels make one LDS add
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            if (bin[k] < 0) continue;
            unsigned n = 1u;
#pragma unroll
            for (int j = k + 1; j < kQuad; ++j) {
                const bool same = bin[j] == bin[k];
                n += same ? 1u : 0u;
                bin[j] = same ? -1 : bin[j];
            }
            atomicAdd(&bins[bin[k]], n);
        }
    }
    __syncthreads();
    unsigned long long *cb = conf + static_cast<int64_t>(b) * nbins;
    for (int i = threadIdx.x; i < nbins; i += kThreads) {
        const unsigned int v = bins[i];
        if (v) atomicAdd(&cb[i], static_cast<unsigned long long>(v));
    }
}

// ---- (b) the depth statistics ------------------------------------------------------------------------------------------------
// sums: |d|/g, d^2/g, d^2, l^2, |l|; counts: valid, r < 1.25, r < 1.25^2, r < 1.25^3 (depth.py:35-78)
template <bool kVec>
__global__ __launch_bounds__(kThreads) void depth_metric_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                                double *__restrict__ psum, unsigned *__restrict__ pcnt, int hw,
                                                                float min_depth, float max_depth) {
    const int b = blockIdx.y, p0 = blockIdx.x * kChunk + threadIdx.x * kQuad;
    const int64_t item = static_cast<int64_t>(b) * hw;
    float pp[kQuad], gg[kQuad];
    load_quad<kVec>(pred + item, p0, hw, 0.f, pp);
    load_quad<kVec>(gt + item, p0, hw, 0.f, gg);
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    unsigned c[4] = {0u, 0u, 0u, 0u};
    constexpr float kA1 = 1.25f, kA2 = 1.5625f, kA3 = 1.953125f;       // 1.25, 1.25^2, 1.25^3: exact in fp32
#pragma unroll
    for (int k = 0; k < kQuad; ++k) {
        const float g = gg[k];
        const bool valid = p0 + k < hw && g > min_depth && g < max_depth;      // false for a NaN g
        const float p = pp[k] == 0.f ? 1e-7f : pp[k];                          // out of place: the input is not written
        const float d = p - g;
        const float dd = d * d;
        const float l = logf(p) - logf(g);
        const float r = fmaxf(p / g, g / p);                                   // both NaN for a NaN p: no count
        s[0] += valid ? static_cast<double>(fabsf(d) / g) : 0.0;
        s[1] += valid ? static_cast<double>(dd / g) : 0.0;
        s[2] += valid ? static_cast<double>(dd) : 0.0;
        s[3] += valid ? static_cast<double>(l * l) : 0.0;
        s[4] += valid ? static_cast<double>(fabsf(l)) : 0.0;
        c[0] += valid ? 1u : 0u;
        c[1] += (valid && r < kA1) ? 1u : 0u;
        c[2] += (valid && r < kA2) ? 1u : 0u;
        c[3] += (valid && r < kA3) ? 1u : 0u;
    }
    leave_partials<5, 4>(s, c, psum, pcnt, static_cast<int64_t>(b) * gridDim.x + blockIdx.x);
}

// ---- (c) the flow statistics ---------------------------------------------------------------------------------------------------
// sums: epe * mask, mask; count: epe * mask > 3 and epe * mask / max(|gt|, 1e-10) > 0.05 (optical_flow.py:28-37, :53-63)
template <bool kVec>
__global__ __launch_bounds__(kThreads) void flow_metric_kernel(const float *__restrict__ fp, const float *__restrict__ fg,
                                                               const float *__restrict__ mask, double *__restrict__ psum,
                                                               unsigned *__restrict__ pcnt, int hw) {
    const int b = blockIdx.y, p0 = blockIdx.x * kChunk + threadIdx.x * kQuad;
    const int64_t item = static_cast<int64_t>(b) * 2 * hw;
    float px[kQuad], py[kQuad], gx[kQuad], gy[kQuad], m[kQuad];
    load_quad<kVec>(fp + item, p0, hw, 0.f, px);
    load_quad<kVec>(fp + item + hw, p0, hw, 0.f, py);
    load_quad<kVec>(fg + item, p0, hw, 0.f, gx);
    load_quad<kVec>(fg + item + hw, p0, hw, 0.f, gy);
    load_quad<kVec>(mask + static_cast<int64_t>(b) * hw, p0, hw, 0.f, m);
    double s[2] = {0.0, 0.0};
    unsigned c[1] = {0u};
#pragma unroll
    for (int k = 0; k < kQuad; ++k) {
        const bool in = p0 + k < hw;
        const float dx = px[k] - gx[k], dy = py[k] - gy[k];
        const float epe = sqrtf(dx * dx + dy * dy);
        const float e = epe * m[k];
        const float mag = fmaxf(sqrtf(gx[k] * gx[k] + gy[k] * gy[k]), 1e-10f);
        s[0] += in ? static_cast<double>(e) : 0.0;
        s[1] += in ? static_cast<double>(m[k]) : 0.0;
        c[0] += (in && e > 3.f && e / mag > 0.05f) ? 1u : 0u;
    }
    leave_partials<2, 1>(s, c, psum, pcnt, static_cast<int64_t>(b) * gridDim.x + blockIdx.x);
}

// ---- (d) the warp's sum of absolute differences -------------------------------------------------------------------------------
// One pixel's bilinear sample of flow_warp's default modes (border padding, the quirk-Q2 normalisation of warp_common.h):
// the position is source_coord's, the weights, flags and the order of the four products are Bilinear's (warp_common.h), so
// that a sample equals the element flow_warp would have written.
__device__ __forceinline__ float sample(const float *__restrict__ plane, const Bilinear<float> &t, int H, int W) {
    const float *q = plane + (t.dead(H, W) ? 0 : t.y0() * W + t.x0());     // the north-west tap (only used where a tap is inside)
    // a tap outside the image is never addressed and counts as an exact zero
    bool nw, ne, sw, se;
    t.inside(H, W, nw, ne, sw, se);
    return t.blend(nw ? q[0] : 0.f, ne ? q[1] : 0.f, sw ? q[W] : 0.f, se ? q[W + 1] : 0.f);
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void warp_sad_kernel(const float *__restrict__ image, const float *__restrict__ source,
                                                            const float *__restrict__ flow, double *__restrict__ psum, int C, int H,
                                                            int W) {
    const int hw = H * W;
    const int b = blockIdx.y, p0 = blockIdx.x * kChunk + threadIdx.x * kQuad;
    const float *fl = flow + static_cast<int64_t>(b) * 2 * hw;
    const float *img = image + static_cast<int64_t>(b) * C * hw, *src = source + static_cast<int64_t>(b) * C * hw;
    float fx[kQuad], fy[kQuad];
    load_quad<kVec>(fl, p0, hw, 0.f, fx);
    load_quad<kVec>(fl + hw, p0, hw, 0.f, fy);
    Bilinear<float> taps[kQuad];
    const int y0 = p0 / W, x0 = p0 - y0 * W;
#pragma unroll
    for (int k = 0; k < kQuad; ++k) {
        int x = x0 + k, y = y0;                  // a lane's 4 pixels may cross a row (more than once when W < 4)
        while (x >= W) { x -= W; ++y; }
        const bool in = p0 + k < hw;
        taps[k] = Bilinear<float>(source_coord<float>(in ? x : 0, fx[k], W, CERB_PAD_BORDER).pos,
                                  source_coord<float>(in ? y : 0, fy[k], H, CERB_PAD_BORDER).pos);
    }
    double acc[kQuad] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < C; ++c) {
        const int64_t o = static_cast<int64_t>(c) * hw;
        float v[kQuad];
        load_quad<kVec>(img + o, p0, hw, 0.f, v);
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            const float term = fabsf(v[k] - sample(src + o, taps[k], H, W));
            acc[k] += p0 + k < hw ? static_cast<double>(term) : 0.0;
        }
    }
    const double s[1] = {((acc[0] + acc[1]) + acc[2]) + acc[3]};
    leave_partials<1, 0>(s, nullptr, psum, nullptr, static_cast<int64_t>(b) * gridDim.x + blockIdx.x);
}

inline int chunks(int64_t n) { return static_cast<int>((n + kChunk - 1) / kChunk); }

inline bool aligned16(const void *a, const void *b, const void *c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

// NS float64 sums and NC uint32 counts per workgroup: the sums first, so that an 8-byte aligned workspace keeps them aligned
inline int64_t partial_bytes(int B, int64_t hw, int ns, int nc) { return static_cast<int64_t>(B) * chunks(hw) * (8 * ns + 4 * nc); }

}  // namespace

// ---- host side ------------------------------------------------------------------------------------------------------
int seg_confusion_max_classes() { return kConfMaxClasses; }

int seg_confusion(const void *logits, const void *target, void *confusion, int B, int C, int H, int W, int64_t ignore_index,
                  hipStream_t s) {
    const float *x = static_cast<const float *>(logits);
    const int64_t *t = static_cast<const int64_t *>(target);
    unsigned long long *conf = static_cast<unsigned long long *>(confusion);
    const int hw = H * W, nchunks = chunks(hw);
    const int64_t cells = static_cast<int64_t>(B) * C * C;
    seg_confusion_zero_kernel<<<static_cast<int>(std::min<int64_t>((cells + kThreads - 1) / kThreads, 1024)), kThreads, 0, s>>>(conf, cells);
    const int rc = launch_status();
    if (rc) return rc;
    const dim3 grid(std::min(nchunks, kConfGroupsPerImage), B);
    if (hw % kQuad == 0 && aligned16(x, t))
        seg_confusion_kernel<true><<<grid, kThreads, 0, s>>>(x, t, conf, C, hw, nchunks, ignore_index);
    else
        seg_confusion_kernel<false><<<grid, kThreads, 0, s>>>(x, t, conf, C, hw, nchunks, ignore_index);
    return launch_status();
}

int64_t depth_metric_workspace_bytes(int B, int h, int w) { return partial_bytes(B, static_cast<int64_t>(h) * w, 5, 4); }

int depth_metric_sums(const void *pred, const void *gt, void *sums, void *counts, void *workspace, int B, int h, int w, float min_depth,
                      float max_depth, hipStream_t s) {
    const float *p = static_cast<const float *>(pred), *g = static_cast<const float *>(gt);
    const int hw = h * w, n = chunks(hw);
    double *psum = static_cast<double *>(workspace);
    unsigned *pcnt = reinterpret_cast<unsigned *>(psum + static_cast<int64_t>(B) * n * 5);
    const dim3 grid(n, B);
    if (hw % kQuad == 0 && aligned16(p, g))
        depth_metric_kernel<true><<<grid, kThreads, 0, s>>>(p, g, psum, pcnt, hw, min_depth, max_depth);
    else
        depth_metric_kernel<false><<<grid, kThreads, 0, s>>>(p, g, psum, pcnt, hw, min_depth, max_depth);
    const int rc = launch_status();
    if (rc) return rc;
    metric_finish_kernel<5, 4><<<B, kThreads, 0, s>>>(psum, pcnt, n, static_cast<double *>(sums), static_cast<long long *>(counts));
    return launch_status();
}

int64_t flow_metric_workspace_bytes(int B, int H, int W) { return partial_bytes(B, static_cast<int64_t>(H) * W, 2, 1); }

int flow_metric_sums(const void *flow_pred, const void *flow_gt, const void *mask, void *sums, void *counts, void *workspace, int B,
                     int H, int W, hipStream_t s) {
    const float *fp = static_cast<const float *>(flow_pred), *fg = static_cast<const float *>(flow_gt);
    const float *m = static_cast<const float *>(mask);
    const int hw = H * W, n = chunks(hw);
    double *psum = static_cast<double *>(workspace);
    unsigned *pcnt = reinterpret_cast<unsigned *>(psum + static_cast<int64_t>(B) * n * 2);
    const dim3 grid(n, B);
    if (hw % kQuad == 0 && aligned16(fp, fg, m))
        flow_metric_kernel<true><<<grid, kThreads, 0, s>>>(fp, fg, m, psum, pcnt, hw);
    else
        flow_metric_kernel<false><<<grid, kThreads, 0, s>>>(fp, fg, m, psum, pcnt, hw);
    const int rc = launch_status();
    if (rc) return rc;
    metric_finish_kernel<2, 1><<<B, kThreads, 0, s>>>(psum, pcnt, n, static_cast<double *>(sums), static_cast<long long *>(counts));
    return launch_status();
}

int64_t warp_sad_workspace_bytes(int B, int H, int W) { return partial_bytes(B, static_cast<int64_t>(H) * W, 1, 0); }

int warp_sad(const void *image, const void *source, const void *flow, void *sad, void *workspace, int B, int C, int H, int W,
             hipStream_t s) {
    const float *im = static_cast<const float *>(image), *src = static_cast<const float *>(source), *fl = static_cast<const float *>(flow);
    const int hw = H * W, n = chunks(hw);
    double *psum = static_cast<double *>(workspace);
    const dim3 grid(n, B);
    // the gathers from `source` are 4-byte loads on both routes: only the image and the flow need the alignment
    if (hw % kQuad == 0 && aligned16(im, fl))
        warp_sad_kernel<true><<<grid, kThreads, 0, s>>>(im, src, fl, psum, C, H, W);
    else
        warp_sad_kernel<false><<<grid, kThreads, 0, s>>>(im, src, fl, psum, C, H, W);
    const int rc = launch_status();
    if (rc) return rc;
    metric_finish_kernel<1, 0><<<B, kThreads, 0, s>>>(psum, nullptr, n, static_cast<double *>(sad), nullptr);
    return launch_status();
}

}  // namespace cerb
