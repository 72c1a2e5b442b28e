// panoptic.hip -- the device side of the panoptic metric, forward only, fp32 / int64: what the reference's
// PanopticMetric (nnet_training/statistics/panoptic.py) and its post-processing (utilities/panoptic_post_processing.py) do to
// the centre heat map, the offset map and the four id / class maps of every image of a step.
//
//   center_peaks     : heat map (B,H,W) -> (B,H,W): the map the reference leaves behind after F.threshold(.., -1, inplace),
//                      max_pool2d(k, stride 1, padding (k-1)/2) and `hmp[hmp != pooled] = -1` (post_processing.py:52-59),
//                      written to a NEW tensor: v = x <= threshold ? -1 : x; out = v == max_window(v) ? v : -1
//   group_pixels     : offsets (B,2,H,W), centres (B,Kmax,2) int64 (y, x), counts (B,) int64, optional classes (B,H,W) int64
//                      -> (B,H,W) int64 = 1 + argmin_k sqrtf(dy dy + dx dx), dy = cy_k - (float(y) + off_y), dx likewise
//                      (post_processing.py:95-114: a (K, H*W, 2) difference and a (K, H*W) distance tensor), times the thing bit
//                      of the pixel's class (:139-149)
//   instance_overlap : four (B,H,W) int64 maps -> inter (B,M,M), pred_cls (B,M,C), tgt_cls (B,M,C) int64: the pixel counts
//                      that panoptic.py:34-70 gathers with np.unique and boolean-mask indexing once per instance
//
// No arithmetic in center_peaks (compares only) and integers in instance_overlap: both exact.  group_pixels computes in fp32
// with contraction off, in the reference's element-wise order.  No host synchronisation, no floating-point atomics: the same
// bits on every run and in a replayed graph.  Ids, classes and counts never form an address or a shift unless they lie in range.
#include <cmath>

#include "warp_common.h"
#include "loss_reduce.h"

#pragma clang fp contract(off)

namespace cerb {
namespace {

constexpr int kThreads = kReduceThreads;
constexpr int kQuad = 4;                       // consecutive pixels per lane (group_pixels, instance_overlap)
constexpr int kChunk = kThreads * kQuad;       // pixels per workgroup and step

// ---- (a) centre NMS ------------------------------------------------------------------------------------------------------------
constexpr int kPeakTileH = 16, kPeakTileW = 64;        // outputs per workgroup: 4 per lane
constexpr int kPeakMaxKernel = 15;                     // odd window sides 1..15: a halo of at most 7
constexpr int kPeakMaxHalo = (kPeakMaxKernel - 1) / 2;
constexpr int kPeakLdsH = kPeakTileH + 2 * kPeakMaxHalo, kPeakLdsW = kPeakTileW + 2 * kPeakMaxHalo;

// max_pool2d's maximum: a NaN in the window makes the maximum a NaN (so that it suppresses every pixel whose window holds it)
__device__ __forceinline__ float pool_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

// grid: (tiles along x, tiles along y, B).  Every pixel of the tile and its halo is read once into LDS as v (the thresholded
// value; -inf outside the image, max_pool2d's padding, so that neither a row's end nor the next image leaks in); the window
// maximum is separable and exact: a pass along the rows, then one along the columns.
__global__ __launch_bounds__(kThreads) void center_peaks_kernel(const float *__restrict__ x, float *__restrict__ out, int H, int W,
                                                                float threshold, int r) {
    __shared__ float v[kPeakLdsH][kPeakLdsW + 1];
    __shared__ float rowmax[kPeakLdsH][kPeakTileW + 1];
    const int x0 = blockIdx.x * kPeakTileW, y0 = blockIdx.y * kPeakTileH;
    const int64_t item = static_cast<int64_t>(blockIdx.z) * H * W;
    const int lh = kPeakTileH + 2 * r, lw = kPeakTileW + 2 * r;
    for (int i = threadIdx.x; i < lh * lw; i += kThreads) {
        const int ly = i / lw, lx = i - ly * lw;
        const int gy = y0 + ly - r, gx = x0 + lx - r;
        float val = -INFINITY;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float s = x[item + static_cast<int64_t>(gy) * W + gx];
            val = s <= threshold ? -1.f : s;                     // F.threshold's compare: a NaN stays a NaN
        }
        v[ly][lx] = val;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < lh * kPeakTileW; i += kThreads) {
        const int ly = i / kPeakTileW, lx = i - ly * kPeakTileW;
        float m = v[ly][lx];
        for (int d = 1; d <= 2 * r; ++d) m = pool_max(m, v[ly][lx + d]);
        rowmax[ly][lx] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kPeakTileH * kPeakTileW; i += kThreads) {
        const int ly = i / kPeakTileW, lx = i - ly * kPeakTileW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        float m = rowmax[ly][lx];
        for (int d = 1; d <= 2 * r; ++d) m = pool_max(m, rowmax[ly + d][lx]);
        const float c = v[ly + r][lx + r];
        out[item + static_cast<int64_t>(gy) * W + gx] = c == m ? c : -1.f;          // never a NaN: NaN == NaN is false
    }
}

// ---- (b) pixel grouping ----------------------------------------------------------------------------------------------------------
constexpr int kCenterChunk = 256;              // centres per LDS fill: 2 KiB; K is walked in such chunks
constexpr int kGroupMaxCenters = 4096;

// torch.argmin's rule, streamed: the first minimal index wins; a NaN counts as the minimum and the first NaN wins
__device__ __forceinline__ void argmin_step(float d, int k, float &best, int &idx) {
    const bool take = d < best || (d != d && best == best);
    best = take ? d : best;
    idx = take ? k : idx;
}

// grid: (chunks of 1024 pixels, B).  A lane owns 4 consecutive pixels, so that one LDS read of a centre serves 4 distances.
// Every lane of the workgroup walks the same number of centre chunks (the count is per image): the barriers are uniform.
__global__ __launch_bounds__(kThreads) void group_pixels_kernel(const float *__restrict__ offsets, const int64_t *__restrict__ centers,
                                                                const int64_t *__restrict__ counts, const int64_t *__restrict__ sem,
                                                                int64_t *__restrict__ out, int H, int W, int kmax,
                                                                unsigned long long thing_mask) {
    __shared__ float2 ctr[kCenterChunk];
    const int hw = H * W, b = blockIdx.y;
    const int p0 = blockIdx.x * kChunk + threadIdx.x * kQuad;
    const int64_t cnt64 = counts[b];
    const int K = cnt64 < 0 ? 0 : (cnt64 > kmax ? kmax : static_cast<int>(cnt64));
    const float *oy = offsets + static_cast<int64_t>(b) * 2 * hw, *ox = oy + hw;
    const int64_t *cb = centers + static_cast<int64_t>(b) * kmax * 2;
    float py[kQuad], px[kQuad], best[kQuad];
    int idx[kQuad];
#pragma unroll
    for (int k = 0; k < kQuad; ++k) {
        const int p = p0 + k;
        const bool in = p < hw;
        const int y = in ? p / W : 0, xx = in ? p - y * W : 0;
        py[k] = static_cast<float>(y) + (in ? oy[p] : 0.f);
        px[k] = static_cast<float>(xx) + (in ? ox[p] : 0.f);
        best[k] = INFINITY;
        idx[k] = 0;
    }
    for (int c0 = 0; c0 < K; c0 += kCenterChunk) {
        const int n = min(kCenterChunk, K - c0);
        __syncthreads();                                         // the previous chunk has been read by every lane
        for (int i = threadIdx.x; i < n; i += kThreads)
            ctr[i] = make_float2(static_cast<float>(cb[2 * (c0 + i)]), static_cast<float>(cb[2 * (c0 + i) + 1]));
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            const float2 c = ctr[i];
#pragma unroll
            for (int k = 0; k < kQuad; ++k) {
                const float dy = c.x - py[k], dx = c.y - px[k];
                argmin_step(sqrtf(dy * dy + dx * dx), c0 + i, best[k], idx[k]);     // all +inf: index 0 stays
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kQuad; ++k) {
        const int p = p0 + k;
        if (p >= hw) continue;
        int64_t id = K > 0 ? idx[k] + 1 : 0;
        if (sem) {
            const int64_t cls = sem[static_cast<int64_t>(b) * hw + p];
            const bool thing = cls >= 0 && cls < 64 && ((thing_mask >> static_cast<unsigned>(cls)) & 1ull);
            id = thing ? id : 0;
        }
        out[static_cast<int64_t>(b) * hw + p] = id;
    }
}

// ---- (c) the overlap matrices ----------------------------------------------------------------------------------------------------
constexpr int kOverlapGroupsPerImage = 256;    // workgroups per image; each walks its chunks by a stride
constexpr int kOverlapMaxBins = 16128;         // M*M + 2*M*C 32-bit LDS bins of a workgroup: 63 KiB

template <bool kVec>
__device__ __forceinline__ void load_quad_ids(const int64_t *__restrict__ t, int p0, int hw, int64_t (&v)[kQuad]) {
    if constexpr (kVec) {          // hw % 4 == 0 on this route: all inside or all outside
        if (p0 < hw) {
            const longlong2 a = *reinterpret_cast<const longlong2 *>(t + p0), b = *reinterpret_cast<const longlong2 *>(t + p0 + 2);
            v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
        } else {
            v[0] = v[1] = v[2] = v[3] = -1;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kQuad; ++k) v[k] = p0 + k < hw ? t[p0 + k] : -1;
    }
}

// equal bins of the lane's 4 pixels make one LDS add (almost every pixel is bin (0,0)); a bin of -1 does not count
__device__ __forceinline__ void add_bins(unsigned int *bins, int (&bin)[kQuad]) {
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

__global__ __launch_bounds__(kThreads) void overlap_zero_kernel(unsigned long long *__restrict__ a, int64_t na,
                                                                unsigned long long *__restrict__ b, unsigned long long *__restrict__ c,
                                                                int64_t nbc) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < na; i += stride) a[i] = 0ull;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < nbc; i += stride) {
        b[i] = 0ull;
        c[i] = 0ull;
    }
}

// bins: [pred id][target id] (M*M), then [pred id][pred class] (M*C), then [target id][target class] (M*C)
template <bool kVec>
__global__ __launch_bounds__(kThreads) void instance_overlap_kernel(const int64_t *__restrict__ pi, const int64_t *__restrict__ ti,
                                                                    const int64_t *__restrict__ ps, const int64_t *__restrict__ ts,
                                                                    unsigned long long *__restrict__ inter,
                                                                    unsigned long long *__restrict__ pcls,
                                                                    unsigned long long *__restrict__ tcls, int M, int C, int hw,
                                                                    int nchunks) {
    extern __shared__ unsigned int bins[];
    const int nmm = M * M, nmc = M * C, nbins = nmm + 2 * nmc, b = blockIdx.y;
    for (int i = threadIdx.x; i < nbins; i += kThreads) bins[i] = 0u;
    __syncthreads();
    const int64_t item = static_cast<int64_t>(b) * hw;
    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int p0 = ch * kChunk + threadIdx.x * kQuad;
        if (p0 >= hw) continue;
        int64_t a[kQuad], t[kQuad], ca[kQuad], ct[kQuad];
        load_quad_ids<kVec>(pi + item, p0, hw, a);
        load_quad_ids<kVec>(ti + item, p0, hw, t);
        load_quad_ids<kVec>(ps + item, p0, hw, ca);
        load_quad_ids<kVec>(ts + item, p0, hw, ct);
        int bi[kQuad], bp[kQuad], bt[kQuad];
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            const bool in = p0 + k < hw && static_cast<uint64_t>(a[k]) < static_cast<uint64_t>(M) &&
                            static_cast<uint64_t>(t[k]) < static_cast<uint64_t>(M);
            const bool pc = in && static_cast<uint64_t>(ca[k]) < static_cast<uint64_t>(C);
            const bool tc = in && static_cast<uint64_t>(ct[k]) < static_cast<uint64_t>(C);
            bi[k] = in ? static_cast<int>(a[k]) * M + static_cast<int>(t[k]) : -1;
            bp[k] = pc ? nmm + static_cast<int>(a[k]) * C + static_cast<int>(ca[k]) : -1;
            bt[k] = tc ? nmm + nmc + static_cast<int>(t[k]) * C + static_cast<int>(ct[k]) : -1;
        }
        add_bins(bins, bi);
        add_bins(bins, bp);
        add_bins(bins, bt);
    }
    __syncthreads();
    unsigned long long *ib = inter + static_cast<int64_t>(b) * nmm;
    unsigned long long *pb = pcls + static_cast<int64_t>(b) * nmc, *tb = tcls + static_cast<int64_t>(b) * nmc;
    for (int i = threadIdx.x; i < nbins; i += kThreads) {
        const unsigned int n = bins[i];
        if (!n) continue;
        unsigned long long *dst = i < nmm ? ib + i : (i < nmm + nmc ? pb + (i - nmm) : tb + (i - nmm - nmc));
        atomicAdd(dst, static_cast<unsigned long long>(n));
    }
}

inline int chunks(int64_t n) { return static_cast<int>((n + kChunk - 1) / kChunk); }

inline bool aligned16(const void *a, const void *b, const void *c, const void *d) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
int center_peaks_max_kernel() { return kPeakMaxKernel; }
int group_pixels_max_centers() { return kGroupMaxCenters; }
int instance_overlap_max_bins() { return kOverlapMaxBins; }

int center_peaks(const void *heatmap, void *out, int B, int H, int W, float threshold, int nms_kernel, hipStream_t s) {
    const dim3 grid((W + kPeakTileW - 1) / kPeakTileW, (H + kPeakTileH - 1) / kPeakTileH, B);
    center_peaks_kernel<<<grid, kThreads, 0, s>>>(static_cast<const float *>(heatmap), static_cast<float *>(out), H, W, threshold,
                                                 (nms_kernel - 1) / 2);
    return launch_status();
}

int group_pixels(const void *offsets, const void *centers, const void *counts, const void *sem, void *out, int B, int H, int W,
                 int kmax, uint64_t thing_mask, hipStream_t s) {
    const dim3 grid(chunks(static_cast<int64_t>(H) * W), B);
    group_pixels_kernel<<<grid, kThreads, 0, s>>>(static_cast<const float *>(offsets), static_cast<const int64_t *>(centers),
                                                  static_cast<const int64_t *>(counts), static_cast<const int64_t *>(sem),
                                                  static_cast<int64_t *>(out), H, W, kmax,
                                                  static_cast<unsigned long long>(thing_mask));
    return launch_status();
}

int instance_overlap(const void *pred_inst, const void *tgt_inst, const void *pred_seg, const void *tgt_seg, void *inter,
                     void *pred_cls, void *tgt_cls, int B, int H, int W, int M, int C, hipStream_t s) {
    const int64_t *pi = static_cast<const int64_t *>(pred_inst), *ti = static_cast<const int64_t *>(tgt_inst);
    const int64_t *ps = static_cast<const int64_t *>(pred_seg), *ts = static_cast<const int64_t *>(tgt_seg);
    unsigned long long *im = static_cast<unsigned long long *>(inter);
    unsigned long long *pc = static_cast<unsigned long long *>(pred_cls), *tc = static_cast<unsigned long long *>(tgt_cls);
    const int hw = H * W, nchunks = chunks(hw);
    const int64_t na = static_cast<int64_t>(B) * M * M, nbc = static_cast<int64_t>(B) * M * C;
    overlap_zero_kernel<<<static_cast<int>(std::min<int64_t>((na + kThreads - 1) / kThreads, 1024)), kThreads, 0, s>>>(im, na, pc, tc, nbc);
    const int rc = launch_status();
    if (rc) return rc;
    const dim3 grid(std::min(nchunks, kOverlapGroupsPerImage), B);
    const size_t lds = static_cast<size_t>(M * M + 2 * M * C) * sizeof(unsigned int);
    if (hw % kQuad == 0 && aligned16(pi, ti, ps, ts))
        instance_overlap_kernel<true><<<grid, kThreads, lds, s>>>(pi, ti, ps, ts, im, pc, tc, M, C, hw, nchunks);
    else
        instance_overlap_kernel<false><<<grid, kThreads, lds, s>>>(pi, ti, ps, ts, im, pc, tc, M, C, hw, nchunks);
    return launch_status();
}

}  // namespace cerb
