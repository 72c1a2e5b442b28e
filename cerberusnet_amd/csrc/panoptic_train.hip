// panoptic_train.hip -- the training side of the panoptic branch: the Panoptic-DeepLab training targets from
// an id map that is already on the device, and the centre / offset regression loss as ONE differentiable scalar op, fp32.
//
// Targets (the reference's PanopticTargetGenerator, datasets/cityscapes_panoptic_transform.py:64-181, a host numpy loop of six
// to eight full-image `panoptic == id` passes per segment).  Here, for a batch, from the id map (B,H,W) and a padded table of
// S <= 256 segments per image (id, category, flags: bit 0 thing, bit 1 crowd; seg_count[b] live rows):
//   zero    : the (B,S,3) 64-bit moments
//   moments : a workgroup stages its image's id table in LDS; every pixel finds its row (or -1) and writes it to a row map;
//             count, sum y and sum x per row are added as INTEGERS -- a wave whose pixels share one row folds them by a
//             butterfly and adds once, 64-bit LDS adds otherwise, then one 64-bit global add per sum and non-empty row.  Integer
//             adds give the same result in any order.
//   finish  : per (image, row): cy = double(sum y) / double(n), cx likewise, (int) of both, has-centre = thing and n > 0,
//             small = thing and n < small_instance_area; center_points (B,S,2) float64, NaN where there is no centre
//   fill    : every output element written once from the row map: semantic, foreground, the three masks, offset =
//             float(cy - double(y)), float(cx - double(x)) on things, centre = the maximum of gauss[y - (Y-3s-1)][x - (X-3s-1)]
//             over the image's centres (Y,X) whose (6s+3)^2 window covers the pixel -- a gather over a centre list kept in LDS
//             (only the centres whose window reaches the workgroup's rows): no zero-fill pass, no atomic maximum.
// The Gaussian is a table the caller makes once: the kernels never call exp.  Ids among an image's live rows must be distinct;
// the result is otherwise unspecified (a pixel takes the first row that matches).
//
// Loss (the reference's DeeplabPanopticLoss, loss_functions/panoptic_loss.py, without `weight`):
//   forward : one pass per term (centre: d^2, offset: |d|) leaves per 1024 elements a partial of sum f(d), of sum m f(d) over
//             the elements with m != 0, and of sum m; one workgroup adds the partials in a fixed order (loss_reduce.h's
//             pattern), applies the mode and the "sum m > 0" gate and leaves the loss and the two scales the backward needs
//   backward: one launch, every gradient element written once
//   mode 0 (reference): term = weight * mean f(d) over ALL elements if the mask is absent or sum m > 0, else 0
//   mode 1 (pixel)    : term = weight * sum m f(d) / sum m (both sums over elements: the offset mask counts twice), 0 if
//                       sum m == 0; an element with m == 0 is skipped by selection
// No floating-point atomics and no host read anywhere: the same bits on every run and in a replayed graph.
//
// Two routes, as in depth_loss.hip and metrics.hip.  Both give a workgroup the SAME 1024 consecutive pixels (elements) and fold
// them in the same order -- four consecutive ones left to right, the 64 groups of a wave by a butterfly, the 4 waves in wave
// order: a call on misaligned pointers gives the bits of the aligned one.
//   vector : H*W % 4 == 0 and 16-byte aligned pointers: a lane owns 4 consecutive pixels, 16-byte loads and stores
//   scalar : everything else: a lane owns one pixel at a time, four times
#include <cmath>

#include "common.h"
#include "loss_reduce.h"

#pragma clang fp contract(off)

namespace cerb {
namespace {

constexpr int kThreads = kReduceThreads;
constexpr int kQuad = 4;
constexpr int kChunk = kThreads * kQuad;      // pixels (elements) per workgroup, both routes
constexpr int kMaxSegments = 256;             // rows of an image's table: one per thread, and the LDS bins

typedef unsigned long long u64;

constexpr int kThing = 1, kCrowd = 2, kHasCentre = 4, kSmall = 8;

inline int chunks(int64_t n) { return static_cast<int>((n + kChunk - 1) / kChunk); }

inline bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

// ====================================================================================================================
// targets
// ====================================================================================================================
struct TargetWs {
    u64 *moments;       // (B,S,3): n, sum y, sum x
    int64_t *cat;       // (B,S)
    int *rowmap;        // (B,HW)
    int *iyx;           // (B,S,2): (int)cy, (int)cx
    int *flags;         // (B,S): kThing | kCrowd | kHasCentre | kSmall; 0 for a row that is not live
};

inline int64_t pad16(int64_t bytes) { return (bytes + 15) & ~static_cast<int64_t>(15); }

inline TargetWs target_ws(void *workspace, int B, int64_t HW, int S) {
    char *p = static_cast<char *>(workspace);
    const int64_t rows = static_cast<int64_t>(B) * S;
    TargetWs w;
    w.moments = reinterpret_cast<u64 *>(p);
    p += rows * 24;
    w.cat = reinterpret_cast<int64_t *>(p);
    p += rows * 8;
    w.rowmap = reinterpret_cast<int *>(p);
    p += pad16(static_cast<int64_t>(B) * HW * 4);
    w.iyx = reinterpret_cast<int *>(p);
    p += rows * 8;
    w.flags = reinterpret_cast<int *>(p);
    return w;
}

__global__ __launch_bounds__(kThreads) void ptarget_zero_kernel(u64 *__restrict__ a, int64_t n) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kThreads) a[i] = 0;
}

__device__ __forceinline__ int live_rows(const int64_t *__restrict__ seg_count, int b, int S) {
    const int64_t c = seg_count[b];
    return c < 0 ? 0 : (c > S ? S : static_cast<int>(c));
}

// the row of an id in the table staged in LDS (the first that matches), or -1
__device__ __forceinline__ int find_row(const int64_t *table, int count, int64_t id) {
    for (int i = 0; i < count; ++i)
        if (table[i] == id) return i;
    return -1;
}

// adds (n, sy, sx) of `row` (-1: nothing) to the workgroup's LDS bins; called by whole waves
__device__ __forceinline__ void add_moments(u64 *bins, int row, unsigned n, u64 sy, u64 sx) {
    const int r0 = __shfl(row, 0, 64);
    if (__all(row == r0)) {          // the usual case: the wave's pixels lie in one segment
        if (r0 < 0) return;
        const u64 tn = wave_sum<u64>(n), ty = wave_sum(sy), tx = wave_sum(sx);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&bins[r0], tn);
            atomicAdd(&bins[kMaxSegments + r0], ty);
            atomicAdd(&bins[2 * kMaxSegments + r0], tx);
        }
    } else if (row >= 0) {
        atomicAdd(&bins[row], static_cast<u64>(n));
        atomicAdd(&bins[kMaxSegments + row], sy);
        atomicAdd(&bins[2 * kMaxSegments + row], sx);
    }
}

template <typename IdT, bool kVec>
__global__ __launch_bounds__(kThreads) void ptarget_moments_kernel(const IdT *__restrict__ ids, const int64_t *__restrict__ seg_ids,
                                                                   const int64_t *__restrict__ seg_count, int *__restrict__ rowmap,
                                                                   u64 *__restrict__ moments, int HW, int W, int S) {
    __shared__ int64_t table[kMaxSegments];
    __shared__ u64 bins[3 * kMaxSegments];
    const int b = blockIdx.y;
    const int count = live_rows(seg_count, b, S);
    if (static_cast<int>(threadIdx.x) < count) table[threadIdx.x] = seg_ids[static_cast<int64_t>(b) * S + threadIdx.x];
    for (int i = threadIdx.x; i < 3 * kMaxSegments; i += kThreads) bins[i] = 0;
    __syncthreads();
    const IdT *im = ids + static_cast<int64_t>(b) * HW;
    int *rm = rowmap + static_cast<int64_t>(b) * HW;
    const int base = blockIdx.x * kChunk;
    if constexpr (kVec) {
        const int p0 = base + threadIdx.x * kQuad;
        int row[kQuad] = {-1, -1, -1, -1}, yy[kQuad] = {0, 0, 0, 0}, xx[kQuad] = {0, 0, 0, 0};
        if (p0 < HW) {              // HW % 4 == 0 on this route: a lane's 4 pixels are all inside
            int64_t id[kQuad];
            if constexpr (sizeof(IdT) == 4) {
                const int4 q = *reinterpret_cast<const int4 *>(im + p0);
                id[0] = q.x, id[1] = q.y, id[2] = q.z, id[3] = q.w;
            } else {
                const longlong2 q0 = *reinterpret_cast<const longlong2 *>(im + p0), q1 = *reinterpret_cast<const longlong2 *>(im + p0 + 2);
                id[0] = q0.x, id[1] = q0.y, id[2] = q1.x, id[3] = q1.y;
            }
            int y = p0 / W, x = p0 - y * W;
#pragma unroll
            for (int k = 0; k < kQuad; ++k) {
                row[k] = (k > 0 && id[k] == id[k - 1]) ? row[k - 1] : find_row(table, count, id[k]);
                yy[k] = y, xx[k] = x;
                if (++x == W) x = 0, ++y;
            }
            *reinterpret_cast<int4 *>(rm + p0) = make_int4(row[0], row[1], row[2], row[3]);
        }
        const bool same = row[0] == row[1] && row[0] == row[2] && row[0] == row[3];
        if (__all(same)) {
            add_moments(bins, row[0], kQuad, static_cast<u64>(yy[0]) + yy[1] + yy[2] + yy[3], static_cast<u64>(xx[0]) + xx[1] + xx[2] + xx[3]);
        } else {
#pragma unroll
            for (int k = 0; k < kQuad; ++k) add_moments(bins, row[k], 1, yy[k], xx[k]);
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < kQuad; ++j) {
            const int p = base + j * kThreads + threadIdx.x;
            int row = -1, y = 0, x = 0;
            if (p < HW) {
                row = find_row(table, count, static_cast<int64_t>(im[p]));
                y = p / W, x = p - y * W;
                rm[p] = row;
            }
            add_moments(bins, row, 1, y, x);
        }
    }
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < count && bins[threadIdx.x]) {
        u64 *m = moments + (static_cast<int64_t>(b) * S + threadIdx.x) * 3;
        atomicAdd(m, bins[threadIdx.x]);
        atomicAdd(m + 1, bins[kMaxSegments + threadIdx.x]);
        atomicAdd(m + 2, bins[2 * kMaxSegments + threadIdx.x]);
    }
}

// one workgroup per image, one thread per row
__global__ __launch_bounds__(kThreads) void ptarget_finish_kernel(const u64 *__restrict__ moments, const int64_t *__restrict__ seg_category,
                                                                  const int *__restrict__ seg_flags, const int64_t *__restrict__ seg_count,
                                                                  int64_t *__restrict__ cat, int *__restrict__ iyx, int *__restrict__ flags,
                                                                  double *__restrict__ center_points, int S, int64_t small_area) {
    const int b = blockIdx.x, r = threadIdx.x;
    if (r >= S) return;
    const int64_t i = static_cast<int64_t>(b) * S + r;
    const bool live = r < live_rows(seg_count, b, S);
    const u64 n = moments[i * 3];
    const int given = live ? seg_flags[i] : 0;
    const bool thing = (given & 1) != 0, has = thing && n > 0;
    double cy = __longlong_as_double(0x7ff8000000000000LL), cx = cy;
    int iy = 0, ix = 0;
    if (has) {
        cy = static_cast<double>(moments[i * 3 + 1]) / static_cast<double>(n);
        cx = static_cast<double>(moments[i * 3 + 2]) / static_cast<double>(n);
        iy = static_cast<int>(cy), ix = static_cast<int>(cx);
    }
    int f = 0;
    if (live) f = (thing ? kThing : 0) | ((given & 2) ? kCrowd : 0) | (has ? kHasCentre : 0) |
                  ((has && static_cast<int64_t>(n) < small_area) ? kSmall : 0);
    cat[i] = live ? seg_category[i] : 0;
    iyx[i * 2] = iy, iyx[i * 2 + 1] = ix;
    flags[i] = f;
    center_points[i * 2] = cy, center_points[i * 2 + 1] = cx;
}

struct FillArgs {
    int64_t *semantic, *foreground;
    float *center, *offset, *semantic_mask, *center_mask, *offset_mask;
    int64_t ignore_label;
    float small_weight;
    int sigma, ignore_stuff, ignore_crowd;
};

struct FillPixel {
    int64_t semantic, foreground;
    float center, off_y, off_x, semantic_mask, center_mask, offset_mask;
};

template <bool kVec>
__global__ __launch_bounds__(kThreads) void ptarget_fill_kernel(const int *__restrict__ rowmap, const int64_t *__restrict__ cat,
                                                                const int *__restrict__ iyx, const int *__restrict__ flags,
                                                                const double *__restrict__ center_points, const float *__restrict__ gauss,
                                                                FillArgs a, int HW, int W, int S) {
    __shared__ int64_t s_cat[kMaxSegments];
    __shared__ double s_cy[kMaxSegments], s_cx[kMaxSegments];
    __shared__ int s_flags[kMaxSegments];
    __shared__ int s_list[2 * kMaxSegments];      // upper-left corners (y, x) of the windows that reach this workgroup's rows
    __shared__ int s_n;
    const int b = blockIdx.y, base = blockIdx.x * kChunk;
    const int reach = 3 * a.sigma + 1, size = 6 * a.sigma + 3;
    const int last = min(base + kChunk, HW) - 1, y_first = base / W, y_last = last / W;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < S) {
        const int64_t i = static_cast<int64_t>(b) * S + threadIdx.x;
        const int f = flags[i];
        s_flags[threadIdx.x] = f;
        s_cat[threadIdx.x] = cat[i];
        s_cy[threadIdx.x] = center_points[i * 2];
        s_cx[threadIdx.x] = center_points[i * 2 + 1];
        if (f & kHasCentre) {
            const int top = iyx[i * 2] - reach;
            if (top <= y_last && top + size > y_first) {        // any order: a maximum does not depend on it
                const int slot = atomicAdd(&s_n, 1);
                s_list[2 * slot] = top;
                s_list[2 * slot + 1] = iyx[i * 2 + 1] - reach;
            }
        }
    }
    __syncthreads();
    const int ncentres = s_n;
    const int *rm = rowmap + static_cast<int64_t>(b) * HW;
    const int64_t o1 = static_cast<int64_t>(b) * HW, o2 = 2 * o1;

    auto pixel = [&](int row, int y, int x) {
        FillPixel px;
        const int f = row >= 0 ? s_flags[row] : 0;
        const bool has = row >= 0, thing = (f & kThing) != 0, crowd = (f & kCrowd) != 0;
        px.semantic = (!has || (crowd && a.ignore_crowd)) ? a.ignore_label : s_cat[row];
        px.foreground = thing ? 1 : 0;
        px.semantic_mask = (f & kSmall) ? a.small_weight : 1.f;
        px.center_mask = (has && !crowd) ? 1.f : 0.f;
        px.offset_mask = (has && !crowd && (thing || !a.ignore_stuff)) ? 1.f : 0.f;
        px.off_y = thing ? static_cast<float>(s_cy[row] - static_cast<double>(y)) : 0.f;
        px.off_x = thing ? static_cast<float>(s_cx[row] - static_cast<double>(x)) : 0.f;
        float c = 0.f;
        for (int k = 0; k < ncentres; ++k) {
            const unsigned gy = static_cast<unsigned>(y - s_list[2 * k]), gx = static_cast<unsigned>(x - s_list[2 * k + 1]);
            if (gy < static_cast<unsigned>(size) && gx < static_cast<unsigned>(size)) c = fmaxf(c, gauss[gy * size + gx]);
        }
        px.center = c;
        return px;
    };

    if constexpr (kVec) {
        const int p0 = base + threadIdx.x * kQuad;
        if (p0 >= HW) return;
        const int4 q = *reinterpret_cast<const int4 *>(rm + p0);
        const int rows[kQuad] = {q.x, q.y, q.z, q.w};
        FillPixel px[kQuad];
        int y = p0 / W, x = p0 - y * W;
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            px[k] = pixel(rows[k], y, x);
            if (++x == W) x = 0, ++y;
        }
        *reinterpret_cast<longlong2 *>(a.semantic + o1 + p0) = make_longlong2(px[0].semantic, px[1].semantic);
        *reinterpret_cast<longlong2 *>(a.semantic + o1 + p0 + 2) = make_longlong2(px[2].semantic, px[3].semantic);
        *reinterpret_cast<longlong2 *>(a.foreground + o1 + p0) = make_longlong2(px[0].foreground, px[1].foreground);
        *reinterpret_cast<longlong2 *>(a.foreground + o1 + p0 + 2) = make_longlong2(px[2].foreground, px[3].foreground);
        *reinterpret_cast<float4 *>(a.center + o1 + p0) = make_float4(px[0].center, px[1].center, px[2].center, px[3].center);
        *reinterpret_cast<float4 *>(a.offset + o2 + p0) = make_float4(px[0].off_y, px[1].off_y, px[2].off_y, px[3].off_y);
        *reinterpret_cast<float4 *>(a.offset + o2 + HW + p0) = make_float4(px[0].off_x, px[1].off_x, px[2].off_x, px[3].off_x);
        *reinterpret_cast<float4 *>(a.semantic_mask + o1 + p0) =
            make_float4(px[0].semantic_mask, px[1].semantic_mask, px[2].semantic_mask, px[3].semantic_mask);
        *reinterpret_cast<float4 *>(a.center_mask + o1 + p0) = make_float4(px[0].center_mask, px[1].center_mask, px[2].center_mask, px[3].center_mask);
        *reinterpret_cast<float4 *>(a.offset_mask + o1 + p0) = make_float4(px[0].offset_mask, px[1].offset_mask, px[2].offset_mask, px[3].offset_mask);
    } else {
#pragma unroll 1
        for (int j = 0; j < kQuad; ++j) {
            const int p = base + j * kThreads + threadIdx.x;
            if (p >= HW) return;
            const int y = p / W, x = p - y * W;
            const FillPixel px = pixel(rm[p], y, x);
            a.semantic[o1 + p] = px.semantic;
            a.foreground[o1 + p] = px.foreground;
            a.center[o1 + p] = px.center;
            a.offset[o2 + p] = px.off_y;
            a.offset[o2 + HW + p] = px.off_x;
            a.semantic_mask[o1 + p] = px.semantic_mask;
            a.center_mask[o1 + p] = px.center_mask;
            a.offset_mask[o1 + p] = px.offset_mask;
        }
    }
}

template <typename IdT>
int launch_moments(const void *ids, const int64_t *seg_ids, const int64_t *seg_count, const TargetWs &w, int B, int HW, int W, int S,
                   hipStream_t s) {
    const IdT *p = static_cast<const IdT *>(ids);
    const dim3 grid(chunks(HW), B);
    if (HW % kQuad == 0 && aligned16(p, w.rowmap))
        ptarget_moments_kernel<IdT, true><<<grid, kThreads, 0, s>>>(p, seg_ids, seg_count, w.rowmap, w.moments, HW, W, S);
    else
        ptarget_moments_kernel<IdT, false><<<grid, kThreads, 0, s>>>(p, seg_ids, seg_count, w.rowmap, w.moments, HW, W, S);
    return launch_status();
}

bool target_size_ok(int B, int H, int W, int S) {
    return B > 0 && B <= 65535 && H > 0 && W > 0 && S > 0 && S <= kMaxSegments && static_cast<int64_t>(H) * W <= 0x7fffffff - 1024;
}

// ====================================================================================================================
// loss
// ====================================================================================================================
// the element range of one term: n elements in planes of hw, `planes` of them per mask image (1: centre, 2: offset)
struct Term {
    const float *pred, *tgt, *mask;     // mask (B,hw) or null
    int n, hw, planes;
};

__device__ __forceinline__ int mask_index(const Term &t, int e) {
    const int per = t.planes * t.hw, b = e / per;
    int r = e - b * per;
    if (r >= t.hw) r -= t.hw;            // planes <= 2
    return b * t.hw + r;
}

// what one element adds: f = d^2 or |d|; mf = m f by selection; m (1 without a mask)
template <bool kAbs>
__device__ __forceinline__ void element(float p, float t, float m, float &f, float &mf, float &mm) {
    const float d = p - t;
    f = kAbs ? fabsf(d) : d * d;
    mf = m != 0.f ? m * f : 0.f;         // a select: what an element with m == 0 holds never counts
    mm = m;
}

template <bool kVec, bool kAbs>
__global__ __launch_bounds__(kThreads) void ploss_partial_kernel(Term t, float *__restrict__ pf, float *__restrict__ pmf,
                                                                 float *__restrict__ pm) {
    __shared__ float red[3][4];
    __shared__ float stage[kVec ? 3 : 3 * kChunk];
    const int base = blockIdx.x * kChunk;
    float f4[kQuad], g4[kQuad], m4[kQuad];
    if constexpr (kVec) {
        const int e0 = base + threadIdx.x * kQuad;
#pragma unroll
        for (int k = 0; k < kQuad; ++k) f4[k] = g4[k] = m4[k] = 0.f;
        if (e0 < t.n) {              // n % 4 == 0 and hw % 4 == 0: the lane's 4 elements lie in one plane
            const float4 a = *reinterpret_cast<const float4 *>(t.pred + e0), b = *reinterpret_cast<const float4 *>(t.tgt + e0);
            const float4 m = t.mask ? *reinterpret_cast<const float4 *>(t.mask + mask_index(t, e0)) : make_float4(1.f, 1.f, 1.f, 1.f);
            element<kAbs>(a.x, b.x, m.x, f4[0], g4[0], m4[0]);
            element<kAbs>(a.y, b.y, m.y, f4[1], g4[1], m4[1]);
            element<kAbs>(a.z, b.z, m.z, f4[2], g4[2], m4[2]);
            element<kAbs>(a.w, b.w, m.w, f4[3], g4[3], m4[3]);
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < kQuad; ++j) {
            const int i = j * kThreads + threadIdx.x, e = base + i;
            float f = 0.f, g = 0.f, m = 0.f;
            if (e < t.n) element<kAbs>(t.pred[e], t.tgt[e], t.mask ? t.mask[mask_index(t, e)] : 1.f, f, g, m);
            stage[i] = f;
            stage[kChunk + i] = g;
            stage[2 * kChunk + i] = m;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            f4[k] = stage[threadIdx.x * kQuad + k];
            g4[k] = stage[kChunk + threadIdx.x * kQuad + k];
            m4[k] = stage[2 * kChunk + threadIdx.x * kQuad + k];
        }
    }
    const float f = quad_sum(f4), g = quad_sum(g4), m = quad_sum(m4);
    const float tf = block_sum(f, red[0]), tg = block_sum(g, red[1]), tm = block_sum(m, red[2]);
    if (threadIdx.x == 0) {
        pf[blockIdx.x] = tf;
        pmf[blockIdx.x] = tg;
        pm[blockIdx.x] = tm;
    }
}

// the scale of one term and its value: mode 0 weight / N behind the gate, mode 1 weight / sum m
__device__ __forceinline__ void term_value(float sf, float smf, float sm, bool masked, int n, float weight, int mode, float &value,
                                           float &scale) {
    const bool on = !masked || sm > 0.f;          // false for a NaN sum too
    if (mode == 0 || !masked) {
        scale = on ? weight / static_cast<float>(n) : 0.f;
        value = on ? sf * scale : 0.f;
    } else {
        scale = on ? weight / sm : 0.f;
        value = on ? smf * scale : 0.f;
    }
}

// one workgroup, fixed order: partials laid out [f | mf | m] for the centre term (nc each), then for the offset term (no each)
__global__ __launch_bounds__(kThreads) void ploss_final_kernel(const float *__restrict__ parts, int nc, int no, int n_c, int n_o,
                                                               int c_masked, int o_masked, float cw, float ow, int mode,
                                                               float *__restrict__ loss, float *__restrict__ state) {
    __shared__ float red[6][kThreads];
    float acc[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float *p = parts + (k < 3 ? k * nc : 3 * nc + (k - 3) * no);
        const int n = k < 3 ? nc : no;
        float a = 0.f;
        for (int i = threadIdx.x; i < n; i += kThreads) a += p[i];
        acc[k] = a;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) red[k][threadIdx.x] = acc[k];
    tree_sum(red);
    if (threadIdx.x == 0) {
        float vc, sc, vo, so;
        term_value(red[0][0], red[1][0], red[2][0], c_masked != 0, n_c, cw, mode, vc, sc);
        term_value(red[3][0], red[4][0], red[5][0], o_masked != 0, n_o, ow, mode, vo, so);
        loss[0] = vc + vo;
        state[0] = sc;
        state[1] = so;
    }
}

// d f / d pred of one element times its scale: 2 d or sign(d), times m in pixel mode; 0.0f by selection where it is off
template <bool kAbs>
__device__ __forceinline__ float element_grad(float p, float t, float m, bool by_mask, float coef) {
    const float d = p - t;
    const float slope = kAbs ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : 2.f * d;
    if (coef == 0.f) return 0.f;                       // gated off, or no element counts: exactly 0 whatever d holds
    if (by_mask) return m != 0.f ? (coef * m) * slope : 0.f;
    return coef * slope;
}

template <bool kVec, bool kAbs>
__device__ __forceinline__ void grad_chunk(const Term &t, float *__restrict__ grad, bool by_mask, float coef, int block) {
    const int base = block * kChunk;
    if constexpr (kVec) {
        const int e0 = base + threadIdx.x * kQuad;
        if (e0 >= t.n) return;
        const float4 a = *reinterpret_cast<const float4 *>(t.pred + e0), b = *reinterpret_cast<const float4 *>(t.tgt + e0);
        const float4 m = (by_mask && t.mask) ? *reinterpret_cast<const float4 *>(t.mask + mask_index(t, e0)) : make_float4(1.f, 1.f, 1.f, 1.f);
        *reinterpret_cast<float4 *>(grad + e0) =
            make_float4(element_grad<kAbs>(a.x, b.x, m.x, by_mask, coef), element_grad<kAbs>(a.y, b.y, m.y, by_mask, coef),
                        element_grad<kAbs>(a.z, b.z, m.z, by_mask, coef), element_grad<kAbs>(a.w, b.w, m.w, by_mask, coef));
    } else {
#pragma unroll
        for (int j = 0; j < kQuad; ++j) {
            const int e = base + j * kThreads + threadIdx.x;
            if (e >= t.n) return;
            grad[e] = element_grad<kAbs>(t.pred[e], t.tgt[e], (by_mask && t.mask) ? t.mask[mask_index(t, e)] : 1.f, by_mask, coef);
        }
    }
}

// workgroups [0, nc) write the centre gradient, [nc, nc + no) the offset gradient
template <bool kVecC, bool kVecO>
__global__ __launch_bounds__(kThreads) void ploss_bwd_kernel(Term c, Term o, const float *__restrict__ state,
                                                             const float *__restrict__ grad_loss, float *__restrict__ gc,
                                                             float *__restrict__ go, int nc, int mode) {
    const float g = grad_loss[0];            // read here, from device memory: no host synchronisation
    if (static_cast<int>(blockIdx.x) < nc)
        grad_chunk<kVecC, false>(c, gc, mode == 1 && c.mask != nullptr, g * state[0], blockIdx.x);
    else
        grad_chunk<kVecO, true>(o, go, mode == 1 && o.mask != nullptr, g * state[1], blockIdx.x - nc);
}

inline Term term(const void *pred, const void *tgt, const void *mask, int B, int HW, int planes) {
    Term t;
    t.pred = static_cast<const float *>(pred);
    t.tgt = static_cast<const float *>(tgt);
    t.mask = static_cast<const float *>(mask);
    t.hw = HW;
    t.planes = planes;
    t.n = B * HW * planes;
    return t;
}

inline bool term_vec(const Term &t, const void *extra = nullptr) { return t.hw % kQuad == 0 && aligned16(t.pred, t.tgt, t.mask, extra); }

int loss_args_ok(int B, int H, int W, int mode, int dtype) {
    if (dtype < CERB_F32 || dtype > CERB_F64) return CERB_EDTYPE;
    if (dtype != CERB_F32) return CERB_EUNSUPPORTED;
    if (B < 0 || H <= 0 || W <= 0 || (mode != 0 && mode != 1)) return CERB_EINVAL;
    if (2 * static_cast<int64_t>(B) * H * W > 0x7fffffff - 1024) return CERB_ETOOLARGE;
    return CERB_OK;
}

int64_t loss_ws_bytes(int B, int H, int W) {
    const int64_t n = static_cast<int64_t>(B) * H * W;
    return 3 * (static_cast<int64_t>(chunks(n)) + chunks(2 * n)) * 4;
}

}  // namespace
}  // namespace cerb

using namespace cerb;

extern "C" {

int cerberus_panoptic_targets_max_segments(void) { return kMaxSegments; }

int64_t cerberus_panoptic_targets_workspace_bytes(int B, int H, int W, int S) {
    if (!target_size_ok(B, H, W, S)) return 0;
    const int64_t rows = static_cast<int64_t>(B) * S;
    return rows * 24 + rows * 8 + pad16(static_cast<int64_t>(B) * H * W * 4) + rows * 8 + rows * 4;
}

int cerberus_panoptic_targets(const void *ids, int ids_int64, const void *seg_ids, const void *seg_category, const void *seg_flags,
                              const void *seg_count, const void *gauss, void *semantic, void *foreground, void *center, void *offset,
                              void *semantic_mask, void *center_mask, void *offset_mask, void *center_points, void *workspace,
                              int64_t workspace_bytes, int B, int H, int W, int S, int sigma, int64_t ignore_label,
                              int ignore_stuff_in_offset, int64_t small_instance_area, float small_instance_weight,
                              int ignore_crowd_in_semantic, void *stream) {
    if (B < 0 || H <= 0 || W <= 0 || S <= 0 || sigma < 1 || (ids_int64 != 0 && ids_int64 != 1)) return CERB_EINVAL;
    if (S > kMaxSegments) return CERB_EUNSUPPORTED;                  // the caller takes the stock ops there
    if (static_cast<int64_t>(H) * W > 0x7fffffff - 1024 || B > 65535 || sigma > 4096) return CERB_ETOOLARGE;
    if (B == 0) return CERB_OK;
    if (!ids || !seg_ids || !seg_category || !seg_flags || !seg_count || !gauss || !semantic || !foreground || !center || !offset ||
        !semantic_mask || !center_mask || !offset_mask || !center_points || !workspace)
        return CERB_EINVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < cerberus_panoptic_targets_workspace_bytes(B, H, W, S))
        return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int HW = H * W;
    const TargetWs w = target_ws(workspace, B, HW, S);
    const int64_t cells = static_cast<int64_t>(B) * S * 3;
    ptarget_zero_kernel<<<static_cast<int>(std::min<int64_t>((cells + kThreads - 1) / kThreads, 1024)), kThreads, 0, s>>>(w.moments, cells);
    int rc = launch_status();
    if (rc) return rc;
    const int64_t *sid = static_cast<const int64_t *>(seg_ids), *cnt = static_cast<const int64_t *>(seg_count);
    rc = ids_int64 ? launch_moments<int64_t>(ids, sid, cnt, w, B, HW, W, S, s) : launch_moments<int>(ids, sid, cnt, w, B, HW, W, S, s);
    if (rc) return rc;
    double *pts = static_cast<double *>(center_points);
    ptarget_finish_kernel<<<B, kThreads, 0, s>>>(w.moments, static_cast<const int64_t *>(seg_category), static_cast<const int *>(seg_flags), cnt,
                                                 w.cat, w.iyx, w.flags, pts, S, small_instance_area);
    rc = launch_status();
    if (rc) return rc;
    FillArgs a;
    a.semantic = static_cast<int64_t *>(semantic);
    a.foreground = static_cast<int64_t *>(foreground);
    a.center = static_cast<float *>(center);
    a.offset = static_cast<float *>(offset);
    a.semantic_mask = static_cast<float *>(semantic_mask);
    a.center_mask = static_cast<float *>(center_mask);
    a.offset_mask = static_cast<float *>(offset_mask);
    a.ignore_label = ignore_label;
    a.small_weight = small_instance_weight;
    a.sigma = sigma;
    a.ignore_stuff = ignore_stuff_in_offset != 0;
    a.ignore_crowd = ignore_crowd_in_semantic != 0;
    const dim3 grid(chunks(HW), B);
    const float *g = static_cast<const float *>(gauss);
    if (HW % kQuad == 0 && aligned16(a.semantic, a.foreground, a.center, a.offset) &&
        aligned16(a.semantic_mask, a.center_mask, a.offset_mask, w.rowmap))
        ptarget_fill_kernel<true><<<grid, kThreads, 0, s>>>(w.rowmap, w.cat, w.iyx, w.flags, pts, g, a, HW, W, S);
    else
        ptarget_fill_kernel<false><<<grid, kThreads, 0, s>>>(w.rowmap, w.cat, w.iyx, w.flags, pts, g, a, HW, W, S);
    return launch_status();
}

int64_t cerberus_panoptic_loss_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || loss_args_ok(B, H, W, 0, CERB_F32)) return 0;
    return loss_ws_bytes(B, H, W);
}

int cerberus_panoptic_loss_forward(const void *center_pred, const void *center_tgt, const void *center_mask, const void *offset_pred,
                                   const void *offset_tgt, const void *offset_mask, void *loss, void *state, void *workspace,
                                   int64_t workspace_bytes, int B, int H, int W, float center_weight, float offset_weight, int mode,
                                   int dtype, void *stream) {
    const int rc0 = loss_args_ok(B, H, W, mode, dtype);
    if (rc0) return rc0;
    if (B == 0) return CERB_OK;
    if (!center_pred || !center_tgt || !offset_pred || !offset_tgt || !loss || !state || !workspace) return CERB_EINVAL;   // masks may be null
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < loss_ws_bytes(B, H, W)) return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int HW = H * W;
    const Term c = term(center_pred, center_tgt, center_mask, B, HW, 1), o = term(offset_pred, offset_tgt, offset_mask, B, HW, 2);
    const int nc = chunks(c.n), no = chunks(o.n);
    float *parts = static_cast<float *>(workspace), *po = parts + 3 * nc;
    if (term_vec(c))
        ploss_partial_kernel<true, false><<<nc, kThreads, 0, s>>>(c, parts, parts + nc, parts + 2 * nc);
    else
        ploss_partial_kernel<false, false><<<nc, kThreads, 0, s>>>(c, parts, parts + nc, parts + 2 * nc);
    int rc = launch_status();
    if (rc) return rc;
    if (term_vec(o))
        ploss_partial_kernel<true, true><<<no, kThreads, 0, s>>>(o, po, po + no, po + 2 * no);
    else
        ploss_partial_kernel<false, true><<<no, kThreads, 0, s>>>(o, po, po + no, po + 2 * no);
    rc = launch_status();
    if (rc) return rc;
    ploss_final_kernel<<<1, kThreads, 0, s>>>(parts, nc, no, c.n, o.n, center_mask != nullptr, offset_mask != nullptr, center_weight,
                                              offset_weight, mode, static_cast<float *>(loss), static_cast<float *>(state));
    return launch_status();
}

int cerberus_panoptic_loss_backward(const void *center_pred, const void *center_tgt, const void *center_mask, const void *offset_pred,
                                    const void *offset_tgt, const void *offset_mask, const void *state, const void *grad_loss,
                                    void *grad_center, void *grad_offset, int B, int H, int W, int mode, int dtype, void *stream) {
    const int rc0 = loss_args_ok(B, H, W, mode, dtype);
    if (rc0) return rc0;
    if (B == 0) return CERB_OK;
    if (!center_pred || !center_tgt || !offset_pred || !offset_tgt || !state || !grad_loss || !grad_center || !grad_offset) return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int HW = H * W;
    const Term c = term(center_pred, center_tgt, center_mask, B, HW, 1), o = term(offset_pred, offset_tgt, offset_mask, B, HW, 2);
    const int nc = chunks(c.n), no = chunks(o.n);
    const float *st = static_cast<const float *>(state), *gl = static_cast<const float *>(grad_loss);
    float *gc = static_cast<float *>(grad_center), *go = static_cast<float *>(grad_offset);
    const bool vc = term_vec(c, gc), vo = term_vec(o, go);
    if (vc && vo)
        ploss_bwd_kernel<true, true><<<nc + no, kThreads, 0, s>>>(c, o, st, gl, gc, go, nc, mode);
    else if (vc)
        ploss_bwd_kernel<true, false><<<nc + no, kThreads, 0, s>>>(c, o, st, gl, gc, go, nc, mode);
    else if (vo)
        ploss_bwd_kernel<false, true><<<nc + no, kThreads, 0, s>>>(c, o, st, gl, gc, go, nc, mode);
    else
        ploss_bwd_kernel<false, false><<<nc + no, kThreads, 0, s>>>(c, o, st, gl, gc, go, nc, mode);
    return launch_status();
}

}  // extern "C"
