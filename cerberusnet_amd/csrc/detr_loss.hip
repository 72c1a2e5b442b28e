// detr_loss.hip -- the DETR set criterion on the device: the Hungarian matcher's cost matrix, the rectangular
// linear sum assignment (shortest augmenting paths, one wavefront per image, everything in LDS) and the three matched loss terms
// with their backward, for all decoder layers of a step at once.  fp32, 1 <= Q <= 256, 0 <= Tmax <= 128, Q Tmax <= 16384,
// 2 <= C1 <= 256.  Nothing is read on the host, no floating-point atomics: capturable, the same bits on every run.
//
//   logits (N,Q,C1), boxes (N,Q,4) cxcywh, N = L B layer-major; tgt_labels (B,Tmax) int64, tgt_boxes (B,Tmax,4), tgt_count (B,) int32;
//   image n reads target row n % B; a slot at or past tgt_count[b] is never read into a result.
#include "common.h"
#include "loss_reduce.h"

namespace cerb {
namespace {

constexpr int kMaxQ = 256;            // queries: 4 columns per lane when the queries are the columns
constexpr int kMaxT = 128;            // targets per image
constexpr int kMaxQT = 16384;         // Q * Tmax: a 64 KiB fp32 cost matrix in LDS
constexpr int kMaxC = 256;            // classes, the no-object class included
constexpr int kSlots = 4;             // columns per lane: kMaxQ / 64
constexpr int kThreads = kReduceThreads;   // the loss kernels: one thread per query
constexpr int kTerms = 5;             // per-image partial sums of the forward: w nll, w, L1, 1 - GIoU, #{argmax != no-object}
constexpr float kBigCost = 1.0e9f;    // what a non-finite cost entry becomes (status bit 0)
constexpr int kStatusNonFinite = 1;
constexpr int kStatusBadLabel = 2;    // a label outside [0, C1) among the counted targets: costed as non-finite, no-object in the loss

// ---- LDS of the two solving kernels: [cost nr x nc][u nr doubles][col4row nr][qmax Q][qsum Q][pbox Q x 4][tbox T x 4][tlabel T] ---
__host__ __device__ constexpr size_t solve_fixed_bytes() {
    return kMaxT * 8 + kMaxT * 4 + 2 * kMaxQ * 4 + kMaxQ * 16 + kMaxT * 16 + kMaxT * 4;
}
static size_t solve_lds_bytes(int Q, int Tmax) {
    const size_t cost_bytes = (static_cast<size_t>(std::max(Q * Tmax, 4)) * 4 + 15) & ~static_cast<size_t>(15);    // as carve() rounds it
    return cost_bytes + solve_fixed_bytes();
}

// order within one wavefront: LDS operations of a wave execute in program order; this keeps the compiler from moving or caching
// them across the point (it emits at most a wait, never a workgroup barrier)
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float4 load_box(const float *p, bool wide) {
    if (wide) return *reinterpret_cast<const float4 *>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void store_box(float *p, float4 v, bool wide) {
    if (wide) {
        *reinterpret_cast<float4 *>(p) = v;
    } else {
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}
static bool wide_ok(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// maximum and sum of exp(x - max) of one row of logits, in index order: the one softmax of every kernel here
__device__ __forceinline__ void softmax_stats(const float *__restrict__ row, int C1, float *m_out, float *s_out) {
    float m = row[0];
    for (int c = 1; c < C1; ++c) m = fmaxf(m, row[c]);
    float s = 0.f;
    for (int c = 0; c < C1; ++c) s += expf(row[c] - m);
    *m_out = m;
    *s_out = s;
}

__device__ __forceinline__ float giou_of(float4 p, float4 t) {
#pragma clang fp contract(off)
    const float px0 = p.x - 0.5f * p.z, py0 = p.y - 0.5f * p.w, px1 = p.x + 0.5f * p.z, py1 = p.y + 0.5f * p.w;
    const float tx0 = t.x - 0.5f * t.z, ty0 = t.y - 0.5f * t.w, tx1 = t.x + 0.5f * t.z, ty1 = t.y + 0.5f * t.w;
    const float area_p = (px1 - px0) * (py1 - py0), area_t = (tx1 - tx0) * (ty1 - ty0);
    const float iw = fmaxf(fminf(px1, tx1) - fmaxf(px0, tx0), 0.f), ih = fmaxf(fminf(py1, ty1) - fmaxf(py0, ty0), 0.f);
    const float inter = iw * ih;
    const float uni = area_p + area_t - inter;
    const float iou = inter / uni;
    const float ew = fmaxf(fmaxf(px1, tx1) - fminf(px0, tx0), 0.f), eh = fmaxf(fmaxf(py1, ty1) - fminf(py0, ty0), 0.f);
    const float area_c = ew * eh;
    return iou - (area_c - uni) / area_c;
}

__device__ __forceinline__ float l1_of(float4 p, float4 t) {
#pragma clang fp contract(off)
    return ((fabsf(p.x - t.x) + fabsf(p.y - t.y)) + fabsf(p.z - t.z)) + fabsf(p.w - t.w);
}

// ONE entry of the matching cost: w_bbox |p - t|_1 - w_class softmax(logits)[label] - w_giou GIoU.  `xl` is the logit at the
// label, (m, s) the row's softmax_stats.  No contraction: the kernel that writes the matrix and the kernel that solves it in LDS
// must form the same bits.
__device__ __forceinline__ float cost_entry(float4 p, float4 t, float xl, float m, float s, float w_class, float w_bbox, float w_giou) {
#pragma clang fp contract(off)
    const float prob = expf(xl - m) / s;
    return (w_bbox * l1_of(p, t) + w_class * (-prob)) + w_giou * (-giou_of(p, t));
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-Inf

// ---- the assignment -------------------------------------------------------------------------------------------------------------
// Shortest augmenting paths for the nr x nc problem, nr <= nc (Jonker-Volgenant as Crouse states it for rectangular matrices).
// One wavefront.  Column j lives in lane j % 64, slot j / 64: its dual v, its path length, its predecessor and its row stay in
// registers; the row duals u and col4row are in LDS.  Duals and path lengths are float64.  Every loop is a `for` whose bound is
// nr or nc: an augmentation closes one column per scan step (at most nc steps) and walks back at most nr rows; there are nr
// augmentations.  The per-step argmin is a butterfly in which the lowest column index wins a tie.
__device__ __forceinline__ void solve(const float *cost, int nr, int nc, double *u, int *col4row, int (&row4col)[kSlots]) {
    const int lane = threadIdx.x & 63;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double v[kSlots];
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        v[k] = 0.0;
        row4col[k] = -1;
    }
    for (int i = lane; i < nr; i += 64) {
        u[i] = 0.0;
        col4row[i] = -1;
    }
    wave_fence();
    for (int cur = 0; cur < nr; ++cur) {
        double sh[kSlots];
        int path[kSlots];
#pragma unroll
        for (int k = 0; k < kSlots; ++k) {
            sh[k] = inf;
            path[k] = -1;
        }
        unsigned closed = 0;            // bit k: this lane's column of slot k is closed (SC)
        double minv = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step < nc; ++step) {
            const double ui = u[i];
            const float *row = cost + i * nc;
            double best = inf;
            int bj = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < kSlots; ++k) {
                const int j = lane + 64 * k;
                if (j < nc && !((closed >> k) & 1u)) {
                    const double r = minv + static_cast<double>(row[j]) - ui - v[k];
                    if (r < sh[k]) {
                        sh[k] = r;
                        path[k] = i;
                    }
                    if (sh[k] < best) {
                        best = sh[k];
                        bj = j;
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int oj = __shfl_xor(bj, o, 64);
                if (ob < best || (ob == best && oj < bj)) {
                    best = ob;
                    bj = oj;
                }
            }
            if (bj >= nc) break;        // no open column (cannot happen: costs are finite and nr <= nc)
            minv = best;
            const int owner = bj & 63, slot = bj >> 6;
            int r4c = row4col[0];
#pragma unroll
            for (int k = 1; k < kSlots; ++k) r4c = (slot == k) ? row4col[k] : r4c;
            r4c = __shfl(r4c, owner, 64);
            if (lane == owner) closed |= 1u << slot;
            if (r4c < 0) {
                sink = bj;
                break;
            }
            i = r4c;
        }
        if (sink < 0) continue;
        // the duals: u of the scanned rows (the start row, and the row of every closed column but the sink), v of the closed columns
        if (lane == 0) u[cur] += minv;
#pragma unroll
        for (int k = 0; k < kSlots; ++k) {
            if ((closed >> k) & 1u) {
                const double d = minv - sh[k];
                if (row4col[k] >= 0) u[row4col[k]] += d;
                v[k] -= d;
            }
        }
        wave_fence();
        // augment along the predecessors, from the sink back to the start row (every lane writes the same col4row values)
        int j = sink;
        for (int step = 0; step <= nr; ++step) {
            const int owner = j & 63, slot = j >> 6;
            int pi = path[0];
#pragma unroll
            for (int k = 1; k < kSlots; ++k) pi = (slot == k) ? path[k] : pi;
            pi = __shfl(pi, owner, 64);
            if (pi < 0 || pi >= nr) break;
            if (lane == owner) {
#pragma unroll
                for (int k = 0; k < kSlots; ++k) row4col[k] = (slot == k) ? pi : row4col[k];
            }
            const int old = col4row[pi];
            col4row[pi] = j;
            j = old;
            if (pi == cur || j < 0 || j >= nc) break;
        }
        wave_fence();
    }
}

// rows = the smaller side: the targets when T <= Q, else the queries
__device__ __forceinline__ void write_match(int *__restrict__ match, int Q, int T, const int *col4row, const int (&row4col)[kSlots]) {
    const int lane = threadIdx.x & 63;
    if (T <= Q) {
#pragma unroll
        for (int k = 0; k < kSlots; ++k) {
            const int q = lane + 64 * k;
            if (q < Q) match[q] = row4col[k];
        }
    } else {
        for (int q = lane; q < Q; q += 64) match[q] = col4row[q];
    }
}

struct SolveLds {
    float *cost;
    double *u;
    int *col4row;
    float *qmax, *qsum, *pbox, *tbox;
    int *tlabel;
};

__device__ __forceinline__ SolveLds carve(unsigned char *base, int Q, int Tmax) {
    SolveLds s;
    size_t cost_bytes = static_cast<size_t>(max(Q * Tmax, 4)) * 4;
    cost_bytes = (cost_bytes + 15) & ~static_cast<size_t>(15);
    s.cost = reinterpret_cast<float *>(base);
    unsigned char *p = base + cost_bytes;
    s.u = reinterpret_cast<double *>(p);        p += kMaxT * 8;
    s.pbox = reinterpret_cast<float *>(p);      p += kMaxQ * 16;
    s.tbox = reinterpret_cast<float *>(p);      p += kMaxT * 16;
    s.col4row = reinterpret_cast<int *>(p);     p += kMaxT * 4;
    s.qmax = reinterpret_cast<float *>(p);      p += kMaxQ * 4;
    s.qsum = reinterpret_cast<float *>(p);      p += kMaxQ * 4;
    s.tlabel = reinterpret_cast<int *>(p);
    return s;
}

__device__ __forceinline__ int clamp_count(const int *tgt_count, int b, int Tmax) { return min(max(tgt_count[b], 0), Tmax); }

// lsap: a caller-given (N,Q,Tmax) matrix
__global__ __launch_bounds__(64) void detr_lsap_kernel(const float *__restrict__ cost, const int *__restrict__ tgt_count,
                                                      int *__restrict__ match, int *__restrict__ status, int B, int Q, int Tmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const SolveLds s = carve(lds, Q, Tmax);
    const int n = blockIdx.x, lane = threadIdx.x;
    const int T = clamp_count(tgt_count, n % B, Tmax);
    match += static_cast<size_t>(n) * Q;
    int row4col[kSlots];
    if (T == 0) {
        for (int q = lane; q < Q; q += 64) match[q] = -1;
        if (status && lane == 0) status[n] = 0;
        return;
    }
    const float *src = cost + static_cast<size_t>(n) * Q * Tmax;
    const bool swap = T <= Q;           // the targets are the rows
    int bad = 0;
    for (int idx = lane; idx < Q * T; idx += 64) {
        const int q = swap ? idx % Q : idx / T, t = swap ? idx / Q : idx % T;
        float c = src[q * Tmax + t];
        if (!finite_f(c)) {
            c = kBigCost;
            bad = kStatusNonFinite;
        }
        s.cost[swap ? t * Q + q : q * T + t] = c;
    }
    wave_fence();
    solve(s.cost, swap ? T : Q, swap ? Q : T, s.u, s.col4row, row4col);
    write_match(match, Q, T, s.col4row, row4col);
    if (status) {
        const int any = __any(bad) ? kStatusNonFinite : 0;
        if (lane == 0) status[n] = any;
    }
}

// hungarian_match: the cost matrix is formed in LDS and never written to memory
__global__ __launch_bounds__(64) void detr_hungarian_kernel(const float *__restrict__ logits, const float *__restrict__ boxes,
                                                           const int64_t *__restrict__ tgt_labels, const float *__restrict__ tgt_boxes,
                                                           const int *__restrict__ tgt_count, int *__restrict__ match,
                                                           int *__restrict__ status, int B, int Q, int C1, int Tmax, float w_class,
                                                           float w_bbox, float w_giou, int wide_p, int wide_t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const SolveLds s = carve(lds, Q, Tmax);
    const int n = blockIdx.x, lane = threadIdx.x, b = n % B;
    const int T = clamp_count(tgt_count, b, Tmax);
    match += static_cast<size_t>(n) * Q;
    int row4col[kSlots];
    if (T == 0) {
        for (int q = lane; q < Q; q += 64) match[q] = -1;
        if (lane == 0) status[n] = 0;
        return;
    }
    logits += static_cast<size_t>(n) * Q * C1;
    boxes += static_cast<size_t>(n) * Q * 4;
    int bad = 0;
    for (int q = lane; q < Q; q += 64) {
        softmax_stats(logits + q * C1, C1, &s.qmax[q], &s.qsum[q]);
        reinterpret_cast<float4 *>(s.pbox)[q] = load_box(boxes + q * 4, wide_p);
    }
    for (int t = lane; t < T; t += 64) {
        reinterpret_cast<float4 *>(s.tbox)[t] = load_box(tgt_boxes + (static_cast<size_t>(b) * Tmax + t) * 4, wide_t);
        const int64_t lab = tgt_labels[static_cast<size_t>(b) * Tmax + t];
        const bool ok = lab >= 0 && lab < C1;
        s.tlabel[t] = ok ? static_cast<int>(lab) : -1;
        if (!ok) bad |= kStatusBadLabel;
    }
    wave_fence();
    const bool swap = T <= Q;
    for (int idx = lane; idx < Q * T; idx += 64) {
        const int q = swap ? idx % Q : idx / T, t = swap ? idx / Q : idx % T;
        const int lab = s.tlabel[t];
        float c = kBigCost;
        if (lab >= 0)
            c = cost_entry(reinterpret_cast<const float4 *>(s.pbox)[q], reinterpret_cast<const float4 *>(s.tbox)[t], logits[q * C1 + lab],
                           s.qmax[q], s.qsum[q], w_class, w_bbox, w_giou);
        if (!finite_f(c)) {
            c = kBigCost;
            bad |= kStatusNonFinite;
        }
        s.cost[swap ? t * Q + q : q * T + t] = c;
    }
    wave_fence();
    solve(s.cost, swap ? T : Q, swap ? Q : T, s.u, s.col4row, row4col);
    write_match(match, Q, T, s.col4row, row4col);
    const int any = (__any(bad & kStatusNonFinite) ? kStatusNonFinite : 0) | (__any(bad & kStatusBadLabel) ? kStatusBadLabel : 0);
    if (lane == 0) status[n] = any;
}

// match_cost: the (N,Q,Tmax) matrix, padding columns zeroed
__global__ __launch_bounds__(kThreads) void detr_match_cost_kernel(const float *__restrict__ logits, const float *__restrict__ boxes,
                                                                  const int64_t *__restrict__ tgt_labels,
                                                                  const float *__restrict__ tgt_boxes, const int *__restrict__ tgt_count,
                                                                  float *__restrict__ cost, int *__restrict__ status, int B, int Q, int C1,
                                                                  int Tmax, float w_class, float w_bbox, float w_giou, int wide_p,
                                                                  int wide_t) {
    __shared__ float qmax[kMaxQ], qsum[kMaxQ];
    const int n = blockIdx.x, b = n % B, tid = threadIdx.x;
    const int T = clamp_count(tgt_count, b, Tmax);
    logits += static_cast<size_t>(n) * Q * C1;
    boxes += static_cast<size_t>(n) * Q * 4;
    cost += static_cast<size_t>(n) * Q * Tmax;
    if (T > 0)
        for (int q = tid; q < Q; q += kThreads) softmax_stats(logits + q * C1, C1, &qmax[q], &qsum[q]);
    __syncthreads();
    int bad = 0;
    for (int idx = tid; idx < Q * Tmax; idx += kThreads) {
        const int q = idx / Tmax, t = idx % Tmax;
        float c = 0.f;
        if (t < T) {
            const int64_t lab = tgt_labels[static_cast<size_t>(b) * Tmax + t];
            c = kBigCost;
            if (lab >= 0 && lab < C1)
                c = cost_entry(load_box(boxes + q * 4, wide_p), load_box(tgt_boxes + (static_cast<size_t>(b) * Tmax + t) * 4, wide_t),
                               logits[q * C1 + lab], qmax[q], qsum[q], w_class, w_bbox, w_giou);
            else
                bad |= kStatusBadLabel;
            if (!finite_f(c)) {
                c = kBigCost;
                bad |= kStatusNonFinite;
            }
        }
        cost[idx] = c;
    }
    if (status) {
        const int nf = __syncthreads_or(bad & kStatusNonFinite), bl = __syncthreads_or(bad & kStatusBadLabel);
        if (tid == 0) status[n] = (nf ? kStatusNonFinite : 0) | (bl ? kStatusBadLabel : 0);
    }
}

// ---- the set loss ---------------------------------------------------------------------------------------------------------------
// the class a query is trained to and its matched target (or -1): a match outside [0, T) counts as unmatched, a label outside
// [0, C1) as no-object
__device__ __forceinline__ int target_of(const int *match_row, int q, int T) {
    const int t = match_row[q];
    return (t >= 0 && t < T) ? t : -1;
}
__device__ __forceinline__ int class_of(const int64_t *labels_row, int t, int C1) {
    if (t < 0) return C1 - 1;
    const int64_t lab = labels_row[t];
    return (lab >= 0 && lab < C1) ? static_cast<int>(lab) : C1 - 1;
}

// one workgroup per image, one thread per query: kTerms float64 partial sums per image, lanes by butterfly, waves in wave order
__global__ __launch_bounds__(kThreads) void detr_loss_fwd_kernel(const float *__restrict__ logits, const float *__restrict__ boxes,
                                                                const int *__restrict__ match, const int64_t *__restrict__ tgt_labels,
                                                                const float *__restrict__ tgt_boxes, const int *__restrict__ tgt_count,
                                                                const float *__restrict__ weight, double *__restrict__ part, int B, int Q,
                                                                int C1, int Tmax, int wide_p, int wide_t) {
    __shared__ double red[kTerms][kThreads / 64];
    const int n = blockIdx.x, b = n % B, q = threadIdx.x;
    const int T = clamp_count(tgt_count, b, Tmax);
    double acc[kTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (q < Q) {
        const float *row = logits + (static_cast<size_t>(n) * Q + q) * C1;
        float m, s;
        softmax_stats(row, C1, &m, &s);
        float bv = row[0];
        int bi = 0;
        for (int c = 1; c < C1; ++c) {          // the first maximum; a NaN is the greatest, as in ATen
            const float x = row[c];
            if (x > bv || (x != x && bv == bv)) {
                bv = x;
                bi = c;
            }
        }
        const int t = target_of(match + static_cast<size_t>(n) * Q, q, T);
        const int cls = class_of(tgt_labels + static_cast<size_t>(b) * Tmax, t, C1);
        const float nll = (m + logf(s)) - row[cls];
        const float w = weight[cls];
        acc[0] = static_cast<double>(w) * static_cast<double>(nll);
        acc[1] = static_cast<double>(w);
        if (t >= 0) {
            const float4 p = load_box(boxes + (static_cast<size_t>(n) * Q + q) * 4, wide_p);
            const float4 g = load_box(tgt_boxes + (static_cast<size_t>(b) * Tmax + t) * 4, wide_t);
            acc[2] = static_cast<double>(l1_of(p, g));
            acc[3] = static_cast<double>(1.f - giou_of(p, g));
        }
        acc[4] = bi != C1 - 1 ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kTerms; ++k) {
        const double v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < kTerms) part[static_cast<size_t>(n) * kTerms + threadIdx.x] = waves_fold<FoldSum>(red[threadIdx.x]);
}

// the fixed-order finish: one workgroup, layer l adds its B images in index order
__global__ __launch_bounds__(kThreads) void detr_loss_finish_kernel(const double *__restrict__ part, const int *__restrict__ tgt_count,
                                                                   const float *__restrict__ num_boxes, float *__restrict__ losses,
                                                                   double *__restrict__ wsum, int L, int B, int Tmax) {
    const double nb = static_cast<double>(num_boxes[0]);
    for (int l = threadIdx.x; l < L; l += kThreads) {
        double a[4] = {0.0, 0.0, 0.0, 0.0}, card = 0.0;
        for (int b = 0; b < B; ++b) {
            const double *p = part + (static_cast<size_t>(l) * B + b) * kTerms;
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] += p[k];
            card += fabs(p[4] - static_cast<double>(clamp_count(tgt_count, b, Tmax)));
        }
        losses[l * 4 + 0] = static_cast<float>(a[0] / a[1]);
        losses[l * 4 + 1] = static_cast<float>(a[2] / nb);
        losses[l * 4 + 2] = static_cast<float>(a[3] / nb);
        losses[l * 4 + 3] = static_cast<float>(card / static_cast<double>(B));
        wsum[l] = a[1];
    }
}

// d(1 - GIoU)/d(cx, cy, w, h) of the predicted box times `g`.  Subgradients as ATen's: clamp(min=0) passes where its argument is
// >= 0, max / min split a tie in halves.
__device__ __forceinline__ float pick_gt(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }   // d max(a,b)/da
__device__ __forceinline__ float pick_lt(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }   // d min(a,b)/da

__device__ __forceinline__ float4 giou_loss_grad(float4 p, float4 t, float g) {
    const float px0 = p.x - 0.5f * p.z, py0 = p.y - 0.5f * p.w, px1 = p.x + 0.5f * p.z, py1 = p.y + 0.5f * p.w;
    const float tx0 = t.x - 0.5f * t.z, ty0 = t.y - 0.5f * t.w, tx1 = t.x + 0.5f * t.z, ty1 = t.y + 0.5f * t.w;
    const float pw = px1 - px0, ph = py1 - py0;
    const float area_p = pw * ph, area_t = (tx1 - tx0) * (ty1 - ty0);
    const float dw = fminf(px1, tx1) - fmaxf(px0, tx0), dh = fminf(py1, ty1) - fmaxf(py0, ty0);
    const float iw = fmaxf(dw, 0.f), ih = fmaxf(dh, 0.f);
    const float inter = iw * ih;
    const float uni = area_p + area_t - inter;
    const float cw = fmaxf(px1, tx1) - fminf(px0, tx0), ch = fmaxf(py1, ty1) - fminf(py0, ty0);
    const float ew = fmaxf(cw, 0.f), eh = fmaxf(ch, 0.f);
    const float area_c = ew * eh;
    // loss = 1 - iou + (area_c - uni) / area_c
    const float d_iou = -g;
    const float d_uni = -d_iou * inter / (uni * uni) - g / area_c;
    const float d_area_c = g * uni / (area_c * area_c);
    const float d_inter = d_iou / uni - d_uni;
    const float d_dw = dw >= 0.f ? d_inter * ih : 0.f, d_dh = dh >= 0.f ? d_inter * iw : 0.f;
    const float d_cw = cw >= 0.f ? d_area_c * eh : 0.f, d_ch = ch >= 0.f ? d_area_c * ew : 0.f;
    const float d_x0 = -d_dw * pick_gt(px0, tx0) - d_cw * pick_lt(px0, tx0) - d_uni * ph;
    const float d_x1 = d_dw * pick_lt(px1, tx1) + d_cw * pick_gt(px1, tx1) + d_uni * ph;
    const float d_y0 = -d_dh * pick_gt(py0, ty0) - d_ch * pick_lt(py0, ty0) - d_uni * pw;
    const float d_y1 = d_dh * pick_lt(py1, ty1) + d_ch * pick_gt(py1, ty1) + d_uni * pw;
    return make_float4(d_x0 + d_x1, d_y0 + d_y1, 0.5f * (d_x1 - d_x0), 0.5f * (d_y1 - d_y0));
}

__device__ __forceinline__ float sign_f(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : v); }   // sign(0) = 0, NaN stays NaN

// one workgroup per image: every element of grad_logits (N,Q,C1) and grad_boxes (N,Q,4)
__global__ __launch_bounds__(kThreads) void detr_loss_bwd_kernel(const float *__restrict__ logits, const float *__restrict__ boxes,
                                                                const int *__restrict__ match, const int64_t *__restrict__ tgt_labels,
                                                                const float *__restrict__ tgt_boxes, const int *__restrict__ tgt_count,
                                                                const float *__restrict__ weight, const float *__restrict__ num_boxes,
                                                                const double *__restrict__ wsum, const float *__restrict__ grad_losses,
                                                                float *__restrict__ grad_logits, float *__restrict__ grad_boxes, int B,
                                                                int Q, int C1, int Tmax, int wide_p, int wide_t, int wide_g) {
    __shared__ float qmax[kMaxQ], qsum[kMaxQ], qcoef[kMaxQ];
    __shared__ int qcls[kMaxQ];
    const int n = blockIdx.x, b = n % B, l = n / B, q = threadIdx.x;
    const int T = clamp_count(tgt_count, b, Tmax);
    const float g_ce = grad_losses[l * 4 + 0], nb = num_boxes[0];
    const float g_l1 = grad_losses[l * 4 + 1] / nb, g_giou = grad_losses[l * 4 + 2] / nb;
    logits += static_cast<size_t>(n) * Q * C1;
    grad_logits += static_cast<size_t>(n) * Q * C1;
    if (q < Q) {
        softmax_stats(logits + q * C1, C1, &qmax[q], &qsum[q]);
        const int t = target_of(match + static_cast<size_t>(n) * Q, q, T);
        const int cls = class_of(tgt_labels + static_cast<size_t>(b) * Tmax, t, C1);
        qcls[q] = cls;
        qcoef[q] = static_cast<float>(static_cast<double>(g_ce) * static_cast<double>(weight[cls]) / wsum[l]);
        float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0) {
            const float4 p = load_box(boxes + (static_cast<size_t>(n) * Q + q) * 4, wide_p);
            const float4 tb = load_box(tgt_boxes + (static_cast<size_t>(b) * Tmax + t) * 4, wide_t);
            const float4 gg = giou_loss_grad(p, tb, g_giou);
            gb = make_float4(g_l1 * sign_f(p.x - tb.x) + gg.x, g_l1 * sign_f(p.y - tb.y) + gg.y, g_l1 * sign_f(p.z - tb.z) + gg.z,
                             g_l1 * sign_f(p.w - tb.w) + gg.w);
        }
        store_box(grad_boxes + (static_cast<size_t>(n) * Q + q) * 4, gb, wide_g);
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < Q * C1; idx += kThreads) {
        const int qq = idx / C1, c = idx % C1;
        const float p = expf(logits[idx] - qmax[qq]) / qsum[qq];
        grad_logits[idx] = qcoef[qq] * (p - (c == qcls[qq] ? 1.f : 0.f));
    }
}

int shape_ok(int N, int B, int Q, int C1, int Tmax, int dtype) {
    if (dtype < CERB_F32 || dtype > CERB_F64) return CERB_EDTYPE;
    if (dtype != CERB_F32) return CERB_EUNSUPPORTED;
    if (N < 0 || B <= 0 || Q <= 0 || C1 < 2 || Tmax < 0) return CERB_EINVAL;
    if (Q > kMaxQ || Tmax > kMaxT || Q * Tmax > kMaxQT || C1 > kMaxC) return CERB_EUNSUPPORTED;
    if (N % B != 0) return CERB_EINVAL;
    if (static_cast<int64_t>(N) * Q * std::max(C1, std::max(Tmax, 4)) > 0x7fffffffll) return CERB_ETOOLARGE;
    return CERB_OK;
}

std::atomic<uint64_t> g_lsap_lds{0}, g_hungarian_lds{0};

}  // namespace
}  // namespace cerb

using namespace cerb;

extern "C" {

int cerberus_detr_fused_ok(int Q, int Tmax, int C1) { return shape_ok(1, 1, Q, C1, Tmax, CERB_F32) == CERB_OK ? 1 : 0; }

int64_t cerberus_detr_workspace_bytes(int N) { return N > 0 ? static_cast<int64_t>(N) * kTerms * 8 : 0; }

int cerberus_detr_match_cost(const void *logits, const void *boxes, const void *tgt_labels, const void *tgt_boxes, const void *tgt_count,
                             void *cost, void *status, int N, int B, int Q, int C1, int Tmax, float w_class, float w_bbox, float w_giou,
                             int dtype, void *stream) {
    const int rc = shape_ok(N, B, Q, C1, Tmax, dtype);
    if (rc) return rc;
    if (N == 0) return CERB_OK;
    if (!logits || !boxes || !tgt_count || (Tmax > 0 && (!tgt_labels || !tgt_boxes || !cost))) return CERB_EINVAL;
    if (Tmax == 0 && !status) return CERB_OK;
    detr_match_cost_kernel<<<N, kThreads, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const float *>(logits), static_cast<const float *>(boxes), static_cast<const int64_t *>(tgt_labels),
        static_cast<const float *>(tgt_boxes), static_cast<const int *>(tgt_count), static_cast<float *>(cost), static_cast<int *>(status),
        B, Q, C1, Tmax, w_class, w_bbox, w_giou, wide_ok(boxes), wide_ok(tgt_boxes));
    return launch_status();
}

int cerberus_detr_lsap(const void *cost, const void *tgt_count, void *match, void *status, int N, int B, int Q, int Tmax, void *stream) {
    int rc = shape_ok(N, B, Q, 2, Tmax, CERB_F32);
    if (rc) return rc;
    if (N == 0) return CERB_OK;
    if (!tgt_count || !match || (Tmax > 0 && !cost)) return CERB_EINVAL;
    const size_t lds = solve_lds_bytes(Q, Tmax);
    rc = ensure_lds(detr_lsap_kernel, lds, &g_lsap_lds);
    if (rc) return rc;
    detr_lsap_kernel<<<N, 64, lds, static_cast<hipStream_t>(stream)>>>(static_cast<const float *>(cost), static_cast<const int *>(tgt_count),
                                                                      static_cast<int *>(match), static_cast<int *>(status), B, Q, Tmax);
    return launch_status();
}

int cerberus_detr_hungarian_match(const void *logits, const void *boxes, const void *tgt_labels, const void *tgt_boxes,
                                  const void *tgt_count, void *match, void *status, int N, int B, int Q, int C1, int Tmax, float w_class,
                                  float w_bbox, float w_giou, int dtype, void *stream) {
    int rc = shape_ok(N, B, Q, C1, Tmax, dtype);
    if (rc) return rc;
    if (N == 0) return CERB_OK;
    if (!logits || !boxes || !tgt_count || !match || !status || (Tmax > 0 && (!tgt_labels || !tgt_boxes))) return CERB_EINVAL;
    const size_t lds = solve_lds_bytes(Q, Tmax);
    rc = ensure_lds(detr_hungarian_kernel, lds, &g_hungarian_lds);
    if (rc) return rc;
    detr_hungarian_kernel<<<N, 64, lds, static_cast<hipStream_t>(stream)>>>(
        static_cast<const float *>(logits), static_cast<const float *>(boxes), static_cast<const int64_t *>(tgt_labels),
        static_cast<const float *>(tgt_boxes), static_cast<const int *>(tgt_count), static_cast<int *>(match), static_cast<int *>(status), B,
        Q, C1, Tmax, w_class, w_bbox, w_giou, wide_ok(boxes), wide_ok(tgt_boxes));
    return launch_status();
}

int cerberus_detr_set_loss_forward(const void *logits, const void *boxes, const void *match, const void *tgt_labels, const void *tgt_boxes,
                                   const void *tgt_count, const void *weight, const void *num_boxes, void *losses, void *wsum,
                                   void *workspace, int64_t workspace_bytes, int N, int B, int Q, int C1, int Tmax, int dtype,
                                   void *stream) {
    const int rc = shape_ok(N, B, Q, C1, Tmax, dtype);
    if (rc) return rc;
    if (N == 0) return CERB_OK;
    if (!logits || !boxes || !match || !tgt_count || !weight || !num_boxes || !losses || !wsum || (Tmax > 0 && (!tgt_labels || !tgt_boxes)))
        return CERB_EINVAL;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) || workspace_bytes < cerberus_detr_workspace_bytes(N)) return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    detr_loss_fwd_kernel<<<N, kThreads, 0, s>>>(static_cast<const float *>(logits), static_cast<const float *>(boxes),
                                                static_cast<const int *>(match), static_cast<const int64_t *>(tgt_labels),
                                                static_cast<const float *>(tgt_boxes), static_cast<const int *>(tgt_count),
                                                static_cast<const float *>(weight), static_cast<double *>(workspace), B, Q, C1, Tmax,
                                                wide_ok(boxes), wide_ok(tgt_boxes));
    const int rc2 = launch_status();
    if (rc2) return rc2;
    detr_loss_finish_kernel<<<1, kThreads, 0, s>>>(static_cast<const double *>(workspace), static_cast<const int *>(tgt_count),
                                                   static_cast<const float *>(num_boxes), static_cast<float *>(losses),
                                                   static_cast<double *>(wsum), N / B, B, Tmax);
    return launch_status();
}

int cerberus_detr_set_loss_backward(const void *logits, const void *boxes, const void *match, const void *tgt_labels, const void *tgt_boxes,
                                    const void *tgt_count, const void *weight, const void *num_boxes, const void *wsum,
                                    const void *grad_losses, void *grad_logits, void *grad_boxes, int N, int B, int Q, int C1, int Tmax,
                                    int dtype, void *stream) {
    const int rc = shape_ok(N, B, Q, C1, Tmax, dtype);
    if (rc) return rc;
    if (N == 0) return CERB_OK;
    if (!logits || !boxes || !match || !tgt_count || !weight || !num_boxes || !wsum || !grad_losses || !grad_logits || !grad_boxes ||
        (Tmax > 0 && (!tgt_labels || !tgt_boxes)))
        return CERB_EINVAL;
    detr_loss_bwd_kernel<<<N, kThreads, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const float *>(logits), static_cast<const float *>(boxes), static_cast<const int *>(match),
        static_cast<const int64_t *>(tgt_labels), static_cast<const float *>(tgt_boxes), static_cast<const int *>(tgt_count),
        static_cast<const float *>(weight), static_cast<const float *>(num_boxes), static_cast<const double *>(wsum),
        static_cast<const float *>(grad_losses), static_cast<float *>(grad_logits), static_cast<float *>(grad_boxes), B, Q, C1, Tmax,
        wide_ok(boxes), wide_ok(tgt_boxes), wide_ok(grad_boxes));
    return launch_status();
}

}  // extern "C"
