// loss_reduce.h -- the fixed-order folds of every fused loss and metric op: photometric.hip, census.hip, seg_loss.hip and
// seg_ohem.hip (through seg_common.h), depth_loss.hip, metrics.hip, rmi_loss.hip, panoptic_train.hip, detr_loss.hip and
// ocr_head.hip.  The order of these folds is the bit-level contract of those ops, and this is its only home:
//   wave  : a butterfly over the wave's 64 lanes, offsets 32, 16, .. 1: v = op(v, the value of lane ^ offset)
//   block : lane 0 of each of the 4 waves leaves its wave's fold in red[wave]; one barrier; op(op(r0, r1), op(r2, r3))
//   tree  : a finish kernel of one workgroup reads the partials by i = threadIdx.x; i += kReduceThreads into one value per
//           thread, and an LDS tree halves the kReduceThreads values: row[t] = op(row[t], row[t + s]), s = 128, 64, .. 1, one
//           barrier per step whatever the number of rows
// No floating-point atomics: the same bits on every run and in a replayed graph.  The helpers only add or take a maximum:
// nothing in them can contract into an fma.  Everything here has internal linkage: each source that includes it gets its own
// copy.
#pragma once
#include "common.h"

namespace cerb {
namespace {

constexpr int kReduceThreads = 256;   // 4 waves: the workgroup size of every kernel that calls a block or a tree fold

struct FoldSum {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct FoldMax {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return max(a, b); }
};

// ---- wave: the same fold in every lane and every run: the order of a butterfly does not depend on timing ---------------
template <class Op, class T> __device__ __forceinline__ T wave_fold(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op()(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- block: the workgroup's 4 waves in wave order (every thread returns the same value); red: 4 elements, free on entry
template <class Op, class T> __device__ __forceinline__ T waves_fold(const T *red) {
    return Op()(Op()(red[0], red[1]), Op()(red[2], red[3]));
}

template <class Op, class T> __device__ __forceinline__ T block_fold(T v, T *red) {
    v = wave_fold<Op>(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return waves_fold<Op>(red);
}

template <class T> __device__ __forceinline__ T wave_sum(T v) { return wave_fold<FoldSum>(v); }
template <class T> __device__ __forceinline__ T block_sum(T v, T *red) { return block_fold<FoldSum>(v, red); }
template <class T> __device__ __forceinline__ T block_max(T v, T *red) { return block_fold<FoldMax>(v, red); }

// a lane's 4 consecutive pixels, left to right, before the wave's butterfly
__device__ __forceinline__ float quad_sum(const float (&v)[4]) { return ((v[0] + v[1]) + v[2]) + v[3]; }

// ---- tree: every argument is a row T[kReduceThreads] or a stack of rows T[R][kReduceThreads] in LDS that each thread has
// just written at threadIdx.x (the barrier behind those writes is the first one here); rows of different element types may be
// mixed; the result of each row is left in its element 0, visible to every thread
template <class Op, class T> __device__ __forceinline__ void tree_step(T (&row)[kReduceThreads], int s) {
    const T upper = row[threadIdx.x + s];
    row[threadIdx.x] = Op()(row[threadIdx.x], upper);
}
template <class Op, class T, int R> __device__ __forceinline__ void tree_step(T (&rows)[R][kReduceThreads], int s) {
#pragma unroll
    for (int r = 0; r < R; ++r) tree_step<Op>(rows[r], s);
}

template <class Op, class... Rows> __device__ __forceinline__ void tree_fold(Rows &...rows) {
    __syncthreads();
    for (int s = kReduceThreads / 2; s > 0; s >>= 1) {
        if (static_cast<int>(threadIdx.x) < s) (tree_step<Op>(rows, s), ...);
        __syncthreads();
    }
}

template <class... Rows> __device__ __forceinline__ void tree_sum(Rows &...rows) { tree_fold<FoldSum>(rows...); }

// ---- the second launch of photometric.hip and census.hip: one workgroup, fixed order -----------------------------------
// out[0] = (sum(p0[0..n)) / count0 + sum(p1[0..n)) / count1) * scale; p1 may be null
__global__ __launch_bounds__(kReduceThreads) void final_sum_kernel(const float *__restrict__ p0, const float *__restrict__ p1, int n,
                                                             float count0, float count1, float scale, float *__restrict__ out) {
    __shared__ float red[2][kReduceThreads];
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < n; i += kReduceThreads) {
        a += p0[i];
        if (p1) b += p1[i];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    tree_sum(red);
    if (threadIdx.x == 0) out[0] = p1 ? (red[0][0] / count0 + red[1][0] / count1) * scale : (red[0][0] / count0) * scale;
}

}  // namespace
}  // namespace cerb
