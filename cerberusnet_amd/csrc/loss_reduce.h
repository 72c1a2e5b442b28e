// loss_reduce.h -- the fixed-order reduction shared by the scalar loss ops (photometric.hip, census.hip): every tile
// workgroup folds its lanes by a butterfly and its 4 waves in wave order into ONE partial, and a second launch of one
// workgroup adds the partials in index order.  No floating-point atomics: the same bits on every run and in a replayed
// graph.  Everything here has internal linkage: each source that includes it gets its own copy.
#pragma once
#include "common.h"

namespace cerb {
namespace {

constexpr int kReduceThreads = 256;   // 4 waves: the workgroup size of every kernel that calls block_sum

// the same fold in every lane and every run: the order of a butterfly does not depend on timing
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the workgroup's 4 waves in wave order (every thread returns the same value)
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- the second launch of every reduction: one workgroup, fixed order ---------------------------------------------
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
    __syncthreads();
    for (int s = kReduceThreads / 2; s > 0; s >>= 1) {
        if (static_cast<int>(threadIdx.x) < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = p1 ? (red[0][0] / count0 + red[1][0] / count1) * scale : (red[0][0] / count0) * scale;
}

}  // namespace
}  // namespace cerb
