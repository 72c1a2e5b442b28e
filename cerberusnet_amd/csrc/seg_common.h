// seg_common.h -- what seg_loss.hip and seg_ohem.hip share: the workgroup's shape, a label as the kernels use it, the
// streamed log-sum-exp step and one element of the gradient.  Everything here has internal linkage and is forced inline:
// each source that includes it compiles its own copy, with contraction into fma off in both (the pragma is in the sources).
#pragma once
#include "common.h"
#include "loss_reduce.h"

namespace cerb {
namespace {

constexpr int kThreads = kReduceThreads;
constexpr int kQuad = 4;                      // consecutive pixels folded first (the vector route's pixels per lane)
constexpr int kChunk = kThreads * kQuad;      // pixels per workgroup, both routes

// a label as the kernels use it: cls = the class, or -1 when no class plane matches (ignored or out of range)
struct Label {
    bool valid;       // not the ignore label
    int cls;
};

__device__ __forceinline__ Label classify(int64_t t, int64_t ignore, int C) {
    Label l;
    l.valid = t != ignore;
    l.cls = (l.valid && static_cast<uint64_t>(t) < static_cast<uint64_t>(C)) ? static_cast<int>(t) : -1;
    return l;
}

// one class plane's value of one pixel: m = max so far, s = sum of exp(x - m) so far.  A NaN x makes s NaN and leaves m.
// x == m takes d = 0 by a select: for finite values x - m is that same zero (its sign reaches neither fabsf's result nor
// d > 0), so no finite path changes a bit; for x = m = -inf (a class switched off while every class before it was too) the
// difference would be inf - inf = NaN, and is now the step "one more term of weight exp(-inf)": m stays -inf, and the
// first finite x that follows resets s to 1 through e = exp(-inf) = 0.
__device__ __forceinline__ void lse_step(float x, bool hit, float &m, float &s, float &xt) {
    const float d = x == m ? 0.f : x - m;
    const float e = expf(-fabsf(d));
    s = d > 0.f ? s * e + 1.f : s + e;
    m = fmaxf(m, x);
    xt = hit ? x : xt;
}

// one element of the gradient; `a` = coef * w[t]; `live` = the pixel counts (valid, in range, weight not 0)
__device__ __forceinline__ float grad_elem(float x, float lse, float a, bool hit, bool live) {
    const float g = a * (expf(x - lse) - (hit ? 1.f : 0.f));
    return live ? g : 0.f;       // a select: a NaN coefficient still leaves 0.0f at a pixel that does not count
}

__device__ __forceinline__ float pixel_coef(const Label &l, float coef, const float *__restrict__ w, bool &live) {
    const float wt = l.cls >= 0 ? w[l.cls] : 0.f;
    live = l.cls >= 0 && wt != 0.f;
    return coef * wt;
}

inline int chunks(int64_t n) { return static_cast<int>((n + kChunk - 1) / kChunk); }

inline bool aligned16(const void *a, const void *b, const void *c, const void *d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

}  // namespace
}  // namespace cerb
