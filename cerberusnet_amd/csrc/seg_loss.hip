// seg_loss.hip -- the segmentation head's loss as ONE differentiable scalar op, fp32 logits, int64 labels:
// weighted cross-entropy with an ignore label, reduced to a mean, times the reference's focal factor of that MEAN.
//
// Reference (nnet_training/loss_functions/seg_losses.py:121-190, FocalLoss2D / SegCrossEntropy): F.cross_entropy(logits,
// target, weight=w, ignore_index=i) -- log_softmax (read + write of the (B,C,H,W) logits), nll_loss2d (read), and in the
// backward nll_loss2d_backward (write) and log_softmax_backward (two reads + write) -- then pow(1 - exp(-ce), gamma) * ce on
// the scalar.  Here: one read of the logits forward, one read + one write backward.
//
//   valid(p) = t(p) != ignore_index,   lse(p) = log sum_c exp(x_c(p))
//   num = sum_{valid p} w[t(p)] (lse(p) - x_{t(p)}(p)),   den = sum_{valid p} w[t(p)],   ce = num / den
//   loss = ce (gamma == 0)   or   (1 - exp(-ce))^gamma ce
//   grad_x_c(p) = grad_loss (dloss/dce) / den * w[t(p)] (exp(x_c(p) - lse(p)) - [c == t(p)])      at a valid pixel, else 0
//
// The classes are streamed: a running maximum m and the sum s of exp(x - m) per pixel (one expf per element: the smaller of
// the two exponents of a step is always 0), x_t picked out on the way by a select.  No per-class register array, any C >= 2.
//
// Two routes, chosen from the shape and the pointers.  Both give a workgroup the SAME 1024 consecutive pixels of the
// flattened (B,H,W) map, run the same per-pixel arithmetic (contraction into fma is off in this file, so the two routes
// cannot be compiled into different roundings) and fold a workgroup's pixels in the same order -- groups of four
// consecutive pixels left to right, the 64 groups of a wave by a butterfly, the 4 waves in wave order: a call on
// misaligned pointers gives the bits of the aligned call.
//   vector : H*W % 4 == 0 and 16-byte aligned pointers: a lane owns 4 consecutive pixels of one batch item, one 16-byte load
//            per class plane, two for its labels
//   scalar : a lane owns one pixel at a time, four times; the per-pixel terms go through LDS to the lane that folds them
// A second launch of one workgroup adds the partials in a fixed order and leaves ce, den and (dloss/dce) / den in device
// memory for the backward: no floating-point atomics, no host round trip, the same bits on every run and in a replayed graph.
//
// Labels never form an address unless they lie in [0, C): an out-of-range label that is not the ignore label adds NaN to
// num (stock PyTorch raises a device-side assertion there) and gets a zero gradient.  An ignored pixel is skipped by
// selection: a NaN logit there changes nothing, and its gradient is 0.0f whatever the upstream gradient holds.
// Logits of -inf (classes switched off) may sit anywhere in a pixel that keeps a finite one: lse is that of the others and
// their gradient is 0.0f.  A counted pixel whose loss is not finite (its target at -inf, every logit -inf, a +inf logit) makes
// the loss +inf or NaN, never a dropped term.
#include "seg_common.h"

#pragma clang fp contract(off)

namespace cerb {
namespace {

constexpr int kHistMaxClasses = 2048;         // LDS bins of class_histogram_kernel

// what a pixel adds to num and den
__device__ __forceinline__ void pixel_terms(const Label &l, float lse, float xt, const float *__restrict__ w, float &n, float &d) {
    n = 0.f;
    d = 0.f;
    if (l.valid) {
        if (l.cls >= 0) {
            const float wt = w[l.cls];
            n = wt * (lse - xt);
            d = wt;
        } else {
            n = __builtin_nanf("");
        }
    }
}

// ---- forward --------------------------------------------------------------------------------------------------------
template <bool kVec>
__global__ __launch_bounds__(kThreads) void seg_ce_fwd_kernel(const float *__restrict__ x, const int64_t *__restrict__ t,
                                                              const float *__restrict__ w, float *__restrict__ lse_out,
                                                              float *__restrict__ pnum, float *__restrict__ pden, int C, int HW, int N,
                                                              int64_t ignore) {
    __shared__ float red_n[4], red_d[4];
    __shared__ float stage[kVec ? 2 : 2 * kChunk];
    const int base = blockIdx.x * kChunk;
    float n4[kQuad], d4[kQuad];
    if constexpr (kVec) {
        const int p0 = base + threadIdx.x * kQuad;
#pragma unroll
        for (int k = 0; k < kQuad; ++k) n4[k] = d4[k] = 0.f;
        if (p0 < N) {       // N % 4 == 0 on this route: a lane's 4 pixels are all inside, and inside one batch item
            const int b = p0 / HW, r = p0 - b * HW;
            const float *px = x + static_cast<int64_t>(b) * C * HW + r;
            const longlong2 ta = *reinterpret_cast<const longlong2 *>(t + p0), tb = *reinterpret_cast<const longlong2 *>(t + p0 + 2);
            const Label lab[kQuad] = {classify(ta.x, ignore, C), classify(ta.y, ignore, C), classify(tb.x, ignore, C),
                                      classify(tb.y, ignore, C)};
            const float4 v0 = *reinterpret_cast<const float4 *>(px);
            float m[kQuad] = {v0.x, v0.y, v0.z, v0.w}, s[kQuad], xt[kQuad];
#pragma unroll
            for (int k = 0; k < kQuad; ++k) {
                s[k] = 1.f;
                xt[k] = lab[k].cls == 0 ? m[k] : 0.f;
            }
#pragma unroll 4
            for (int c = 1; c < C; ++c) {
                const float4 v = *reinterpret_cast<const float4 *>(px + static_cast<int64_t>(c) * HW);
                const float vv[kQuad] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < kQuad; ++k) lse_step(vv[k], c == lab[k].cls, m[k], s[k], xt[k]);
            }
            float l[kQuad];
#pragma unroll
            for (int k = 0; k < kQuad; ++k) {
                l[k] = m[k] + logf(s[k]);
                pixel_terms(lab[k], l[k], xt[k], w, n4[k], d4[k]);
            }
            *reinterpret_cast<float4 *>(lse_out + p0) = make_float4(l[0], l[1], l[2], l[3]);
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < kQuad; ++j) {
            const int q = j * kThreads + threadIdx.x, p = base + q;
            float n = 0.f, d = 0.f;
            if (p < N) {
                const int b = p / HW, r = p - b * HW;
                const float *px = x + static_cast<int64_t>(b) * C * HW + r;
                const Label lab = classify(t[p], ignore, C);
                float m = px[0], s = 1.f, xt = lab.cls == 0 ? m : 0.f;
#pragma unroll 4
                for (int c = 1; c < C; ++c) lse_step(px[static_cast<int64_t>(c) * HW], c == lab.cls, m, s, xt);
                const float l = m + logf(s);
                pixel_terms(lab, l, xt, w, n, d);
                lse_out[p] = l;
            }
            stage[q] = n;
            stage[kChunk + q] = d;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            n4[k] = stage[threadIdx.x * kQuad + k];
            d4[k] = stage[kChunk + threadIdx.x * kQuad + k];
        }
    }
    const float n = quad_sum(n4), d = quad_sum(d4);
    const float tn = block_sum(n, red_n), td = block_sum(d, red_d);
    if (threadIdx.x == 0) {
        pnum[blockIdx.x] = tn;
        pden[blockIdx.x] = td;
    }
}

// ---- the second launch: one workgroup, fixed order ----------------------------------------------------------------------
// loss[0] and state = [ce, den, (dloss/dce) / den, 0]
__global__ __launch_bounds__(kThreads) void seg_ce_final_kernel(const float *__restrict__ pnum, const float *__restrict__ pden, int n,
                                                                float gamma, float *__restrict__ loss, float *__restrict__ state) {
    __shared__ float red[2][kThreads];
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        a += pnum[i];
        b += pden[i];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    tree_sum(red);
    if (threadIdx.x == 0) {
        const float num = red[0][0], den = red[1][0];
        const float ce = num / den;              // 0 / 0 = NaN when nothing counts, as the stock mean
        float value = ce, slope = 1.f;
        if (gamma != 0.f) {                      // gamma == 0 is exactly ce: a branch, not pow(., 0)
            const float q = -expm1f(-ce);        // 1 - exp(-ce) without the cancellation at small ce
            const float f = powf(q, gamma);
            value = f * ce;
            // ce == 0 exactly with gamma < 1: powf(0, gamma - 1) is Inf and the slope 0 * Inf = NaN, as the stock pow backward's
            slope = f + ce * (gamma * powf(q, gamma - 1.f) * expf(-ce));
        }
        loss[0] = value;
        state[0] = ce;
        state[1] = den;
        state[2] = slope / den;
        state[3] = 0.f;
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------
template <bool kVec>
__global__ __launch_bounds__(kThreads) void seg_ce_bwd_kernel(const float *__restrict__ x, const int64_t *__restrict__ t,
                                                              const float *__restrict__ w, const float *__restrict__ lse,
                                                              const float *__restrict__ state, const float *__restrict__ grad_loss,
                                                              float *__restrict__ gx, int C, int HW, int N, int64_t ignore) {
    // both read here, from device memory: no host synchronisation.  Scaling by a power of two is exact in every product
    // below: the gradient is exactly linear in such an upstream gradient.
    const float coef = grad_loss[0] * state[2];
    const int base = blockIdx.x * kChunk;
    if constexpr (kVec) {
        const int p0 = base + threadIdx.x * kQuad;
        if (p0 >= N) return;
        const int b = p0 / HW, r = p0 - b * HW;
        const int64_t item = static_cast<int64_t>(b) * C * HW + r;
        const longlong2 ta = *reinterpret_cast<const longlong2 *>(t + p0), tb = *reinterpret_cast<const longlong2 *>(t + p0 + 2);
        const Label lab[kQuad] = {classify(ta.x, ignore, C), classify(ta.y, ignore, C), classify(tb.x, ignore, C),
                                  classify(tb.y, ignore, C)};
        const float4 l4 = *reinterpret_cast<const float4 *>(lse + p0);
        const float l[kQuad] = {l4.x, l4.y, l4.z, l4.w};
        float a[kQuad];
        bool live[kQuad];
#pragma unroll
        for (int k = 0; k < kQuad; ++k) a[k] = pixel_coef(lab[k], coef, w, live[k]);
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            const int64_t o = item + static_cast<int64_t>(c) * HW;
            const float4 v = *reinterpret_cast<const float4 *>(x + o);
            const float vv[kQuad] = {v.x, v.y, v.z, v.w};
            float g[kQuad];
#pragma unroll
            for (int k = 0; k < kQuad; ++k) g[k] = grad_elem(vv[k], l[k], a[k], c == lab[k].cls, live[k]);
            *reinterpret_cast<float4 *>(gx + o) = make_float4(g[0], g[1], g[2], g[3]);
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < kQuad; ++j) {
            const int p = base + j * kThreads + threadIdx.x;
            if (p >= N) return;
            const int b = p / HW, r = p - b * HW;
            const int64_t item = static_cast<int64_t>(b) * C * HW + r;
            const Label lab = classify(t[p], ignore, C);
            const float l = lse[p];
            bool live;
            const float a = pixel_coef(lab, coef, w, live);
#pragma unroll 4
            for (int c = 0; c < C; ++c) {
                const int64_t o = item + static_cast<int64_t>(c) * HW;
                gx[o] = grad_elem(x[o], l, a, c == lab.cls, live);
            }
        }
    }
}

// ---- class histogram ------------------------------------------------------------------------------------------------
// counts[c] += the labels equal to c, for c in [0, C) other than `ignore`; counts is zeroed on the stream by the launch
// function with a kernel node of its own (as occlusion.hip zeroes its accumulators).  Integers throughout: LDS adds per
// workgroup, one 64-bit global add per non-empty bin -- any order, same result.
__global__ __launch_bounds__(kThreads) void class_histogram_zero_kernel(unsigned long long *__restrict__ counts, int C) {
    for (int i = threadIdx.x; i < C; i += kThreads) counts[i] = 0ull;
}

__global__ __launch_bounds__(kThreads) void class_histogram_kernel(const int64_t *__restrict__ t, unsigned long long *__restrict__ counts,
                                                                   int64_t n, int C, int64_t ignore) {
    __shared__ unsigned int bins[kHistMaxClasses];
    for (int i = threadIdx.x; i < C; i += kThreads) bins[i] = 0u;
    __syncthreads();
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        const Label l = classify(t[i], ignore, C);
        if (l.cls >= 0) atomicAdd(&bins[l.cls], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += kThreads) {
        const unsigned int v = bins[i];
        if (v) atomicAdd(&counts[i], static_cast<unsigned long long>(v));
    }
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------------------------------
int64_t seg_ce_workspace_bytes(int B, int H, int W) {
    return 2 * static_cast<int64_t>(chunks(static_cast<int64_t>(B) * H * W)) * 4;     // a num and a den partial per workgroup
}

int seg_ce_forward(const void *logits, const void *target, const void *weight, void *loss, void *lse, void *state, void *workspace,
                   int B, int C, int H, int W, int64_t ignore_index, float gamma, hipStream_t s) {
    const float *x = static_cast<const float *>(logits), *w = static_cast<const float *>(weight);
    const int64_t *t = static_cast<const int64_t *>(target);
    float *l = static_cast<float *>(lse);
    const int HW = H * W, N = B * HW, nblocks = chunks(N);
    float *pnum = static_cast<float *>(workspace), *pden = pnum + nblocks;
    if (HW % kQuad == 0 && aligned16(x, t, l))
        seg_ce_fwd_kernel<true><<<nblocks, kThreads, 0, s>>>(x, t, w, l, pnum, pden, C, HW, N, ignore_index);
    else
        seg_ce_fwd_kernel<false><<<nblocks, kThreads, 0, s>>>(x, t, w, l, pnum, pden, C, HW, N, ignore_index);
    const int rc = launch_status();
    if (rc) return rc;
    seg_ce_final_kernel<<<1, kThreads, 0, s>>>(pnum, pden, nblocks, gamma, static_cast<float *>(loss), static_cast<float *>(state));
    return launch_status();
}

int seg_ce_backward(const void *logits, const void *target, const void *weight, const void *lse, const void *state,
                    const void *grad_loss, void *grad_logits, int B, int C, int H, int W, int64_t ignore_index, hipStream_t s) {
    const float *x = static_cast<const float *>(logits), *w = static_cast<const float *>(weight);
    const float *l = static_cast<const float *>(lse), *st = static_cast<const float *>(state), *g = static_cast<const float *>(grad_loss);
    const int64_t *t = static_cast<const int64_t *>(target);
    float *gx = static_cast<float *>(grad_logits);
    const int HW = H * W, N = B * HW, nblocks = chunks(N);
    if (HW % kQuad == 0 && aligned16(x, t, l, gx))
        seg_ce_bwd_kernel<true><<<nblocks, kThreads, 0, s>>>(x, t, w, l, st, g, gx, C, HW, N, ignore_index);
    else
        seg_ce_bwd_kernel<false><<<nblocks, kThreads, 0, s>>>(x, t, w, l, st, g, gx, C, HW, N, ignore_index);
    return launch_status();
}

int class_histogram_max_classes() { return kHistMaxClasses; }

int class_histogram(const void *target, void *counts, int64_t count, int num_classes, int64_t ignore_index, hipStream_t s) {
    class_histogram_zero_kernel<<<1, kThreads, 0, s>>>(static_cast<unsigned long long *>(counts), num_classes);
    const int rc = launch_status();
    if (rc) return rc;
    // memory-bound: enough workgroups to fill the chip, the rest of the labels by a grid stride
    const int64_t want = (count + kThreads * 8 - 1) / (kThreads * 8);
    const int nblocks = static_cast<int>(std::min<int64_t>(std::max<int64_t>(want, 1), 2048));
    class_histogram_kernel<<<nblocks, kThreads, 0, s>>>(static_cast<const int64_t *>(target), static_cast<unsigned long long *>(counts),
                                                       count, num_classes, ignore_index);
    return launch_status();
}

}  // namespace cerb
