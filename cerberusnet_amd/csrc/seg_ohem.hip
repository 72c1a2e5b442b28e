// seg_ohem.hip -- cross-entropy with online hard example mining (OHEM) as ONE differentiable scalar op, fp32 logits, int64
// labels, the selection on the device.
//
// Reference (nnet_training/loss_functions/seg_losses.py:56-95, SoftmaxCrossEntropyOHEMLoss.forward): the logits go to the
// host, numpy computes a softmax and argsorts every valid pixel's target probability, the target is rewritten on the host and
// copied back, then CrossEntropyLoss reads the logits again.  Here nothing leaves the device and nothing is sorted:
//
//   valid(p) = t(p) != ignore_index && 0 <= t(p) < C          prob(p) = exp(x_t(p) - lse(p))   (-1 where not valid)
//   num_valid = #valid;   min_kept >= num_valid : every valid pixel is kept (NaN ones too), threshold = +inf
//                         min_kept > 0          : kth = the min_kept-th smallest prob (NaN orders above every number);
//                                                 threshold = kth > thresh ? kth : thresh, a NaN kth gives thresh
//                         otherwise             : threshold = thresh
//   kept(p) = valid(p) && prob(p) <= threshold   (ties at kth are all kept)
//   loss = sum_kept w[t] (lse - x_t) / sum_kept w[t]
//   grad_x_c(p) = grad_loss / den * w[t] (softmax_c - [c == t]) at kept pixels, exactly 0.0f elsewhere
//
// kth is exact: a radix select over the bits of prob.  prob >= 0, so its bit pattern as uint32 is monotonic; a NaN becomes
// all ones.  The digits are 11 / 11 / 10 bits from the top.  The probability pass counts the first digit of every valid key
// while it streams the logits; a one-workgroup "pick" kernel prefix-scans the bins, finds the digit that holds rank min_kept
// and leaves the prefix and the remaining rank in device memory; a filtered histogram pass over the (B,H,W) prob map counts
// the next digit of the keys that share the prefix; and so on until all 32 bits are fixed.  Counts are integer adds (LDS per
// workgroup, one global add per non-empty bin): any order, the same result, so every run and every replayed graph gives the
// same bits.  Floating-point sums are partials per workgroup in a fixed order and one fixed-order launch, as in seg_loss.hip.
//
// Launches of a forward: zero (bins and select state), probability pass, pick, histogram, pick, histogram, pick, sum, final.
// The logits are read exactly once; lse - x_t is kept per pixel in the workspace so that the sum pass adds the very terms of
// seg_loss.hip without the logits.  The backward reads the logits once and writes the gradient once; kept is re-derived from
// prob <= threshold with the threshold read from device memory.
//
// Both routes of the probability pass and of the backward (vector: H*W % 4 == 0 and 16-byte aligned pointers; scalar) run
// the same per-pixel arithmetic, contraction off: a call on misaligned pointers gives the bits of the aligned call.
#include "seg_common.h"

#pragma clang fp contract(off)

namespace cerb {
namespace {

constexpr int kDigits = 3;
constexpr int kBins = 2048;                                 // bins of one digit's histogram (the last digit uses 1024)
__host__ __device__ constexpr int digit_bits(int digit) { return digit == 2 ? 10 : 11; }
__host__ __device__ constexpr int digit_low(int digit) { return digit == 0 ? 21 : (digit == 1 ? 10 : 0); }      // its lowest bit
constexpr int kSelWords = 8;                                // the select state, see below
// select state (uint32, in the workspace): [0] the prefix fixed so far, [1] the rank (1-based) among the keys that share it,
// [2] num_valid, [3] the branch: 0 = select, 1 = keep every valid pixel, 2 = thresh alone
enum { kSelPrefix = 0, kSelRank = 1, kSelValid = 2, kSelMode = 3 };
enum { kModeSelect = 0, kModeAll = 1, kModeThresh = 2 };
// state (fp32): [ce, den, 1 / den, threshold, keep_all (1 or 0), the rank left among the pixels tied at kth, 0, 0]

// the sort key of a prob: monotonic in prob for prob >= 0, all ones for a NaN
__device__ __forceinline__ unsigned key_of(float prob) { return prob != prob ? 0xffffffffu : __float_as_uint(prob); }

// kept, from what the forward left: prob is -1 where the pixel is not valid
__device__ __forceinline__ bool kept_of(float prob, float threshold, bool keep_all) {
    return keep_all ? !(prob < 0.f) : (prob >= 0.f && prob <= threshold);
}

// bins[digit] += 1 for every active lane of the wave.  Confident logits put most keys of a wave into a few bins, and LDS
// adds to one address serialise: up to four rounds take the digit of the first lane still active and add the number of lanes
// that hold it with one add; what is left after that adds singly.  Every lane of the wave must call this.
__device__ __forceinline__ void wave_bin_add(unsigned *bins, unsigned digit, bool active) {
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int it = 0; it < 4; ++it) {
        const unsigned long long live = __ballot(active);
        if (!live) return;
        const int lead = __ffsll(static_cast<long long>(live)) - 1;
        const unsigned d = __shfl(digit, lead, 64);
        const bool same = active && digit == d;
        const unsigned long long votes = __ballot(same);
        if (lane == lead) atomicAdd(&bins[d], static_cast<unsigned>(__popcll(votes)));
        active = active && !same;
    }
    if (active) atomicAdd(&bins[digit], 1u);
}

__device__ __forceinline__ void flush_bins(const unsigned *bins, unsigned *__restrict__ out, int n) {
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const unsigned v = bins[i];
        if (v) atomicAdd(&out[i], v);
    }
}

// ---- zero: the bins of the three digits and the select state -------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ohem_zero_kernel(unsigned *__restrict__ words, int n) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) words[i] = 0u;
}

// ---- the probability pass --------------------------------------------------------------------------------------------------
// what a pixel leaves: lse, prob (-1 where not valid), nll = lse - x_t (0 where not valid)
__device__ __forceinline__ void pixel_outputs(const Label &l, float lse, float xt, float &prob, float &nll) {
    prob = l.cls >= 0 ? expf(xt - lse) : -1.f;
    nll = l.cls >= 0 ? lse - xt : 0.f;
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void ohem_prob_kernel(const float *__restrict__ x, const int64_t *__restrict__ t,
                                                             float *__restrict__ lse_out, float *__restrict__ prob_out,
                                                             float *__restrict__ nll_out, unsigned *__restrict__ hist, int C, int HW,
                                                             int N, int64_t ignore) {
    __shared__ unsigned bins[kBins];
    for (int i = threadIdx.x; i < kBins; i += kThreads) bins[i] = 0u;
    __syncthreads();
    const int base = blockIdx.x * kChunk;
    if constexpr (kVec) {
        const int p0 = base + threadIdx.x * kQuad;
        float pr[kQuad] = {-1.f, -1.f, -1.f, -1.f};
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
            float l[kQuad], nl[kQuad];
#pragma unroll
            for (int k = 0; k < kQuad; ++k) {
                l[k] = m[k] + logf(s[k]);
                pixel_outputs(lab[k], l[k], xt[k], pr[k], nl[k]);
            }
            *reinterpret_cast<float4 *>(lse_out + p0) = make_float4(l[0], l[1], l[2], l[3]);
            *reinterpret_cast<float4 *>(prob_out + p0) = make_float4(pr[0], pr[1], pr[2], pr[3]);
            *reinterpret_cast<float4 *>(nll_out + p0) = make_float4(nl[0], nl[1], nl[2], nl[3]);
        }
#pragma unroll
        for (int k = 0; k < kQuad; ++k) wave_bin_add(bins, key_of(pr[k]) >> digit_low(0), !(pr[k] < 0.f));
    } else {
#pragma unroll 1
        for (int j = 0; j < kQuad; ++j) {
            const int p = base + j * kThreads + threadIdx.x;
            float pr = -1.f;
            if (p < N) {
                const int b = p / HW, r = p - b * HW;
                const float *px = x + static_cast<int64_t>(b) * C * HW + r;
                const Label lab = classify(t[p], ignore, C);
                float m = px[0], s = 1.f, xt = lab.cls == 0 ? m : 0.f;
#pragma unroll 4
                for (int c = 1; c < C; ++c) lse_step(px[static_cast<int64_t>(c) * HW], c == lab.cls, m, s, xt);
                const float l = m + logf(s);
                float nl;
                pixel_outputs(lab, l, xt, pr, nl);
                lse_out[p] = l;
                prob_out[p] = pr;
                nll_out[p] = nl;
            }
            wave_bin_add(bins, key_of(pr) >> digit_low(0), !(pr < 0.f));
        }
    }
    __syncthreads();
    flush_bins(bins, hist, kBins);
}

// ---- pick: one workgroup fixes one digit -----------------------------------------------------------------------------------
// Round 0 also counts the valid pixels (every valid key is in one of its bins) and chooses the branch; the last round writes
// the threshold.  A thread owns kBins / 256 consecutive bins; the 256 sums are scanned in LDS.
__global__ __launch_bounds__(kThreads) void ohem_pick_kernel(const unsigned *__restrict__ hist_all, unsigned *__restrict__ sel,
                                                             float *__restrict__ state, int round, int64_t min_kept, float thresh) {
    constexpr int kPer = kBins / kThreads;
    __shared__ unsigned scan[kThreads];
    const unsigned *hist = hist_all + round * kBins;
    const int nbins = 1 << digit_bits(round);               // the bins past nbins were zeroed and are never added to
    unsigned prefix = sel[kSelPrefix], rank = sel[kSelRank], mode = sel[kSelMode];
    unsigned c[kPer], mine = 0u;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int bin = threadIdx.x * kPer + i;
        c[i] = bin < nbins ? hist[bin] : 0u;
        mine += c[i];
    }
    scan[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const unsigned v = static_cast<int>(threadIdx.x) >= off ? scan[threadIdx.x - off] : 0u;
        __syncthreads();
        scan[threadIdx.x] += v;
        __syncthreads();
    }
    const unsigned incl = scan[threadIdx.x], excl = incl - mine, total = scan[kThreads - 1];
    if (round == 0) {
        mode = min_kept >= static_cast<int64_t>(total) ? kModeAll : (min_kept > 0 ? kModeSelect : kModeThresh);
        rank = mode == kModeSelect ? static_cast<unsigned>(min_kept) : 0u;
        prefix = 0u;
        if (threadIdx.x == 0) {
            sel[kSelValid] = total;
            sel[kSelMode] = mode;
        }
    }
    const bool last = round == kDigits - 1;
    if (mode != kModeSelect) {
        if (last && threadIdx.x == 0) {
            state[3] = mode == kModeAll ? __builtin_inff() : thresh;
            state[4] = mode == kModeAll ? 1.f : 0.f;
            state[5] = 0.f;
        }
        return;
    }
    // 1 <= rank <= total holds in every round: exactly one thread's bins hold it
    if (excl < rank && rank <= incl) {
        unsigned run = excl;
        int digit = -1;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {                    // the first bin whose running count reaches the rank
            if (digit < 0) {
                if (run + c[i] >= rank)
                    digit = i;
                else
                    run += c[i];
            }
        }
        prefix |= static_cast<unsigned>(threadIdx.x * kPer + digit) << digit_low(round);
        rank -= run;
        sel[kSelPrefix] = prefix;
        sel[kSelRank] = rank;
        if (last) {
            const bool nan_kth = prefix == 0xffffffffu;     // the key of every NaN
            const float kth = __uint_as_float(prefix);
            state[3] = (!nan_kth && kth > thresh) ? kth : thresh;
            state[4] = 0.f;
            state[5] = static_cast<float>(rank);
        }
    }
}

// ---- the filtered histogram of digit `round` (1 or 2): only the keys that share the prefix fixed so far -----------------------
__global__ __launch_bounds__(kThreads) void ohem_hist_kernel(const float *__restrict__ prob, const unsigned *__restrict__ sel,
                                                             unsigned *__restrict__ hist_all, int round, int N) {
    __shared__ unsigned bins[kBins];
    if (sel[kSelMode] != kModeSelect) return;               // the same word for every thread: nothing to select
    const int nbins = 1 << digit_bits(round);
    for (int i = threadIdx.x; i < nbins; i += kThreads) bins[i] = 0u;
    __syncthreads();
    const int high = digit_low(round - 1), low = digit_low(round);
    const unsigned want = sel[kSelPrefix] >> high, mask = static_cast<unsigned>(nbins - 1);
    const int base = blockIdx.x * kChunk;
#pragma unroll
    for (int j = 0; j < kQuad; ++j) {
        const int p = base + j * kThreads + threadIdx.x;
        const float pr = p < N ? prob[p] : -1.f;
        const unsigned key = key_of(pr);
        wave_bin_add(bins, (key >> low) & mask, !(pr < 0.f) && (key >> high) == want);
    }
    __syncthreads();
    flush_bins(bins, hist_all + round * kBins, nbins);
}

// ---- the sum pass: prob, nll and the labels; a lane owns 4 consecutive pixels as in seg_loss.hip ------------------------------
template <bool kVec>
__global__ __launch_bounds__(kThreads) void ohem_sum_kernel(const float *__restrict__ prob, const float *__restrict__ nll,
                                                            const int64_t *__restrict__ t, const float *__restrict__ w,
                                                            const float *__restrict__ state, float *__restrict__ pnum,
                                                            float *__restrict__ pden, unsigned *__restrict__ pkept, int C, int N,
                                                            int64_t ignore) {
    __shared__ float red_n[4], red_d[4];
    __shared__ unsigned red_k[4];
    const float threshold = state[3];
    const bool keep_all = state[4] != 0.f;
    const int p0 = blockIdx.x * kChunk + threadIdx.x * kQuad;
    float pr[kQuad], nl[kQuad];
    int64_t tt[kQuad];
    if (kVec && p0 + kQuad <= N) {
        const float4 a = *reinterpret_cast<const float4 *>(prob + p0), b = *reinterpret_cast<const float4 *>(nll + p0);
        const longlong2 ta = *reinterpret_cast<const longlong2 *>(t + p0), tb = *reinterpret_cast<const longlong2 *>(t + p0 + 2);
        pr[0] = a.x, pr[1] = a.y, pr[2] = a.z, pr[3] = a.w;
        nl[0] = b.x, nl[1] = b.y, nl[2] = b.z, nl[3] = b.w;
        tt[0] = ta.x, tt[1] = ta.y, tt[2] = tb.x, tt[3] = tb.y;
    } else {
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            const bool in = p0 + k < N;
            pr[k] = in ? prob[p0 + k] : -1.f;
            nl[k] = in ? nll[p0 + k] : 0.f;
            tt[k] = in ? t[p0 + k] : ignore;
        }
    }
    float n4[kQuad], d4[kQuad];
    unsigned kept = 0u;
#pragma unroll
    for (int k = 0; k < kQuad; ++k) {
        const Label l = classify(tt[k], ignore, C);
        n4[k] = d4[k] = 0.f;
        if (l.cls >= 0) {
            if (kept_of(pr[k], threshold, keep_all)) {
                const float wt = w[l.cls];
                n4[k] = wt * nl[k];
                d4[k] = wt;
                ++kept;
            }
        } else if (l.valid) {
            n4[k] = __builtin_nanf("");                     // a label outside [0, C) that is not the ignore value, as seg_loss.hip
        }
    }
    const float n = quad_sum(n4), d = quad_sum(d4);
    const float tn = block_sum(n, red_n), td = block_sum(d, red_d);
    const unsigned tk = block_sum(kept, red_k);
    if (threadIdx.x == 0) {
        pnum[blockIdx.x] = tn;
        pden[blockIdx.x] = td;
        pkept[blockIdx.x] = tk;
    }
}

// ---- the last launch: one workgroup, the order of seg_ce_final_kernel ----------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ohem_final_kernel(const float *__restrict__ pnum, const float *__restrict__ pden,
                                                              const unsigned *__restrict__ pkept, const unsigned *__restrict__ sel, int n,
                                                              float *__restrict__ loss, float *__restrict__ state,
                                                              long long *__restrict__ counts) {
    __shared__ float red[2][kThreads];
    __shared__ unsigned long long redk[kThreads];
    float a = 0.f, b = 0.f;
    unsigned long long k = 0ull;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        a += pnum[i];
        b += pden[i];
        k += pkept[i];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    redk[threadIdx.x] = k;
    tree_sum(red, redk);
    if (threadIdx.x == 0) {
        const float num = red[0][0], den = red[1][0];
        const float ce = num / den;              // 0 / 0 = NaN when nothing is kept, as the stock mean
        loss[0] = ce;
        state[0] = ce;
        state[1] = den;
        state[2] = 1.f / den;
        state[6] = 0.f;
        state[7] = 0.f;
        counts[0] = static_cast<long long>(sel[kSelValid]);
        counts[1] = static_cast<long long>(redk[0]);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
template <bool kVec>
__global__ __launch_bounds__(kThreads) void ohem_bwd_kernel(const float *__restrict__ x, const int64_t *__restrict__ t,
                                                            const float *__restrict__ w, const float *__restrict__ prob,
                                                            const float *__restrict__ lse, const float *__restrict__ state,
                                                            const float *__restrict__ grad_loss, float *__restrict__ gx, int C, int HW,
                                                            int N, int64_t ignore) {
    // all read here, from device memory: no host synchronisation
    const float coef = grad_loss[0] * state[2], threshold = state[3];
    const bool keep_all = state[4] != 0.f;
    const int base = blockIdx.x * kChunk;
    if constexpr (kVec) {
        const int p0 = base + threadIdx.x * kQuad;
        if (p0 >= N) return;
        const int b = p0 / HW, r = p0 - b * HW;
        const int64_t item = static_cast<int64_t>(b) * C * HW + r;
        const longlong2 ta = *reinterpret_cast<const longlong2 *>(t + p0), tb = *reinterpret_cast<const longlong2 *>(t + p0 + 2);
        const Label lab[kQuad] = {classify(ta.x, ignore, C), classify(ta.y, ignore, C), classify(tb.x, ignore, C),
                                  classify(tb.y, ignore, C)};
        const float4 l4 = *reinterpret_cast<const float4 *>(lse + p0), p4 = *reinterpret_cast<const float4 *>(prob + p0);
        const float l[kQuad] = {l4.x, l4.y, l4.z, l4.w}, pr[kQuad] = {p4.x, p4.y, p4.z, p4.w};
        float a[kQuad];
        bool live[kQuad];
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            a[k] = pixel_coef(lab[k], coef, w, live[k]);
            live[k] = live[k] && kept_of(pr[k], threshold, keep_all);
        }
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
            live = live && kept_of(prob[p], threshold, keep_all);
#pragma unroll 4
            for (int c = 0; c < C; ++c) {
                const int64_t o = item + static_cast<int64_t>(c) * HW;
                gx[o] = grad_elem(x[o], l, a, c == lab.cls, live);
            }
        }
    }
}

// the workspace, in 4-byte words: nll (the pixels rounded up to a multiple of 4, so that what follows stays 16-byte
// aligned), a num, a den and a kept partial per workgroup, the bins of the three digits, the select state
struct Workspace {
    float *nll, *pnum, *pden;
    unsigned *pkept, *hist, *sel;
};

inline int64_t padded(int64_t N) { return (N + 3) & ~static_cast<int64_t>(3); }

inline int64_t workspace_words(int64_t N) { return padded(N) + 3 * static_cast<int64_t>(chunks(N)) + kDigits * kBins + kSelWords; }

inline Workspace carve(void *workspace, int64_t N) {
    const int64_t npad = padded(N), n = chunks(N);
    Workspace ws;
    float *f = static_cast<float *>(workspace);
    ws.nll = f;
    ws.pnum = f + npad;
    ws.pden = ws.pnum + n;
    ws.pkept = reinterpret_cast<unsigned *>(ws.pden + n);
    ws.hist = ws.pkept + n;
    ws.sel = ws.hist + kDigits * kBins;
    return ws;
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------------------------------
int64_t seg_ohem_workspace_bytes(int B, int H, int W) { return workspace_words(static_cast<int64_t>(B) * H * W) * 4; }

int seg_ohem_forward(const void *logits, const void *target, const void *weight, void *loss, void *prob, void *lse, void *state,
                     void *counts, void *workspace, int B, int C, int H, int W, int64_t ignore_index, float thresh, int64_t min_kept,
                     hipStream_t s) {
    const float *x = static_cast<const float *>(logits), *w = static_cast<const float *>(weight);
    const int64_t *t = static_cast<const int64_t *>(target);
    float *l = static_cast<float *>(lse), *pr = static_cast<float *>(prob), *st = static_cast<float *>(state);
    const int HW = H * W, N = B * HW, nblocks = chunks(N);
    const Workspace ws = carve(workspace, N);
    const int nzero = kDigits * kBins + kSelWords;          // hist and sel are adjacent
    ohem_zero_kernel<<<(nzero + kThreads - 1) / kThreads, kThreads, 0, s>>>(ws.hist, nzero);
    int rc = launch_status();
    if (rc) return rc;
    const bool quads = HW % kQuad == 0;
    if (quads && aligned16(x, t, l, pr) && aligned16(ws.nll, nullptr, nullptr))
        ohem_prob_kernel<true><<<nblocks, kThreads, 0, s>>>(x, t, l, pr, ws.nll, ws.hist, C, HW, N, ignore_index);
    else
        ohem_prob_kernel<false><<<nblocks, kThreads, 0, s>>>(x, t, l, pr, ws.nll, ws.hist, C, HW, N, ignore_index);
    if ((rc = launch_status())) return rc;
    for (int round = 0; round < kDigits; ++round) {
        if (round > 0) {
            ohem_hist_kernel<<<nblocks, kThreads, 0, s>>>(pr, ws.sel, ws.hist, round, N);
            if ((rc = launch_status())) return rc;
        }
        ohem_pick_kernel<<<1, kThreads, 0, s>>>(ws.hist, ws.sel, st, round, min_kept, thresh);
        if ((rc = launch_status())) return rc;
    }
    if (aligned16(pr, t, ws.nll))
        ohem_sum_kernel<true><<<nblocks, kThreads, 0, s>>>(pr, ws.nll, t, w, st, ws.pnum, ws.pden, ws.pkept, C, N, ignore_index);
    else
        ohem_sum_kernel<false><<<nblocks, kThreads, 0, s>>>(pr, ws.nll, t, w, st, ws.pnum, ws.pden, ws.pkept, C, N, ignore_index);
    if ((rc = launch_status())) return rc;
    ohem_final_kernel<<<1, kThreads, 0, s>>>(ws.pnum, ws.pden, ws.pkept, ws.sel, nblocks, static_cast<float *>(loss), st,
                                             static_cast<long long *>(counts));
    return launch_status();
}

int seg_ohem_backward(const void *logits, const void *target, const void *weight, const void *prob, const void *lse, const void *state,
                      const void *grad_loss, void *grad_logits, int B, int C, int H, int W, int64_t ignore_index, hipStream_t s) {
    const float *x = static_cast<const float *>(logits), *w = static_cast<const float *>(weight);
    const float *pr = static_cast<const float *>(prob), *l = static_cast<const float *>(lse);
    const float *st = static_cast<const float *>(state), *g = static_cast<const float *>(grad_loss);
    const int64_t *t = static_cast<const int64_t *>(target);
    float *gx = static_cast<float *>(grad_logits);
    const int HW = H * W, N = B * HW, nblocks = chunks(N);
    if (HW % kQuad == 0 && aligned16(x, t, l, gx) && aligned16(pr, nullptr, nullptr))
        ohem_bwd_kernel<true><<<nblocks, kThreads, 0, s>>>(x, t, w, pr, l, st, g, gx, C, HW, N, ignore_index);
    else
        ohem_bwd_kernel<false><<<nblocks, kThreads, 0, s>>>(x, t, w, pr, l, st, g, gx, C, HW, N, ignore_index);
    return launch_status();
}

int seg_ohem_digit_bits(int digit) { return digit >= 0 && digit < kDigits ? digit_bits(digit) : 0; }
int seg_ohem_bins() { return kBins; }

}  // namespace cerb
