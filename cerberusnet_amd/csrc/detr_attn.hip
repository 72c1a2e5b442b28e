// detr_attn.hip -- the multi-head attention core of the DETR head's transformer (nnet_models/detr/transformer.py), fp32, forward and
// backward, D = 32 channels per head:
//
//   out[i,b,h,:] = sum_j dropout(softmax_j(scale q[i,b,h,:] . k[j,b,h,:] + key_padding_mask[b,j])) v[j,b,h,:]
//
// q (Lq,B,H D), k / v (Lk,B,H D) and out (Lq,B,H D) are read and written where F.linear leaves them and out_proj wants them: one
// (token, batch, head) row is 32 contiguous floats, a token step is B H 32 floats.  Nothing of size Lq x Lk reaches memory
// (DESIGN.md 3.27).
//
// One tile computation serves all three big kernels: a wave owns 32 rows of one side in registers (lane l: row l & 31, the channels
// 2 kk + (l >> 5), kk = 0..15), the other side's 32 rows sit in LDS (33 floats per row), and 16 v_mfma_f32_32x32x2_f32 (exact fp32)
// give the 32 x 32 similarities with the OWNED row along the lanes: lane l holds 16 entries of its own row, the lane l ^ 32 the other
// 16 (walked row (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r).  The second product takes those registers as its B operand
// unchanged, so no probability ever moves between lanes.
//   forward      a workgroup owns 128 queries (4 waves x 32) and walks the keys 32 at a time with an online softmax: a row's
//                maximum and sum are its lane's 16 registers and one exchange with lane l ^ 32
//   delta        delta[b,h,i] = sum_d dO[i,b,h,d] O[i,b,h,d]: one lane per row, channels ascending
//   dk / dv      a workgroup owns 128 keys and walks the queries 32 at a time
//   dq           a workgroup owns 128 queries and walks the keys 32 at a time
// Probabilities are recomputed in the backward from the row maximum and the row sum the forward saved beside the log-sum-exp
// (exp(s - max) / sum, the forward's own expression: exp(s - lse) would round s - lse at the size of lse, 2^-22 for a hundred keys);
// the dropout keep decision is the stateless hash of attn_dropout.h.  The walked tile is prefetched into registers while the previous one is multiplied.
//
// No atomics, every sum in a fixed order: two runs give the same bits; every global access is 4 bytes per lane, so a base pointer 4
// bytes into a buffer gives the same bits.  A row whose keys are all masked gives 0 (log-sum-exp -inf) and sends zero gradients.
// The entry points at the bottom check their arguments before anything touches a device.
#include <math.h>

#include "common.h"
#include "attn_dropout.h"

namespace cerb {
namespace {

constexpr int kThreads = 256;
constexpr int kD = 32;                       // channels per head
constexpr int kOwn = 128;                    // rows a workgroup owns: 32 per wave
constexpr int kWalk = 32;                    // rows per walked tile
constexpr int64_t kMaxLaunchThreads = 0xffffffffll;   // HIP rejects a grid of 2^32 threads or more
constexpr int kStride = kD + 1;              // LDS row: lanes = rows read a column, lanes = channels read a row, both conflict-free
constexpr int kStage = kWalk * kD / kThreads;   // elements of a walked tile a thread stages: 4

typedef float f16v __attribute__((ext_vector_type(16)));

// register r of a 32x32 MFMA result in lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
__device__ __forceinline__ int tile_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ f16v zero16() {
    f16v z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

// acc[row = side in LDS][col = the lane's own row] += sum_d tile[row][d] own[d]
__device__ __forceinline__ f16v dot_tile(const float *tile, const float (&own)[16], int col, int half) {
    f16v acc = zero16();
    const float *a = tile + col * kStride + half;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * kk], own[kk], acc, 0, 0, 0);
    return acc;
}

// acc[row = channel][col = the lane's own row] += sum over the tile's rows of tile[row][channel] w[row][own]
__device__ __forceinline__ f16v accumulate_tile(const float *tile, const f16v &w, f16v acc, int col, int half) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(tile[tile_row(r, half) * kStride + col], w[r], acc, 0, 0, 0);
    return acc;
}

// the lane's 16 channels of one (token, batch, head) row, times mul; zeros when the row does not exist
__device__ __forceinline__ void load_own(const float *__restrict__ x, size_t row_offset, bool live, int half, float mul, float (&own)[16]) {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) own[kk] = live ? mul * x[row_offset + 2 * kk + half] : 0.f;
}

// one walked tile's share of a thread: rows (tid >> 5) + 8 r, channel tid & 31
struct Stage {
    float a[kStage], b[kStage];
};

__device__ __forceinline__ void stage_load(Stage &st, const float *__restrict__ xa, const float *__restrict__ xb, int row0, int rows,
                                           size_t token_step, size_t head_offset, float mul_a) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 0; r < kStage; ++r) {
        const int row = row0 + (tid >> 5) + 8 * r;
        const bool ok = row < rows;
        const size_t at = static_cast<size_t>(ok ? row : 0) * token_step + head_offset + (tid & 31);
        const float va = xa[at], vb = xb[at];
        st.a[r] = ok ? mul_a * va : 0.f;
        st.b[r] = ok ? vb : 0.f;
    }
}

__device__ __forceinline__ void stage_store(const Stage &st, float *sa, float *sb) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 0; r < kStage; ++r) {
        const int at = ((tid >> 5) + 8 * r) * kStride + (tid & 31);
        sa[at] = st.a[r];
        sb[at] = st.b[r];
    }
}

// 0 for a key that takes part, -inf for one that is masked or past the last
__device__ __forceinline__ float key_bias(const uint8_t *__restrict__ mask, int b, int j, int Lk) {
    if (j >= Lk) return -INFINITY;
    return (mask && mask[static_cast<size_t>(b) * Lk + j]) ? -INFINITY : 0.f;
}

// 1 / (a row's sum of exponentials); 0 for a row whose keys are all masked
__device__ __forceinline__ float recip_sum(float l) { return l > 0.f ? 1.f / l : 0.f; }

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <bool kDrop>
__global__ __launch_bounds__(kThreads) void attn_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                            const float *__restrict__ v, const uint8_t *__restrict__ mask,
                                                            const int64_t *__restrict__ seed, float *__restrict__ out,
                                                            float *__restrict__ lse, float *__restrict__ stats, int Lq, int Lk, int B,
                                                            int H, float scale, uint32_t threshold, float inv_keep, int nblk) {
    __shared__ float sk[kWalk * kStride], sv[kWalk * kStride], sbias[kWalk];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int bh = blockIdx.x / nblk, b = bh / H, h = bh % H;
    const int i = (blockIdx.x % nblk) * kOwn + wave * 32 + col;
    const bool live = i < Lq;
    const size_t token_step = static_cast<size_t>(B) * H * kD, head_offset = (static_cast<size_t>(b) * H + h) * kD;
    const size_t own_offset = static_cast<size_t>(live ? i : 0) * token_step + head_offset;
    float qs[16];
    load_own(q, own_offset, live, half, scale, qs);
    uint32_t row_key = 0;
    if (kDrop) row_key = attn_row_key(attn_plane_key(seed[0], bh), i);

    float m = -INFINITY, l = 0.f;
    f16v o = zero16();
    Stage st;
    float bias = 0.f;
    stage_load(st, k, v, 0, Lk, token_step, head_offset, 1.f);
    if (tid < kWalk) bias = key_bias(mask, b, tid, Lk);
    for (int j0 = 0; j0 < Lk; j0 += kWalk) {
        __syncthreads();          // the previous tile is consumed
        stage_store(st, sk, sv);
        if (tid < kWalk) sbias[tid] = bias;
        __syncthreads();
        if (j0 + kWalk < Lk) {    // in flight while this tile is multiplied
            stage_load(st, k, v, j0 + kWalk, Lk, token_step, head_offset, 1.f);
            if (tid < kWalk) bias = key_bias(mask, b, j0 + kWalk + tid, Lk);
        }
        f16v s = dot_tile(sk, qs, col, half);
        float mb = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] += sbias[tile_row(r, half)];
            mb = fmaxf(mb, s[r]);
        }
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float mn = fmaxf(m, mb);
        const float ms = (mn == -INFINITY) ? 0.f : mn;      // a wholly masked start leaves the maximum at -inf and every term at 0
        const float alpha = expf(m - ms);
        float ls = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = expf(s[r] - ms);
            ls += s[r];
        }
        ls += __shfl_xor(ls, 32);
        l = l * alpha + ls;
        m = mn;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o[r] *= alpha;
            if (kDrop && !attn_keep(row_key, j0 + tile_row(r, half), threshold)) s[r] = 0.f;
        }
        o = accumulate_tile(sv, s, o, col, half);
    }
    if (!live) return;
    const float inv = l > 0.f ? inv_keep / l : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[own_offset + tile_row(r, half)] = o[r] * inv;
    if (half == 0) {
        const size_t row = static_cast<size_t>(bh) * Lq + i;
        lse[row] = l > 0.f ? m + logf(l) : -INFINITY;
        stats[2 * row] = m;
        stats[2 * row + 1] = l;
    }
}

// ---- backward: delta ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void attn_delta_kernel(const float *__restrict__ grad_out, const float *__restrict__ out,
                                                              float *__restrict__ delta, int Lq, int B, int H, int64_t rows) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (idx >= rows) return;
    const int bh = static_cast<int>(idx / Lq), i = static_cast<int>(idx % Lq), b = bh / H, h = bh % H;
    const size_t at = ((static_cast<size_t>(i) * B + b) * H + h) * kD;
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < kD; ++d) acc = fmaf(grad_out[at + d], out[at + d], acc);
    delta[idx] = acc;
}

// ---- backward: dk, dv -------------------------------------------------------------------------------------------------------------
template <bool kDrop>
__global__ __launch_bounds__(kThreads) void attn_bwd_kv_kernel(const float *__restrict__ grad_out, const float *__restrict__ q,
                                                               const float *__restrict__ k, const float *__restrict__ v,
                                                               const uint8_t *__restrict__ mask, const int64_t *__restrict__ seed,
                                                               const float *__restrict__ stats, const float *__restrict__ delta,
                                                               float *__restrict__ grad_k, float *__restrict__ grad_v, int Lq, int Lk,
                                                               int B, int H, float scale, uint32_t threshold, float inv_keep, int nblk) {
    __shared__ float sq[kWalk * kStride], sg[kWalk * kStride], smax[kWalk], srsum[kWalk], sdelta[kWalk];
    __shared__ uint32_t srow[kWalk];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int bh = blockIdx.x / nblk, b = bh / H, h = bh % H;
    const int j = (blockIdx.x % nblk) * kOwn + wave * 32 + col;
    const bool live = j < Lk;
    const size_t token_step = static_cast<size_t>(B) * H * kD, head_offset = (static_cast<size_t>(b) * H + h) * kD;
    const size_t own_offset = static_cast<size_t>(live ? j : 0) * token_step + head_offset;
    float kr[16], vr[16];
    load_own(k, own_offset, live, half, 1.f, kr);
    load_own(v, own_offset, live, half, 1.f, vr);
    const bool masked = key_bias(mask, b, j, Lk) != 0.f;
    uint32_t plane_key = 0;
    if (kDrop) plane_key = attn_plane_key(seed[0], bh);

    f16v dk = zero16(), dv = zero16();
    Stage st;
    float row_max = 0.f, row_rsum = 0.f, row_delta = 0.f;         // a query past the last: probability exp(s) * 0 = 0
    const size_t stat0 = static_cast<size_t>(bh) * Lq;
    stage_load(st, q, grad_out, 0, Lq, token_step, head_offset, scale);
    if (tid < kWalk && tid < Lq) {
        row_max = stats[2 * (stat0 + tid)];
        row_rsum = recip_sum(stats[2 * (stat0 + tid) + 1]);
        row_delta = delta[stat0 + tid];
    }
    for (int i0 = 0; i0 < Lq; i0 += kWalk) {
        __syncthreads();          // the previous tile is consumed
        stage_store(st, sq, sg);
        if (tid < kWalk) {
            smax[tid] = row_max;
            srsum[tid] = row_rsum;
            sdelta[tid] = row_delta;
            if (kDrop) srow[tid] = attn_row_key(plane_key, i0 + tid);
        }
        __syncthreads();
        if (i0 + kWalk < Lq) {
            stage_load(st, q, grad_out, i0 + kWalk, Lq, token_step, head_offset, scale);
            if (tid < kWalk) {
                const int i = i0 + kWalk + tid;
                row_max = i < Lq ? stats[2 * (stat0 + i)] : 0.f;
                row_rsum = i < Lq ? recip_sum(stats[2 * (stat0 + i) + 1]) : 0.f;
                row_delta = i < Lq ? delta[stat0 + i] : 0.f;
            }
        }
        f16v s = dot_tile(sq, kr, col, half);
        f16v dp = dot_tile(sg, vr, col, half);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ir = tile_row(r, half);
            const float p = masked ? 0.f : expf(s[r] - smax[ir]) * srsum[ir];
            float keep_scale = 1.f;
            if (kDrop) keep_scale = attn_keep(srow[ir], j, threshold) ? inv_keep : 0.f;
            s[r] = p * keep_scale;                                    // what multiplied v in the forward
            dp[r] = p * (dp[r] * keep_scale - sdelta[ir]);            // the gradient of the scaled similarity
        }
        dv = accumulate_tile(sg, s, dv, col, half);
        dk = accumulate_tile(sq, dp, dk, col, half);
    }
    if (!live) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (grad_k) grad_k[own_offset + tile_row(r, half)] = dk[r];   // sq holds scale * q
        if (grad_v) grad_v[own_offset + tile_row(r, half)] = dv[r];
    }
}

// ---- backward: dq -----------------------------------------------------------------------------------------------------------------
template <bool kDrop>
__global__ __launch_bounds__(kThreads) void attn_bwd_q_kernel(const float *__restrict__ grad_out, const float *__restrict__ q,
                                                              const float *__restrict__ k, const float *__restrict__ v,
                                                              const uint8_t *__restrict__ mask, const int64_t *__restrict__ seed,
                                                              const float *__restrict__ stats, const float *__restrict__ delta,
                                                              float *__restrict__ grad_q, int Lq, int Lk, int B, int H, float scale,
                                                              uint32_t threshold, float inv_keep, int nblk) {
    __shared__ float sk[kWalk * kStride], sv[kWalk * kStride], sbias[kWalk];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int bh = blockIdx.x / nblk, b = bh / H, h = bh % H;
    const int i = (blockIdx.x % nblk) * kOwn + wave * 32 + col;
    const bool live = i < Lq;
    const size_t token_step = static_cast<size_t>(B) * H * kD, head_offset = (static_cast<size_t>(b) * H + h) * kD;
    const size_t own_offset = static_cast<size_t>(live ? i : 0) * token_step + head_offset;
    float qs[16], g[16];
    load_own(q, own_offset, live, half, scale, qs);
    load_own(grad_out, own_offset, live, half, 1.f, g);
    const size_t stat = static_cast<size_t>(bh) * Lq + (live ? i : 0);
    const float row_max = live ? stats[2 * stat] : 0.f;
    const float row_rsum = live ? recip_sum(stats[2 * stat + 1]) : 0.f;
    const float row_delta = live ? delta[stat] : 0.f;
    uint32_t row_key = 0;
    if (kDrop) row_key = attn_row_key(attn_plane_key(seed[0], bh), i);

    f16v dq = zero16();
    Stage st;
    float bias = 0.f;
    stage_load(st, k, v, 0, Lk, token_step, head_offset, 1.f);
    if (tid < kWalk) bias = key_bias(mask, b, tid, Lk);
    for (int j0 = 0; j0 < Lk; j0 += kWalk) {
        __syncthreads();          // the previous tile is consumed
        stage_store(st, sk, sv);
        if (tid < kWalk) sbias[tid] = bias;
        __syncthreads();
        if (j0 + kWalk < Lk) {
            stage_load(st, k, v, j0 + kWalk, Lk, token_step, head_offset, 1.f);
            if (tid < kWalk) bias = key_bias(mask, b, j0 + kWalk + tid, Lk);
        }
        f16v s = dot_tile(sk, qs, col, half);
        f16v dp = dot_tile(sv, g, col, half);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int jr = tile_row(r, half);
            const float p = sbias[jr] != 0.f ? 0.f : expf(s[r] - row_max) * row_rsum;
            float keep_scale = 1.f;
            if (kDrop) keep_scale = attn_keep(row_key, j0 + jr, threshold) ? inv_keep : 0.f;
            s[r] = p * (dp[r] * keep_scale - row_delta);
        }
        dq = accumulate_tile(sk, s, dq, col, half);
    }
    if (!live) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) grad_q[own_offset + tile_row(r, half)] = scale * dq[r];
}

// ---- the keep mask, written out ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void attn_keep_kernel(const int64_t *__restrict__ seed, uint8_t *__restrict__ keep, int Lq, int Lk,
                                                             int64_t count, uint32_t threshold) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (idx >= count) return;
    const int j = static_cast<int>(idx % Lk);
    const int64_t row = idx / Lk;
    const int i = static_cast<int>(row % Lq), plane = static_cast<int>(row / Lq);
    keep[idx] = threshold == 0 ? 1 : attn_keep(attn_row_key(attn_plane_key(seed[0], plane), i), j, threshold);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int64_t blocks_of(int rows) { return (static_cast<int64_t>(rows) + kOwn - 1) / kOwn; }
bool aligned(const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

int args_ok(int Lq, int Lk, int B, int H, int D, float scale, float p, int dtype) {
    if (dtype < CERB_F32 || dtype > CERB_F64) return CERB_EDTYPE;
    if (dtype != CERB_F32) return CERB_EUNSUPPORTED;
    if (Lq <= 0 || Lk <= 0 || B <= 0 || H <= 0 || D <= 0) return CERB_EINVAL;
    if (!(p >= 0.f && p < 1.f) || !isfinite(scale)) return CERB_EINVAL;
    if (D != kD) return CERB_EUNSUPPORTED;                   // the caller takes the stock ops there
    const int64_t lim = 0x7fffffff, bh = static_cast<int64_t>(B) * H;
    // every element index and the statistics' index are ints; a launch has fewer than 2^32 threads
    if (bh > lim || std::max(Lq, Lk) * bh * kD > lim || bh * blocks_of(std::max(Lq, Lk)) * kThreads > kMaxLaunchThreads) return CERB_ETOOLARGE;
    return CERB_OK;
}

}  // namespace
}  // namespace cerb

using namespace cerb;

extern "C" {

int cerberus_attn_forward(const void *q, const void *k, const void *v, const void *key_padding_mask, const void *seed, void *out,
                          void *lse, void *stats, int Lq, int Lk, int B, int H, int D, float scale, float dropout_p, int dtype, void *stream) {
    const int rc = args_ok(Lq, Lk, B, H, D, scale, dropout_p, dtype);
    if (rc) return rc;
    if (!q || !k || !v || !out || !lse || !stats || (dropout_p > 0.f && !seed)) return CERB_EINVAL;
    if (!aligned(q, 4) || !aligned(k, 4) || !aligned(v, 4) || !aligned(out, 4) || !aligned(lse, 4) || !aligned(stats, 4) || !aligned(seed, 8))
        return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = static_cast<int>(blocks_of(Lq));
    const uint8_t *mask = static_cast<const uint8_t *>(key_padding_mask);
#define ATTN_FWD(DROP)                                                                                                                 \
    attn_fwd_kernel<DROP><<<B * H * nblk, kThreads, 0, s>>>(static_cast<const float *>(q), static_cast<const float *>(k),             \
                                                            static_cast<const float *>(v), mask, static_cast<const int64_t *>(seed),  \
                                                            static_cast<float *>(out), static_cast<float *>(lse), static_cast<float *>(stats), \
                                                            Lq, Lk, B, H, scale, attn_threshold(dropout_p), 1.f / (1.f - dropout_p), nblk)
    if (dropout_p > 0.f) ATTN_FWD(true); else ATTN_FWD(false);
#undef ATTN_FWD
    return launch_status();
}

int cerberus_attn_backward(const void *grad_out, const void *q, const void *k, const void *v, const void *key_padding_mask,
                           const void *seed, const void *out, const void *stats, void *grad_q, void *grad_k, void *grad_v, void *delta,
                           int Lq, int Lk, int B, int H, int D, float scale, float dropout_p, int dtype, void *stream) {
    int rc = args_ok(Lq, Lk, B, H, D, scale, dropout_p, dtype);
    if (rc) return rc;
    if (!grad_out || !q || !k || !v || !out || !stats || !delta || (dropout_p > 0.f && !seed)) return CERB_EINVAL;
    if (!grad_q && !grad_k && !grad_v) return CERB_EINVAL;
    if (!aligned(grad_out, 4) || !aligned(q, 4) || !aligned(k, 4) || !aligned(v, 4) || !aligned(out, 4) || !aligned(stats, 4) ||
        !aligned(grad_q, 4) || !aligned(grad_k, 4) || !aligned(grad_v, 4) || !aligned(delta, 4) || !aligned(seed, 8))
        return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t *mask = static_cast<const uint8_t *>(key_padding_mask);
    const float *g = static_cast<const float *>(grad_out), *qf = static_cast<const float *>(q), *kf = static_cast<const float *>(k),
                *vf = static_cast<const float *>(v), *lf = static_cast<const float *>(stats);
    const int64_t *sd = static_cast<const int64_t *>(seed);
    float *df = static_cast<float *>(delta);
    const uint32_t threshold = attn_threshold(dropout_p);
    const float inv_keep = 1.f / (1.f - dropout_p);
    const int64_t rows = static_cast<int64_t>(B) * H * Lq;
    attn_delta_kernel<<<static_cast<unsigned>((rows + kThreads - 1) / kThreads), kThreads, 0, s>>>(g, static_cast<const float *>(out), df,
                                                                                                   Lq, B, H, rows);
    rc = launch_status();
    if (rc) return rc;
    if (grad_k || grad_v) {
        const int nblk = static_cast<int>(blocks_of(Lk));
#define ATTN_BWD_KV(DROP)                                                                                                              \
    attn_bwd_kv_kernel<DROP><<<B * H * nblk, kThreads, 0, s>>>(g, qf, kf, vf, mask, sd, lf, df, static_cast<float *>(grad_k),         \
                                                               static_cast<float *>(grad_v), Lq, Lk, B, H, scale, threshold, inv_keep, \
                                                               nblk)
        if (dropout_p > 0.f) ATTN_BWD_KV(true); else ATTN_BWD_KV(false);
#undef ATTN_BWD_KV
        rc = launch_status();
        if (rc) return rc;
    }
    if (grad_q) {
        const int nblk = static_cast<int>(blocks_of(Lq));
#define ATTN_BWD_Q(DROP)                                                                                                               \
    attn_bwd_q_kernel<DROP><<<B * H * nblk, kThreads, 0, s>>>(g, qf, kf, vf, mask, sd, lf, df, static_cast<float *>(grad_q), Lq, Lk, B, \
                                                              H, scale, threshold, inv_keep, nblk)
        if (dropout_p > 0.f) ATTN_BWD_Q(true); else ATTN_BWD_Q(false);
#undef ATTN_BWD_Q
        rc = launch_status();
    }
    return rc;
}

int cerberus_attn_dropout_keep(const void *seed, void *keep, int B, int H, int Lq, int Lk, float dropout_p, void *stream) {
    if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0 || !(dropout_p >= 0.f && dropout_p < 1.f)) return CERB_EINVAL;
    const int64_t lim = 0x7fffffff, planes = static_cast<int64_t>(B) * H;
    if (planes > lim) return CERB_ETOOLARGE;
    const int64_t per_plane = static_cast<int64_t>(Lq) * Lk;
    if (per_plane > (kMaxLaunchThreads - kThreads) / planes) return CERB_ETOOLARGE;     // one thread per element
    if (!seed || !keep || !aligned(seed, 8)) return CERB_EINVAL;
    const int64_t count = planes * per_plane;
    attn_keep_kernel<<<static_cast<unsigned>((count + kThreads - 1) / kThreads), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const int64_t *>(seed), static_cast<uint8_t *>(keep), Lq, Lk, count, attn_threshold(dropout_p));
    return launch_status();
}

}  // extern "C"
