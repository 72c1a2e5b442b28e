// ocr_head.hip -- the two steps that make the segmentation head an OCR head (nnet_models/ocr_utils.py), fp32, forward and backward:
//
//   spatial gather    context[b,c,k] = sum_p softmax_p(scale * logits[b,k,:])[p] * feats[b,c,p]
//   object attention  a[b,:,p] = softmax_r(scale * sum_c query[b,c,p] key[b,c,r]);  context[b,c,p] = sum_r a[b,r,p] value[b,c,r]
//
// Five pieces:
//   row statistics   one workgroup per (b,k) plane: the maximum of scale * x and 1 / sum exp(scale * x - max)
//   region pooling   out[b,c,r] = sum_p w[b,r,p] x[b,c,p]: a workgroup owns a chunk of P = 256 pixels of one image, stages the chunk's
//                    weights once in LDS (or forms them there from the logits and the row statistics), walks the channels in tiles of 32
//                    rows staged through LDS (coalesced along p), multiplies on the matrix cores in exact fp32 (32 channels x 32
//                    regions per wave, v_mfma_f32_32x32x2_f32) and writes ONE partial per (chunk,b,c,r); a second launch adds the
//                    partials in chunk order.  Used for the gather forward, dkey and dvalue.
//   gather backward  lane = pixel: the R probabilities and R running sums live in registers, one pass over the features
//   attention        lane = pixel: pass 1 accumulates the R similarities, the softmax stays in registers, pass 2 writes the context
//   forward/backward in (B,C,H,W) order; key / value / the upstream context gradient are wave-uniform operands served from LDS tables
//                    of T = 64 channels (rows padded with zeros to a multiple of 4: every inner loop is unguarded)
//
// No floating-point atomics: every sum has a fixed order (a lane's own sequence, then chunk order), so two runs give the same bits,
// and the 16-byte and the 4-byte loads of the row statistics feed the same sequence (every other access is 4 bytes per lane, 256 B
// per wave instruction): a base pointer 4 bytes into a buffer gives the same bits.
// The entry points at the bottom check their arguments before anything touches a device.
#include <math.h>

#include "common.h"
#include "loss_reduce.h"

namespace cerb {
namespace {

constexpr int kThreads = kReduceThreads;
constexpr int kMaxRegions = 32;
constexpr int kChunk = 256;                  // P: pixels per pooling workgroup, and per workgroup of the lane-per-pixel kernels
constexpr int kPoolTile = 32;                // channels per LDS tile of the pooling kernel
constexpr int kPoolStride = kChunk + 1;      // lanes = pixels write a row, lanes = rows read a column: both without bank conflicts
constexpr int kTile = 64;                    // T: channels per LDS table of the lane-per-pixel kernels
constexpr int kFoldRound = 8;                // partials loaded per round of the fold
constexpr int kUnroll = 8;                   // channel loads in flight per lane (256 B per wave instruction each)
constexpr int kGatherUnroll = 4;             // the gather backward holds 2 R values per pixel and the table rows of a round: fewer rounds in flight

// elements 4q .. 4q+3 of a row of n floats; `wide`: the row is 16-byte aligned and n % 4 == 0.  Elements past n read as `fill`.
__device__ __forceinline__ void load4(const float *__restrict__ row, int q, int n, bool wide, float fill, float (&v)[4]) {
    const int i = q << 2;
    if (wide && n - i >= 4) {
        const float4 t = *reinterpret_cast<const float4 *>(row + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (n - i > j) ? row[i + j] : fill;
    }
}

// ---- row statistics -----------------------------------------------------------------------------------------------------------
// stats[2 i] = max_p scale * x[i,p], stats[2 i + 1] = 1 / sum_p exp(scale * x[i,p] - max); lse[i] = max + log(sum) (may be null).
// A thread owns the quads q = tid, tid + 256, ... in that order whichever load width serves them.
__global__ __launch_bounds__(kThreads) void ocr_row_stats_kernel(const float *__restrict__ logits, float scale, int HW, int wide,
                                                                 float *__restrict__ stats, float *__restrict__ lse) {
    __shared__ float red[kThreads];
    const float *row = logits + static_cast<size_t>(blockIdx.x) * HW;
    const int tid = threadIdx.x;
    const int quads = (HW >> 2) + ((HW & 3) ? 1 : 0);
    float m = -INFINITY;
    for (int q = tid; q < quads; q += kThreads) {
        float v[4];
        load4(row, q, HW, wide, -INFINITY, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (HW - (q << 2) > j) m = fmaxf(m, scale * v[j]);
    }
    red[tid] = m;
    tree_fold<FoldMax>(red);
    m = red[0];
    __syncthreads();
    float sum = 0.f;
    for (int q = tid; q < quads; q += kThreads) {
        float v[4];
        load4(row, q, HW, wide, 0.f, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (HW - (q << 2) > j) sum += expf(scale * v[j] - m);
    }
    red[tid] = sum;
    tree_sum(red);
    if (tid == 0) {
        stats[2 * static_cast<size_t>(blockIdx.x)] = m;
        stats[2 * static_cast<size_t>(blockIdx.x) + 1] = 1.f / red[0];
        if (lse) lse[blockIdx.x] = m + logf(red[0]);
    }
}

// ---- region pooling -----------------------------------------------------------------------------------------------------------
// part[b][chunk][c][r] = sum over the chunk's pixels of w[b,r,p] * x[b,c,p].  kSoftmax: w = exp(scale * wsrc - max) / sum from the row
// statistics, else w = wsrc.  Dynamic LDS: R rows of weights, then kPoolTile rows of features, kPoolStride floats each.
typedef float f16v __attribute__((ext_vector_type(16)));
template <bool kSoftmax>
__global__ __launch_bounds__(kThreads) void ocr_pool_kernel(const float *__restrict__ wsrc, const float *__restrict__ stats, float scale,
                                                            const float *__restrict__ x, float *__restrict__ part, int C, int R, int HW,
                                                            int nchunks) {
    extern __shared__ float4 ocr_pool_lds[];
    float *sw = reinterpret_cast<float *>(ocr_pool_lds);
    float *sx = sw + R * kPoolStride;
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x % nchunks, b = blockIdx.x / nchunks;
    const int p0 = chunk * kChunk;
    const int np = min(kChunk, HW - p0);

    // the chunk's weights, once: lane = pixel, 256 B per wave instruction; pixels past the image read as zero
    for (int r = 0; r < R; ++r) {
        const size_t plane = static_cast<size_t>(b) * R + r;
        float v = 0.f;
        if (tid < np) {
            v = wsrc[plane * HW + p0 + tid];
            if (kSoftmax) v = expf(scale * v - stats[2 * plane]) * stats[2 * plane + 1];
        }
        sw[r * kPoolStride + tid] = v;
    }

    // a wave owns 64 pixels of the chunk; its lane supplies the operands of one v_mfma_f32_32x32x2_f32 (exact fp32):
    // A[i = channel l & 31][k = pixel l >> 5] and B[k][j = region l & 31] -- a region past R contributes a zero column
    const int lane = tid & 63, wave = tid >> 6;
    const int row = lane & 31, half = lane >> 5;
    const bool region = row < R;
    const float *ax = sx + row * kPoolStride + wave * 64 + half;
    const float *bw = sw + (region ? row : 0) * kPoolStride + wave * 64 + half;
    for (int c0 = 0; c0 < C; c0 += kPoolTile) {
        __syncthreads();          // the weights are staged; the previous tile's sums are read
        // 32 loads in flight per lane, one row of the tile each: unconditional, from clamped addresses, so that none waits for a branch
        float v[kPoolTile];
#pragma unroll
        for (int k = 0; k < kPoolTile; ++k) v[k] = x[(static_cast<size_t>(b) * C + min(c0 + k, C - 1)) * HW + p0 + min(tid, np - 1)];
#pragma unroll
        for (int k = 0; k < kPoolTile; ++k) sx[k * kPoolStride + tid] = (c0 + k < C && tid < np) ? v[k] : 0.f;
        __syncthreads();
        f16v acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int k = 0; k < 32; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ax[2 * k], region ? bw[2 * k] : 0.f, acc, 0, 0, 0);
        __syncthreads();          // every wave has read the tile: its rows now hold the four waves' sums
#pragma unroll
        for (int i = 0; i < 16; ++i) sx[(wave * 16 + i) * 64 + lane] = acc[i];
        __syncthreads();
        // the waves in wave order; element (i, l) of a wave's tile is channel (i & 3) + 8 (i >> 2) + 4 (l >> 5), region l & 31
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid + j * kThreads, i = e >> 6, l = e & 63;
            const float v = ((sx[e] + sx[1024 + e]) + sx[2048 + e]) + sx[3072 + e];
            const int c = c0 + (i & 3) + 8 * (i >> 2) + 4 * (l >> 5), r = l & 31;
            if (c < C && r < R) part[((static_cast<size_t>(b) * nchunks + chunk) * C + c) * R + r] = v;
        }
    }
}

// out[b][e] = mul * (part[b][0][e] + part[b][1][e] + ...), e = c R + r: chunk order, kFoldRound loads in flight
__global__ __launch_bounds__(kThreads) void ocr_fold_kernel(const float *__restrict__ part, float *__restrict__ out, int CR, int nchunks,
                                                            int blocks_per_image, float mul) {
    const int b = blockIdx.x / blocks_per_image;
    const int64_t e = static_cast<int64_t>(blockIdx.x % blocks_per_image) * kThreads + threadIdx.x;   // the last block may pass 2^31
    if (e >= CR) return;
    const float *p = part + static_cast<size_t>(b) * nchunks * CR + e;
    float acc = 0.f;
    int k = 0;
    for (; k + kFoldRound <= nchunks; k += kFoldRound) {
        float v[kFoldRound];
#pragma unroll
        for (int j = 0; j < kFoldRound; ++j) v[j] = p[static_cast<size_t>(k + j) * CR];
#pragma unroll
        for (int j = 0; j < kFoldRound; ++j) acc += v[j];
    }
    for (; k < nchunks; ++k) acc += p[static_cast<size_t>(k) * CR];
    out[static_cast<size_t>(b) * CR + e] = acc * mul;
}

// dot[b,k] = sum_c g[b,c,k] ctx[b,c,k]: one wave per (b,k), a lane's channels in order, then the butterfly
__global__ __launch_bounds__(64) void ocr_dot_kernel(const float *__restrict__ g, const float *__restrict__ ctx, float *__restrict__ dot,
                                                     int C, int R) {
    const int b = blockIdx.x / R, k = blockIdx.x % R;
    float acc = 0.f;
    for (int c = threadIdx.x; c < C; c += 64) {
        const size_t i = (static_cast<size_t>(b) * C + c) * R + k;
        acc = fmaf(g[i], ctx[i], acc);
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) dot[blockIdx.x] = acc;
}

// ---- the LDS table of the lane-per-pixel kernels -------------------------------------------------------------------------------
// table[cc][r] = src[b, c0 + cc, r] for the channels of one tile, rows padded to RMAX with zeros (so are the channels past C)
template <int RMAX>
__device__ __forceinline__ void stage_table(float *table, const float *__restrict__ src, int b, int c0, int C, int R) {
    __syncthreads();              // the previous table is consumed
    for (int i = threadIdx.x; i < kTile * RMAX; i += kThreads) {
        const int cc = i / RMAX, r = i % RMAX;
        table[i] = (c0 + cc < C && r < R) ? src[(static_cast<size_t>(b) * C + c0 + cc) * R + r] : 0.f;
    }
    __syncthreads();
}

// In the three kernels below a lane past the image's last pixel reads pixel 0 of its image (in bounds, no branch around a load) and
// stores nothing.
// ---- gather backward ----------------------------------------------------------------------------------------------------------
// dfeats[c,p] = sum_k p[k,p] g[c,k];  dlogits[k,p] = scale p[k,p] (sum_c g[c,k] f[c,p] - dot[k])
template <int RMAX>
__global__ __launch_bounds__(kThreads) void ocr_gather_bwd_kernel(const float *__restrict__ feats, const float *__restrict__ logits,
                                                                  const float *__restrict__ stats, const float *__restrict__ g,
                                                                  const float *__restrict__ dot, float scale,
                                                                  float *__restrict__ dfeats, float *__restrict__ dlogits, int C, int R,
                                                                  int HW, int nblk) {
    __shared__ __attribute__((aligned(16))) float table[kTile * RMAX];
    const int b = blockIdx.x / nblk;
    const int p = (blockIdx.x % nblk) * kChunk + threadIdx.x;
    const bool live = p < HW;
    float pr[RMAX], acc[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        acc[r] = 0.f;
        pr[r] = 0.f;
        if (r < R && live) {
            const size_t plane = static_cast<size_t>(b) * R + r;
            pr[r] = expf(scale * logits[plane * HW + p] - stats[2 * plane]) * stats[2 * plane + 1];
        }
    }
    const float *f = feats + static_cast<size_t>(b) * C * HW + (live ? p : 0);
    float *df = dfeats + static_cast<size_t>(b) * C * HW + (live ? p : 0);
    for (int c0 = 0; c0 < C; c0 += kTile) {
        stage_table<RMAX>(table, g, b, c0, C, R);
        const int nc = min(kTile, C - c0);
        int cc = 0;
        for (; cc + kGatherUnroll <= nc; cc += kGatherUnroll) {
            float fv[kGatherUnroll];
#pragma unroll
            for (int u = 0; u < kGatherUnroll; ++u) fv[u] = f[static_cast<size_t>(c0 + cc + u) * HW];
#pragma unroll
            for (int u = 0; u < kGatherUnroll; ++u) {
                const float *row = table + (cc + u) * RMAX;
                float d = 0.f;
#pragma unroll
                for (int r = 0; r < RMAX; ++r) {
                    acc[r] = fmaf(row[r], fv[u], acc[r]);
                    d = fmaf(pr[r], row[r], d);
                }
                if (live) df[static_cast<size_t>(c0 + cc + u) * HW] = d;
            }
        }
        for (; cc < nc; ++cc) {
            const float fv = f[static_cast<size_t>(c0 + cc) * HW];
            const float *row = table + cc * RMAX;
            float d = 0.f;
#pragma unroll
            for (int r = 0; r < RMAX; ++r) {
                acc[r] = fmaf(row[r], fv, acc[r]);
                d = fmaf(pr[r], row[r], d);
            }
            if (live) df[static_cast<size_t>(c0 + cc) * HW] = d;
        }
    }
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
        if (r < R && live) dlogits[(static_cast<size_t>(b) * R + r) * HW + p] = scale * pr[r] * (acc[r] - dot[b * R + r]);
}

// ---- attention forward --------------------------------------------------------------------------------------------------------
template <int RMAX>
__global__ __launch_bounds__(kThreads) void ocr_attn_fwd_kernel(const float *__restrict__ query, const float *__restrict__ key,
                                                                const float *__restrict__ value, float scale, float *__restrict__ ctx,
                                                                float *__restrict__ attn, int C, int R, int HW, int nblk) {
    __shared__ __attribute__((aligned(16))) float table[kTile * RMAX];
    const int b = blockIdx.x / nblk;
    const int p = (blockIdx.x % nblk) * kChunk + threadIdx.x;
    const bool live = p < HW;
    const float *qp = query + static_cast<size_t>(b) * C * HW + (live ? p : 0);
    float *op = ctx + static_cast<size_t>(b) * C * HW + (live ? p : 0);
    float a[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) a[r] = 0.f;
    // pass 1: the similarities
    for (int c0 = 0; c0 < C; c0 += kTile) {
        stage_table<RMAX>(table, key, b, c0, C, R);
        const int nc = min(kTile, C - c0);
        int cc = 0;
        for (; cc + kUnroll <= nc; cc += kUnroll) {
            float qv[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) qv[u] = qp[static_cast<size_t>(c0 + cc + u) * HW];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const float *row = table + (cc + u) * RMAX;
#pragma unroll
                for (int r = 0; r < RMAX; ++r) a[r] = fmaf(qv[u], row[r], a[r]);
            }
        }
        for (; cc < nc; ++cc) {
            const float qv = qp[static_cast<size_t>(c0 + cc) * HW];
            const float *row = table + cc * RMAX;
#pragma unroll
            for (int r = 0; r < RMAX; ++r) a[r] = fmaf(qv, row[r], a[r]);
        }
    }
    // the softmax over the regions, in registers
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
        if (r < R) {
            a[r] *= scale;
            mx = fmaxf(mx, a[r]);
        }
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        a[r] = (r < R) ? expf(a[r] - mx) : 0.f;
        sum += a[r];
    }
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        a[r] = a[r] / sum;
        if (r < R && live) attn[(static_cast<size_t>(b) * R + r) * HW + p] = a[r];
    }
    // pass 2: the context, in (B,C,H,W) order
    for (int c0 = 0; c0 < C; c0 += kTile) {
        stage_table<RMAX>(table, value, b, c0, C, R);
        const int nc = min(kTile, C - c0);
        for (int cc = 0; cc < nc; ++cc) {
            const float *row = table + cc * RMAX;
            float o = a[0] * row[0];
#pragma unroll
            for (int r = 1; r < RMAX; ++r) o = fmaf(a[r], row[r], o);
            if (live) op[static_cast<size_t>(c0 + cc) * HW] = o;
        }
    }
}

// ---- attention backward, the pixel kernel ---------------------------------------------------------------------------------------
// da[r] = sum_c g[c,p] value[c,r];  dsim = a (da - sum_r a da);  dq[c,p] = scale sum_r dsim[r] key[c,r]
template <int RMAX>
__global__ __launch_bounds__(kThreads) void ocr_attn_bwd_kernel(const float *__restrict__ gctx, const float *__restrict__ attn,
                                                                const float *__restrict__ key, const float *__restrict__ value,
                                                                float scale, float *__restrict__ dq, float *__restrict__ dsim, int C,
                                                                int R, int HW, int nblk) {
    __shared__ __attribute__((aligned(16))) float table[kTile * RMAX];
    const int b = blockIdx.x / nblk;
    const int p = (blockIdx.x % nblk) * kChunk + threadIdx.x;
    const bool live = p < HW;
    const float *gp = gctx + static_cast<size_t>(b) * C * HW + (live ? p : 0);
    float *op = dq + static_cast<size_t>(b) * C * HW + (live ? p : 0);
    float a[RMAX], da[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        da[r] = 0.f;
        a[r] = (r < R && live) ? attn[(static_cast<size_t>(b) * R + r) * HW + p] : 0.f;
    }
    for (int c0 = 0; c0 < C; c0 += kTile) {
        stage_table<RMAX>(table, value, b, c0, C, R);
        const int nc = min(kTile, C - c0);
        int cc = 0;
        for (; cc + kUnroll <= nc; cc += kUnroll) {
            float gv[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) gv[u] = gp[static_cast<size_t>(c0 + cc + u) * HW];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const float *row = table + (cc + u) * RMAX;
#pragma unroll
                for (int r = 0; r < RMAX; ++r) da[r] = fmaf(gv[u], row[r], da[r]);
            }
        }
        for (; cc < nc; ++cc) {
            const float gv = gp[static_cast<size_t>(c0 + cc) * HW];
            const float *row = table + cc * RMAX;
#pragma unroll
            for (int r = 0; r < RMAX; ++r) da[r] = fmaf(gv, row[r], da[r]);
        }
    }
    float dotv = 0.f;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) dotv = fmaf(a[r], da[r], dotv);
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        da[r] = a[r] * (da[r] - dotv);          // dsim; zero past R
        if (r < R && live) dsim[(static_cast<size_t>(b) * R + r) * HW + p] = da[r];
    }
    for (int c0 = 0; c0 < C; c0 += kTile) {
        stage_table<RMAX>(table, key, b, c0, C, R);
        const int nc = min(kTile, C - c0);
        for (int cc = 0; cc < nc; ++cc) {
            const float *row = table + cc * RMAX;
            float o = da[0] * row[0];
#pragma unroll
            for (int r = 1; r < RMAX; ++r) o = fmaf(da[r], row[r], o);
            if (live) op[static_cast<size_t>(c0 + cc) * HW] = scale * o;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int64_t chunks_of(int HW) { return (static_cast<int64_t>(HW) + kChunk - 1) / kChunk; }
int64_t align4(int64_t n) { return (n + 3) & ~static_cast<int64_t>(3); }

// the workspace in floats: [row statistics 2 B R][dot B R], padded to 16 bytes, then [partials B chunks C R]
int64_t head_floats(int B, int R) { return align4(3 * static_cast<int64_t>(B) * R); }
int64_t workspace_floats(int B, int C, int R, int HW) { return head_floats(B, R) + static_cast<int64_t>(B) * chunks_of(HW) * C * R; }

bool wide_ok(const void *p, int HW) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (HW & 3) == 0; }

int args_ok(int B, int C, int R, int HW, int dtype) {
    if (dtype < CERB_F32 || dtype > CERB_F64) return CERB_EDTYPE;
    if (dtype != CERB_F32) return CERB_EUNSUPPORTED;
    if (B <= 0 || C <= 0 || R <= 0 || HW <= 0) return CERB_EINVAL;
    if (R > kMaxRegions) return CERB_EUNSUPPORTED;           // the caller takes the stock ops there
    const int64_t cr = static_cast<int64_t>(C) * R;
    // a lane's pixel index, the launch grids and c R + r are ints
    if (HW > 0x7fffffff - 1024 || cr > 0x7fffffff || static_cast<int64_t>(B) * chunks_of(HW) > 0x7fffffff ||
        static_cast<int64_t>(B) * ((cr + kThreads - 1) / kThreads) > 0x7fffffff || static_cast<int64_t>(B) * R > 0x7fffffff)
        return CERB_ETOOLARGE;
    return CERB_OK;
}

template <bool kSoftmax>
int pool(const float *wsrc, const float *stats, float scale, const float *x, float *part, float *out, float mul, int B, int C, int R, int HW,
         hipStream_t s) {
    static std::atomic<uint64_t> lds_done{0};
    const size_t lds = static_cast<size_t>(R + kPoolTile) * kPoolStride * sizeof(float);
    int rc = ensure_lds(ocr_pool_kernel<kSoftmax>, lds, &lds_done);
    if (rc) return rc;
    const int nchunks = static_cast<int>(chunks_of(HW));
    ocr_pool_kernel<kSoftmax><<<B * nchunks, kThreads, lds, s>>>(wsrc, stats, scale, x, part, C, R, HW, nchunks);
    rc = launch_status();
    if (rc) return rc;
    const int cr = C * R, blocks = (cr + kThreads - 1) / kThreads;
    ocr_fold_kernel<<<B * blocks, kThreads, 0, s>>>(part, out, cr, nchunks, blocks, mul);
    return launch_status();
}

// K(RMAX) for the smallest multiple of 4 that holds R
#define OCR_DISPATCH(R, K)              \
    switch (((R) + 3) / 4) {            \
        case 1: K(4); break;            \
        case 2: K(8); break;            \
        case 3: K(12); break;           \
        case 4: K(16); break;           \
        case 5: K(20); break;           \
        case 6: K(24); break;           \
        case 7: K(28); break;           \
        default: K(32); break;          \
    }

}  // namespace
}  // namespace cerb

using namespace cerb;

extern "C" {

int64_t cerberus_ocr_workspace_bytes(int B, int C, int R, int HW) {
    if (args_ok(B, C, R, HW, CERB_F32)) return 0;
    return 4 * workspace_floats(B, C, R, HW);
}

static int workspace_ok(const void *workspace, int64_t workspace_bytes, int B, int C, int R, int HW) {
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < 4 * workspace_floats(B, C, R, HW)) return CERB_EINVAL;
    return CERB_OK;
}

int cerberus_ocr_gather_forward(const void *feats, const void *logits, void *context, void *lse, void *workspace,
                                int64_t workspace_bytes, int B, int C, int K, int HW, float scale, int dtype, void *stream) {
    int rc = args_ok(B, C, K, HW, dtype);
    if (rc) return rc;
    if (!feats || !logits || !context || !lse) return CERB_EINVAL;
    rc = workspace_ok(workspace, workspace_bytes, B, C, K, HW);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *stats = static_cast<float *>(workspace), *part = stats + head_floats(B, K);
    const float *x = static_cast<const float *>(logits);
    ocr_row_stats_kernel<<<B * K, kThreads, 0, s>>>(x, scale, HW, wide_ok(x, HW), stats, static_cast<float *>(lse));
    rc = launch_status();
    if (rc) return rc;
    return pool<true>(x, stats, scale, static_cast<const float *>(feats), part, static_cast<float *>(context), 1.f, B, C, K, HW, s);
}

int cerberus_ocr_gather_backward(const void *feats, const void *logits, const void *context, const void *grad_context, void *grad_feats,
                                 void *grad_logits, void *workspace, int64_t workspace_bytes, int B, int C, int K, int HW, float scale,
                                 int dtype, void *stream) {
    int rc = args_ok(B, C, K, HW, dtype);
    if (rc) return rc;
    if (!feats || !logits || !context || !grad_context || !grad_feats || !grad_logits) return CERB_EINVAL;
    rc = workspace_ok(workspace, workspace_bytes, B, C, K, HW);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *stats = static_cast<float *>(workspace), *dot = stats + 2 * static_cast<size_t>(B) * K;
    const float *x = static_cast<const float *>(logits), *g = static_cast<const float *>(grad_context);
    ocr_row_stats_kernel<<<B * K, kThreads, 0, s>>>(x, scale, HW, wide_ok(x, HW), stats, nullptr);
    rc = launch_status();
    if (rc) return rc;
    ocr_dot_kernel<<<B * K, 64, 0, s>>>(g, static_cast<const float *>(context), dot, C, K);
    rc = launch_status();
    if (rc) return rc;
    const int nblk = static_cast<int>(chunks_of(HW));
#define OCR_GATHER_BWD(RMAX)                                                                                                          \
    ocr_gather_bwd_kernel<RMAX><<<B * nblk, kThreads, 0, s>>>(static_cast<const float *>(feats), x, stats, g, dot, scale,             \
                                                              static_cast<float *>(grad_feats), static_cast<float *>(grad_logits), C, \
                                                              K, HW, nblk)
    OCR_DISPATCH(K, OCR_GATHER_BWD)
#undef OCR_GATHER_BWD
    return launch_status();
}

int cerberus_ocr_attention_forward(const void *query, const void *key, const void *value, void *context, void *attn, int B, int C, int R,
                                   int HW, float scale, int dtype, void *stream) {
    const int rc = args_ok(B, C, R, HW, dtype);
    if (rc) return rc;
    if (!query || !key || !value || !context || !attn) return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nblk = static_cast<int>(chunks_of(HW));
#define OCR_ATTN_FWD(RMAX)                                                                                                              \
    ocr_attn_fwd_kernel<RMAX><<<B * nblk, kThreads, 0, s>>>(static_cast<const float *>(query), static_cast<const float *>(key),        \
                                                            static_cast<const float *>(value), scale, static_cast<float *>(context),  \
                                                            static_cast<float *>(attn), C, R, HW, nblk)
    OCR_DISPATCH(R, OCR_ATTN_FWD)
#undef OCR_ATTN_FWD
    return launch_status();
}

int cerberus_ocr_attention_backward(const void *grad_context, const void *query, const void *key, const void *value, const void *attn,
                                    void *grad_query, void *grad_key, void *grad_value, void *dsim, void *workspace,
                                    int64_t workspace_bytes, int B, int C, int R, int HW, float scale, int dtype, void *stream) {
    int rc = args_ok(B, C, R, HW, dtype);
    if (rc) return rc;
    if (!grad_context || !query || !key || !value || !attn || !grad_query || !grad_key || !grad_value || !dsim) return CERB_EINVAL;
    rc = workspace_ok(workspace, workspace_bytes, B, C, R, HW);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float *g = static_cast<const float *>(grad_context), *a = static_cast<const float *>(attn);
    float *ds = static_cast<float *>(dsim), *part = static_cast<float *>(workspace) + head_floats(B, R);
    const int nblk = static_cast<int>(chunks_of(HW));
#define OCR_ATTN_BWD(RMAX)                                                                                                             \
    ocr_attn_bwd_kernel<RMAX><<<B * nblk, kThreads, 0, s>>>(g, a, static_cast<const float *>(key), static_cast<const float *>(value), \
                                                            scale, static_cast<float *>(grad_query), ds, C, R, HW, nblk)
    OCR_DISPATCH(R, OCR_ATTN_BWD)
#undef OCR_ATTN_BWD
    rc = launch_status();
    if (rc) return rc;
    // the two poolings share the partials: they run in stream order
    rc = pool<false>(ds, nullptr, 0.f, static_cast<const float *>(query), part, static_cast<float *>(grad_key), scale, B, C, R, HW, s);
    if (rc) return rc;
    return pool<false>(a, nullptr, 0.f, g, part, static_cast<float *>(grad_value), 1.f, B, C, R, HW, s);
}

}  // extern "C"
