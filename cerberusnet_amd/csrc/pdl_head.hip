// pdl_head.hip -- the Panoptic-DeepLab decoder head's own step (nnet_models/deeplab_panoptic.py): the depthwise 5x5 convolution
// (stride 1, zero padding 2, no bias, fp32 NCHW) of every `fuse` block and classifier, alone or over the virtual tensor
//     cat(interpolate(low, (H,W), bilinear, align_corners=True), skip)
// of a decoder stage: neither the upsampled map nor the concatenation exists in memory.  DESIGN.md 3.26.
//
// One workgroup of 256 lanes per (plane, tile of 32 x 64 pixels): the tile's (32+4) x (64+8) window goes to LDS once (channels
// below Ca sample `low` on the way, with ATen's fp32 operation order), then a lane owns 4 adjacent pixels of 2 rows and slides
// over its 6 window rows: a row segment is read from LDS once for all the output rows it feeds.  The channel's 25 weights are
// uniform over the workgroup.  The window starts 4 columns left of the tile, so that its 16-byte slots are the 16-byte slots of
// the image row: wide loads and stores wherever the pointer and W allow them (a flag per tensor), scalar ones elsewhere; both
// routes move the same values, so the bits do not depend on the alignment.
//
// Backward, at most three launches: (1) the same stencil with the flipped weights over grad_y -- channels >= Ca write grad_skip,
// channels < Ca write the gradient of the upsampled map into the workspace -- and, in the same workgroup, the tile's 25 products
// of grad_weight from the input window built again from low / skip: fp32 over a lane's 8 pixels, float64 above (loss_reduce.h:
// wave butterfly, the 4 waves in order), one partial per (channel, tap, image, tile); (2) grad_low: every low-res pixel gathers
// the high-res pixels that sampled it, rows then columns ascending, with the forward's weights; (3) one workgroup per (channel,
// tap) adds the partials with the tree fold.  No atomics anywhere: the same bits on every run and in a replayed graph.
#include "loss_reduce.h"

namespace cerb {
namespace {

constexpr int kTH = 32, kTW = 64;             // the tile
constexpr int kRows = 2;                      // output rows per lane: 16 lane rows x 16 lane columns of 4 pixels
constexpr int kWinH = kTH + 4;                // window rows: y0 - 2 .. y0 + kTH + 1
constexpr int kWinW = kTW + 8;                // window columns: x0 - 4 .. x0 + kTW + 3 (x0 - 2 .. x0 + kTW + 1 are used)
constexpr int kSlots = kWinW / 4;             // 16-byte slots per window row
constexpr int kTaps = 25;
constexpr int kAdjoint = 8;                   // candidate columns of a low-res pixel whose weights the gather keeps in registers
static_assert(kReduceThreads == (kTH / kRows) * (kTW / 4), "a lane owns kRows x 4 pixels of the tile");

struct PdlArgs {
    const float *low;       // (B,Ca,h,w): the map the stage upsamples; unused when Ca == 0
    const float *skip;      // (B,Cb,H,W): the channels Ca .. Ca+Cb-1 of the virtual input
    const float *gy;        // backward: grad_y (B,Ca+Cb,H,W)
    const float *weight;    // (Ca+Cb,25)
    float *out_a;           // forward: y (B,Ca+Cb,H,W); backward: the gradient of the upsampled channels (B,Ca,H,W), workspace
    float *out_b;           // backward: grad_skip (B,Cb,H,W)
    double *part;           // backward: grad_weight partials [Ca+Cb][25][B * tiles]
    int Ca, Cb, h, w, H, W;
    float sy, sx;           // (h-1)/(H-1), (w-1)/(W-1) in fp32; 0 when the output side is 1
    int tiles_x, tiles;     // per plane
    int wide_skip, wide_gy, wide_a, wide_b;     // the tensor's rows start on 16 bytes: pointer and W both allow wide accesses
    int need_a, need_b;     // backward: which input gradients are asked for
};

// ATen's upsample_bilinear2d, align_corners = true, in fp32: src = scale * dst, i0 = (int)src, i1 = min(i0 + 1, n - 1),
// lambda = src - i0.  i0 is clamped as well: scale * (N - 1) may round to a hair above n - 1.
__device__ __forceinline__ void source_index(float scale, int dst, int n, int &i0, int &i1, float &lam) {
    const float src = scale * static_cast<float>(dst);
    i0 = min(static_cast<int>(src), n - 1);
    i1 = min(i0 + 1, n - 1);
    lam = src - static_cast<float>(i0);
}

__device__ __forceinline__ float sample_low(const float *__restrict__ plane, int w, int y0, int y1, float ly, float sx, int x, int wl) {
    int x0, x1;
    float lx;
    source_index(sx, x, wl, x0, x1, lx);
    const float *r0 = plane + static_cast<size_t>(y0) * w, *r1 = plane + static_cast<size_t>(y1) * w;
    const float hx = 1.f - lx, hy = 1.f - ly;
    return hy * (hx * r0[x0] + lx * r0[x1]) + ly * (hx * r1[x0] + lx * r1[x1]);
}

// a plane's window: zero outside the image
__device__ __forceinline__ void stage_plane(float *__restrict__ win, const float *__restrict__ plane, int H, int W, int y0, int x0, bool wide) {
    for (int i = threadIdx.x; i < kWinH * kSlots; i += kReduceThreads) {
        const int row = i / kSlots, slot = i - row * kSlots;
        const int y = y0 - 2 + row, x = x0 - 4 + 4 * slot;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (y >= 0 && y < H) {
            const float *p = plane + static_cast<size_t>(y) * W;
            if (wide) {         // W % 4 == 0 and x % 4 == 0: the slot lies inside the row or outside it
                if (x >= 0 && x < W) v = *reinterpret_cast<const float4 *>(p + x);
            } else {
                if (x >= 0 && x < W) v.x = p[x];
                if (x + 1 >= 0 && x + 1 < W) v.y = p[x + 1];
                if (x + 2 >= 0 && x + 2 < W) v.z = p[x + 2];
                if (x + 3 >= 0 && x + 3 < W) v.w = p[x + 3];
            }
        }
        *reinterpret_cast<float4 *>(win + row * kWinW + 4 * slot) = v;
    }
}

// the window of an upsampled channel: every element sampled from the low-res plane
__device__ __forceinline__ void stage_up(float *__restrict__ win, const float *__restrict__ plane, const PdlArgs &a, int y0, int x0) {
    for (int i = threadIdx.x; i < kWinH * kSlots; i += kReduceThreads) {
        const int row = i / kSlots, slot = i - row * kSlots;
        const int y = y0 - 2 + row, x = x0 - 4 + 4 * slot;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (y >= 0 && y < a.H) {
            int i0, i1;
            float ly;
            source_index(a.sy, y, a.h, i0, i1, ly);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e >= 0 && x + e < a.W) v[e] = sample_low(plane, a.w, i0, i1, ly, a.sx, x + e, a.w);
        }
        *reinterpret_cast<float4 *>(win + row * kWinW + 4 * slot) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// 12 window floats of one row: the lane's 4 pixels are elements 4..7, its taps reach elements 2..9
__device__ __forceinline__ void load_row(const float *__restrict__ win, int row, int cx, float (&v)[12]) {
    const float4 *p = reinterpret_cast<const float4 *>(win + row * kWinW + 4 * cx);
    const float4 q0 = p[0], q1 = p[1], q2 = p[2];
    v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w;
    v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
    v[8] = q2.x; v[9] = q2.y; v[10] = q2.z; v[11] = q2.w;
}

__device__ __forceinline__ void store_rows(float *__restrict__ plane, const float (&acc)[kRows][4], int H, int W, int y, int x, bool wide) {
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
        if (y + o >= H) break;
        float *p = plane + static_cast<size_t>(y + o) * W + x;
        if (wide) {             // W % 4 == 0 and x % 4 == 0: all 4 pixels are inside or none is
            if (x < W) *reinterpret_cast<float4 *>(p) = make_float4(acc[o][0], acc[o][1], acc[o][2], acc[o][3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < W) p[e] = acc[o][e];
        }
    }
}

// kMode 0: forward; 1: backward, input gradients only; 2: backward with the grad_weight partials
template <int kMode>
__global__ __launch_bounds__(kReduceThreads) void pdl_dwconv_kernel(const PdlArgs a) {
    __shared__ __attribute__((aligned(16))) float win[(kMode == 2 ? 2 : 1) * kWinH * kWinW];
    __shared__ double red[kMode == 2 ? kTaps * 4 : 1];
    const int C = a.Ca + a.Cb;
    const int plane = blockIdx.x, b = plane / C, c = plane - b * C;
    const int tile = blockIdx.y, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int y0 = ty * kTH, x0 = tx * kTW;
    const size_t HW = static_cast<size_t>(a.H) * a.W;
    const bool up = c < a.Ca;
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;

    // the stencil's source: the virtual input (forward) or grad_y (backward); the backward flips the taps
    float wt[kTaps];
#pragma unroll
    for (int k = 0; k < kTaps; ++k) wt[k] = a.weight[c * kTaps + (kMode == 0 ? k : kTaps - 1 - k)];

    float *out;
    bool wide_out, do_out = true;
    if (kMode == 1 && !(up ? a.need_a : a.need_b)) return;         // uniform over the workgroup: nothing to write for this plane
    if (kMode == 0) {
        if (up) stage_up(win, a.low + (static_cast<size_t>(b) * a.Ca + c) * a.h * a.w, a, y0, x0);
        else stage_plane(win, a.skip + (static_cast<size_t>(b) * a.Cb + (c - a.Ca)) * HW, a.H, a.W, y0, x0, a.wide_skip);
        out = a.out_a + static_cast<size_t>(plane) * HW;
        wide_out = a.wide_a;
    } else {
        stage_plane(win, a.gy + static_cast<size_t>(plane) * HW, a.H, a.W, y0, x0, a.wide_gy);
        if (kMode == 2) {
            float *in = win + kWinH * kWinW;
            if (up) stage_up(in, a.low + (static_cast<size_t>(b) * a.Ca + c) * a.h * a.w, a, y0, x0);
            else stage_plane(in, a.skip + (static_cast<size_t>(b) * a.Cb + (c - a.Ca)) * HW, a.H, a.W, y0, x0, a.wide_skip);
        }
        out = up ? a.out_a + (static_cast<size_t>(b) * a.Ca + c) * HW : a.out_b + (static_cast<size_t>(b) * a.Cb + (c - a.Ca)) * HW;
        wide_out = up ? a.wide_a : a.wide_b;
        do_out = up ? a.need_a : a.need_b;
    }
    __syncthreads();

    if (do_out) {
        float acc[kRows][4] = {};
#pragma unroll
        for (int r = 0; r < kRows + 4; ++r) {
            float v[12];
            load_row(win, kRows * ry + r, cx, v);
#pragma unroll
            for (int o = 0; o < kRows; ++o) {
                const int ky = r - o;
                if (ky < 0 || ky > 4) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int kx = 0; kx < 5; ++kx) acc[o][e] = fmaf(v[2 + e + kx], wt[ky * 5 + kx], acc[o][e]);
            }
        }
        store_rows(out, acc, a.H, a.W, y0 + kRows * ry, x0 + 4 * cx, wide_out);
    }

    if (kMode == 2) {
        // grad_weight[c][ky][kx] += grad_y[y][x] in[y + ky - 2][x + kx - 2]: grad_y is zero outside the image (its window is)
        const float *in = win + kWinH * kWinW;
        float g[kRows][4];
#pragma unroll
        for (int o = 0; o < kRows; ++o) {
            const float4 q = *reinterpret_cast<const float4 *>(win + (kRows * ry + o + 2) * kWinW + 4 * cx + 4);
            g[o][0] = q.x; g[o][1] = q.y; g[o][2] = q.z; g[o][3] = q.w;
        }
        float gw[kTaps] = {};
#pragma unroll
        for (int r = 0; r < kRows + 4; ++r) {
            float v[12];
            load_row(in, kRows * ry + r, cx, v);
#pragma unroll
            for (int o = 0; o < kRows; ++o) {
                const int ky = r - o;
                if (ky < 0 || ky > 4) continue;
#pragma unroll
                for (int kx = 0; kx < 5; ++kx)
#pragma unroll
                    for (int e = 0; e < 4; ++e) gw[ky * 5 + kx] = fmaf(g[o][e], v[2 + e + kx], gw[ky * 5 + kx]);
            }
        }
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const double s = wave_sum(static_cast<double>(gw[k]));
            if ((threadIdx.x & 63) == 0) red[k * 4 + (threadIdx.x >> 6)] = s;
        }
        __syncthreads();
        if (threadIdx.x < kTaps) {
            const size_t n = static_cast<size_t>(gridDim.x / C) * a.tiles;      // partials per (channel, tap)
            a.part[(static_cast<size_t>(c) * kTaps + threadIdx.x) * n + static_cast<size_t>(b) * a.tiles + tile] =
                waves_fold<FoldSum>(red + threadIdx.x * 4);
        }
    }
}

// grad_weight[c][k] = the partials of (c, k) in index order: one value per thread, then the tree
__global__ __launch_bounds__(kReduceThreads) void pdl_weight_fold_kernel(const double *__restrict__ part, float *__restrict__ gw, int64_t n) {
    __shared__ double row[kReduceThreads];
    const double *p = part + static_cast<size_t>(blockIdx.x) * n;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kReduceThreads) s += p[i];
    row[threadIdx.x] = s;
    tree_sum(row);
    if (threadIdx.x == 0) gw[blockIdx.x] = static_cast<float>(row[0]);
}

// the weight of low-res index `i` in the sample of high-res index `dst`; false when `dst` does not touch it
__device__ __forceinline__ bool adjoint_weight(float scale, int dst, int n, int i, float &wgt) {
    int i0, i1;
    float lam;
    source_index(scale, dst, n, i0, i1, lam);
    if (i0 != i && i1 != i) return false;
    wgt = (i0 == i ? 1.f - lam : 0.f) + (i1 == i ? lam : 0.f);
    return true;
}

// high-res indices that may sample low-res index i: scale * dst within one pixel of i, one more on either side for rounding
__device__ __forceinline__ void adjoint_range(float scale, int i, int N, int &lo, int &hi) {
    lo = 0;
    hi = N - 1;
    if (scale > 0.f) {
        const float top = static_cast<float>(N - 1);
        lo = max(0, static_cast<int>(fminf(floorf(static_cast<float>(i - 1) / scale), top)) - 1);
        hi = min(N - 1, static_cast<int>(fminf(ceilf(static_cast<float>(i + 1) / scale), top)) + 1);
    }
}

// grad_low (B,Ca,h,w) from the gradient of the upsampled channels (B,Ca,H,W): owner computes, rows then columns ascending
__global__ __launch_bounds__(kReduceThreads) void pdl_grad_low_kernel(const float *__restrict__ gup, float *__restrict__ glow, int64_t planes,
                                                                int h, int w, int H, int W, float sy, float sx) {
    const int64_t total = planes * h * w;
    for (int64_t idx = static_cast<int64_t>(blockIdx.x) * kReduceThreads + threadIdx.x; idx < total;
         idx += static_cast<int64_t>(gridDim.x) * kReduceThreads) {
        const int j = static_cast<int>(idx % w), i = static_cast<int>((idx / w) % h);
        const int64_t plane = idx / (static_cast<int64_t>(h) * w);
        const float *g = gup + static_cast<size_t>(plane) * H * W;
        int ylo, yhi, xlo, xhi;
        adjoint_range(sy, i, H, ylo, yhi);
        adjoint_range(sx, j, W, xlo, xhi);
        // the column weights are the same on every row: up to kAdjoint candidate columns keep them in registers (ratios >= 0.5 on
        // this axis); a wider range computes them again per row.  Same terms in the same order either way.
        const int nx = xhi - xlo + 1;
        float wxs[kAdjoint];
        unsigned hits = 0;
        if (nx <= kAdjoint) {
#pragma unroll
            for (int t = 0; t < kAdjoint; ++t) {
                float wx = 0.f;
                if (t < nx && adjoint_weight(sx, xlo + t, w, j, wx)) hits |= 1u << t;
                wxs[t] = wx;
            }
        }
        float sum = 0.f;
        for (int y = ylo; y <= yhi; ++y) {
            float wy;
            if (!adjoint_weight(sy, y, h, i, wy)) continue;
            const float *gr = g + static_cast<size_t>(y) * W;
            float rowsum = 0.f;
            if (nx <= kAdjoint) {
#pragma unroll
                for (int t = 0; t < kAdjoint; ++t)
                    if ((hits >> t) & 1u) rowsum = fmaf(wxs[t], gr[xlo + t], rowsum);
            } else {
                for (int x = xlo; x <= xhi; ++x) {
                    float wx;
                    if (adjoint_weight(sx, x, w, j, wx)) rowsum = fmaf(wx, gr[x], rowsum);
                }
            }
            sum = fmaf(wy, rowsum, sum);
        }
        glow[idx] = sum;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int64_t tiles_of(int H, int W) { return (static_cast<int64_t>(H) + kTH - 1) / kTH * ((static_cast<int64_t>(W) + kTW - 1) / kTW); }
int64_t up_floats(int B, int Ca, int H, int W) { return (static_cast<int64_t>(B) * Ca * H * W + 3) & ~static_cast<int64_t>(3); }
int64_t part_count(int B, int Ca, int Cb, int H, int W) { return (static_cast<int64_t>(Ca) + Cb) * kTaps * B * tiles_of(H, W); }
int64_t workspace_need(int B, int Ca, int Cb, int H, int W) { return 4 * up_floats(B, Ca, H, W) + 8 * part_count(B, Ca, Cb, H, W); }

int sizes_ok(int B, int Ca, int Cb, int h, int w, int H, int W) {
    if (B <= 0 || Ca < 0 || Cb <= 0 || H <= 0 || W <= 0) return CERB_EINVAL;
    if (Ca > 0 && (h <= 0 || w <= 0)) return CERB_EINVAL;
    const int64_t lim = 0x7fffffff, C = static_cast<int64_t>(Ca) + Cb;
    // pixel and window coordinates, B C (grid.x), C 25 and the partials per tap are ints; the tiles of a plane are grid.y
    if (static_cast<int64_t>(H) * W > lim - 1024 || W > lim - 1024 || B * C > lim || C * kTaps > lim || tiles_of(H, W) > 65535 ||
        B * tiles_of(H, W) > lim)
        return CERB_ETOOLARGE;
    if (Ca > 0 && static_cast<int64_t>(h) * w > lim) return CERB_ETOOLARGE;
    return CERB_OK;
}

int args_ok(int B, int Ca, int Cb, int h, int w, int H, int W, int dtype) {
    if (dtype < CERB_F32 || dtype > CERB_F64) return CERB_EDTYPE;
    if (dtype != CERB_F32) return CERB_EUNSUPPORTED;
    return sizes_ok(B, Ca, Cb, h, w, H, W);
}

bool bad_ptr(const void *p) { return !p || (reinterpret_cast<uintptr_t>(p) & 3); }
int wide_ok(const void *p, int W) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (W & 3) == 0; }

PdlArgs geometry(int Ca, int Cb, int h, int w, int H, int W) {
    PdlArgs a = {};
    a.Ca = Ca; a.Cb = Cb; a.h = Ca > 0 ? h : 1; a.w = Ca > 0 ? w : 1; a.H = H; a.W = W;
    a.sy = H > 1 ? static_cast<float>(a.h - 1) / (H - 1) : 0.f;
    a.sx = W > 1 ? static_cast<float>(a.w - 1) / (W - 1) : 0.f;
    a.tiles_x = (W + kTW - 1) / kTW;
    a.tiles = static_cast<int>(tiles_of(H, W));
    return a;
}

}  // namespace
}  // namespace cerb

using namespace cerb;

extern "C" {

int64_t cerberus_pdl_workspace_bytes(int B, int Ca, int Cb, int H, int W) {
    if (sizes_ok(B, Ca, Cb, 1, 1, H, W)) return 0;
    return workspace_need(B, Ca, Cb, H, W);
}

int cerberus_pdl_dwconv_forward(const void *low, const void *skip, const void *weight, void *out, int B, int Ca, int Cb, int h, int w,
                                int H, int W, int dtype, void *stream) {
    const int rc = args_ok(B, Ca, Cb, h, w, H, W, dtype);
    if (rc) return rc;
    if ((Ca > 0 && bad_ptr(low)) || bad_ptr(skip) || bad_ptr(weight) || bad_ptr(out)) return CERB_EINVAL;
    PdlArgs a = geometry(Ca, Cb, h, w, H, W);
    a.low = static_cast<const float *>(low);
    a.skip = static_cast<const float *>(skip);
    a.weight = static_cast<const float *>(weight);
    a.out_a = static_cast<float *>(out);
    a.wide_skip = wide_ok(skip, W);
    a.wide_a = wide_ok(out, W);
    pdl_dwconv_kernel<0><<<dim3(B * (Ca + Cb), a.tiles), kReduceThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    return launch_status();
}

int cerberus_pdl_dwconv_backward(const void *grad_out, const void *low, const void *skip, const void *weight, void *grad_low,
                                 void *grad_skip, void *grad_weight, void *workspace, int64_t workspace_bytes, int B, int Ca, int Cb,
                                 int h, int w, int H, int W, int dtype, void *stream) {
    const int rc = args_ok(B, Ca, Cb, h, w, H, W, dtype);
    if (rc) return rc;
    if (Ca == 0) grad_low = nullptr;
    if (bad_ptr(grad_out) || (Ca > 0 && bad_ptr(low)) || bad_ptr(skip) || bad_ptr(weight)) return CERB_EINVAL;
    if (!grad_low && !grad_skip && !grad_weight) return CERB_EINVAL;                   // nothing asked for
    if ((grad_low && bad_ptr(grad_low)) || (grad_skip && bad_ptr(grad_skip)) || (grad_weight && bad_ptr(grad_weight))) return CERB_EINVAL;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < workspace_need(B, Ca, Cb, H, W)) return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PdlArgs a = geometry(Ca, Cb, h, w, H, W);
    a.low = static_cast<const float *>(low);
    a.skip = static_cast<const float *>(skip);
    a.gy = static_cast<const float *>(grad_out);
    a.weight = static_cast<const float *>(weight);
    a.out_a = static_cast<float *>(workspace);
    a.out_b = static_cast<float *>(grad_skip);
    a.part = reinterpret_cast<double *>(static_cast<float *>(workspace) + up_floats(B, Ca, H, W));
    a.wide_skip = wide_ok(skip, W);
    a.wide_gy = wide_ok(grad_out, W);
    a.wide_a = wide_ok(workspace, W);
    a.wide_b = wide_ok(grad_skip, W);
    a.need_a = grad_low != nullptr;
    a.need_b = grad_skip != nullptr;
    const dim3 grid(B * (Ca + Cb), a.tiles);
    if (grad_weight) pdl_dwconv_kernel<2><<<grid, kReduceThreads, 0, s>>>(a);
    else pdl_dwconv_kernel<1><<<grid, kReduceThreads, 0, s>>>(a);
    int st = launch_status();
    if (st) return st;
    if (grad_low) {
        const int64_t total = static_cast<int64_t>(B) * Ca * a.h * a.w;
        const int blocks = static_cast<int>(std::min<int64_t>((total + kReduceThreads - 1) / kReduceThreads, 1 << 20));
        pdl_grad_low_kernel<<<blocks, kReduceThreads, 0, s>>>(a.out_a, static_cast<float *>(grad_low), static_cast<int64_t>(B) * Ca, a.h, a.w,
                                                              H, W, a.sy, a.sx);
        st = launch_status();
        if (st) return st;
    }
    if (grad_weight) {
        pdl_weight_fold_kernel<<<(Ca + Cb) * kTaps, kReduceThreads, 0, s>>>(a.part, static_cast<float *>(grad_weight),
                                                                             static_cast<int64_t>(B) * a.tiles);
        st = launch_status();
    }
    return st;
}

}  // extern "C"
