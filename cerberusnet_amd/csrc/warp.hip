// warp.hip -- fused flow_warp forward / backward.
//
// Replaces the whole body of the reference's flow_warp
// (/root/reference/nnet_training/loss_functions/UnFlowLoss.py:83-94):
//   mesh_grid (:11-20, built on the CPU and copied to the device every call)
//   + flow -> norm_grid (:22-32) -> F.grid_sample(align_corners=False) (:92-93)
// and the autograd chain behind it, in ONE kernel per direction: no (B,H,W,2)
// grid tensor, no host mesh, no elementwise kernels.
//
// The coordinate arithmetic reproduces the reference's fp32 rounding sequence
// exactly (x + f, *2, /(W-1), -1, then ATen's unnormalise), with contraction
// disabled, because at x ~ 256 one fp32 ulp of coordinate (3e-5 px) is already
// above the 1e-5 parity budget (hard part 2).  Quirk Q2 is
// reproduced: the grid is normalised by (W-1) but sampled with
// align_corners=False, so zero flow is not the identity.
//
// Work decomposition: a workgroup is 64 consecutive pixels (the lanes of a
// wave: coalesced flow loads, output stores and near-coalesced taps) times
// kCg channel groups (one wave each).  The flow gradient is a sum over
// channels: each wave reduces its own channels in registers, the kCg partials
// meet in LDS, wave 0 stores -- deterministic, no atomics.  The image gradient
// is a data-dependent scatter: fp32/fp64 hardware atomics, as ATen does.
#include <algorithm>
#include <type_traits>

#include "warp16_common.h"

namespace cerb {
namespace {

// Grid: 1-D over the B * strips-per-image pixel strips, one per workgroup.  T: image / output
// storage type, F: flow type
// (F = float with a 16-bit image keeps full flow precision: the reference's grid_sample runs
// in fp32 under autocast with whatever precision the flow arrives in).
template <typename T, typename F, bool PAIR, int kCg>
__global__ __launch_bounds__(kPix * kCg) void warp_fwd_kernel(
    const T *__restrict__ image, const F *__restrict__ flow, T *__restrict__ out,
    void *__restrict__ ctx, int B, int C, int H, int W, int pad_mode, int interp) {
    using A = typename Acc<T>::type;
    const int64_t plane = static_cast<int64_t>(H) * W;
    const int lane = threadIdx.x & (kPix - 1);
    const int cg = threadIdx.x / kPix;
    const Strips strips(H, W);
    const int spp = strips.per_image();
    const int64_t nstrips = static_cast<int64_t>(B) * spp;
    TapRange range;
    const int first = xcd_chunk(blockIdx.x, gridDim.x);
    for (int64_t strip = first; strip < nstrips; strip += gridDim.x) {
        const int b = static_cast<int>(strip / spp);
        int x, y;
        if (!strips.pixel(static_cast<int>(strip % spp), lane, H, W, x, y)) continue;
        const int64_t p = static_cast<int64_t>(y) * W + x;
        const F *fl = flow + static_cast<int64_t>(b) * 2 * plane + p;
        const Coord<A> cx = source_coord<A>(x, static_cast<A>(ld(fl)), W, pad_mode);
        const Coord<A> cy = source_coord<A>(y, static_cast<A>(ld(fl + plane)), H, pad_mode);
        const T *img = image + static_cast<int64_t>(b) * C * plane;
        T *dst = out + static_cast<int64_t>(b) * C * plane + p;
        if (interp == CERB_INTERP_NEAREST) {
            if (ctx && cg == 0) {   // the backward's context: positions and the floor taps' ranges (the snapped tap is one of them)
                float *pos = ctx_pos(ctx, B, H, W) + static_cast<int64_t>(b) * 2 * plane + p;
                pos[0] = static_cast<float>(cx.pos);
                pos[plane] = static_cast<float>(cy.pos);
                range.add(x, y, tap_index(static_cast<float>(floor(cx.pos))), tap_index(static_cast<float>(floor(cy.pos))), W, H);
            }
            const A xn = nearbyint(cx.pos), yn = nearbyint(cy.pos);
            const bool ok = xn >= A(0) && xn < static_cast<A>(W) && yn >= A(0) && yn < static_cast<A>(H);
            const int64_t off = ok ? static_cast<int64_t>(yn) * W + static_cast<int64_t>(xn) : 0;
            for (int c = cg; c < C; c += kCg)
                st(dst + c * plane, ok ? ld(img + c * plane + off) : A(0));
            continue;
        }
        const A x0f = floor(cx.pos), y0f = floor(cy.pos);
        const A x1f = x0f + A(1), y1f = y0f + A(1);
        const A wnw = (x1f - cx.pos) * (y1f - cy.pos);
        const A wne = (cx.pos - x0f) * (y1f - cy.pos);
        const A wsw = (x1f - cx.pos) * (cy.pos - y0f);
        const A wse = (cx.pos - x0f) * (cy.pos - y0f);
        const int x0 = tap_index(static_cast<float>(x0f)), y0 = tap_index(static_cast<float>(y0f));
        const bool okx0 = x0 >= 0 && x0 < W, okx1 = x0 + 1 >= 0 && x0 + 1 < W;
        const bool oky0 = y0 >= 0 && y0 < H, oky1 = y0 + 1 >= 0 && y0 + 1 < H;
        const int64_t o00 = static_cast<int64_t>(y0) * W + x0;
        if (ctx && cg == 0) {
            float *pos = ctx_pos(ctx, B, H, W) + static_cast<int64_t>(b) * 2 * plane + p;
            pos[0] = static_cast<float>(cx.pos);
            pos[plane] = static_cast<float>(cy.pos);
            range.add(x, y, x0, y0, W, H);
        }
        constexpr int kU = 4;  // channels per trip: 16 independent taps in flight per lane (8: no faster)
        for (int c = cg; c < C; c += kU * kCg) {
            A v[kU][4];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int cc = min(c + u * kCg, C - 1);
                const T *q = img + cc * plane + o00;
                load_taps<PAIR, T, A>(q, oky0 && okx0, oky0 && okx1, v[u][0], v[u][1]);
                load_taps<PAIR, T, A>(q + W, oky1 && okx0, oky1 && okx1, v[u][2], v[u][3]);
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int cc = c + u * kCg;
                if (cc >= C) break;
                // absent taps contribute exact zeros
                A acc = v[u][0] * wnw;
                acc += v[u][1] * wne;
                acc += v[u][2] * wsw;
                acc += v[u][3] * wse;
                st(dst + cc * plane, acc);
            }
        }
    }
    // one wave per workgroup publishes; every slot < gridDim.x is written
    if (ctx && cg == 0) range.publish(ctx, first, lane);
}

template <typename T, typename F>
__global__ __launch_bounds__(256) void warp_fwd_staged_kernel(
    const T *__restrict__ image, const F *__restrict__ flow, T *__restrict__ out,
    void *__restrict__ ctx, int B, int C, int H, int W, int pad_mode, int crange, int nrange) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(16))) float win[kStageCap];
    __shared__ int4 boxes[4];

    constexpr int esz = sizeof(T);
    const int plane = H * W;   // the launcher guarantees C * plane * esz < 2^31
    const int tid = threadIdx.x;
    const int lane = tid & (kPix - 1), wave = __builtin_amdgcn_readfirstlane(tid / kPix);
    const Strips strips(H, W);
    const int tyn = (strips.ny + kStageRows - 1) / kStageRows;
    int id = xcd_chunk(blockIdx.x, gridDim.x);
    const int r = __builtin_amdgcn_readfirstlane(id % nrange); id /= nrange;
    const int tx = __builtin_amdgcn_readfirstlane(id % strips.nx); id /= strips.nx;
    const int ty = __builtin_amdgcn_readfirstlane(id % tyn);
    const int b = __builtin_amdgcn_readfirstlane(id / tyn);
    const int jy = ty * kStageRows + wave;
    int x = 0, y = 0;
    const bool live = jy < strips.ny && strips.pixel(jy * strips.nx + tx, lane, H, W, x, y);
    const int p = y * W + x;
    float wnw = 0.f, wne = 0.f, wsw = 0.f, wse = 0.f;
    int x0 = -2, y0 = -2;   // a lane outside the image has no in-image tap
    TapRange range;
    if (live) {
        const F *fl = flow + static_cast<int64_t>(b) * 2 * plane + p;
        const Coord<float> cx = source_coord<float>(x, static_cast<float>(ld(fl)), W, pad_mode);
        const Coord<float> cy = source_coord<float>(y, static_cast<float>(ld(fl + plane)), H, pad_mode);
        const float x0f = floorf(cx.pos), y0f = floorf(cy.pos);
        const float x1f = x0f + 1.f, y1f = y0f + 1.f;
        wnw = (x1f - cx.pos) * (y1f - cy.pos);
        wne = (cx.pos - x0f) * (y1f - cy.pos);
        wsw = (x1f - cx.pos) * (cy.pos - y0f);
        wse = (cx.pos - x0f) * (cy.pos - y0f);
        x0 = tap_index(x0f); y0 = tap_index(y0f);
        if (ctx && r == 0) {
            float *pos = ctx_pos(ctx, B, H, W) + static_cast<int64_t>(b) * 2 * plane + p;
            pos[0] = cx.pos;
            pos[plane] = cy.pos;
            range.add(x, y, x0, y0, W, H);
        }
    }
    if (ctx && r == 0 && jy < strips.ny) {
        const int xl = wave_minmax<false>(range.xlo), xh = wave_minmax<true>(range.xhi);
        const int yl = wave_minmax<false>(range.ylo), yh = wave_minmax<true>(range.yhi);
        if (lane == 0)
            static_cast<int4 *>(ctx)[b * strips.per_image() + jy * strips.nx + tx] = make_int4(xl, xh, yl, yh);
    }
    // A lane is dead when no tap of it is inside the image (its output is the same sum of
    // zero products for every channel); the others have x0 in [-1, W-1], y0 in [-1, H-1].
    const bool dead = !(x0 >= -1 && x0 <= W - 1 && y0 >= -1 && y0 <= H - 1);
    const float zsum = [&] { float a = 0.f * wnw; a += 0.f * wne; a += 0.f * wsw; a += 0.f * wse; return a; }();
    StageWindow w;
    w.reduce(dead, x0, y0, boxes, wave, lane);

    const int c_begin = r * crange, c_end = min(C, c_begin + crange);
    const T *img = image + static_cast<int64_t>(b) * C * plane;
    const __amdgpu_buffer_rsrc_t rsrc_img = uniform_rsrc(img, C * plane * esz);
    const __amdgpu_buffer_rsrc_t rsrc_out =
        uniform_rsrc(out + static_cast<int64_t>(b) * C * plane, C * plane * esz);
    const int out_voff = live ? p * esz : kDeadOffset;
    if (w.empty) {   // no tap of the tile is inside the image
        for (int c = c_begin; c < c_end; ++c) buffer_store_px<T>(rsrc_out, out_voff, c * plane * esz, zsum);
        return;
    }
    if (!w.fits()) {
        // diverged flow: direct gather, four channels in flight
        if (!live) return;
        const bool okx0 = x0 >= 0 && x0 < W, okx1 = x0 + 1 >= 0 && x0 + 1 < W;
        const bool oky0 = y0 >= 0 && y0 < H, oky1 = y0 + 1 >= 0 && y0 + 1 < H;
        const int64_t o00 = static_cast<int64_t>(y0) * W + x0;
        T *dst = out + static_cast<int64_t>(b) * C * plane + p;
        for (int c = c_begin; c < c_end; c += 4) {
            float v[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T *q = img + static_cast<int64_t>(min(c + u, c_end - 1)) * plane + o00;
                load_taps<true, T, float>(q, oky0 && okx0, oky0 && okx1, v[u][0], v[u][1]);
                load_taps<true, T, float>(q + W, oky1 && okx0, oky1 && okx1, v[u][2], v[u][3]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c + u >= c_end) break;
                float acc = v[u][0] * wnw;
                acc += v[u][1] * wne;
                acc += v[u][2] * wsw;
                acc += v[u][3] * wse;
                st(dst + static_cast<int64_t>(c + u) * plane, acc);
            }
        }
        return;
    }
    w.map_cells(tid, H, W, esz);
    const int cch = min(crange, kStageCap / w.area);
    const float *tap = win + (dead ? 0 : (y0 - w.wy0) * w.pitch + (x0 - w.wx0));
    for (int c = c_begin; c < c_end; c += cch) {
        const int n = min(cch, c_end - c);
        if (c != c_begin) __syncthreads();   // the previous group's taps have been read
        w.stage<T>(win, rsrc_img, c, n, plane);
        __syncthreads();
        for (int h = 0; h < n; ++h) {
            const float *wc = tap + h * w.area;
            const float v0 = wc[0], v1 = wc[1], v2 = wc[w.pitch], v3 = wc[w.pitch + 1];
            float acc = v0 * wnw;
            acc += v1 * wne;
            acc += v2 * wsw;
            acc += v3 * wse;
            buffer_store_px<T>(rsrc_out, out_voff, (c + h) * plane * esz, dead ? zsum : acc);
        }
    }
#endif
}

// Context from the flow alone (backward called without a forward context): same strip ->
// workgroup mapping as the forward, one wavefront per workgroup.
template <typename F>
__global__ __launch_bounds__(kPix) void warp_context_kernel(const F *__restrict__ flow,
                                                             void *__restrict__ ctx, int B, int H,
                                                             int W, int pad_mode) {
    const int64_t plane = static_cast<int64_t>(H) * W;
    const int lane = threadIdx.x;
    const Strips strips(H, W);
    const int spp = strips.per_image();
    const int64_t nstrips = static_cast<int64_t>(B) * spp;
    TapRange range;
    const int first = xcd_chunk(blockIdx.x, gridDim.x);
    for (int64_t strip = first; strip < nstrips; strip += gridDim.x) {
        const int b = static_cast<int>(strip / spp);
        int x, y;
        if (!strips.pixel(static_cast<int>(strip % spp), lane, H, W, x, y)) continue;
        const int64_t p = static_cast<int64_t>(y) * W + x;
        const F *fl = flow + static_cast<int64_t>(b) * 2 * plane + p;
        const Coord<float> cx = source_coord<float>(x, static_cast<float>(ld(fl)), W, pad_mode);
        const Coord<float> cy = source_coord<float>(y, static_cast<float>(ld(fl + plane)), H, pad_mode);
        float *pos = ctx_pos(ctx, B, H, W) + static_cast<int64_t>(b) * 2 * plane + p;
        pos[0] = cx.pos;
        pos[plane] = cy.pos;
        const Bilinear<float> t(cx.pos, cy.pos);
        range.add(x, y, t.x0(), t.y0(), W, H);
    }
    range.publish(ctx, first, lane);
}

// ---- atomics ----------------------------------------------------------------
__device__ __forceinline__ void atomic_accumulate(float *p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void atomic_accumulate(double *p, double v) { unsafeAtomicAdd(p, v); }
// 16-bit storage: CAS on the containing dword (AMP path only; not on the fp32 headline path)
template <typename H16> __device__ __forceinline__ void atomic_accumulate_16(H16 *p, float v) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    unsigned int *word = reinterpret_cast<unsigned int *>(addr & ~uintptr_t(3));
    const bool upper = addr & 2;
    unsigned int seen = *word, assumed;
    do {
        assumed = seen;
        unsigned short bits = upper ? static_cast<unsigned short>(assumed >> 16)
                                    : static_cast<unsigned short>(assumed & 0xFFFFu);
        H16 cur;
        __builtin_memcpy(&cur, &bits, 2);
        H16 next;
        st(&next, ld(&cur) + v);
        unsigned short nb;
        __builtin_memcpy(&nb, &next, 2);
        const unsigned int repl = upper ? ((assumed & 0x0000FFFFu) | (static_cast<unsigned int>(nb) << 16))
                                        : ((assumed & 0xFFFF0000u) | nb);
        seen = atomicCAS(word, assumed, repl);
    } while (seen != assumed);
}
__device__ __forceinline__ void atomic_accumulate(__half *p, float v) { atomic_accumulate_16(p, v); }
__device__ __forceinline__ void atomic_accumulate(hip_bfloat16 *p, float v) { atomic_accumulate_16(p, v); }

// ---- backward, per-pixel kernel ---------------------------------------------------
// grad_flow by a deterministic gather + grad_image by global float atomics, as ATen does.
// Used when the tiled path does not apply (fp64, or neither context nor workspace) and for
// grad_flow alone when grad_image is not wanted.
template <typename T, typename F, bool PAIR, int kCg>
__global__ __launch_bounds__(kPix * kCg) void warp_bwd_kernel(
    const T *__restrict__ image, const F *__restrict__ flow, const T *__restrict__ gout,
    T *__restrict__ gimage, F *__restrict__ gflow, int B, int C, int H, int W, int pad_mode, int interp) {
    using A = typename Acc<T>::type;
    __shared__ A part[kCg][2][kPix];
    const int64_t plane = static_cast<int64_t>(H) * W;
    const int lane = threadIdx.x & (kPix - 1);
    const int cg = threadIdx.x / kPix;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kPix + lane;
    const int b = blockIdx.y;
    const bool live = p < plane;
    A giy = 0, gix = 0;   // (y first: the compiler pairs the two sums, and this lane order costs two VGPRs fewer -- 72, not 74, in fp32)
    Coord<A> cx{0, 0}, cy{0, 0};
    if (live) {
        const int y = static_cast<int>(p / W), x = static_cast<int>(p % W);
        const F *fl = flow + static_cast<int64_t>(b) * 2 * plane + p;
        cx = source_coord<A>(x, static_cast<A>(ld(fl)), W, pad_mode);
        cy = source_coord<A>(y, static_cast<A>(ld(fl + plane)), H, pad_mode);
        const Bilinear<A> t(cx.pos, cy.pos);
        const int64_t o00 = static_cast<int64_t>(t.y0()) * W + t.x0();
        const int64_t base = static_cast<int64_t>(b) * C * plane;
        if (interp == CERB_INTERP_NEAREST) {
            // grad_image: gradOutput added to the nearbyint tap (ATen's scatter); grad_flow: zero, stored below
            const A xn = nearbyint(cx.pos), yn = nearbyint(cy.pos);
            const bool ok = xn >= A(0) && xn < static_cast<A>(W) && yn >= A(0) && yn < static_cast<A>(H);
            if (gimage && ok) {
                const int64_t q = base + static_cast<int64_t>(yn) * W + static_cast<int64_t>(xn);
                for (int c = cg; c < C; c += kCg) atomic_accumulate(gimage + q + c * plane, ld(gout + base + c * plane + p));
            }
        }
        bool nw, ne, sw, se;
        t.inside(H, W, nw, ne, sw, se);
        // kU channels per trip: all loads of a trip are issued before any is consumed
        constexpr int kU = 4;
        for (int c = cg; c < C && interp != CERB_INTERP_NEAREST; c += kU * kCg) {
            A g[kU], vnw[kU], vne[kU], vsw[kU], vse[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int cc = c + u * kCg;
                const bool on = cc < C;
                const int64_t q = base + (on ? cc : c) * plane + o00;
                g[u] = ld(tap_ptr(gout + base + (on ? cc : c) * plane + p, on));
                vnw[u] = vne[u] = vsw[u] = vse[u] = A(0);
                if (gflow) {  // kernel-uniform
                    load_taps<PAIR, T, A>(image + q, nw, ne, vnw[u], vne[u]);
                    load_taps<PAIR, T, A>(image + q + W, sw, se, vsw[u], vse[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int cc = c + u * kCg;
                if (cc >= C) break;
                if (gimage) {
                    const int64_t q = base + cc * plane + o00;
                    if (nw) atomic_accumulate(gimage + q, t.wnw() * g[u]);
                    if (ne) atomic_accumulate(gimage + q + 1, t.wne() * g[u]);
                    if (sw) atomic_accumulate(gimage + q + W, t.wsw() * g[u]);
                    if (se) atomic_accumulate(gimage + q + W + 1, t.wse() * g[u]);
                }
                if (gflow) flow_grad_terms<A>(vnw[u], vne[u], vsw[u], vse[u], t.ax(), t.bx(), t.ay(), t.by(), g[u], gix, giy);
            }
        }
    }
    if (!gflow) return;
    part[cg][0][lane] = gix;
    part[cg][1][lane] = giy;
    __syncthreads();
    if (cg == 0 && live) {
        A sx = 0, sy = 0;
#pragma unroll
        for (int k = 0; k < kCg; ++k) { sx += part[k][0][lane]; sy += part[k][1][lane]; }
        F *gf = gflow + static_cast<int64_t>(b) * 2 * plane + p;
        const bool nearest = interp == CERB_INTERP_NEAREST;   // no gradient by the position: exact zeros
        st(gf, nearest ? A(0) : flow_grad_out(cx.mult, sx, W));
        st(gf + plane, nearest ? A(0) : flow_grad_out(cy.mult, sy, H));
    }
}

// ---- few channels: the photometric loss's RGB warps (UnFlowLoss.py:282-283) --------------------------
// The loss warps a 3-channel target image by every predicted flow: 8 forward + 8 backward launches per training
// step, the full-resolution ones (4 x 3 x 512 x 1024) the largest warps of the whole step.  The image carries no
// gradient there (no context to save, no grad_image), and with C <= 4 the channel-group kernels above leave a
// quarter of every 256-thread workgroup idle (4 groups for 3 channels), meet in LDS behind a barrier to add up
// ONE value per group, and walk their channels in trips.  Here a lane owns its pixels with ALL their channels:
// every load (flow, gradOutput, 4 x NC taps per pixel) is issued before the first is used, nothing crosses lanes.
//   * a wavefront owns PX x 64 consecutive pixels of ONE image row (the row and the segment are wave-uniform: no
//     per-lane division); a lane's PX pixels lie 64 apart, so every memory instruction still has its 64 lanes on 64
//     consecutive pixels.  (Four ADJACENT pixels per lane -- 16-byte flow loads and stores -- measured slower, 48 vs
//     30 us at full resolution: a tap gather's lanes then lie 16 bytes apart and touch four times the cache lines.)
//   * every access goes through a buffer resource with 32-bit byte offsets: the channel is the scalar offset, a tap
//     outside the image (or a lane past the row's end) gets an out-of-range offset -- reads 0, drops the store -- by
//     ONE select, where 64-bit pointers cost two selects and a 64-bit add per tap.  The first version of this kernel
//     (pointers, a division per pixel) executed ~300 vector instructions per pixel and was bound by them: 30 us for
//     67 MB at full resolution, one pixel per lane or four.
// Measured at (4, 3, 512, 1024), us forward / grad_flow: 13.9 / 16.0 under a translation (67 / 84 MB: 60 / 65 % of
// the HBM roofline), 29.0 / 30.6 under the bench's synthetic "smooth" field (channel-group kernels: 43.4 with context /
// 97.9).  The difference is the gather itself, not memory, instructions or latency: that field's slope reaches 1.5
// px per px, the 64 taps of one gather instruction then spread over up to 13 image rows, and the texture path walks
// every cache line they touch (ablation, same launch: taps redirected to the lane's own pixel 13.5 / 15.5 us; no taps
// 12.6 / 14.0; no stores 27.7; one or four pixels per lane: the same).
// Taps, weights and the order of the sum from Bilinear, the terms from flow_grad_terms / flow_grad_out, as in warp_fwd_kernel
// / warp_bwd_kernel (the backward adds its per-channel terms in the four-group order of warp_bwd_kernel<.., 4>):
// bit-identical results (test).
// Work items in row-major order, XCD-contiguous (an XCD's L2 sees whole image rows and their vertical neighbours).
template <typename T, typename F, int NC, int PX, bool BWD>
__global__ __launch_bounds__(256) void warp_fewc_kernel(const T *__restrict__ image, const F *__restrict__ flow,
                                                        const T *__restrict__ gout, T *__restrict__ out,
                                                        F *__restrict__ gflow, int items, int segs, int H, int W,
                                                        int pad_mode, int interp) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int esz = sizeof(T), fsz = sizeof(F);
    const int plane = H * W;            // the launcher guarantees 4 * plane * 4 < 2^31
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kPix), lane = threadIdx.x & (kPix - 1);
    const int item = xcd_chunk(blockIdx.x, gridDim.x) * 4 + wave;       // (image, row, segment), wave-uniform
    if (item >= items) return;
    const int sg = item % segs, row = item / segs;
    const int y = row % H, b = row / H;
    const __amdgpu_buffer_rsrc_t r_img = uniform_rsrc(image + static_cast<int64_t>(b) * NC * plane, NC * plane * esz);
    const __amdgpu_buffer_rsrc_t r_flow = uniform_rsrc(flow + static_cast<int64_t>(b) * 2 * plane, 2 * plane * fsz);
    const __amdgpu_buffer_rsrc_t r_go = uniform_rsrc(BWD ? gout + static_cast<int64_t>(b) * NC * plane : image, NC * plane * esz);
    if (BWD && interp == CERB_INTERP_NEAREST) {
        // nearest: grad_flow is exactly zero (the op allocates it uninitialised)
        const __amdgpu_buffer_rsrc_t r_gf = uniform_rsrc(gflow + static_cast<int64_t>(b) * 2 * plane, 2 * plane * fsz);
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const int xz = sg * (PX * kPix) + i * kPix + lane;
            const int pz = xz < W ? y * W + xz : kDeadOffset / 4;
            buffer_store_px<F>(r_gf, pz * fsz, 0, 0.f);
            buffer_store_px<F>(r_gf, pz * fsz, plane * fsz, 0.f);
        }
        return;
    }
    float fx[PX], fy[PX], g[NC][PX];
    int pix[PX], xs[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        xs[i] = sg * (PX * kPix) + i * kPix + lane;
        pix[i] = xs[i] < W ? y * W + xs[i] : kDeadOffset / 4;      // a lane past the row's end: reads 0, stores nothing
        fx[i] = buffer_load_px1<F>(r_flow, pix[i] * fsz, 0);
        fy[i] = buffer_load_px1<F>(r_flow, pix[i] * fsz, plane * fsz);
        if constexpr (BWD) {
#pragma unroll
            for (int c = 0; c < NC; ++c) g[c][i] = buffer_load_px1<T>(r_go, pix[i] * esz, c * plane * esz);
        }
    }
    float v[PX][NC][4], ax[PX], bx[PX], ay[PX], by[PX], mx[PX], my[PX];
    Bilinear<float> t[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        const Coord<float> cx = source_coord<float>(xs[i], fx[i], W, pad_mode);
        const Coord<float> cy = source_coord<float>(y, fy[i], H, pad_mode);
        t[i] = Bilinear<float>(cx.pos, cy.pos);
        // The fractions are formed HERE, under the loads in flight, and kept: both directions use these values (the forward's
        // t[i].blend folds onto them).  Asked for after the loads instead, the backward's four pixels' fractions are packed into
        // v_pk ops with 35 more moves, and the 16-bit form loses a wave per SIMD (96 VGPRs).
        ax[i] = t[i].ax(); bx[i] = t[i].bx(); ay[i] = t[i].ay(); by[i] = t[i].by();
        mx[i] = cx.mult; my[i] = cy.mult;
        int onw, one, osw, ose;
        t[i].byte_offsets(H, W, esz, onw, one, osw, ose);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            v[i][c][0] = buffer_load_px1<T>(r_img, onw, c * plane * esz);
            v[i][c][1] = buffer_load_px1<T>(r_img, one, c * plane * esz);
            v[i][c][2] = buffer_load_px1<T>(r_img, osw, c * plane * esz);
            v[i][c][3] = buffer_load_px1<T>(r_img, ose, c * plane * esz);
        }
    }
    if constexpr (!BWD) {
        const __amdgpu_buffer_rsrc_t r_out = uniform_rsrc(out + static_cast<int64_t>(b) * NC * plane, NC * plane * esz);
#pragma unroll
        for (int i = 0; i < PX; ++i) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
                buffer_store_px<T>(r_out, pix[i] * esz, c * plane * esz, t[i].blend(v[i][c][0], v[i][c][1], v[i][c][2], v[i][c][3]));
        }
    } else {
        const __amdgpu_buffer_rsrc_t r_gf = uniform_rsrc(gflow + static_cast<int64_t>(b) * 2 * plane, 2 * plane * fsz);
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            // warp_bwd_kernel<.., 4>: channel c adds into partial c & 3, the partials are summed 0..3
            float sx = 0, sy = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float px = 0, py = 0;
                if (k < NC)
                    flow_grad_terms<float>(v[i][k][0], v[i][k][1], v[i][k][2], v[i][k][3], ax[i], bx[i], ay[i], by[i],
                                           g[k][i], px, py);
                sx += px; sy += py;
            }
            buffer_store_px<F>(r_gf, pix[i] * fsz, 0, flow_grad_out(mx[i], sx, W));
            buffer_store_px<F>(r_gf, pix[i] * fsz, plane * fsz, flow_grad_out(my[i], sy, H));
        }
    }
#endif
}

// ---- backward, owner-computes tiles ------------------------------------------------
// ATen's image gradient is a global float-atomic scatter: 4 atomics per (pixel, channel),
// ~0.1 TB/s when neighbouring lanes hit different rows (measured: 555 us at the 32x128x256
// level).  Here ONE launch holds two kinds of workgroup:
//
//  * TILE workgroups own a TH x 64 tile of grad_image for a range of channels.  They find the
//    source pixels whose taps can reach the tile from the context -- the strips whose signed
//    tap-displacement range reaches it, clipped to (tile shifted by those ranges) --, keep
//    each source's tile offset and four bilinear weights in REGISTERS, and then walk their
//    channels in groups of CW: load gradOutput at the sources (the next group's loads are in
//    flight while this group accumulates), add the taps into LDS, write the group's tile with
//    plain coalesced stores.  No global atomics, no memset, every output element written
//    exactly once.  (Round 1 gave every 4-channel group its own workgroup: 8 workgroups per
//    tile at 32 channels, each re-reading the positions, re-classifying the region and
//    walking load -> reduce -> add -> store in lock-step with everyone else.)
//  * FLOW workgroups (64 pixels x 4 channel groups, like the forward) finish grad_flow: a
//    gather over the pixel's own taps, independent of the tiles, so the two kinds overlap.
//
// The LDS accumulators are FIXED POINT: ds_add_f32 runs at 0.3 lanes/clk/CU on gfx950
// (tools/ubench/lds_atomic.hip) against 6.7 for the integer adds.  Two channels share one
// 64-bit slot as two int32 sums: one ds_add_u64 adds (a + (b << 32)) -- half the LDS atomics
// of one-slot-per-channel, and the LDS-atomic pipe is what bounds this kernel (round 2 PMC:
// 8.8 us of LDS-busy time per CU at the 32x128x256 level with one channel per slot).  A
// negative a borrows from the upper half; the borrows add up consistently, so the sums come
// back exactly: A = int32(low word), B = (V - A) >> 32.
// Scale: 2^(30 - e - S) with max|gradOutput| < 2^e over the sources of this (tile, channel
// group) (a block reduction) and 2^S >= the tile's largest tap DENSITY (the sum of bilinear
// weights landing on one element, measured once per tile with the same adds on a weight
// plane; ~1 under smooth flows, so S = 1): every |sum| < 2^31, with a resolution of 2^-29 of
// the tile's largest gradient (fp32 itself resolves 2^-24).  Integer addition commutes, so
// the result is bit-reproducible (ATen's is not).
// A plane of accumulators is the tile plus a one-pixel ring: a source is taken iff its
// north-west tap lies in [-1, TW-1] x [-1, TH-1] of the tile, all four taps then address the
// padded plane without any per-tap test, and what lands in the ring (taps that belong to a
// neighbouring tile or fall outside the image) is simply never written out.
// Non-finite gradients: the block maximum is taken on the bit patterns (NaN > Inf > finite),
// so one NaN / Inf among the sources is seen; that (tile, group) then accumulates in float
// (ds_add_f32 on the two halves of the slot: slow, but only diverged steps get here) and
// NaN / Inf reach exactly the elements they reach in ATen's scatter.

// ---- backward, grad_flow with an LDS-staged source window --------------------------------
// The FLOW role of warp_bwd_tile_kernel as an 8 x 32 pixel tile (4 strips, one per wave) over
// ALL channels: the tile's source window is copied into LDS a few channels at a time
// (StageWindow) and the four taps of a channel come from LDS; gradOutput at the lane's own
// pixel is a coalesced buffer load whose channel is the scalar offset.  Channel c adds into
// partial c & 3 in ascending order and the partials are summed 0..3 -- the order of the
// four-wave strip role below, so the two produce identical bits.
// Used when the map has >= 512 such tiles.  (Measured, 4 pairs, whole backward, us strip role
// / this: 32x128x256 27.7 / 25.9, 64x128x256 46.3 / 42.9, 32x256x512 87.7 / 71.9, fp16 80.0 /
// 65.3.  Splitting the channels of a smaller tile over the waves -- 2 x 32 or 4 x 32 pixels,
// for the deep levels with few pixels and many channels -- measured SLOWER than the strip
// role at every level (12.4 -> 25.4 us at 128x32x64): the window halo and the two barriers
// per pass outweigh the gathers they replace.)
// Returns false (nothing written) when a group of four channels' windows does not fit.
template <typename T, typename F>
__device__ __forceinline__ bool flow_role_staged(
    float *__restrict__ win, int cap, int4 *__restrict__ boxes, const T *__restrict__ image,
    const T *__restrict__ gout, const void *__restrict__ ctx, const F *__restrict__ flow, F *__restrict__ gflow,
    int flow_block, int nflow_blocks, int B, int C, int H, int W, int pad_mode) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int esz = sizeof(T);
    constexpr int SR = kStageRows, NPL = 4;   // strips per workgroup, partial sums per lane
    const int plane = H * W;
    const int tid = threadIdx.x;
    const int lane = tid & (kPix - 1), wave = __builtin_amdgcn_readfirstlane(tid / kPix);
    const Strips strips(H, W);
    const int tyn = (strips.ny + SR - 1) / SR;
    int id = xcd_chunk(flow_block, nflow_blocks);
    const int tx = __builtin_amdgcn_readfirstlane(id % strips.nx); id /= strips.nx;
    const int ty = __builtin_amdgcn_readfirstlane(id % tyn);
    const int b = __builtin_amdgcn_readfirstlane(id / tyn);
    const int jy = ty * SR + wave;
    int x = 0, y = 0;
    const bool live = jy < strips.ny && strips.pixel(jy * strips.nx + tx, lane, H, W, x, y);
    const int p = y * W + x;
    const int pc = live ? p : 0;
    const float *pos = ctx_pos(ctx, B, H, W) + static_cast<int64_t>(b) * 2 * plane;
    const float ixp = pos[pc], iyp = pos[plane + pc];
    const float x0f = floorf(ixp), y0f = floorf(iyp);
    const float x1f = x0f + 1.f, y1f = y0f + 1.f;
    const int x0 = live ? tap_index(x0f) : -2, y0 = live ? tap_index(y0f) : -2;
    const bool dead = !(x0 >= -1 && x0 <= W - 1 && y0 >= -1 && y0 <= H - 1);
    StageWindow w;
    w.reduce(dead, x0, y0, boxes, wave, lane);
    if (!w.fits() || w.area * 4 > cap) return false;   // uniform: a diverged flow
    w.map_cells(tid, H, W, esz);
    const int cch = (cap / w.area) & ~3;   // whole groups of four partials per pass

    const __amdgpu_buffer_rsrc_t rsrc_img =
        uniform_rsrc(image + static_cast<int64_t>(b) * C * plane, C * plane * esz);
    const __amdgpu_buffer_rsrc_t rsrc_go =
        uniform_rsrc(gout + static_cast<int64_t>(b) * C * plane, C * plane * esz);
    const int go_voff = live ? p * esz : kDeadOffset;
    const float *tap = win + (dead ? 0 : (y0 - w.wy0) * w.pitch + (x0 - w.wx0));
    float gix[NPL], giy[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) gix[k] = giy[k] = 0.f;
    for (int c = 0; c < C; c += cch) {
        const int n = min(cch, C - c);
        if (c != 0) __syncthreads();   // the previous group's taps have been read
        w.stage<T>(win, rsrc_img, c, n, plane);
        __syncthreads();
        for (int h0 = 0; h0 < n; h0 += 8) {   // c and h0 are multiples of 4: channel c + h0 + u is partial u & 3
            float g[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                g[u] = buffer_load_px1<T>(rsrc_go, h0 + u < n ? go_voff : kDeadOffset,
                                          (c + min(h0 + u, n - 1)) * plane * esz);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int h = h0 + u;
                if (h >= n) break;   // uniform
                const float *wc = tap + h * w.area;
                const float vnw = dead ? 0.f : wc[0], vne = dead ? 0.f : wc[1];
                const float vsw = dead ? 0.f : wc[w.pitch], vse = dead ? 0.f : wc[w.pitch + 1];
                flow_grad_terms<float>(vnw, vne, vsw, vse, x1f - ixp, ixp - x0f, y1f - iyp, iyp - y0f, g[u],
                                       gix[u % NPL], giy[u % NPL]);
            }
        }
    }
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { sx += gix[k]; sy += giy[k]; }
    if (live) {
        const F *fl = flow + static_cast<int64_t>(b) * 2 * plane + p;
        const float mx = ctx_grad_mult(ixp, x, fl, W, pad_mode), my = ctx_grad_mult(iyp, y, fl + plane, H, pad_mode);
        F *gf = gflow + static_cast<int64_t>(b) * 2 * plane + p;
        st(gf, mx * sx / static_cast<float>(W - 1) * 2.0f);
        st(gf + plane, my * sy / static_cast<float>(H - 1) * 2.0f);
    }
    return true;
#else
    return false;
#endif
}

// One pixel's grad_flow by direct gathers (the window of a diverged flow does not fit LDS): the lane walks all
// channels, eight in flight; channel c adds into partial c & 3, the partials are summed 0..3 (the order of every role).
template <typename T, typename F>
__device__ __forceinline__ void flow_pixel_direct(
    const T *__restrict__ image, const T *__restrict__ gout, const void *__restrict__ ctx, const F *__restrict__ flow,
    F *__restrict__ gflow, int b, int p, int B, int C, int H, int W, int pad_mode) {
    const int plane = H * W;
    const float *pos = ctx_pos(ctx, B, H, W) + static_cast<int64_t>(b) * 2 * plane;
    const float ixp = pos[p], iyp = pos[plane + p];
    const float x0f = floorf(ixp), y0f = floorf(iyp);
    const float x1f = x0f + 1.f, y1f = y0f + 1.f;
    const int x0 = tap_index(x0f), y0 = tap_index(y0f);
    const bool okx0 = x0 >= 0 && x0 < W, okx1 = x0 + 1 >= 0 && x0 + 1 < W;
    const bool oky0 = y0 >= 0 && y0 < H, oky1 = y0 + 1 >= 0 && y0 + 1 < H;
    const int o00 = y0 * W + x0;
    const T *im = image + static_cast<int64_t>(b) * C * plane;
    const T *gob = gout + static_cast<int64_t>(b) * C * plane;
    float gix[4] = {0.f, 0.f, 0.f, 0.f}, giy[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; c += 8) {
        float g[8], vnw[8], vne[8], vsw[8], vse[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t cp = static_cast<int64_t>(min(c + u, C - 1)) * plane;
            g[u] = ld(gob + cp + p);
            load_taps<false, T, float>(im + cp + o00, oky0 && okx0, oky0 && okx1, vnw[u], vne[u]);
            load_taps<false, T, float>(im + cp + o00 + W, oky1 && okx0, oky1 && okx1, vsw[u], vse[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (c + u >= C) break;
            flow_grad_terms<float>(vnw[u], vne[u], vsw[u], vse[u], x1f - ixp, ixp - x0f, y1f - iyp, iyp - y0f, g[u],
                                   gix[u & 3], giy[u & 3]);
        }
    }
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { sx += gix[k]; sy += giy[k]; }
    const F *fl = flow + static_cast<int64_t>(b) * 2 * plane + p;
    const float mx = ctx_grad_mult(ixp, p % W, fl, W, pad_mode), my = ctx_grad_mult(iyp, p / W, fl + plane, H, pad_mode);
    F *gf = gflow + static_cast<int64_t>(b) * 2 * plane + p;
    st(gf, mx * sx / static_cast<float>(W - 1) * 2.0f);
    st(gf + plane, my * sy / static_cast<float>(H - 1) * 2.0f);
}

// The 8 x 32 tile of flow_role_staged by direct gathers: one wave per strip
template <typename T, typename F>
__device__ __forceinline__ void flow_role_tile_direct(
    const T *__restrict__ image, const T *__restrict__ gout, const void *__restrict__ ctx, const F *__restrict__ flow,
    F *__restrict__ gflow, int flow_block, int nflow_blocks, int B, int C, int H, int W, int pad_mode) {
    const int lane = threadIdx.x & (kPix - 1), wave = threadIdx.x / kPix;
    constexpr int SR = kStageRows;
    const Strips strips(H, W);
    const int tyn = (strips.ny + SR - 1) / SR;
    int id = xcd_chunk(flow_block, nflow_blocks);
    const int tx = id % strips.nx; id /= strips.nx;
    const int ty = id % tyn;
    const int b = id / tyn;
    const int jy = ty * SR + wave;
    int x = 0, y = 0;
    if (!(jy < strips.ny && strips.pixel(jy * strips.nx + tx, lane, H, W, x, y))) return;
    flow_pixel_direct<T, F>(image, gout, ctx, flow, gflow, b, y * W + x, B, C, H, W, pad_mode);
}

// The 8 x 64 tile of flow_role16 (16-bit storage) by direct gathers: a lane's two pixels one after the other
template <typename T, typename F>
__device__ __forceinline__ void flow_role16_direct(
    const T *__restrict__ image, const T *__restrict__ gout, const void *__restrict__ ctx, const F *__restrict__ flow,
    F *__restrict__ gflow, int flow_block, int nflow_blocks, int B, int C, int H, int W, int pad_mode) {
    const int lane = threadIdx.x & (kPix - 1), wave = threadIdx.x / kPix;
    const int ntx = (W + kTile16W - 1) / kTile16W, nty = (H + kTile16H - 1) / kTile16H;
    int id = xcd_chunk(flow_block, nflow_blocks);
    const int tx = id % ntx; id /= ntx;
    const int ty = id % nty;
    const int b = id / nty;
    const int y = ty * kTile16H + wave * 2 + (lane >> 5), xa = tx * kTile16W + 2 * (lane & 31);
    if (!(y < H && xa < W)) return;
    flow_pixel_direct<T, F>(image, gout, ctx, flow, gflow, b, y * W + xa, B, C, H, W, pad_mode);
    if (xa + 1 < W) flow_pixel_direct<T, F>(image, gout, ctx, flow, gflow, b, y * W + xa + 1, B, C, H, W, pad_mode);
}

#ifdef CERB_STAMP
// diagnostic build only (-DCERB_STAMP): s_memtime at the phase boundaries of the first 64 tile
// workgroups, fetched with cerberus_debug_stamps(); never compiled into the product
__device__ unsigned long long g_stamps[64][16];
#define CERB_STAMP_AT(k)                                                         \
    do {                                                                         \
        if (threadIdx.x == 0 && blockIdx.x < 64) g_stamps[blockIdx.x][k] = __builtin_readcyclecounter(); \
    } while (0)
#else
#define CERB_STAMP_AT(k) do {} while (0)
#endif

constexpr int kTileW = 64;
#ifndef CERB_TILE_PAD
#define CERB_TILE_PAD 2     // >= 2 (the one-pixel ring); more = row padding against LDS bank conflicts (tools/lds_conflicts_warp.py)
#endif
template <int TH> struct TileGeom {
    static constexpr int PW = kTileW + CERB_TILE_PAD;          // padded row, in accumulators
    static constexpr int PS = (TH + 2) * PW;       // accumulators per channel plane
};

#ifndef CERB_TILE16_WPS
#define CERB_TILE16_WPS 4
#endif
// REFL: the reflection pad's instantiation -- its flow roles recompute the multiplier's sign from the flow; kept out of the
// border / zeros kernels, where that code costs the 16-bit forms (at their 128 VGPRs) two more spilled registers
template <typename T, typename F, int TH, int CW, int NS, int PR = 0, bool REFL = false>
__global__ __launch_bounds__(256, TH == 16 ? CERB_TILE16_WPS : 4) void warp_bwd_tile_kernel(
    const T *__restrict__ image, const T *__restrict__ gout, const void *__restrict__ ctx, const F *__restrict__ flow,
    T *__restrict__ gimage, F *__restrict__ gflow, int B, int C, int H, int W,
    int tiles_x, int tiles_y, int nrange, int crange, int ntile_blocks, int pad_arg, int interp,
    int flow_staged, int flow_sub, int stagger) {
    // (a pad mode the compiler can see is not reflection unless REFL)
    const int pad_mode = REFL ? CERB_PAD_REFLECTION : pad_arg == CERB_PAD_BORDER ? CERB_PAD_BORDER : CERB_PAD_ZEROS;
    constexpr int TW = kTileW, PW = TileGeom<TH>::PW, PS = TileGeom<TH>::PS;
    constexpr int NP = CW / 2;                       // channel pairs = planes of 64-bit slots
    static_assert(CW % 2 == 0, "channels are accumulated in pairs");
    __shared__ __attribute__((aligned(16))) long long acc[NP * PS];
    __shared__ __attribute__((aligned(16))) int red[4][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int plane = H * W;

    if (stagger > 0) {   // phase shift of the co-resident workgroups of a CU (blocks i, i + 256, i + 512, i + 768): launch_tiles
        const int q = (blockIdx.x >> 8) & 3;
        const unsigned long long wait = q == 0 ? 0ull : static_cast<unsigned long long>((stagger >> (8 * (q - 1))) & 255) * 1024ull;
        const unsigned long long t0 = __builtin_readcyclecounter();
        while (__builtin_readcyclecounter() - t0 < wait) __builtin_amdgcn_s_sleep(16);
    }
    if (static_cast<int>(blockIdx.x) >= ntile_blocks) {
        // ------------------------------ FLOW workgroup ------------------------------
        if constexpr (sizeof(T) == 2) {
            if (flow_staged == 2) {
                // 16-bit storage: an 8 x 64 tile, two pixels per lane, the raw 16-bit window by LDS-DMA (warp16_common.h)
                const int fb = blockIdx.x - ntile_blocks, nfb = gridDim.x - ntile_blocks;
                if (!flow_role16<T, F>(reinterpret_cast<char *>(acc), NP * PS * 8, reinterpret_cast<int4 *>(&red[0][0]), image,
                                       gout, ctx, flow, gflow, fb, nfb, B, C, H, W, pad_mode))
                    flow_role16_direct<T, F>(image, gout, ctx, flow, gflow, fb, nfb, B, C, H, W, pad_mode);
                return;
            }
        }
        if (flow_staged) {
            // an 8 x 32 tile x all channels through an LDS window (the accumulators' LDS)
            const int fb = blockIdx.x - ntile_blocks, nfb = gridDim.x - ntile_blocks;
            if (!flow_role_staged<T, F>(reinterpret_cast<float *>(acc), NP * PS * 2,
                                        reinterpret_cast<int4 *>(&red[0][0]), image, gout, ctx, flow, gflow,
                                        fb, nfb, B, C, H, W, pad_mode))
                flow_role_tile_direct<T, F>(image, gout, ctx, flow, gflow, fb, nfb, B, C, H, W, pad_mode);
            return;
        }
        // one strip of 64 pixels x 4 channel groups (one wave each); positions from the context.
        // flow_sub = 2 / 4 (deep levels: few pixels, many channels): the workgroup takes a half / a quarter
        // of the strip and its lanes 2 / 4 channel subgroups each, so that the channel loop -- a chain of
        // dependent round trips to HBM when the image is cold, as it is inside a training step -- is 2 / 4
        // times shorter (4 pairs of 128 x 32 x 64, image cold: 20.6 -> 12.6 us; one trip instead of four)
        float(*part)[2][kPix] = reinterpret_cast<float(*)[2][kPix]>(acc);
        const Strips strips(H, W);
        const int spp = strips.per_image();
        const int fbid = xcd_chunk(blockIdx.x - ntile_blocks, gridDim.x - ntile_blocks);
        const int strip = fbid / flow_sub;
        const int npx = kPix / flow_sub;                       // pixels of the strip this workgroup owns
        const int slane = (fbid % flow_sub) * npx + lane % npx;  // the lane's pixel inside the strip
        const int cg0 = wave * flow_sub + lane / npx;          // the lane's channel group
        const int ncg = 4 * flow_sub;
        const int b = strip / spp;
        int x, y;
        const bool live = strips.pixel(strip % spp, slane, H, W, x, y);
        const int p = y * W + x;
        if (interp == CERB_INTERP_NEAREST) {
            // nearest: no gradient by the position -- exact zeros (the launcher gives nearest this role with flow_sub = 1)
            if (wave == 0 && live) {
                F *gf = gflow + static_cast<int64_t>(b) * 2 * plane + p;
                st(gf, 0.f);
                st(gf + plane, 0.f);
            }
            return;
        }
        const int pc = live ? p : 0;
        const float *pos = ctx_pos(ctx, B, H, W) + static_cast<int64_t>(b) * 2 * plane;
        const float ixp = pos[pc], iyp = pos[plane + pc];
        const float x0f = floorf(ixp), y0f = floorf(iyp);
        const float x1f = x0f + 1.f, y1f = y0f + 1.f;
        const int x0 = tap_index(x0f), y0 = tap_index(y0f);
        const bool okx0 = x0 >= 0 && x0 < W, okx1 = x0 + 1 >= 0 && x0 + 1 < W;
        const bool oky0 = y0 >= 0 && y0 < H, oky1 = y0 + 1 >= 0 && y0 + 1 < H;
        const int o00 = y0 * W + x0;
        const T *im = image + static_cast<int64_t>(b) * C * plane;
        const T *gob = gout + static_cast<int64_t>(b) * C * plane;
        float gix = 0.f, giy = 0.f;
        constexpr int kU = 8;  // channels per trip: 40 independent loads in flight per lane
        for (int c = cg0; c < C; c += kU * ncg) {
            float g[kU], vnw[kU], vne[kU], vsw[kU], vse[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int cc = c + u * ncg;
                const bool on = cc < C;
                const int64_t cp = static_cast<int64_t>(on ? cc : c) * plane;
                g[u] = ld(tap_ptr(gob + cp + pc, on));
                const T *qd = im + cp + o00;
                // (unpaired: pairing the taps here measured no gain for fp32 and a loss for fp16)
                load_taps<false, T, float>(qd, oky0 && okx0, oky0 && okx1, vnw[u], vne[u]);
                load_taps<false, T, float>(qd + W, oky1 && okx0, oky1 && okx1, vsw[u], vse[u]);
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                if (c + u * ncg >= C) continue;   // no 0 * Inf from a repeated channel
                flow_grad_terms<float>(vnw[u], vne[u], vsw[u], vse[u], x1f - ixp, ixp - x0f, y1f - iyp, iyp - y0f, g[u],
                                       gix, giy);
            }
        }
        part[wave][0][lane] = gix;
        part[wave][1][lane] = giy;
        __syncthreads();
        if (wave == 0 && live && lane < npx) {
            float sx = 0.f, sy = 0.f;
            for (int q = 0; q < flow_sub; ++q)
#pragma unroll
                for (int k = 0; k < 4; ++k) { sx += part[k][0][q * npx + lane]; sy += part[k][1][q * npx + lane]; }
            // the pad mode's multiplier, then autograd's order:
            // grad_grid = mult * sum ; through norm_grid: / (size-1) then * 2.0
            const F *fl = flow + static_cast<int64_t>(b) * 2 * plane + p;
            const float mx = ctx_grad_mult(ixp, x, fl, W, pad_mode), my = ctx_grad_mult(iyp, y, fl + plane, H, pad_mode);
            F *gf = gflow + static_cast<int64_t>(b) * 2 * plane + p;
            st(gf, mx * sx / static_cast<float>(W - 1) * 2.0f);
            st(gf + plane, my * sy / static_cast<float>(H - 1) * 2.0f);
        }
        return;
    }

    // -------------------------------- TILE workgroup --------------------------------

    // (image, tile row, tile column, channel range) with the RANGE fastest: an XCD's contiguous share is then a
    // spatial region of one image with all its channel ranges -- the same region its share of the FLOW
    // workgroups covers (also image-major, row-major), so that gradOutput, which both roles read, goes over
    // the fabric once and is found in the XCD's L2 the second time (round 3: range-major tiles, the two
    // roles of a region on different XCDs: 26.2 -> 24.0 us at level 3, profiles/r04_warp_lists_experiment.txt)
    int bid = xcd_chunk(blockIdx.x, ntile_blocks);
    const int range = bid % nrange; bid /= nrange;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y; bid /= tiles_y;
    const int b = bid;
    const int tx0 = tx * TW, ty0 = ty * TH;
    const int tx1 = min(tx0 + TW, W) - 1, ty1 = min(ty0 + TH, H) - 1;   // last pixel of the tile
    const int c_begin = range * crange, c_end = min(C, c_begin + crange);
    const float *pos = ctx_pos(ctx, B, H, W) + static_cast<int64_t>(b) * 2 * plane;

    CERB_STAMP_AT(0);
    // ---- scan region ----
    // The context holds one signed tap-displacement range per 64-pixel strip.  A strip
    // matters to this tile only if its pixels displaced by its OWN range can reach the tile;
    // the region is the bounding box of those strips clipped to the tile displaced by the
    // union of their ranges.  A fast object therefore widens only the tiles it feeds: there
    // is no global limit and no fallback.
    int rx0 = kExtEmptyLo, rx1 = kExtEmptyHi, ry0 = kExtEmptyLo, ry1 = kExtEmptyHi;
    int dxl = kExtEmptyLo, dxh = kExtEmptyHi, dyl = kExtEmptyLo, dyh = kExtEmptyHi;
    {
        const int4 *ext = static_cast<const int4 *>(ctx);
        const Strips strips(H, W);
        const int spp = strips.per_image();
        // strip j = tid + 256 k as (jy, jx), advanced without divisions in the loop
        int jy = tid / strips.nx, jx = tid % strips.nx;
        const int qy = 256 / strips.nx, qx = 256 % strips.nx;
        // four strips per trip, their ranges requested together (round 5: one load per trip -- at 256 x 512 pixels the
        // eight dependent round trips to L2 were 11 % of a tile workgroup's time, profiles/r06_warp_bwd_tile_stamps_baseline.txt)
        constexpr int SU = 4;
        for (int j = tid; j < spp; j += 256 * SU) {
            int4 e[SU];
#pragma unroll
            for (int u = 0; u < SU; ++u) e[u] = ext[b * spp + min(j + 256 * u, spp - 1)];
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int sy0 = jy * kStripH, sy1 = min(sy0 + kStripH, H) - 1;
                const int sx0 = jx * kStripW, sx1 = min(sx0 + kStripW, W) - 1;
                const bool hit = j + 256 * u < spp && e[u].x <= e[u].y && sx0 + e[u].x <= tx1 && sx1 + e[u].y >= tx0 &&
                                 sy0 + e[u].z <= ty1 && sy1 + e[u].w >= ty0;
                if (hit) {
                    rx0 = min(rx0, sx0); rx1 = max(rx1, sx1);
                    ry0 = min(ry0, sy0); ry1 = max(ry1, sy1);
                    dxl = min(dxl, e[u].x); dxh = max(dxh, e[u].y);
                    dyl = min(dyl, e[u].z); dyh = max(dyh, e[u].w);
                }
                jx += qx; jy += qy;
                if (jx >= strips.nx) { jx -= strips.nx; ++jy; }
            }
        }
    }
    // wave-wide folds on the DPP path (6 VALU each, result uniform); round 3 folded these eight values with
    // 48 __shfl_xor = 48 ds_bpermute_b32 through the LDS crossbar the accumulators' atomics also use
    rx0 = wave_minmax<false>(rx0); rx1 = wave_minmax<true>(rx1);
    ry0 = wave_minmax<false>(ry0); ry1 = wave_minmax<true>(ry1);
    dxl = wave_minmax<false>(dxl); dxh = wave_minmax<true>(dxh);
    dyl = wave_minmax<false>(dyl); dyh = wave_minmax<true>(dyh);
    // (folding the boxes with LDS min/max atomics instead of shuffles: 64 lanes on 8 addresses
    // serialise -- 19k instead of 5k cycles for this phase, measured)
    if (lane == 0) {
        red[wave][0] = rx0; red[wave][1] = rx1; red[wave][2] = ry0; red[wave][3] = ry1;
        red[wave][4] = dxl; red[wave][5] = dxh; red[wave][6] = dyl; red[wave][7] = dyh;
    }
    __syncthreads();
    rx0 = min(min(red[0][0], red[1][0]), min(red[2][0], red[3][0]));
    rx1 = max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1]));
    ry0 = min(min(red[0][2], red[1][2]), min(red[2][2], red[3][2]));
    ry1 = max(max(red[0][3], red[1][3]), max(red[2][3], red[3][3]));
    dxl = min(min(red[0][4], red[1][4]), min(red[2][4], red[3][4]));
    dxh = max(max(red[0][5], red[1][5]), max(red[2][5], red[3][5]));
    dyl = min(min(red[0][6], red[1][6]), min(red[2][6], red[3][6]));
    dyh = max(max(red[0][7], red[1][7]), max(red[2][7], red[3][7]));
    // 16-bit storage (round 6): sources are handled as horizontally adjacent PAIRS -- one dword of gradOutput per pair and
    // channel instead of two halfword loads (a wave-level load costs the address path ~9 cycles whether its lanes fetch 2
    // or 4 bytes: 23 % of a channel group's time at the 256 x 512 level was the ISSUE of these loads,
    // profiles/r06_warp_bwd_tile_stamps_baseline.txt) -- so the region starts at an even column and has an even width
    // (PR: a template parameter, chosen by the launcher -- with both forms in one kernel the 16-row variant spilled 76 VGPRs)
    constexpr bool kPair16 = PR != 0 && sizeof(T) == 2 && NS % 2 == 0;
    constexpr bool pairs = kPair16;
    int n = 0, xs = 0, ys = 0, rw = 1, rh = 0;
    if (rx0 <= rx1) {   // at least one strip reaches the tile (ranges are small ints here)
        xs = max(rx0, tx0 - dxh);
        ys = max(ry0, ty0 - dyh);
        int x_end = min(rx1, tx1 - dxl) + 1;       // one past the region's last column
        if (pairs) { xs &= ~1; x_end = (x_end + 1) & ~1; }   // (W is even: the last pair ends inside the row)
        rw = max(x_end - xs, 0);
        rh = max(min(ry1, ty1 - dyl) + 1 - ys, 0);
        n = rw * rh;
        rw = max(rw, 1);
    }
    __syncthreads();    // red[] is reused below
    CERB_STAMP_AT(1);

    T *dst = gimage + static_cast<int64_t>(b) * C * plane;
    [[maybe_unused]] const T *go = gout + static_cast<int64_t>(b) * C * plane;   // (host pass: only the device code reads it)
    unsigned long long *acc64 = reinterpret_cast<unsigned long long *>(acc);

    // One source = one pixel whose taps touch the tile: its pixel index, its offset in the
    // padded plane and the two tap fractions.  The four weights are rebuilt from the fractions
    // with the forward's roundings: ix - x0f is exact, and (x0f + 1) - ix is the correctly
    // rounded 1 - (ix - x0f) either way.
    struct Src { int pv, o; float fx, fy; };
    // region pixel (row ry, column rx of the region; `on` = inside it)
    auto classify = [&](bool on, int ry, int rx, Src &s) -> bool {
        s.pv = on ? (ys + ry) * W + xs + rx : 0;
        const float ixj = pos[s.pv], iyj = pos[plane + s.pv];
        const float x0f = floorf(ixj), y0f = floorf(iyj);
        const int lx = tap_index(x0f) - tx0 + 1, ly = tap_index(y0f) - ty0 + 1;
        const bool in = on && lx >= 0 && lx <= TW && ly >= 0 && ly <= TH;
        s.o = in ? ly * PW + lx : -1;
        s.fx = tap_fraction(ixj, x0f, interp);
        s.fy = tap_fraction(iyj, y0f, interp);
        return in;
    };
    // walks idx = tid + 256 k over the region as (row, column) without divisions
    struct Walk {
        int ry, rx, qy, qx, rw;
        __device__ Walk(int tid, int rw_) : ry(tid / rw_), rx(tid % rw_), qy(256 / rw_), qx(256 % rw_), rw(rw_) {}
        __device__ __forceinline__ void next() { rx += qx; ry += qy; if (rx >= rw) { rx -= rw; ++ry; } }
    };
    // gradOutput of CW channels at one source (channels past the range re-read the last one)
    // Through a buffer resource: the channel is a SCALAR offset and the source pixel one 32-bit VGPR offset (round 3: a
    // 64-bit address per load -- v_lshl_add_u64 on a VGPR pair each, 48 of them in flight per thread; the last two loaded
    // values were spilled behind an s_waitcnt vmcnt(0), which serialised the batch).  The launcher guarantees
    // C * plane * sizeof(T) < 2^31.
#if defined(__HIP_DEVICE_COMPILE__)
    const __amdgpu_buffer_rsrc_t rsrc_go = uniform_rsrc(go, C * plane * static_cast<int>(sizeof(T)));
#endif
    auto load_g = [&](const Src &s, int c0, float (&g)[CW]) {
#if defined(__HIP_DEVICE_COMPILE__)
        const int voff = s.pv * static_cast<int>(sizeof(T));
#pragma unroll
        for (int c = 0; c < CW; ++c)
            g[c] = buffer_load_px1<T>(rsrc_go, voff, __builtin_amdgcn_readfirstlane(min(c0 + c, c_end - 1) * plane * static_cast<int>(sizeof(T))));
#endif
    };
    auto absmax_bits = [&](const Src &, const float (&g)[CW], int gb) {
        // integer order of |g| bit patterns: NaN > Inf > every finite value.  Unmasked: every slot of the register
        // path holds a live source or a repeat of one (see the deal); round 3 masked per value (3 VALU instead of 2)
#pragma unroll
        for (int c = 0; c < CW; ++c)
            gb = max(gb, __float_as_int(g[c]) & 0x7fffffff);
        return gb;
    };
    auto absmax_bits_masked = [&](const Src &s, const float (&g)[CW], int gb) {   // the region-walking path: non-members masked
#pragma unroll
        for (int c = 0; c < CW; ++c)
            gb = max(gb, s.o >= 0 ? (__float_as_int(g[c]) & 0x7fffffff) : 0);
        return gb;
    };
    // block maximum of two non-negative ints at once
    auto block_max2 = [&](int &u, int &v) {
        u = wave_minmax<true>(u);
        v = wave_minmax<true>(v);
        if (lane == 0) { red[wave][0] = u; red[wave][1] = v; }
        __syncthreads();
        u = max(max(red[0][0], red[1][0]), max(red[2][0], red[3][0]));
        v = max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1]));
        __syncthreads();   // red[] free again
    };
    auto block_max = [&](int v) { int u = 0; block_max2(u, v); return v; };
    // tap density: the same four adds with the weights alone (16.16 fixed point) on a 32-bit
    // view of the first plane
    auto add_density = [&](const Src &s) {
        if (s.o < 0) return;
        const float ax = 1.0f - s.fx, ay = 1.0f - s.fy;
        unsigned *d = reinterpret_cast<unsigned *>(acc) + s.o;
        atomicAdd(d, static_cast<unsigned>(__float2int_rn(ax * ay * 65536.f)));
        atomicAdd(d + 1, static_cast<unsigned>(__float2int_rn(s.fx * ay * 65536.f)));
        atomicAdd(d + PW, static_cast<unsigned>(__float2int_rn(ax * s.fy * 65536.f)));
        atomicAdd(d + PW + 1, static_cast<unsigned>(__float2int_rn(s.fx * s.fy * 65536.f)));
    };
    // largest density of the tile (ring included: conservative) -> headroom bits; leaves the
    // plane zeroed.  `nsrc` bounds the rounding of the 16.16 weights.  The block reduction also
    // carries the first group's gradient maximum `gb`.
    auto density_bits = [&](int nsrc, int &gb) {
        __syncthreads();
        unsigned *d = reinterpret_cast<unsigned *>(acc);
        unsigned m = 0;
        for (int i = tid; i < PS; i += 256) { m = max(m, d[i]); d[i] = 0; }
        int mi = static_cast<int>(min(m, 0x3fffffffu));
        block_max2(mi, gb);
        const unsigned dmax = static_cast<unsigned>(mi) + static_cast<unsigned>(nsrc);
        // 2^S >= dmax / 65536
        return max(0, 32 - __clz(static_cast<int>(dmax)) - 16);
    };
    // block maximum -> fixed-point scale (or "non-finite": accumulate in float)
    auto block_scale = [&](int gb, bool reduced, int sbits, float &scale, float &unscale,
                           bool &nonfinite) {
        if (!reduced) gb = block_max(gb);   // its barriers also order: accumulators zeroed, write-out done
        nonfinite = gb >= 0x7f800000;
        int gexp = 0;
        frexpf(__int_as_float(gb), &gexp);            // gmax < 2^gexp
        gexp = max(gexp, -90) + sbits;                // keep the scale finite for denormal maxima
        scale = ldexpf(1.0f, 30 - gexp);
        unscale = ldexpf(1.0f, gexp - 30);
    };
    auto add_taps = [&](const Src &s, const float (&g)[CW], int cw, float scale, bool nonfinite) {
        if (s.o < 0) return;
        const float ax = 1.0f - s.fx, ay = 1.0f - s.fy;
        const float w00 = ax * ay, w01 = s.fx * ay, w10 = ax * s.fy, w11 = s.fx * s.fy;
        unsigned long long *a = acc64 + s.o;
        if (!nonfinite) {
            // (a, b) -> a + (b << 32) as two's complement: low word a, high word b + (a >> 31).  Round 4: rounded by ONE
            // instruction each (v_cvt_rpi_i32_f32 = floor(x + 0.5); __float2int_rn is v_rndne_f32 + v_cvt_i32_f32): 26 instead
            // of 34 VALU per source and channel pair (multiplying the two channels as a v_pk_mul_f32 pair saves four more but
            // the aligned register pairs it needs spill 48 VGPRs of this kernel's 128).  Ties round up instead of to even: a fixed rule, so the integer sums stay
            // order-independent, and half a unit of 2^-29 of the group's maximum either way.
            auto pack = [](float va, float vb) {
                int ia, ib;
                asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(ia) : "v"(va));
                asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(ib) : "v"(vb));
                return (static_cast<unsigned long long>(static_cast<unsigned>(ib + (ia >> 31))) << 32) |
                       static_cast<unsigned>(ia);
            };
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                if (2 * q >= cw) break;
                const float ga = g[2 * q] * scale, gb2 = (2 * q + 1 < cw) ? g[2 * q + 1] * scale : 0.f;
                atomicAdd(a + q * PS, pack(w00 * ga, w00 * gb2));
                atomicAdd(a + q * PS + 1, pack(w01 * ga, w01 * gb2));
                atomicAdd(a + q * PS + PW, pack(w10 * ga, w10 * gb2));
                atomicAdd(a + q * PS + PW + 1, pack(w11 * ga, w11 * gb2));
            }
        } else {
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                if (c >= cw) break;
                float *f = reinterpret_cast<float *>(a + (c / 2) * PS) + (c & 1);
                if (interp == CERB_INTERP_NEAREST) {
                    // only the snapped tap: 0 * NaN must not reach the three others (ATen adds to one tap)
                    atomicAdd(f + (s.fy != 0.f ? 2 * PW : 0) + (s.fx != 0.f ? 2 : 0), g[c]);
                    continue;
                }
                atomicAdd(f, w00 * g[c]);
                atomicAdd(f + 2, w01 * g[c]);
                atomicAdd(f + 2 * PW, w10 * g[c]);
                atomicAdd(f + 2 * PW + 2, w11 * g[c]);
            }
        }
    };
    // the group's tile -> global memory; accumulators back to zero for the next group
    // Stores of one dword per lane are issue-bound (MI355X_MICROARCH.md, "store tail": ~7 B/clk/CU); a thread
    // that owns four neighbouring elements of a row stores 16 bytes per channel instead: a quarter of the
    // store instructions (level 3: the write-out phase 6.1k -> ~3k cycles of the workgroup's 35k).
    const bool wide = W % 4 == 0 && (reinterpret_cast<uintptr_t>(gimage) & 15) == 0 && plane % 4 == 0;
    auto write_out = [&](int c0, int cw, float unscale, bool nonfinite) {
        const int npair = (cw + 1) / 2;
        const bool last = c0 + CW >= c_end;          // nothing accumulates after the last group
        if (wide) {
            for (int i = tid; i < npair * TH * (TW / 4); i += 256) {
                const int q = i / (TH * (TW / 4)), rem = i % (TH * (TW / 4));
                const int yy = rem / (TW / 4), xx = (rem % (TW / 4)) * 4;
                const int slot = q * PS + (yy + 1) * PW + xx + 1;
                long long v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = acc[slot + k];
                if (!last) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[slot + k] = 0;
                }
                if (ty0 + yy < H && tx0 + xx < W) {      // (W % 4 == 0: the four columns are in or out together)
                    T *d = dst + static_cast<int64_t>(c0 + 2 * q) * plane + (ty0 + yy) * W + tx0 + xx;
                    // one channel at a time (four results live, not eight: the kernel sits at its 128 VGPRs)
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        if (half == 1 && 2 * q + 1 >= cw) break;
                        float r[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int lo = static_cast<int>(v[k]);
                            const int word = half == 0 ? lo : (nonfinite ? static_cast<int>(v[k] >> 32)
                                                                         : static_cast<int>((v[k] - lo) >> 32));
                            r[k] = nonfinite ? __int_as_float(word) : static_cast<float>(word) * unscale;
                        }
                        T *dh = d + half * plane;
                        if constexpr (sizeof(T) == 4) {
                            *reinterpret_cast<float4 *>(dh) = make_float4(r[0], r[1], r[2], r[3]);
                        } else {
                            T t4[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) st(&t4[k], r[k]);
                            uint2 pk;
                            __builtin_memcpy(&pk, t4, 8);
                            *reinterpret_cast<uint2 *>(dh) = pk;
                        }
                    }
                }
            }
            return;
        }
        for (int i = tid; i < npair * TH * TW; i += 256) {
            const int q = i / (TH * TW), rem = i % (TH * TW);
            const int yy = rem / TW, xx = rem % TW;
            const int slot = q * PS + (yy + 1) * PW + xx + 1;
            const long long v = acc[slot];
            if (!last) acc[slot] = 0;
            if (ty0 + yy < H && tx0 + xx < W) {
                const int lo = static_cast<int>(v);
                const int hi = static_cast<int>((v - lo) >> 32);
                const float ra = nonfinite ? __int_as_float(lo) : static_cast<float>(lo) * unscale;
                const float rb = nonfinite ? __int_as_float(static_cast<int>(v >> 32))
                                           : static_cast<float>(hi) * unscale;
                T *d = dst + static_cast<int64_t>(c0 + 2 * q) * plane + (ty0 + yy) * W + tx0 + xx;
                st(d, ra);
                if (2 * q + 1 < cw) st(d + plane, rb);
            }
        }
    };

    // ---- region scan: the sources that touch the tile, compacted ----
    // The region is walked ONCE per workgroup, in batches with all position loads in flight;
    // the sources whose taps touch the tile (under a rough flow half of the region misses it)
    // are appended to a list that borrows the accumulators' LDS, then dealt to the threads:
    // every thread keeps its NS sources in registers for all channel groups, so a group is
    // one set of gradOutput loads, one block reduction, the adds and the write-out.  The
    // list order depends on the waves' arrival order; the sums do not (integer adds commute).
    constexpr int kCap = (NP * PS * 8) / 16 < 256 * NS ? (NP * PS * 8) / 16 : 256 * NS;
    constexpr int NSP = NS / 2;                                  // pairs per thread (16-bit storage)
    constexpr int kCapP = (NP * PS * 8) / 32 < 256 * NSP ? (NP * PS * 8) / 32 : 256 * NSP;   // list capacity in pairs (two int4 each)
    int4 *list = reinterpret_cast<int4 *>(acc);
    if (tid == 0) red[1][1] = 0;
    __syncthreads();
    if constexpr (!pairs) {
        // regions of up to 2560 pixels (a 16 x 64 tile under +-7 px of flow variation) are
        // classified in ONE batch: all position loads of the workgroup in flight together,
        // one counter update per wave
        constexpr int NB = 10;
        Walk w(tid, rw);
        for (int base = 0; base < n; base += 256 * NB) {
            Src s[NB];
            bool in[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                in[j] = classify(base + j * 256 + tid < n, w.ry, w.rx, s[j]);
                w.next();
            }
            // ranks by (j, lane) order
            int rank[NB], total = 0;
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const unsigned long long m = __ballot(in[j]);
                rank[j] = total + __popcll(m & ((1ull << lane) - 1ull));
                total += __popcll(m);
            }
            int start = 0;
            if (lane == 0 && total) start = atomicAdd(&red[1][1], total);
            start = __shfl(start, 0, 64);
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if (in[j] && start + rank[j] < kCap)
                    list[start + rank[j]] = make_int4(s[j].pv, s[j].o, __float_as_int(s[j].fx),
                                                      __float_as_int(s[j].fy));
        }
    } else {
        // the same walk over PAIRS of region pixels (the region is rw / 2 pairs wide): a pair is kept when either pixel
        // touches the tile; its entry is two int4 (pixel index, the two tile offsets -- -1: does not touch --, four fractions)
        constexpr int NBP = 5;
        const int rwp = rw >> 1, npairs = rwp * rh;
        Walk w(tid, max(rwp, 1));
        for (int base = 0; base < npairs; base += 256 * NBP) {
            Src s[NBP][2];
            bool in[NBP];
#pragma unroll
            for (int j = 0; j < NBP; ++j) {
                const bool on = base + j * 256 + tid < npairs;
                const bool i0 = classify(on, w.ry, 2 * w.rx, s[j][0]);
                const bool i1 = classify(on, w.ry, 2 * w.rx + 1, s[j][1]);
                in[j] = i0 || i1;
                w.next();
            }
            int rank[NBP], total = 0;
#pragma unroll
            for (int j = 0; j < NBP; ++j) {
                const unsigned long long m = __ballot(in[j]);
                rank[j] = total + __popcll(m & ((1ull << lane) - 1ull));
                total += __popcll(m);
            }
            int start = 0;
            if (lane == 0 && total) start = atomicAdd(&red[1][1], total);
            start = __shfl(start, 0, 64);
#pragma unroll
            for (int j = 0; j < NBP; ++j)
                if (in[j] && start + rank[j] < kCapP) {
                    list[2 * (start + rank[j])] = make_int4(s[j][0].pv, s[j][0].o, __float_as_int(s[j][0].fx), __float_as_int(s[j][0].fy));
                    list[2 * (start + rank[j]) + 1] = make_int4(s[j][1].o, __float_as_int(s[j][1].fx), __float_as_int(s[j][1].fy), 0);
                }
        }
    }
    __syncthreads();
    const int count = red[1][1];               // sources, or pairs of them
    __syncthreads();
    CERB_STAMP_AT(2);

    if (count <= (pairs ? kCapP : kCap)) {
        Src src[NS];
        float g[NS][CW];
        const int ns = pairs ? 2 * ((count + 255) / 256) : (count + 255) / 256;   // sources per thread actually present
        const int first_pv = count > 0 ? list[0].x : 0;
        if constexpr (!pairs) {
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const int e = j * 256 + tid;
                const int4 v = list[min(e, kCap - 1)];
                const bool have = e < count;
                // an idle slot (past the end of the list) points at the list's FIRST source: its gradOutput values then take
                // part in the block maximum unmasked (a repeated value cannot change a maximum or add a non-finite one)
                src[j].pv = have ? v.x : first_pv;
                src[j].o = have ? v.y : -1;
                src[j].fx = __int_as_float(v.z);
                src[j].fy = __int_as_float(v.w);
            }
        } else {
#pragma unroll
            for (int jp = 0; jp < NSP; ++jp) {
                const int e = jp * 256 + tid;
                const int4 v0 = list[2 * min(e, kCapP - 1)], v1 = list[2 * min(e, kCapP - 1) + 1];
                const bool have = e < count;
                // (an idle pair points at the list's first pair, as above; a pixel of a live pair that does not touch the tile
                // has o = -1: skipped by the adds and masked out of the block maximum)
                src[2 * jp].pv = have ? v0.x : first_pv;
                src[2 * jp].o = have ? v0.y : -1;
                src[2 * jp].fx = __int_as_float(v0.z);
                src[2 * jp].fy = __int_as_float(v0.w);
                src[2 * jp + 1].pv = src[2 * jp].pv + 1;
                src[2 * jp + 1].o = have ? v1.x : -1;
                src[2 * jp + 1].fx = __int_as_float(v1.y);
                src[2 * jp + 1].fy = __int_as_float(v1.z);
            }
        }
        // gradOutput of the channel group [c0, c0 + CW) at every source of the thread
        auto load_all = [&](int c0) {
            if constexpr (!pairs) {
#pragma unroll
                for (int j = 0; j < NS; ++j)
                    if (j < ns) load_g(src[j], c0, g[j]);
            } else {
#if defined(__HIP_DEVICE_COMPILE__)
                if constexpr (kPair16) {
#pragma unroll
                    for (int jp = 0; jp < NSP; ++jp)
                        if (2 * jp < ns) {
                            const int voff = src[2 * jp].pv * 2;      // an even pixel: a dword holds it and its right neighbour
#pragma unroll
                            for (int c = 0; c < CW; ++c) {
                                const unsigned q = __builtin_amdgcn_raw_buffer_load_b32(
                                    rsrc_go, voff, __builtin_amdgcn_readfirstlane(min(c0 + c, c_end - 1) * plane * 2), 0);
                                g[2 * jp][c] = widen16<T>(static_cast<unsigned short>(q & 0xFFFFu));
                                g[2 * jp + 1][c] = widen16<T>(static_cast<unsigned short>(q >> 16));
                            }
                        }
                }
#endif
            }
        };
        __syncthreads();                       // everyone has its sources: the LDS becomes accumulators
        static_assert((NP * PS) % 2 == 0, "accumulators are zeroed 16 bytes at a time");
        for (int i = tid; i < NP * PS / 2; i += 256) reinterpret_cast<int4 *>(acc)[i] = make_int4(0, 0, 0, 0);
        load_all(c_begin);
        __syncthreads();
        CERB_STAMP_AT(3);
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (j < ns) add_density(src[j]);
        // (pairs: a pixel of a live pair that does not touch the tile is masked out of the maximum -- the scale, and with
        // it every bit of the result, is then the one the pixel-by-pixel form computes)
        int gb0 = 0;
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (j < ns) gb0 = pairs ? absmax_bits_masked(src[j], g[j], gb0) : absmax_bits(src[j], g[j], gb0);
        const int sbits = density_bits(pairs ? 2 * count : count, gb0);
        CERB_STAMP_AT(4);
        for (int c0 = c_begin; c0 < c_end; c0 += CW) {
            const int cw = min(CW, c_end - c0);
            int gb = gb0;
            if (c0 != c_begin) {
                gb = 0;
#pragma unroll
                for (int j = 0; j < NS; ++j)
                    if (j < ns) gb = pairs ? absmax_bits_masked(src[j], g[j], gb) : absmax_bits(src[j], g[j], gb);
            }
            float scale, unscale;
            bool nonfinite;
            block_scale(gb, c0 == c_begin, sbits, scale, unscale, nonfinite);
            if (c0 == c_begin) CERB_STAMP_AT(5);
#pragma unroll
            for (int j = 0; j < NS; ++j)
                if (j < ns) add_taps(src[j], g[j], cw, scale, nonfinite);
            if (c0 == c_begin) CERB_STAMP_AT(6);
            // the next group's gradOutput travels while this group's tile is written out
            if (c0 + CW < c_end) load_all(c0 + CW);
            __syncthreads();   // every tap of the group has been added
            if (c0 == c_begin) CERB_STAMP_AT(7);
            write_out(c0, cw, unscale, nonfinite);
            if (c0 == c_begin) CERB_STAMP_AT(8);
        }
        CERB_STAMP_AT(9);
    } else {
        // ---- more sources than the list holds (flows that pile thousands of pixels onto one
        // tile): walk the region again per channel group; pass A finds the maximum, pass B
        // reloads (L1/L2) and adds ----
        for (int i = tid; i < NP * PS; i += 256) acc[i] = 0;
        __syncthreads();
        constexpr int NB = 4;
        {
            Walk w(tid, rw);
            for (int base = 0; base < n; base += 256 * NB) {
                Src src[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    classify(base + j * 256 + tid < n, w.ry, w.rx, src[j]);
                    w.next();
                }
#pragma unroll
                for (int j = 0; j < NB; ++j) add_density(src[j]);
            }
        }
        int unused_gb = 0;
        const int sbits = density_bits(min(n, 0x3fffffff), unused_gb);
        for (int c0 = c_begin; c0 < c_end; c0 += CW) {
            const int cw = min(CW, c_end - c0);
            float scale = 1.f, unscale = 1.f;
            bool nonfinite = false;
            int gb = 0;
            for (int pass = 0; pass < 2; ++pass) {
                Walk w(tid, rw);
                for (int base = 0; base < n; base += 256 * NB) {
                    Src src[NB];
                    float g[NB][CW];
#pragma unroll
                    for (int j = 0; j < NB; ++j) {
                        classify(base + j * 256 + tid < n, w.ry, w.rx, src[j]);
                        w.next();
                    }
#pragma unroll
                    for (int j = 0; j < NB; ++j) load_g(src[j], c0, g[j]);
                    if (pass == 0) {
#pragma unroll
                        for (int j = 0; j < NB; ++j) gb = absmax_bits_masked(src[j], g[j], gb);
                    } else {
#pragma unroll
                        for (int j = 0; j < NB; ++j) add_taps(src[j], g[j], cw, scale, nonfinite);
                    }
                }
                if (pass == 0) block_scale(gb, false, sbits, scale, unscale, nonfinite);
            }
            __syncthreads();
            write_out(c0, cw, unscale, nonfinite);
        }
    }
}

size_t dtype_size(int dtype) {
    switch (dtype) {
        case CERB_F32: return 4;
        case CERB_F16: case CERB_BF16: return 2;
        case CERB_F64: return 8;
    }
    return 0;
}

}  // namespace

// (image dtype, flow dtype) pairs: the flow has the image's type or is fp32
#define CERB_DISPATCH2(dtype, fdtype, ...)                                              \
    switch (dtype) {                                                                    \
        case CERB_F32:  { using T = float; using F = float; __VA_ARGS__; break; }       \
        case CERB_F16:  if (fdtype == CERB_F32) { using T = __half; using F = float; __VA_ARGS__; } \
                        else { using T = __half; using F = __half; __VA_ARGS__; } break; \
        case CERB_BF16: if (fdtype == CERB_F32) { using T = hip_bfloat16; using F = float; __VA_ARGS__; } \
                        else { using T = hip_bfloat16; using F = hip_bfloat16; __VA_ARGS__; } break; \
        case CERB_F64:  { using T = double; using F = double; __VA_ARGS__; break; }     \
        default: return CERB_EDTYPE;                                                    \
    }

// channel groups per workgroup: keep ~8 channels (two 4-channel trips) per lane so that the
// per-lane chain of dependent gather round trips stays short on the wide, small levels
#define CERB_PICK_CG(C, ...)                                   \
    if ((C) >= 128) { constexpr int CG = 16; __VA_ARGS__; }    \
    else { constexpr int CG = 4; __VA_ARGS__; }

// the few-channel kernels; CERB_EUNSUPPORTED when they do not apply (C > 4, fp64, or a batch item beyond 32-bit offsets)
template <bool BWD>
static int launch_fewc(const void *image, const void *flow, const void *gout, void *out, void *gflow, int B, int C, int H,
                       int W, int pad_mode, int interp, int dtype, int flow_dtype, hipStream_t s) {
    const int64_t plane = static_cast<int64_t>(H) * W;
    if (C > 4 || dtype == CERB_F64 || plane * 16 >= (1ll << 31)) return CERB_EUNSUPPORTED;
    // four pixels per lane once a row has them and the launch is large (>= 2 workgroups per CU either way), else one
    const bool px4 = W >= 256 && static_cast<int64_t>(B) * plane >= 512ll * 1024;
    const int per_wave = kPix * (px4 ? 4 : 1);
    const int segs = (W + per_wave - 1) / per_wave;
    const int64_t items = static_cast<int64_t>(B) * H * segs;
    if (items > 0x7fffffff) return CERB_ETOOLARGE;
    const dim3 grid(static_cast<unsigned>((items + 3) / 4));
#define CERB_FEWC(NC, PX)                                                                                          \
    CERB_DISPATCH2(dtype, flow_dtype, if constexpr (!std::is_same<T, double>::value)                              \
        hipLaunchKernelGGL((warp_fewc_kernel<T, F, NC, PX, BWD>), grid, dim3(256), 0, s,                          \
        static_cast<const T *>(image), static_cast<const F *>(flow), static_cast<const T *>(gout),               \
        static_cast<T *>(out), static_cast<F *>(gflow), static_cast<int>(items), segs, H, W, pad_mode, interp))
#define CERB_FEWC_PX(NC) if (px4) { CERB_FEWC(NC, 4) } else { CERB_FEWC(NC, 1) }
    switch (C) {
        case 1: CERB_FEWC_PX(1) break;
        case 2: CERB_FEWC_PX(2) break;
        case 3: CERB_FEWC_PX(3) break;
        default: CERB_FEWC_PX(4) break;
    }
#undef CERB_FEWC_PX
#undef CERB_FEWC
    return launch_status();
}

int64_t warp_context_bytes(int B, int H, int W) { return ctx_bytes(B, H, W); }

#ifdef CERB_STAMP
extern "C" int cerberus_debug_stamps(void *dst, int bytes) {
    return static_cast<int>(hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps),
                                                std::min<size_t>(bytes, sizeof(g_stamps))));
}
#endif

// strips (= tap-range slots of a context) of this shape
static int ctx_partials(int B, int H, int W) {
    return static_cast<int>(static_cast<int64_t>(B) * Strips(H, W).per_image());
}

// workspace of the tiled backward: 16 reserved bytes + room for a context in case the caller
// has none from the forward
int64_t warp_backward_workspace_bytes(int B, int C, int H, int W) {
    (void)C;
    return 16 + ctx_bytes(B, H, W);
}

static bool flow_dtype_ok(int dtype, int flow_dtype) {
    return flow_dtype == dtype || (flow_dtype == CERB_F32 && (dtype == CERB_F16 || dtype == CERB_BF16));
}

int warp_forward(const void *image, const void *flow, void *out, void *ctx, int64_t ctx_size,
                 int B, int C, int H, int W, int pad_mode, int interp, int dtype, int flow_dtype,
                 hipStream_t s) {
    if (B == 0) return CERB_OK;
    if (!flow_dtype_ok(dtype, flow_dtype)) return CERB_EDTYPE;
    if (ctx && (ctx_size < ctx_bytes(B, H, W) || (reinterpret_cast<uintptr_t>(ctx) & 15)))
        return CERB_EINVAL;
    const int64_t nstrips = static_cast<int64_t>(B) * Strips(H, W).per_image();
    if (nstrips > 0x7fffffff) return CERB_ETOOLARGE;
    if (!ctx && C <= 4 && interp == CERB_INTERP_BILINEAR && option(OPT_WARP_FEWC) >= 0) {
        // no context wanted and <= 4 channels (the loss's RGB warps): a lane owns its pixels with all their channels
        const int rc = launch_fewc<false>(image, flow, nullptr, out, nullptr, B, C, H, W, pad_mode, interp, dtype, flow_dtype, s);
        if (rc != CERB_EUNSUPPORTED) return rc;
    }
    const int staged_opt = option(OPT_WARP_STAGED);
    // LDS-staged window: bilinear, 16-byte-aligned rows, 32-bit byte offsets.  Channels per
    // workgroup: as few as keep the launch at <= 1024 workgroups (the per-workgroup box
    // reduction and window set-up amortise over the channels), between 8 and 32.  Measured, 4
    // pairs, smooth flow, fwd + context, us direct / staged: 64x64x128 9.4 / 8.6, 32x128x256
    // 14.8 / 13.5, 64x128x256 23.8 / 21.2, 32x256x512 44.6 / 37.6 in fp32 and 12.9 / 8.3,
    // 15.5 / 12.0, 28.6 / 19.3, 50.1 / 34.4 in fp16.
    const bool staged = interp == CERB_INTERP_BILINEAR && dtype != CERB_F64 && W % 4 == 0 &&
                        (reinterpret_cast<uintptr_t>(image) & 15) == 0 && staged_opt != 2 &&
                        static_cast<int64_t>(C) * H * W * 4 < 0x7fffffff;
    if (staged && (((dtype == CERB_F16 || dtype == CERB_BF16) && option(OPT_WARP_PAIR16) >= 0) ||
                   (dtype == CERB_F32 && option(OPT_WARP_PAIR16) == 1))) {      // fp32: opt-in (A/B: profiles/r06_warp_fp32_dma_ab.txt)
        // 16-bit storage: two pixels per lane, two channels per LDS dword (warp16.hip); same bits
        const int rc = warp16_forward(image, flow, out, ctx, B, C, H, W, pad_mode, dtype, flow_dtype, staged_opt, s);
        if (rc != CERB_EUNSUPPORTED) return rc;
    }
    if (staged) {
        const Strips strips(H, W);
        const int64_t tiles = static_cast<int64_t>(B) * ((strips.ny + kStageRows - 1) / kStageRows) * strips.nx;
        int crange = 8;
        while (crange < 32 && tiles * ((C + crange - 1) / crange) > 1024) crange *= 2;
        if (staged_opt >= 4) crange = staged_opt;
        crange = std::max(1, std::min(C, crange));
        const int nrange = (C + crange - 1) / crange;
        const int64_t blocks = static_cast<int64_t>(B) * ((strips.ny + kStageRows - 1) / kStageRows) *
                               strips.nx * nrange;
        if (blocks > 0x7fffffff) return CERB_ETOOLARGE;
        CERB_DISPATCH2(dtype, flow_dtype, if constexpr (!std::is_same<T, double>::value)
            hipLaunchKernelGGL((warp_fwd_staged_kernel<T, F>), dim3(static_cast<unsigned>(blocks)),
                               dim3(256), 0, s, static_cast<const T *>(image),
                               static_cast<const F *>(flow), static_cast<T *>(out), ctx, B, C, H, W,
                               pad_mode, crange, nrange))
        return launch_status();
    }
    const dim3 grid(static_cast<unsigned>(nstrips));
    if (option(OPT_WARP_PAIR_TAPS) != 2) {  // default: paired taps in the forward gather
        CERB_PICK_CG(C, CERB_DISPATCH2(dtype, flow_dtype, hipLaunchKernelGGL(
            (warp_fwd_kernel<T, F, true, CG>), grid, dim3(kPix * CG), 0, s,
            static_cast<const T *>(image), static_cast<const F *>(flow), static_cast<T *>(out), ctx,
            B, C, H, W, pad_mode, interp)))
    } else {
        CERB_PICK_CG(C, CERB_DISPATCH2(dtype, flow_dtype, hipLaunchKernelGGL(
            (warp_fwd_kernel<T, F, false, CG>), grid, dim3(kPix * CG), 0, s,
            static_cast<const T *>(image), static_cast<const F *>(flow), static_cast<T *>(out), ctx,
            B, C, H, W, pad_mode, interp)))
    }
    return launch_status();
}

template <typename T, typename F, int TH, int NS>
static int launch_tiles(const void *image, const void *flow, const void *gout, const void *ctx, void *gimage,
                        void *gflow, int B, int C, int H, int W, int pad_mode, int interp, hipStream_t s) {
    constexpr int CW = 8;
    const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + TH - 1) / TH;
    const int64_t tiles = static_cast<int64_t>(B) * tiles_x * tiles_y;
    // channel ranges per tile: every range repeats the tile's region scan, so split only as
    // far as it takes to fill the chip (~2 workgroups per CU), in whole groups of CW channels
    int nrange = 1;
    const int groups = (C + CW - 1) / CW;
    while (nrange < groups && tiles * nrange < 512) nrange *= 2;
    if (const int forced = option(OPT_WARP_TILE_RANGES)) nrange = forced;
    nrange = std::max(1, std::min(nrange, groups));
    const int crange = (groups + nrange - 1) / nrange * CW;
    nrange = (C + crange - 1) / crange;
    const int64_t tile_blocks = gimage ? tiles * nrange : 0;     // (no grad_image: flow workgroups only)
    // grad_flow: 8 x 32 tiles through an LDS window (16-byte aligned rows, 32-bit byte
    // offsets), else 2 x 32 strips x 4 channel-group waves by direct gathers
    const Strips strips(H, W);
    const int64_t flow_tiles = static_cast<int64_t>(B) * ((strips.ny + kStageRows - 1) / kStageRows) * strips.nx;
    const int staged_opt = option(OPT_WARP_STAGED);
    // strip role on a deep level (few pixels, many channels): quarter strips x 16 channel groups.  The choice
    // looks at one image only: an item's grad_flow must not depend on the batch it travels in (the summation
    // order differs from the four-group order the staged role shares with the plain strip role)
    // nearest: grad_flow is all zeros, stored by the plain strip role without a single load
    const bool nearest = interp == CERB_INTERP_NEAREST;
    const int flow_sub = (C >= 64 && strips.per_image() <= 32 && staged_opt < 4 && !nearest) ? 4 : 1;
    const bool flow_staged = gflow && !nearest && W % 4 == 0 && (reinterpret_cast<uintptr_t>(image) & 15) == 0 &&
                             static_cast<int64_t>(C) * H * W * 4 < 0x7fffffff && staged_opt != 2 && flow_sub == 1 &&
                             (flow_tiles >= 512 || staged_opt >= 4);
    const int64_t nstrips = static_cast<int64_t>(B) * strips.per_image();
    // 16-bit storage: the staged role as 8 x 64 tiles with two pixels per lane and an LDS-DMA window (same bits)
    const bool flow16 = flow_staged && sizeof(T) == 2 && W % 8 == 0 && option(OPT_WARP_PAIR16) >= 0 &&
                        (reinterpret_cast<uintptr_t>(gflow) & 7) == 0 && (reinterpret_cast<uintptr_t>(gout) & 3) == 0;
    const int64_t flow16_tiles = static_cast<int64_t>(B) * ((H + kTile16H - 1) / kTile16H) * ((W + kTile16W - 1) / kTile16W);
    const int64_t flow_blocks = !gflow ? 0 : flow16 ? flow16_tiles : flow_staged ? flow_tiles : nstrips * flow_sub;
    if (tile_blocks + flow_blocks > 0x7fffffff) return CERB_ETOOLARGE;
    // PHASE SHIFT (round 4).  When the whole launch is resident at once (<= 4 workgroups per CU) every workgroup runs the
    // same phase at the same time and each phase is bound by a throughput the chip shares -- the gradOutput gather by the
    // memory system, the adds by the LDS-atomic pipe and the VALU, the write-out by store issue -- so the launch takes the
    // SUM of its phases (section 3.4 of DESIGN.md).  Workgroups i, i + 256, i + 512, i + 768 share a CU: starting some of
    // them a few thousand cycles late lets one's gather run under another's adds.  Measured (4 pairs, us, off -> on):
    // 32 x 128 x 256 (two 16-row tile workgroups per CU: the second starts 6 k cycles late) 24.7 -> 22.8; 128 x 32 x 64 (one
    // tile workgroup per CU: the two halves of the flow workgroups 6 k and 2 k cycles late) 11.1 -> 10.1; 64 x 64 x 128 loses with
    // every pattern tried (15.0 -> 15.3 .. 17.3) and keeps none.  "warp_stagger": 0 = this rule, -1 = off, else delays of the
    // second / third / fourth 256 workgroups in units of 1024 cycles, one byte each.
    int stagger = option(OPT_WARP_STAGGER);
    if (stagger == 0) {
        const int64_t total = tile_blocks + flow_blocks;
        if (TH == 16 && tile_blocks == 512 && total <= 1024) stagger = 6;
        else if (tile_blocks == 256 && total > 512 && total <= 1024) stagger = 6 | (2 << 8);
    }
    if (stagger < 0) stagger = 0;
    // 16-bit storage: the tile role takes its sources as horizontally adjacent pairs (one dword of gradOutput per pair)
    constexpr bool can_pair = sizeof(T) == 2 && NS % 2 == 0;
    const bool pair_sources = can_pair && W % 2 == 0 && (reinterpret_cast<uintptr_t>(gout) & 3) == 0 && option(OPT_WARP_PAIR16) >= 0;
#define CERB_LAUNCH_TILES(PR, REFL)                                                                    \
    hipLaunchKernelGGL((warp_bwd_tile_kernel<T, F, TH, CW, NS, PR, REFL>),                             \
                       dim3(static_cast<unsigned>(tile_blocks + flow_blocks)), dim3(256), 0, s,        \
                       static_cast<const T *>(image), static_cast<const T *>(gout), ctx,               \
                       static_cast<const F *>(flow), static_cast<T *>(gimage), static_cast<F *>(gflow), \
                       B, C, H, W, tiles_x, tiles_y, nrange, crange, static_cast<int>(tile_blocks),    \
                       pad_mode, interp, flow16 ? 2 : flow_staged ? 1 : 0, flow_sub, stagger)
    const bool refl = pad_mode == CERB_PAD_REFLECTION;
    if constexpr (can_pair) {
        if (pair_sources) { if (refl) CERB_LAUNCH_TILES(1, true); else CERB_LAUNCH_TILES(1, false); }
        else { if (refl) CERB_LAUNCH_TILES(0, true); else CERB_LAUNCH_TILES(0, false); }
    } else {
        (void)pair_sources;
        if (refl) CERB_LAUNCH_TILES(0, true); else CERB_LAUNCH_TILES(0, false);
    }
#undef CERB_LAUNCH_TILES
    return launch_status();
}

int warp_backward(const void *image, const void *flow, const void *gout, void *gimage,
                  void *gflow, const void *ctx, int64_t ctx_size, void *workspace,
                  int64_t workspace_bytes, int B, int C, int H, int W, int pad_mode, int interp,
                  int dtype, int flow_dtype, hipStream_t s) {
    const int64_t plane = static_cast<int64_t>(H) * W;
    if (B == 0) return CERB_OK;
    const size_t esz = dtype_size(dtype);
    if (!esz) return CERB_EDTYPE;
    if (!flow_dtype_ok(dtype, flow_dtype)) return CERB_EDTYPE;
    if (ctx && (ctx_size < ctx_bytes(B, H, W) || (reinterpret_cast<uintptr_t>(ctx) & 15)))
        return CERB_EINVAL;
    const dim3 grid(static_cast<unsigned>((plane + kPix - 1) / kPix), B);
    // tiled (owner-computes) path: grad_image wanted, fp32 or 16-bit storage, and a context --
    // the forward's, or one built here in the caller's workspace
    const bool ws_ok = workspace && workspace_bytes >= warp_backward_workspace_bytes(B, C, H, W) &&
                       (reinterpret_cast<uintptr_t>(workspace) & 15) == 0;
    // (round 6: grad_flow ALONE with more than 4 channels takes the same launch with no tile workgroups -- its flow role's
    // LDS window beats the per-pixel gathers of warp_bwd_kernel: 32 x 256 x 512 fp16 68.8 -> 30 us)
    const bool tiled = (gimage || (gflow && C > 4)) && dtype != CERB_F64 && (ctx || ws_ok) &&
                       static_cast<int64_t>(C) * plane * static_cast<int64_t>(esz) < 0x7fffffff &&
                       option(OPT_WARP_FORCE_SCATTER) == 0;
    if (tiled) {
        int rc;
        if (!ctx) {
            // no forward context: positions + tap ranges from the flow (one extra launch)
            void *own = static_cast<char *>(workspace) + 16;
            if (flow_dtype == CERB_F32)
                hipLaunchKernelGGL(warp_context_kernel<float>, dim3(ctx_partials(B, H, W)), dim3(kPix),
                                   0, s, static_cast<const float *>(flow), own, B, H, W, pad_mode);
            else if (flow_dtype == CERB_F16)
                hipLaunchKernelGGL(warp_context_kernel<__half>, dim3(ctx_partials(B, H, W)), dim3(kPix),
                                   0, s, static_cast<const __half *>(flow), own, B, H, W, pad_mode);
            else
                hipLaunchKernelGGL(warp_context_kernel<hip_bfloat16>, dim3(ctx_partials(B, H, W)),
                                   dim3(kPix), 0, s, static_cast<const hip_bfloat16 *>(flow), own, B,
                                   H, W, pad_mode);
            if ((rc = launch_status())) return rc;
            ctx = own;
        }
        // ONE launch: grad_image tiles + grad_flow strips.  Tile height: 16 rows, 8 on small
        // maps (twice the workgroups, a smaller region per workgroup).
        const int th_opt = option(OPT_WARP_TILE_H);
        const bool th8 = th_opt ? th_opt == 8 : static_cast<int64_t>(B) * H * W <= 64 * 128 * 4;
        if (th8) {
            // (16-bit storage: six sources per thread instead of five, an even number: they are taken as pairs)
            CERB_DISPATCH2(dtype, flow_dtype, if constexpr (!std::is_same<T, double>::value)
                return (launch_tiles<T, F, 8, sizeof(T) == 2 ? 6 : 5>(image, flow, gout, ctx, gimage, gflow, B, C, H, W, pad_mode, interp, s)))
        } else {
            CERB_DISPATCH2(dtype, flow_dtype, if constexpr (!std::is_same<T, double>::value)
                return (launch_tiles<T, F, 16, 6>(image, flow, gout, ctx, gimage, gflow, B, C, H, W, pad_mode, interp, s)))
        }
        return CERB_EDTYPE;
    }
    if (!gimage && gflow && C <= 4 && option(OPT_WARP_FEWC) >= 0) {
        // grad_flow alone for <= 4 channels (the loss's RGB warps: the target image carries no gradient)
        const int rc = launch_fewc<true>(image, flow, gout, nullptr, gflow, B, C, H, W, pad_mode, interp, dtype, flow_dtype, s);
        if (rc != CERB_EUNSUPPORTED) return rc;
    }
    if (gimage) {
        hipError_t e = hipMemsetAsync(gimage, 0, static_cast<size_t>(B) * C * plane * esz, s);
        if (e != hipSuccess) return static_cast<int>(e);
    }
    if (option(OPT_WARP_PAIR_TAPS) == 1) {
        CERB_PICK_CG(C, CERB_DISPATCH2(dtype, flow_dtype, hipLaunchKernelGGL(
            (warp_bwd_kernel<T, F, true, CG>), grid, dim3(kPix * CG), 0, s,
            static_cast<const T *>(image), static_cast<const F *>(flow),
            static_cast<const T *>(gout), static_cast<T *>(gimage), static_cast<F *>(gflow), B, C,
            H, W, pad_mode, interp)))
    } else {
        CERB_PICK_CG(C, CERB_DISPATCH2(dtype, flow_dtype, hipLaunchKernelGGL(
            (warp_bwd_kernel<T, F, false, CG>), grid, dim3(kPix * CG), 0, s,
            static_cast<const T *>(image), static_cast<const F *>(flow),
            static_cast<const T *>(gout), static_cast<T *>(gimage), static_cast<F *>(gflow), B, C,
            H, W, pad_mode, interp)))
    }
    return launch_status();
}

}  // namespace cerb
