// api.hip -- the extern "C" surface declared in include/cerberus_hip.h.
// Argument validation + dispatch only; kernels live in corr_d4.hip / corr_d4_bwd.hip / corr_strip.hip / corr_coarse.hip /
// corr_mfma.hip / corr_generic.hip, corr_grad_prep.hip, warp.hip, warp16.hip, warp_corr.hip, upsample.hip, photometric.hip,
// census.hip, occlusion.hip, reproject.hip, seg_loss.hip, depth_loss.hip, metrics.hip and rmi_loss.hip.
// (panoptic_train.hip carries the entry points of its own ops.)
#include <atomic>
#include <cstring>

#include "common.h"

namespace cerb {
namespace {
// indexed by OptId (common.h)
const char *const g_option_names[OPT_COUNT] = {
    "corr_force_generic",   // 1: always use the generic kernels
    "corr_fwd_variant",     // 0: auto, 1..8: force a register-staged variant, 9..13: LDS-DMA, 14: matrix cores (16-bit), 15: coarse-level kernel, 16: auto without it, 17: persistent pipelined forward (-DCERB_EXPERIMENTS builds only), 20 / 26: the matrix-core forward register-staged / without the walk
    "corr_bwd_variant",     // 0: auto, 1: all-81 per lane, 2/3: 3 dy groups, 4/5: LDS-DMA, 6-9: dy-streaming, 10: column walk, 11: matrix cores, row per wave (16-bit; auto: segment per wave), 12/13: strip, 14/15: coarse-level kernel forced / off
    "corr_bwd_cslice",      // 0: auto, else channels per backward workgroup (matrix-core backward: tiles per column walk)
    "corr_no_mfma",         // 1: 16-bit storage never takes the matrix-core kernels (vector kernels, auto-selected)
    "warp_pair_taps",       // 0: default, 1: pairs everywhere, 2: none
    "warp_tile_ranges",     // 0: auto, else channel ranges per warp-backward tile
    "warp_tile_h",          // 0: auto, 8 / 16: rows per warp-backward tile
    "warp_force_scatter",   // 1: warp backward by global atomics (ATen's method) even with a context
    "warp_staged",          // 0: auto (warp gathers through an LDS window), 2: never, >= 4: that many channels per forward workgroup
    "warp_stagger",         // warp backward phase shift: 0 auto, -1 off, else delays (x 1024 cycles) of the 2nd / 3rd / 4th 256 workgroups, a byte each
    "warp_fewc",            // 0: auto (<= 4 channels without context / grad_image take the lane-per-pixel kernels), -1: off
    "warp_pair16",          // 0: auto (16-bit images take the two-elements-per-lane kernels of warp16.hip), -1: off
#ifdef CERB_ABLATE
    "corr_debug_ablate",    // timing ablation mask (WRONG results when != 0); ablation builds only
#endif
};
std::atomic<int> g_option_values[OPT_COUNT];
// process-wide (diagnostics): autograd runs the backward on its own thread, and the caller that asks
// "which kernel ran" sits on another one; names are string literals, so a relaxed pointer store is enough
std::atomic<const char *> g_last_kernel[2] = {{"none"}, {"none"}};

int find_option(const char *key) {
    for (int i = 0; i < OPT_COUNT; ++i)
        if (!std::strcmp(g_option_names[i], key)) return i;
    return -1;
}

bool dtype_ok(int dtype) { return dtype >= CERB_F32 && dtype <= CERB_F64; }
}  // namespace

int option(OptId id) { return g_option_values[id].load(std::memory_order_relaxed); }
void note_kernel(int which, const char *name) { g_last_kernel[which & 1].store(name, std::memory_order_relaxed); }
}  // namespace cerb

using namespace cerb;

extern "C" {

int cerberus_abi_version(void) { return CERBERUS_HIP_ABI_VERSION; }

const char *cerberus_error_string(int code) {
    switch (code) {
        case CERB_OK: return "success";
        case CERB_EINVAL: return "invalid argument (null pointer, non-positive size or empty output)";
        case CERB_EDTYPE: return "unknown dtype";
        case CERB_ESTRIDE1: return "correlation backward requires stride1 == 1";
        case CERB_EMODE: return "unknown padding or interpolation mode";
        case CERB_EUNSUPPORTED: return "valid request that is not implemented";
        case CERB_ETOOLARGE: return "dimension exceeds launch/index limits";
        default: break;
    }
    if (code > 0) return hipGetErrorString(static_cast<hipError_t>(code));
    return "unknown cerberus_hip error";
}

int cerberus_correlation_out_shape(int H, int W, int pad_size, int kernel_size,
                                   int max_displacement, int stride1, int stride2,
                                   int *out_channels, int *out_height, int *out_width) {
    if (!out_channels || !out_height || !out_width) return CERB_EINVAL;
    CorrGeom g;
    const int rc = corr_geom_init(g, 1, 1, H, W, pad_size, kernel_size, max_displacement, stride1,
                                  stride2);
    if (rc) return rc;
    *out_channels = g.oC; *out_height = g.oH; *out_width = g.oW;
    return CERB_OK;
}

int cerberus_correlation_forward_ex(const void *input1, const void *input2, void *output, int B,
                                    int C, int H, int W, int pad_size, int kernel_size,
                                    int max_displacement, int stride1, int stride2,
                                    float negative_slope, int64_t out_batch_stride, int dtype,
                                    void *stream) {
    if (!dtype_ok(dtype)) return CERB_EDTYPE;
    CorrGeom g;
    int rc = corr_geom_init(g, B, C, H, W, pad_size, kernel_size, max_displacement, stride1,
                            stride2);
    if (rc) return rc;
    if (B == 0) return CERB_OK;
    if (!input1 || !input2 || !output) return CERB_EINVAL;
    if (out_batch_stride != 0 &&
        out_batch_stride < static_cast<int64_t>(g.oC) * g.oH * g.oW)
        return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!option(OPT_CORR_FORCE_GENERIC)) {
        rc = corr_d4_forward(input1, input2, output, g, negative_slope, out_batch_stride, dtype, s);
        if (rc != CERB_EUNSUPPORTED) return rc;
    }
    note_kernel(0, "corr_fwd_generic");
    return corr_generic_forward(input1, input2, output, g, negative_slope, out_batch_stride, dtype,
                                s);
}

int cerberus_correlation_forward(const void *input1, const void *input2, void *output, int B,
                                 int C, int H, int W, int pad_size, int kernel_size,
                                 int max_displacement, int stride1, int stride2,
                                 int corr_type_multiply, int dtype, void *stream) {
    (void)corr_type_multiply;  // accepted and ignored, exactly like the reference
    return cerberus_correlation_forward_ex(input1, input2, output, B, C, H, W, pad_size,
                                           kernel_size, max_displacement, stride1, stride2, 1.0f,
                                           0, dtype, stream);
}

int cerberus_correlation_backward(const void *input1, const void *input2, const void *grad_output,
                                  void *grad_input1, void *grad_input2, int B, int C, int H,
                                  int W, int pad_size, int kernel_size, int max_displacement,
                                  int stride1, int stride2, int corr_type_multiply, int dtype,
                                  void *stream) {
    (void)corr_type_multiply;
    if (!dtype_ok(dtype)) return CERB_EDTYPE;
    CorrGeom g;
    int rc = corr_geom_init(g, B, C, H, W, pad_size, kernel_size, max_displacement, stride1,
                            stride2);
    if (rc) return rc;
    if (stride1 != 1) return CERB_ESTRIDE1;
    if (B == 0) return CERB_OK;
    if (!input1 || !input2 || !grad_output || !grad_input1 || !grad_input2) return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!option(OPT_CORR_FORCE_GENERIC)) {
        rc = corr_d4_backward(input1, input2, grad_output, grad_input1, grad_input2, g, dtype, s);
        if (rc != CERB_EUNSUPPORTED) return rc;
    }
    note_kernel(1, "corr_bwd_generic");
    return corr_generic_backward(input1, input2, grad_output, grad_input1, grad_input2, g, dtype,
                                 s);
}

int64_t cerberus_correlation_backward_ex_workspace_bytes(int B, int H, int W, int pad_size, int kernel_size,
                                                         int max_displacement, int stride1, int stride2, int dtype) {
    if (!dtype_ok(dtype)) return 0;
    CorrGeom g;
    if (corr_geom_init(g, B, 1, H, W, pad_size, kernel_size, max_displacement, stride1, stride2)) return 0;
    const int64_t esz = dtype == CERB_F32 ? 4 : dtype == CERB_F64 ? 8 : 2;
    return static_cast<int64_t>(B) * g.oC * g.oH * g.oW * esz;
}

int cerberus_correlation_backward_ex(const void *input1, const void *input2, const void *grad_output,
                                     int64_t grad_out_batch_stride, const void *fwd_output,
                                     int64_t fwd_out_batch_stride, float negative_slope, void *workspace,
                                     int64_t workspace_bytes, void *grad_input1, void *grad_input2, int B, int C,
                                     int H, int W, int pad_size, int kernel_size, int max_displacement, int stride1,
                                     int stride2, int dtype, void *stream) {
    if (!dtype_ok(dtype)) return CERB_EDTYPE;
    CorrGeom g;
    int rc = corr_geom_init(g, B, C, H, W, pad_size, kernel_size, max_displacement, stride1, stride2);
    if (rc) return rc;
    if (stride1 != 1) return CERB_ESTRIDE1;
    if (B == 0) return CERB_OK;
    const int64_t item = static_cast<int64_t>(g.oC) * g.oH * g.oW;
    if ((grad_out_batch_stride != 0 && grad_out_batch_stride < item) ||
        (fwd_output && fwd_out_batch_stride != 0 && fwd_out_batch_stride < item))
        return CERB_EINVAL;
    const bool dense = B == 1 || grad_out_batch_stride == 0 || grad_out_batch_stride == item;   // one item: no stride to honour
    if (dense && !fwd_output)
        return cerberus_correlation_backward(input1, input2, grad_output, grad_input1, grad_input2, B, C, H, W, pad_size,
                                             kernel_size, max_displacement, stride1, stride2, 1, dtype, stream);
    if (!input1 || !input2 || !grad_output || !grad_input1 || !grad_input2) return CERB_EINVAL;
    const int64_t need = cerberus_correlation_backward_ex_workspace_bytes(B, H, W, pad_size, kernel_size, max_displacement,
                                                                          stride1, stride2, dtype);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)) return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = corr_grad_prep(grad_output, dense ? item : grad_out_batch_stride, fwd_output,
                        fwd_out_batch_stride ? fwd_out_batch_stride : item, workspace, B, item, negative_slope, dtype, s);
    if (rc) return rc;
    return cerberus_correlation_backward(input1, input2, workspace, grad_input1, grad_input2, B, C, H, W, pad_size,
                                         kernel_size, max_displacement, stride1, stride2, 1, dtype, stream);
}

static int warp_args_ok(int B, int C, int H, int W, int pad_mode, int interp_mode, int dtype) {
    if (!dtype_ok(dtype)) return CERB_EDTYPE;
    if (B < 0 || C <= 0 || H <= 0 || W <= 0) return CERB_EINVAL;
    if (pad_mode < CERB_PAD_ZEROS || pad_mode > CERB_PAD_REFLECTION) return CERB_EMODE;
    if (interp_mode < CERB_INTERP_BILINEAR || interp_mode > CERB_INTERP_NEAREST) return CERB_EMODE;
    return CERB_OK;
}

int cerberus_flow_warp_forward(const void *image, const void *flow, void *out, int B, int C, int H,
                               int W, int pad_mode, int interp_mode, int dtype, void *stream) {
    return cerberus_flow_warp_forward_ctx(image, flow, out, nullptr, 0, B, C, H, W, pad_mode,
                                          interp_mode, dtype, dtype, stream);
}

int64_t cerberus_flow_warp_context_bytes(int B, int H, int W) {
    if (B < 0 || H < 0 || W < 0) return 0;
    return warp_context_bytes(B, H, W);
}

int cerberus_flow_warp_forward_ctx(const void *image, const void *flow, void *out, void *context,
                                   int64_t context_bytes, int B, int C, int H, int W,
                                   int pad_mode, int interp_mode, int dtype, int flow_dtype,
                                   void *stream) {
    const int rc = warp_args_ok(B, C, H, W, pad_mode, interp_mode, dtype);
    if (rc) return rc;
    if (!dtype_ok(flow_dtype)) return CERB_EDTYPE;
    if (B == 0) return CERB_OK;
    if (!image || !flow || !out) return CERB_EINVAL;
    return warp_forward(image, flow, out, context, context_bytes, B, C, H, W, pad_mode,
                        interp_mode, dtype, flow_dtype, static_cast<hipStream_t>(stream));
}

int64_t cerberus_warp_correlation_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return warp_corr_workspace_bytes(B, C, H, W);
}

int cerberus_warp_correlation_forward(const void *input1, const void *input2, const void *flow, void *output, void *workspace,
                                      int64_t workspace_bytes, int B, int C, int H, int W, int pad_mode, float negative_slope,
                                      int64_t out_batch_stride, int dtype, int flow_dtype, void *stream) {
    const int rc = warp_args_ok(B, C, H, W, pad_mode, CERB_INTERP_BILINEAR, dtype);
    if (rc) return rc;
    if (!dtype_ok(flow_dtype)) return CERB_EDTYPE;
    if (pad_mode == CERB_PAD_REFLECTION) return CERB_EUNSUPPORTED;   // (no reference caller; not built into the fused kernel)
    if (B == 0) return CERB_OK;
    if (!input1 || !input2 || !flow || !output) return CERB_EINVAL;
    if (out_batch_stride != 0 && out_batch_stride < static_cast<int64_t>(81) * H * W) return CERB_EINVAL;
    return warp_corr_forward(input1, input2, flow, output, workspace, workspace_bytes, B, C, H, W, pad_mode, negative_slope,
                             out_batch_stride, dtype, flow_dtype, static_cast<hipStream_t>(stream));
}

int64_t cerberus_flow_warp_backward_workspace_bytes(int B, int C, int H, int W) {
    if (B < 0 || C < 0 || H < 0 || W < 0) return 0;
    return warp_backward_workspace_bytes(B, C, H, W);
}

int cerberus_flow_warp_backward(const void *image, const void *flow, const void *grad_out,
                                void *grad_image, void *grad_flow, const void *context,
                                int64_t context_bytes, void *workspace, int64_t workspace_bytes,
                                int B, int C, int H, int W, int pad_mode, int interp_mode,
                                int dtype, int flow_dtype, void *stream) {
    const int rc = warp_args_ok(B, C, H, W, pad_mode, interp_mode, dtype);
    if (rc) return rc;
    if (!dtype_ok(flow_dtype)) return CERB_EDTYPE;
    if (B == 0) return CERB_OK;
    if (!image || !flow || !grad_out) return CERB_EINVAL;
    if (!grad_image && !grad_flow) return CERB_OK;
    return warp_backward(image, flow, grad_out, grad_image, grad_flow, context, context_bytes,
                         workspace, workspace_bytes, B, C, H, W, pad_mode, interp_mode, dtype,
                         flow_dtype, static_cast<hipStream_t>(stream));
}

static int upsample_entry(bool fwd, const void *src, void *dst, int64_t planes, int H, int W, int factor,
                          int dtype, void *stream) {
    if (!dtype_ok(dtype)) return CERB_EDTYPE;
    if (planes < 0 || H <= 0 || W <= 0 || factor < 1) return CERB_EINVAL;
    if (planes == 0) return CERB_OK;
    if (!src || !dst) return CERB_EINVAL;
    if (static_cast<int64_t>(H) * factor > 0x7fffffff || static_cast<int64_t>(W) * factor > 0x7fffffff)
        return CERB_ETOOLARGE;
    return flow_upsample(fwd, src, dst, planes, H, W, factor, dtype, static_cast<hipStream_t>(stream));
}

int cerberus_flow_upsample_forward(const void *src, void *dst, int64_t planes, int H, int W, int factor,
                                   int dtype, void *stream) {
    return upsample_entry(true, src, dst, planes, H, W, factor, dtype, stream);
}

int cerberus_flow_upsample_backward(const void *grad_out, void *grad_in, int64_t planes, int H, int W,
                                    int factor, int dtype, void *stream) {
    return upsample_entry(false, grad_out, grad_in, planes, H, W, factor, dtype, stream);
}

int cerberus_area_resize(const void *src, void *dst, int64_t planes, int H, int W, int out_h, int out_w,
                         int dtype, void *stream) {
    if (!dtype_ok(dtype)) return CERB_EDTYPE;
    if (planes < 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0) return CERB_EINVAL;
    if (planes == 0) return CERB_OK;
    if (!src || !dst) return CERB_EINVAL;
    return area_resize(src, dst, planes, H, W, out_h, out_w, dtype, static_cast<hipStream_t>(stream));
}

int cerberus_area_pyramid(const void *src, void *const *dsts, const int *out_h, const int *out_w, int n_scales,
                          int64_t planes, int H, int W, int dtype, void *stream) {
    if (!dtype_ok(dtype)) return CERB_EDTYPE;
    if (planes < 0 || H <= 0 || W <= 0 || n_scales < 0) return CERB_EINVAL;
    if (n_scales == 0 || planes == 0) return CERB_OK;
    if (!src || !dsts || !out_h || !out_w) return CERB_EINVAL;
    for (int i = 0; i < n_scales; ++i)
        if (!dsts[i] || out_h[i] <= 0 || out_w[i] <= 0) return CERB_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = area_pyramid(src, dsts, out_h, out_w, n_scales, planes, H, W, dtype, s);
    if (rc != CERB_EUNSUPPORTED) return rc;
    // general ratios (or more scales than one launch holds): scale by scale
    for (int i = 0; i < n_scales; ++i) {
        const int r = area_resize(src, dsts[i], planes, H, W, out_h[i], out_w[i], dtype, s);
        if (r) return r;
    }
    return CERB_OK;
}

// the scalar loss ops are fp32 only: a known 16-bit / 64-bit dtype is "valid but not implemented"
static int loss_dtype_ok(int dtype) {
    if (!dtype_ok(dtype)) return CERB_EDTYPE;
    return dtype == CERB_F32 ? CERB_OK : CERB_EUNSUPPORTED;
}

// one NCHW tensor's elements must be addressable with 32-bit offsets inside a batch item, the workgroups with an int
static int loss_size_ok(int64_t B, int64_t C, int64_t H, int64_t W, int64_t workgroups) {
    if (C * H * W > 0x7fffffff || workgroups > 0x7fffffff) return CERB_ETOOLARGE;
    (void)B;
    return CERB_OK;
}

static int photometric_args_ok(int B, int C, int H, int W, int dtype) {
    const int rc = loss_dtype_ok(dtype);
    if (rc) return rc;
    if (B <= 0 || C <= 0 || H < 2 || W < 2) return CERB_EINVAL;     // ReflectionPad2d(1) needs two rows and columns
    return loss_size_ok(B, C, H, W, photometric_workspace_bytes(B, C, H, W) / 4);
}

int64_t cerberus_photometric_loss_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return photometric_workspace_bytes(B, C, H, W);
}

int cerberus_photometric_loss_forward(const void *im_orig, const void *im_recons, void *loss, void *workspace,
                                      int64_t workspace_bytes, int B, int C, int H, int W, float l1_weight, float ssim_weight,
                                      int dtype, void *stream) {
    const int rc = photometric_args_ok(B, C, H, W, dtype);
    if (rc) return rc;
    if (!im_orig || !im_recons || !loss || !workspace) return CERB_EINVAL;
    if (workspace_bytes < photometric_workspace_bytes(B, C, H, W)) return CERB_EINVAL;
    return photometric_forward(im_orig, im_recons, loss, workspace, B, C, H, W, l1_weight, ssim_weight,
                               static_cast<hipStream_t>(stream));
}

int cerberus_photometric_loss_backward(const void *im_orig, const void *im_recons, const void *grad_loss, void *grad_recons,
                                       int B, int C, int H, int W, float l1_weight, float ssim_weight, int dtype, void *stream) {
    const int rc = photometric_args_ok(B, C, H, W, dtype);
    if (rc) return rc;
    if (!im_orig || !im_recons || !grad_loss || !grad_recons) return CERB_EINVAL;
    return photometric_backward(im_orig, im_recons, grad_loss, grad_recons, B, C, H, W, l1_weight, ssim_weight,
                                static_cast<hipStream_t>(stream));
}

static int census_args_ok(int B, int H, int W, int max_distance, int dtype) {
    const int rc = loss_dtype_ok(dtype);
    if (rc) return rc;
    if (max_distance < 1 || max_distance > 3) return CERB_EINVAL;    // the compiled window sizes: 3 x 3, 5 x 5, 7 x 7
    const int patch = 2 * max_distance + 1;
    if (B <= 0 || H < patch || W < patch) return CERB_EINVAL;        // the valid mask needs one interior pixel
    return loss_size_ok(B, 3, H, W, census_workspace_bytes(B, H, W) / 4);
}

int64_t cerberus_census_loss_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return census_workspace_bytes(B, H, W);
}

int cerberus_census_loss_forward(const void *im, const void *im_warp, void *loss, void *workspace, int64_t workspace_bytes, int B,
                                 int H, int W, int max_distance, int dtype, void *stream) {
    const int rc = census_args_ok(B, H, W, max_distance, dtype);
    if (rc) return rc;
    if (!im || !im_warp || !loss || !workspace) return CERB_EINVAL;
    if (workspace_bytes < census_workspace_bytes(B, H, W)) return CERB_EINVAL;
    return census_forward(im, im_warp, loss, workspace, B, H, W, max_distance, static_cast<hipStream_t>(stream));
}

int cerberus_census_loss_backward(const void *im, const void *im_warp, const void *grad_loss, void *grad_warp, int B, int H, int W,
                                  int max_distance, int dtype, void *stream) {
    const int rc = census_args_ok(B, H, W, max_distance, dtype);
    if (rc) return rc;
    if (!im || !im_warp || !grad_loss || !grad_warp) return CERB_EINVAL;
    return census_backward(im, im_warp, grad_loss, grad_warp, B, H, W, max_distance, static_cast<hipStream_t>(stream));
}

// the occlusion ops: (B,2,H,W) fp32 in, (B,1,H,W) fp32 out.  2 * H * W < 2^31 is what keeps the splat's 64-bit fixed-point sum
// from wrapping (occlusion.hip), H, W <= 2^24 keeps floor(x) + 1 exact in fp32 wherever a tap counts.
static int occlusion_args_ok(int B, int H, int W, int dtype) {
    const int rc = loss_dtype_ok(dtype);
    if (rc) return rc;
    if (B <= 0 || H <= 0 || W <= 0) return CERB_EINVAL;
    if (H > (1 << 24) || W > (1 << 24)) return CERB_ETOOLARGE;
    const int64_t tiles = (static_cast<int64_t>(W) + 63) / 64 * ((static_cast<int64_t>(H) + 15) / 16) * B;
    const int64_t blocks = (static_cast<int64_t>(B) * H * W + 255) / 256;
    return loss_size_ok(B, 2, H, W, tiles > blocks ? tiles : blocks);
}

int64_t cerberus_corresponding_map_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return corresponding_map_workspace_bytes(B, H, W);
}

int cerberus_corresponding_map(const void *data, void *map, void *workspace, int64_t workspace_bytes, int B, int H, int W,
                               int is_flow, int dtype, void *stream) {
    const int rc = occlusion_args_ok(B, H, W, dtype);
    if (rc) return rc;
    if (!data || !map || !workspace) return CERB_EINVAL;
    if (is_flow != 0 && is_flow != 1) return CERB_EINVAL;
    if (workspace_bytes < corresponding_map_workspace_bytes(B, H, W)) return CERB_EINVAL;
    return corresponding_map(data, map, workspace, B, H, W, is_flow, static_cast<hipStream_t>(stream));
}

int cerberus_occlusion_mask_bidirection(const void *flow12, const void *flow21, void *mask, int B, int H, int W, float scale,
                                        float bias, int dtype, void *stream) {
    const int rc = occlusion_args_ok(B, H, W, dtype);
    if (rc) return rc;
    if (!flow12 || !flow21 || !mask) return CERB_EINVAL;
    return occlusion_mask_bidirection(flow12, flow21, mask, B, H, W, scale, bias, static_cast<hipStream_t>(stream));
}

// the reprojection warp: image (B,C,H,W), depth (B,1,H,W), fp32.  The reference divides by W - 1 and H - 1; the whole image
// tensor is addressed with one 31-bit element count.
static int reproject_args_ok(int B, int C, int H, int W, int dtype) {
    const int rc = loss_dtype_ok(dtype);
    if (rc) return rc;
    if (B <= 0 || C <= 0 || H < 2 || W < 2) return CERB_EINVAL;
    if (static_cast<int64_t>(B) * C * H * W > 0x7fffffff) return CERB_EINVAL;
    return CERB_OK;
}

int cerberus_reproject_warp_forward(const void *image, const void *depth, const void *inv_K, const void *proj, void *out, int B,
                                    int C, int H, int W, float eps, int dtype, void *stream) {
    const int rc = reproject_args_ok(B, C, H, W, dtype);
    if (rc) return rc;
    if (!image || !depth || !inv_K || !proj || !out) return CERB_EINVAL;
    return reproject_warp_forward(image, depth, inv_K, proj, out, B, C, H, W, eps, static_cast<hipStream_t>(stream));
}

int cerberus_reproject_warp_backward(const void *image, const void *depth, const void *inv_K, const void *proj, const void *grad_out,
                                     void *grad_depth, int B, int C, int H, int W, float eps, int dtype, void *stream) {
    const int rc = reproject_args_ok(B, C, H, W, dtype);
    if (rc) return rc;
    if (!image || !depth || !inv_K || !proj || !grad_out || !grad_depth) return CERB_EINVAL;
    return reproject_warp_backward(image, depth, inv_K, proj, grad_out, grad_depth, B, C, H, W, eps,
                                   static_cast<hipStream_t>(stream));
}

// the segmentation loss: logits (B,C,H,W) fp32, labels (B,H,W) int64.  Pixels are counted with an int (a workgroup's last
// pixel index may run 1023 past the end before it is tested); offsets into the logits are 64-bit.
static int seg_ce_args_ok(int B, int C, int H, int W, int dtype) {
    const int rc = loss_dtype_ok(dtype);
    if (rc) return rc;
    if (B < 0 || C < 2 || H <= 0 || W <= 0) return CERB_EINVAL;
    if (static_cast<int64_t>(B) * H * W > 0x7fffffff - 1024) return CERB_ETOOLARGE;
    return CERB_OK;
}

int64_t cerberus_seg_cross_entropy_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || static_cast<int64_t>(B) * H * W > 0x7fffffff - 1024) return 0;
    return seg_ce_workspace_bytes(B, H, W);
}

int cerberus_seg_cross_entropy_forward(const void *logits, const void *target, const void *weight, void *loss, void *lse,
                                       void *state, void *workspace, int64_t workspace_bytes, int B, int C, int H, int W,
                                       int64_t ignore_index, float gamma, int dtype, void *stream) {
    const int rc = seg_ce_args_ok(B, C, H, W, dtype);
    if (rc) return rc;
    if (!(gamma >= 0.f)) return CERB_EINVAL;                     // a NaN gamma too
    if (B == 0) return CERB_OK;
    if (!logits || !target || !weight || !loss || !lse || !state || !workspace) return CERB_EINVAL;
    if (workspace_bytes < seg_ce_workspace_bytes(B, H, W)) return CERB_EINVAL;
    return seg_ce_forward(logits, target, weight, loss, lse, state, workspace, B, C, H, W, ignore_index, gamma,
                          static_cast<hipStream_t>(stream));
}

int cerberus_seg_cross_entropy_backward(const void *logits, const void *target, const void *weight, const void *lse,
                                        const void *state, const void *grad_loss, void *grad_logits, int B, int C, int H, int W,
                                        int64_t ignore_index, int dtype, void *stream) {
    const int rc = seg_ce_args_ok(B, C, H, W, dtype);
    if (rc) return rc;
    if (B == 0) return CERB_OK;
    if (!logits || !target || !weight || !lse || !state || !grad_loss || !grad_logits) return CERB_EINVAL;
    return seg_ce_backward(logits, target, weight, lse, state, grad_loss, grad_logits, B, C, H, W, ignore_index,
                           static_cast<hipStream_t>(stream));
}

int cerberus_class_histogram(const void *target, void *counts, int64_t count, int num_classes, int64_t ignore_index, void *stream) {
    if (count < 0 || num_classes < 1) return CERB_EINVAL;
    if (num_classes > class_histogram_max_classes()) return CERB_EUNSUPPORTED;
    if (count > (static_cast<int64_t>(1) << 40)) return CERB_ETOOLARGE;       // a workgroup's 32-bit LDS bins cannot wrap
    if (count == 0) return CERB_OK;
    if (!target || !counts) return CERB_EINVAL;
    return class_histogram(target, counts, count, num_classes, ignore_index, static_cast<hipStream_t>(stream));
}

// OHEM cross-entropy: the tensors of the segmentation loss.  Pixels are counted with an int, as above.
static int seg_ohem_args_ok(int B, int C, int H, int W, int dtype) {
    const int rc = loss_dtype_ok(dtype);
    if (rc) return rc;
    if (B < 0 || C < 1 || H <= 0 || W <= 0) return CERB_EINVAL;
    if (C < 2 || static_cast<int64_t>(B) * H * W > 0x7fffffff - 1024) return CERB_EUNSUPPORTED;
    return CERB_OK;
}

int64_t cerberus_seg_ohem_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || static_cast<int64_t>(B) * H * W > 0x7fffffff - 1024) return 0;
    return seg_ohem_workspace_bytes(B, H, W);
}

int cerberus_seg_ohem_forward(const void *logits, const void *target, const void *weight, void *loss, void *prob, void *lse,
                              void *state, void *counts, void *workspace, int64_t workspace_bytes, int B, int C, int H, int W,
                              int64_t ignore_index, float thresh, int64_t min_kept, int dtype, void *stream) {
    const int rc = seg_ohem_args_ok(B, C, H, W, dtype);
    if (rc) return rc;
    if (thresh != thresh) return CERB_EINVAL;
    if (B == 0) return CERB_OK;
    if (!logits || !target || !weight || !loss || !prob || !lse || !state || !counts || !workspace) return CERB_EINVAL;
    if (workspace_bytes < seg_ohem_workspace_bytes(B, H, W) || (reinterpret_cast<uintptr_t>(workspace) & 15)) return CERB_EINVAL;
    return seg_ohem_forward(logits, target, weight, loss, prob, lse, state, counts, workspace, B, C, H, W, ignore_index, thresh,
                            min_kept, static_cast<hipStream_t>(stream));
}

int cerberus_seg_ohem_backward(const void *logits, const void *target, const void *weight, const void *prob, const void *lse,
                               const void *state, const void *grad_loss, void *grad_logits, int B, int C, int H, int W,
                               int64_t ignore_index, int dtype, void *stream) {
    const int rc = seg_ohem_args_ok(B, C, H, W, dtype);
    if (rc) return rc;
    if (B == 0) return CERB_OK;
    if (!logits || !target || !weight || !prob || !lse || !state || !grad_loss || !grad_logits) return CERB_EINVAL;
    return seg_ohem_backward(logits, target, weight, prob, lse, state, grad_loss, grad_logits, B, C, H, W, ignore_index,
                             static_cast<hipStream_t>(stream));
}

int cerberus_seg_ohem_digit_bits(int digit) { return seg_ohem_digit_bits(digit); }
int cerberus_seg_ohem_bins(void) { return seg_ohem_bins(); }

// the supervised depth loss: prediction (B,h,w), ground truth (B,H,W), fp32.  Pixels of the prediction are counted with an int
// (a workgroup's last pixel index may run 1023 past the end before it is tested); offsets into the ground truth are 64-bit.
static int inv_huber_args_ok(int B, int h, int w, int H, int W, int dtype) {
    const int rc = loss_dtype_ok(dtype);
    if (rc) return rc;
    if (B < 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return CERB_EINVAL;
    if (H % h != 0 || W % w != 0) return CERB_EUNSUPPORTED;     // the caller resizes the ground truth for any other ratio
    if (static_cast<int64_t>(B) * h * w > 0x7fffffff - 1024) return CERB_ETOOLARGE;
    return CERB_OK;
}

int64_t cerberus_inv_huber_workspace_bytes(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0 || static_cast<int64_t>(B) * h * w > 0x7fffffff - 1024) return 0;
    return inv_huber_workspace_bytes(B, h, w);
}

int cerberus_inv_huber_forward(const void *pred, const void *gt, void *loss, void *state, void *workspace, int64_t workspace_bytes,
                               int B, int h, int w, int H, int W, int dtype, void *stream) {
    const int rc = inv_huber_args_ok(B, h, w, H, W, dtype);
    if (rc) return rc;
    if (B == 0) return CERB_OK;
    if (!pred || !gt || !loss || !state || !workspace) return CERB_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return CERB_EINVAL;
    if (workspace_bytes < inv_huber_workspace_bytes(B, h, w)) return CERB_EINVAL;
    return inv_huber_forward(pred, gt, loss, state, workspace, B, h, w, H, W, static_cast<hipStream_t>(stream));
}

int cerberus_inv_huber_backward(const void *pred, const void *gt, const void *state, const void *grad_loss, void *grad_pred, int B,
                                int h, int w, int H, int W, int dtype, void *stream) {
    const int rc = inv_huber_args_ok(B, h, w, H, W, dtype);
    if (rc) return rc;
    if (B == 0) return CERB_OK;
    if (!pred || !gt || !state || !grad_loss || !grad_pred) return CERB_EINVAL;
    return inv_huber_backward(pred, gt, state, grad_loss, grad_pred, B, h, w, H, W, static_cast<hipStream_t>(stream));
}

// the training metrics: one image's pixels are counted with an int (a workgroup's last pixel index may run 1023 past the end
// before it is tested), the image is the launch grid's second dimension; offsets into the tensors are 64-bit.
static int metric_args_ok(int B, int C, int H, int W, int min_channels, int dtype) {
    const int rc = loss_dtype_ok(dtype);
    if (rc) return rc;
    if (B < 0 || C < min_channels || H <= 0 || W <= 0) return CERB_EINVAL;
    if (static_cast<int64_t>(H) * W > 0x7fffffff - 1024 || B > 65535) return CERB_ETOOLARGE;
    return CERB_OK;
}

static bool metric_size_ok(int B, int H, int W) {
    return B > 0 && B <= 65535 && H > 0 && W > 0 && static_cast<int64_t>(H) * W <= 0x7fffffff - 1024;
}

static int metric_workspace_ok(const void *workspace, int64_t have, int64_t need) {
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) || have < need) return CERB_EINVAL;
    return CERB_OK;
}

int cerberus_seg_confusion(const void *logits, const void *target, void *confusion, int B, int C, int H, int W, int64_t ignore_index,
                           int dtype, void *stream) {
    const int rc = metric_args_ok(B, C, H, W, 2, dtype);
    if (rc) return rc;
    if (C > seg_confusion_max_classes()) return CERB_EUNSUPPORTED;          // the C*C bins of a workgroup live in LDS
    if (B == 0) return CERB_OK;
    if (!logits || !target || !confusion) return CERB_EINVAL;
    return seg_confusion(logits, target, confusion, B, C, H, W, ignore_index, static_cast<hipStream_t>(stream));
}

int64_t cerberus_depth_metric_workspace_bytes(int B, int h, int w) {
    return metric_size_ok(B, h, w) ? depth_metric_workspace_bytes(B, h, w) : 0;
}

int cerberus_depth_metric_sums(const void *pred, const void *gt, void *sums, void *counts, void *workspace, int64_t workspace_bytes,
                               int B, int h, int w, float min_depth, float max_depth, int dtype, void *stream) {
    const int rc = metric_args_ok(B, 1, h, w, 1, dtype);
    if (rc) return rc;
    if (!(min_depth < max_depth)) return CERB_EINVAL;                     // a NaN bound too
    if (B == 0) return CERB_OK;
    if (!pred || !gt || !sums || !counts) return CERB_EINVAL;
    if (metric_workspace_ok(workspace, workspace_bytes, depth_metric_workspace_bytes(B, h, w))) return CERB_EINVAL;
    return depth_metric_sums(pred, gt, sums, counts, workspace, B, h, w, min_depth, max_depth, static_cast<hipStream_t>(stream));
}

int64_t cerberus_flow_metric_workspace_bytes(int B, int H, int W) {
    return metric_size_ok(B, H, W) ? flow_metric_workspace_bytes(B, H, W) : 0;
}

int cerberus_flow_metric_sums(const void *flow_pred, const void *flow_gt, const void *mask, void *sums, void *counts, void *workspace,
                              int64_t workspace_bytes, int B, int H, int W, int dtype, void *stream) {
    const int rc = metric_args_ok(B, 2, H, W, 2, dtype);
    if (rc) return rc;
    if (B == 0) return CERB_OK;
    if (!flow_pred || !flow_gt || !mask || !sums || !counts) return CERB_EINVAL;
    if (metric_workspace_ok(workspace, workspace_bytes, flow_metric_workspace_bytes(B, H, W))) return CERB_EINVAL;
    return flow_metric_sums(flow_pred, flow_gt, mask, sums, counts, workspace, B, H, W, static_cast<hipStream_t>(stream));
}

int64_t cerberus_warp_sad_workspace_bytes(int B, int H, int W) {
    return metric_size_ok(B, H, W) ? warp_sad_workspace_bytes(B, H, W) : 0;
}

int cerberus_warp_sad(const void *image, const void *source, const void *flow, void *sad, void *workspace, int64_t workspace_bytes,
                      int B, int C, int H, int W, int dtype, void *stream) {
    const int rc = metric_args_ok(B, C, H, W, 1, dtype);
    if (rc) return rc;
    if (B == 0) return CERB_OK;
    if (!image || !source || !flow || !sad) return CERB_EINVAL;
    if (metric_workspace_ok(workspace, workspace_bytes, warp_sad_workspace_bytes(B, H, W))) return CERB_EINVAL;
    return warp_sad(image, source, flow, sad, workspace, B, C, H, W, static_cast<hipStream_t>(stream));
}

// the panoptic metric: fp32 heat map and offsets, int64 centres, counts, ids and classes.  The size limits are the metrics'
// (an image's pixels are counted with an int, the image is a dimension of the launch grid).
int cerberus_center_peaks_max_kernel(void) { return center_peaks_max_kernel(); }
int cerberus_group_pixels_max_centers(void) { return group_pixels_max_centers(); }
int cerberus_instance_overlap_max_bins(void) { return instance_overlap_max_bins(); }

int cerberus_center_peaks(const void *heatmap, void *out, int B, int H, int W, float threshold, int nms_kernel, int dtype,
                          void *stream) {
    const int rc = metric_args_ok(B, 1, H, W, 1, dtype);
    if (rc) return rc;
    if (nms_kernel < 1 || nms_kernel % 2 == 0 || nms_kernel > center_peaks_max_kernel()) return CERB_EINVAL;
    if (H > 65535 * 16) return CERB_ETOOLARGE;                              // 16-row tiles are the grid's second dimension
    if (B == 0) return CERB_OK;
    if (!heatmap || !out) return CERB_EINVAL;
    return center_peaks(heatmap, out, B, H, W, threshold, nms_kernel, static_cast<hipStream_t>(stream));
}

int cerberus_group_pixels(const void *offsets, const void *centers, const void *counts, const void *sem, void *out, int B, int H,
                          int W, int max_centers, uint64_t thing_mask, int dtype, void *stream) {
    const int rc = metric_args_ok(B, 2, H, W, 2, dtype);
    if (rc) return rc;
    if (max_centers < 1) return CERB_EINVAL;
    if (max_centers > group_pixels_max_centers()) return CERB_EUNSUPPORTED;    // the caller takes the stock ops there
    if (B == 0) return CERB_OK;
    if (!offsets || !centers || !counts || !out) return CERB_EINVAL;           // sem may be null: every pixel is a thing
    return group_pixels(offsets, centers, counts, sem, out, B, H, W, max_centers, thing_mask, static_cast<hipStream_t>(stream));
}

int cerberus_instance_overlap(const void *pred_inst, const void *tgt_inst, const void *pred_seg, const void *tgt_seg, void *inter,
                              void *pred_cls, void *tgt_cls, int B, int H, int W, int max_ids, int num_classes, void *stream) {
    const int rc = metric_args_ok(B, 1, H, W, 1, CERB_F32);
    if (rc) return rc;
    if (max_ids < 1 || num_classes < 1) return CERB_EINVAL;
    if (static_cast<int64_t>(max_ids) * (static_cast<int64_t>(max_ids) + 2 * static_cast<int64_t>(num_classes)) >
        instance_overlap_max_bins())
        return CERB_EUNSUPPORTED;                                            // a workgroup's bins live in LDS
    if (B == 0) return CERB_OK;
    if (!pred_inst || !tgt_inst || !pred_seg || !tgt_seg || !inter || !pred_cls || !tgt_cls) return CERB_EINVAL;
    return instance_overlap(pred_inst, tgt_inst, pred_seg, tgt_seg, inter, pred_cls, tgt_cls, B, H, W, max_ids, num_classes,
                            static_cast<hipStream_t>(stream));
}

// the RMI loss: logits (B,C,H,W) fp32, labels (B,H,W) int64.  The image is the launch grid's third dimension and the class
// groups its second; a class is kept in 16 bits; one image's pixels are counted with an int.
static int rmi_args_ok(int B, int C, int H, int W, int radius, int pool, int dtype) {
    const int rc = loss_dtype_ok(dtype);
    if (rc) return rc;
    if (B < 0 || C < 1 || H <= 0 || W <= 0 || radius < 1 || pool < 1) return CERB_EINVAL;
    if (radius != 3 || pool > rmi_max_pool()) return CERB_EUNSUPPORTED;      // the caller takes the stock ops there
    if (static_cast<int64_t>(H) * W > 0x7fffffff - 1024 || B > 65535 || C > 32767) return CERB_ETOOLARGE;
    int h, w;
    if (!rmi_pooled_size(H, W, pool, &h, &w)) return CERB_EUNSUPPORTED;       // no 3 x 3 slice fits the pooled map
    if (rmi_moment_workgroups(B, C, H, W, pool) > 0x7fffffff) return CERB_ETOOLARGE;
    return CERB_OK;
}

int64_t cerberus_rmi_workspace_bytes(int B, int C, int H, int W, int pool) {
    if (rmi_args_ok(B, C, H, W, 3, pool, CERB_F32) || B == 0) return 0;
    return rmi_workspace_bytes(B, C, H, W, pool);
}

int cerberus_rmi_forward(const void *logits, const void *target, void *bce, void *state, void *la_map, void *pr_map, void *means,
                         void *la_cov, void *pr_cov, void *la_pr_cov, void *workspace, int64_t workspace_bytes, int B, int C, int H,
                         int W, int radius, int pool, int do_rmi, int dtype, void *stream) {
    const int rc = rmi_args_ok(B, C, H, W, radius, pool, dtype);
    if (rc) return rc;
    if (B == 0) return CERB_OK;
    if (!logits || !target || !bce || !state || !workspace) return CERB_EINVAL;
    if (do_rmi && (!la_map || !pr_map || !means || !la_cov || !pr_cov || !la_pr_cov)) return CERB_EINVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) || workspace_bytes < rmi_workspace_bytes(B, C, H, W, pool)) return CERB_EINVAL;
    return rmi_forward(logits, target, bce, state, la_map, pr_map, means, la_cov, pr_cov, la_pr_cov, workspace, B, C, H, W, pool,
                       do_rmi != 0, static_cast<hipStream_t>(stream));
}

int cerberus_rmi_backward(const void *logits, const void *target, const void *state, const void *la_map, const void *pr_map,
                          const void *means, const void *grad_bce, const void *grad_pr_cov, const void *grad_la_pr_cov,
                          void *grad_logits, int B, int C, int H, int W, int radius, int pool, int do_rmi, int dtype, void *stream) {
    const int rc = rmi_args_ok(B, C, H, W, radius, pool, dtype);
    if (rc) return rc;
    if (B == 0) return CERB_OK;
    if (!logits || !target || !state || !grad_bce || !grad_logits) return CERB_EINVAL;
    if (do_rmi && (!la_map || !pr_map || !means || !grad_pr_cov || !grad_la_pr_cov)) return CERB_EINVAL;
    return rmi_backward(logits, target, state, la_map, pr_map, means, grad_bce, grad_pr_cov, grad_la_pr_cov, grad_logits, B, C, H, W,
                        pool, do_rmi != 0, static_cast<hipStream_t>(stream));
}

static int smoothness_args_ok(int B, int Cf, int Ci, int H, int W, int degree, int dtype) {
    const int rc = loss_dtype_ok(dtype);
    if (rc) return rc;
    if (degree != 1 && degree != 2) return CERB_EINVAL;
    if (B <= 0 || Cf <= 0 || Ci <= 0 || H <= degree || W <= degree) return CERB_EINVAL;   // every term needs one element
    return loss_size_ok(B, Cf > Ci ? Cf : Ci, H, W, smoothness_workspace_bytes(B, H, W) / 8);
}

int64_t cerberus_edge_smoothness_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return smoothness_workspace_bytes(B, H, W);
}

int cerberus_edge_smoothness_forward(const void *flow, const void *image, void *loss, void *workspace, int64_t workspace_bytes,
                                     int B, int flow_channels, int image_channels, int H, int W, float alpha, int degree,
                                     int dtype, void *stream) {
    const int rc = smoothness_args_ok(B, flow_channels, image_channels, H, W, degree, dtype);
    if (rc) return rc;
    if (!flow || !image || !loss || !workspace) return CERB_EINVAL;
    if (workspace_bytes < smoothness_workspace_bytes(B, H, W)) return CERB_EINVAL;
    return smoothness_forward(flow, image, loss, workspace, B, flow_channels, image_channels, H, W, alpha, degree,
                              static_cast<hipStream_t>(stream));
}

int cerberus_edge_smoothness_backward(const void *flow, const void *image, const void *grad_loss, void *grad_flow, int B,
                                      int flow_channels, int image_channels, int H, int W, float alpha, int degree, int dtype,
                                      void *stream) {
    const int rc = smoothness_args_ok(B, flow_channels, image_channels, H, W, degree, dtype);
    if (rc) return rc;
    if (!flow || !image || !grad_loss || !grad_flow) return CERB_EINVAL;
    return smoothness_backward(flow, image, grad_loss, grad_flow, B, flow_channels, image_channels, H, W, alpha, degree,
                               static_cast<hipStream_t>(stream));
}

int cerberus_set_option(const char *key, int value) {
    if (!key) return CERB_EINVAL;
    const int i = find_option(key);
    if (i < 0) return CERB_EINVAL;
    g_option_values[i].store(value, std::memory_order_relaxed);
    return CERB_OK;
}

int cerberus_get_option(const char *key, int *value) {
    if (!key || !value) return CERB_EINVAL;
    // read-only: 1 when the library was built with -DCERB_EXPERIMENTS (the measured-and-rejected
    // kernel variants the dispatcher never picks exist only in such test builds)
    if (!strcmp(key, "experiments_build")) {
#ifdef CERB_EXPERIMENTS
        *value = 1;
#else
        *value = 0;
#endif
        return CERB_OK;
    }
    const int i = find_option(key);
    if (i < 0) return CERB_EINVAL;
    *value = g_option_values[i].load(std::memory_order_relaxed);
    return CERB_OK;
}

const char *cerberus_last_kernel(int which) { return g_last_kernel[which & 1].load(std::memory_order_relaxed); }

}  // extern "C"
