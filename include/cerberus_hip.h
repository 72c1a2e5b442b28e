/*
 * cerberus_hip.h -- C ABI of libcerberus_hip.so, the MI355X (gfx950) drop-in for
 * CerberusNet's cost-volume correlation + flow-warp hot path.
 *
 * Plain pointers and sizes only: no torch types, no C++ in the signatures.  All
 * tensors are dense, contiguous NCHW device buffers owned by the caller
 * (outputs included: the caller allocates, the library fully overwrites them).
 * Every entry point enqueues asynchronously on `stream` (a hipStream_t passed
 * as void*, NULL = default stream), never synchronises, allocates nothing
 * (scratch, where needed, is a caller-provided workspace), keeps no per-call state
 * (re-entrant: autograd may call backward from its own engine thread; the only process-wide
 * state is atomic: the tuning knobs below and a per-device "large LDS opted in" mask) and is
 * therefore safe to capture into a hipGraph.
 *
 * Return value: 0 on success; a negative CERB_E* code for rejected arguments;
 * a positive value is the hipError_t reported by the launch.
 * cerberus_error_string() turns either into text.
 *
 * Reference interfaces these replace (paths under /root/reference/):
 *   nnet_training/correlation_package/correlation_cuda.cpp:3-26   correlation_forward_cuda
 *   nnet_training/correlation_package/correlation_cuda.cpp:28-43  correlation_backward_cuda
 *   nnet_training/correlation_package/correlation_cuda_kernel.cuh:5-14 (kernel launchers)
 *   nnet_training/loss_functions/UnFlowLoss.py:83-94              flow_warp (-> ATen grid_sampler_2d fwd/bwd)
 * The Python binding that registers torch.ops.cerberus.{correlation,
 * correlation_backward} on top of this ABI is cerberusnet_amd/ops.py; the
 * reference-side stub a maintainer would add is shown in INTEGRATION.md.
 */
#ifndef CERBERUS_HIP_H
#define CERBERUS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CERBERUS_HIP_ABI_VERSION 7   /* 7: cerberus_warp_correlation_forward (f2), option warp_pair16 (round 6); 6: cerberus_correlation_backward_ex, cerberus_area_pyramid, option warp_fewc (round 5) */

/* element types (AT_DISPATCH_FLOATING_TYPES_AND_HALF in the reference,
 * correlation_cuda_kernel.cu:269,303; bf16 is an extension) */
enum cerb_dtype {
    CERB_F32  = 0,
    CERB_F16  = 1,  /* fp16 storage, fp32 accumulation (reference accumulates in fp16: Q6) */
    CERB_BF16 = 2,  /* bf16 storage, fp32 accumulation (not in the reference)             */
    CERB_F64  = 3
};

/* grid_sample modes used by flow_warp(image, flow12, pad='border', mode='bilinear') */
enum cerb_pad_mode    { CERB_PAD_ZEROS = 0, CERB_PAD_BORDER = 1, CERB_PAD_REFLECTION = 2 };
enum cerb_interp_mode { CERB_INTERP_BILINEAR = 0, CERB_INTERP_NEAREST = 1 };

/* argument-rejection codes (negative) */
#define CERB_OK            0
#define CERB_EINVAL       -1  /* null pointer, non-positive size, empty output          */
#define CERB_EDTYPE       -2  /* unknown dtype                                          */
#define CERB_ESTRIDE1     -3  /* correlation backward with stride1 != 1 (reference is   */
                              /* memory-unsafe there, correlation_cuda_kernel.cu:106)   */
#define CERB_EMODE        -4  /* unknown padding / interpolation mode                   */
#define CERB_EUNSUPPORTED -5  /* valid but not implemented (reflection pad in the f2 fused warp) */
#define CERB_ETOOLARGE    -6  /* a dimension exceeds 32-bit launch / index limits       */

/* Pointer alignment (tests/test_alignment_gpu.py):
 *   Tensor pointers -- inputs, outputs, gradients -- need the alignment of their element type and no more.  The
 *   correlation, flow_warp and flow_upsample calls test each pointer and take their vector / LDS-DMA / matrix-core kernels
 *   where the pointers allow it: 16 bytes on every tensor for fp32; 8 bytes for fp16 / bf16 (16 on input1 and input2 for
 *   the matrix-core forward's column walk).  flow_warp with a 16-bit image: 16 bytes on image and grad_image, 8 on out, 4 on
 *   grad_out, and 8 on flow and grad_flow whatever the flow's type (fp32 or 16-bit); with an fp32 image: 16 on image and
 *   grad_image.  Any other pointer takes a slower kernel: the result stays within the same bound of the reference, and has
 *   the same bits wherever the kernel is the same.  What torch's allocator returns passes every test.
 *   A warp context must be 16-byte aligned: CERB_EINVAL otherwise, before any launch.  A workspace must be 16-byte aligned
 *   unless its comment names less, and is rejected with CERB_EINVAL otherwise, with two exceptions that fall back instead
 *   and return CERB_OK: cerberus_flow_warp_backward treats a workspace that is misaligned or too small as no workspace
 *   (without a context: the scatter kernel, global float atomics, grad_image's summation order not fixed), and
 *   cerberus_warp_correlation_forward takes its one-launch form. */

int cerberus_abi_version(void);

/* Human-readable text for a return code of any function below. */
const char *cerberus_error_string(int code);

/* Output geometry, exactly correlation_cuda.cpp:6-14:
 *   oC = ((d/s2)*2+1)^2, oH = ceil((H+2p-2(kr+d))/s1), oW likewise, kr=(k-1)/2. */
int cerberus_correlation_out_shape(int H, int W, int pad_size, int kernel_size,
                                   int max_displacement, int stride1,
                                   int stride2, int *out_channels,
                                   int *out_height, int *out_width);

/* correlation forward.  Replaces correlation_forward_cuda
 * (correlation_cuda.cpp:3-26 -> correlation_cuda_kernel.cu:244-324).
 *   input1,input2 : (B,C,H,W)      output : (B,oC,oH,oW), fully overwritten
 *   out[n][(tj+dr)*D+(ti+dr)][y][x] = 1/(k*k*C) * sum_{j,i in kernel} sum_c
 *        pad(in1)[n][c][y*s1+d+j][x*s1+d+i] * pad(in2)[n][c][y*s1+d+tj*s2+j][x*s1+d+ti*s2+i]
 * corr_type_multiply is accepted and ignored, as in the reference. */
int cerberus_correlation_forward(const void *input1, const void *input2,
                                 void *output, int B, int C, int H, int W,
                                 int pad_size, int kernel_size,
                                 int max_displacement, int stride1, int stride2,
                                 int corr_type_multiply, int dtype,
                                 void *stream);

/* Same, with the consumer's epilogue fused (the caller
 * pwcnet_sfd.py:181-187 applies leaky_relu(0.1) in place and concatenates):
 *   out = v > 0 ? v : v * negative_slope   (negative_slope = 1.0f -> identity)
 *   written at output + n*out_batch_stride elements (out_batch_stride = 0 means
 *   dense oC*oH*oW), so the 81 channels can land inside a wider concat buffer. */
int cerberus_correlation_forward_ex(const void *input1, const void *input2,
                                    void *output, int B, int C, int H, int W,
                                    int pad_size, int kernel_size,
                                    int max_displacement, int stride1,
                                    int stride2, float negative_slope,
                                    int64_t out_batch_stride, int dtype,
                                    void *stream);

/* correlation backward.  Replaces correlation_backward_cuda
 * (correlation_cuda.cpp:28-43 -> correlation_cuda_kernel.cu:326-429).
 *   grad_output : (B,oC,oH,oW)   grad_input1, grad_input2 : (B,C,H,W), fully
 *   overwritten (zeros where the reference's kernels early-return).
 *   Requires stride1 == 1 (CERB_ESTRIDE1 otherwise). */
int cerberus_correlation_backward(const void *input1, const void *input2,
                                  const void *grad_output, void *grad_input1,
                                  void *grad_input2, int B, int C, int H, int W,
                                  int pad_size, int kernel_size,
                                  int max_displacement, int stride1,
                                  int stride2, int corr_type_multiply,
                                  int dtype, void *stream);

/* Same, for the gradient of the buffer cerberus_correlation_forward_ex wrote into (round 5; the caller
 * pwcnet_sfd.py:181-187, seen from autograd: the cost volume is channels [0, oC) of the estimator's
 * concatenation buffer, with leaky_relu already applied):
 *   grad_output item n starts at grad_output + n * grad_out_batch_stride elements (0 = dense oC*oH*oW);
 *   its oC planes are contiguous.
 *   fwd_output (may be NULL): the volume the forward stored, item n at fwd_output + n *
 *   fwd_out_batch_stride (0 = dense).  The gradient the kernels see is
 *       g_eff = fwd_output > 0 ? g : g * negative_slope
 *   -- the derivative of the forward's fused LeakyReLU, taken from the stored value's sign (a positive
 *   slope keeps the sign; a NaN stored value takes the slope branch, as torch.where(out > 0, g, g * slope)).
 *   workspace: cerberus_correlation_backward_ex_workspace_bytes() bytes, 16-byte aligned, caller-owned,
 *   needed whenever the gradient is strided or masked (one pass writes the dense g_eff there; the backward
 *   kernels stream gradOutput by LDS-DMA and cannot apply a mask on the way).  With a dense gradient and
 *   fwd_output == NULL this is cerberus_correlation_backward and the workspace is not touched. */
int64_t cerberus_correlation_backward_ex_workspace_bytes(int B, int H, int W, int pad_size,
                                                         int kernel_size, int max_displacement,
                                                         int stride1, int stride2, int dtype);
int cerberus_correlation_backward_ex(const void *input1, const void *input2,
                                     const void *grad_output, int64_t grad_out_batch_stride,
                                     const void *fwd_output, int64_t fwd_out_batch_stride,
                                     float negative_slope, void *workspace, int64_t workspace_bytes,
                                     void *grad_input1, void *grad_input2, int B, int C, int H, int W,
                                     int pad_size, int kernel_size, int max_displacement, int stride1,
                                     int stride2, int dtype, void *stream);

/* flow_warp forward.  Replaces the body of flow_warp (UnFlowLoss.py:83-94):
 * mesh_grid + flow -> norm_grid by (W-1),(H-1) -> grid_sample(align_corners=False),
 * fused: no grid tensor is materialised.
 *   image : (B,C,H,W)  flow : (B,2,H,W) (ch0 = x, ch1 = y, pixels)  out : (B,C,H,W) */
int cerberus_flow_warp_forward(const void *image, const void *flow, void *out,
                               int B, int C, int H, int W, int pad_mode,
                               int interp_mode, int dtype, void *stream);

/* The same forward, additionally saving what the backward needs again (what autograd's
 * save_for_backward is to the reference's grid_sample): every pixel's sample position and,
 * per 64-pixel strip, the signed range of tap displacements.
 *   context    : caller-owned device buffer of cerberus_flow_warp_context_bytes(B,H,W) bytes
 *                (16-byte aligned, contents irrelevant, fully written); NULL = plain forward.
 *                The layout is private to the library (an opaque blob between the two calls).
 *   flow_dtype : element type of `flow`: equal to `dtype`, or CERB_F32 with a 16-bit image
 *                (under autocast the reference's grid_sample runs in fp32 on whatever
 *                precision the flow arrives in: an fp32 flow is not rounded to 16 bits). */
int64_t cerberus_flow_warp_context_bytes(int B, int H, int W);
int cerberus_flow_warp_forward_ctx(const void *image, const void *flow, void *out,
                                   void *context, int64_t context_bytes, int B, int C,
                                   int H, int W, int pad_mode, int interp_mode,
                                   int dtype, int flow_dtype, void *stream);

/* f2 of SURVEY.md section 8(f): flow_warp FUSED into the correlation forward -- what the reference's head computes at
 * nnet_models/pwcnet_sfd.py:178 -> :181-182 with pad_size = max_displacement = 4, kernel_size = stride1 = stride2 = 1:
 *   output[b][(dy+4)*9 + (dx+4)][y][x] = leaky( mean_c input1[b][c][y][x] * warped[b][c][y+dy][x+dx] ),
 *   warped = flow_warp(input2, flow, pad_mode, bilinear), zero outside the image,
 * without ever writing `warped` (no round trip, nothing to save for the backward: the training path recomputes the warp).
 * Same arithmetic as the two stand-alone calls (the warp's coordinate rounding order; a 16-bit warped value is rounded through
 * the storage type as the stand-alone warp's output is); the channel sum runs in another order (fp32 rounding).
 *   input1, input2 : (B,C,H,W), dtype (CERB_F32 / F16 / BF16);  flow : (B,2,H,W), flow_dtype (= dtype, or CERB_F32)
 *   output         : (B,81,H,W), dtype; batch stride out_batch_stride elements (0 = dense) as in cerberus_correlation_forward_ex
 *   negative_slope : LeakyReLU slope applied to the result (1.0f = none)
 *   workspace      : caller-owned device scratch of cerberus_warp_correlation_workspace_bytes(B,C,H,W) bytes (4-byte aligned,
 *                    contents irrelevant), or NULL.  Only small maps need it (fewer than 256 tiles of 8 x 32 pixels: the channel
 *                    sum is then split over several workgroups per tile, summed with float atomics in an fp32 volume and
 *                    finished by a second launch: results agree to fp32 rounding run to run, not bit for bit); without it
 *                    such a map takes the one-launch form (bit-reproducible, few workgroups).
 * Built in round 6 so that the row exists as code; measured SLOWER than the two tuned launches (bench.py extra.f2_fused): opt-in. */
int64_t cerberus_warp_correlation_workspace_bytes(int B, int C, int H, int W);
int cerberus_warp_correlation_forward(const void *input1, const void *input2, const void *flow, void *output, void *workspace,
                                      int64_t workspace_bytes, int B, int C, int H, int W, int pad_mode, float negative_slope,
                                      int64_t out_batch_stride, int dtype, int flow_dtype, void *stream);

/* flow_warp backward (autograd of the above w.r.t. image and flow).
 *   grad_image : (B,C,H,W), dtype -- fully overwritten.  With a context or a workspace
 *                (fp32 / fp16 / bf16): built tile by tile in LDS in 64-bit fixed point, no
 *                global atomics, bit-reproducible; NaN / Inf in grad_out reach the same
 *                elements as in ATen's scatter.  With neither (or fp64): global float atomics
 *                as ATen's (summation order not fixed).
 *   grad_flow  : (B,2,H,W), flow_dtype -- fully overwritten, deterministic.  With a context or a workspace
 *                it comes from the LDS-window role of the tile launch -- round 6: also when grad_image is NULL
 *                and C > 4 (the bits are the both-gradients call's); with neither, from per-pixel gathers
 *                (another channel-group order: equal within rounding)
 *   context    : the buffer a cerberus_flow_warp_forward_ctx call with the SAME flow,
 *                shape and pad_mode filled, or NULL (the backward then derives it from the
 *                flow with one extra launch, into the workspace).
 *   workspace  : caller-owned device scratch of at least
 *                cerberus_flow_warp_backward_workspace_bytes(B,C,H,W) bytes (16-byte
 *                aligned, contents irrelevant), private to this call until it completes;
 *                only needed when context is NULL.  A workspace that is NULL, too small or not
 *                16-byte aligned is no error: the call then runs as "with neither" above.
 * Every pad_mode x interp_mode pair is differentiable, with ATen's rules (align_corners = false):
 * reflection multiplies the position gradient by the reflection's sign and zeroes it where the
 * reflected position clips onto an edge; nearest adds grad_out to the nearbyint tap (ties to
 * even) and writes grad_flow as exact zeros.
 * Either grad pointer may be NULL to skip that gradient. */
int64_t cerberus_flow_warp_backward_workspace_bytes(int B, int C, int H, int W);
int cerberus_flow_warp_backward(const void *image, const void *flow,
                                const void *grad_out, void *grad_image,
                                void *grad_flow, const void *context,
                                int64_t context_bytes, void *workspace,
                                int64_t workspace_bytes, int B, int C, int H, int W,
                                int pad_mode, int interp_mode, int dtype,
                                int flow_dtype, void *stream);

/* The flow pyramid's upsampling step, fused.  Replaces
 *   F.interpolate(flow * factor, scale_factor=factor, mode='bilinear', align_corners=True)
 * (nnet_training/nnet_models/pwcnet_sfd.py:176 with factor 2, :199-201 with factor 4): one launch
 * instead of a multiply + ATen upsample_bilinear2d; the backward is a deterministic gather
 * instead of ATen's float-atomic scatter.
 *   forward : src (planes, H, W) -> dst (planes, H*factor, W*factor)
 *   backward: src = grad of the upsampled tensor (planes, H*factor, W*factor) -> dst (planes, H, W)
 * planes = B * channels of the contiguous NCHW tensor; factor >= 1; fp32 / fp16 / bf16. */
int cerberus_flow_upsample_forward(const void *src, void *dst, int64_t planes, int H, int W,
                                   int factor, int dtype, void *stream);
int cerberus_flow_upsample_backward(const void *grad_out, void *grad_in, int64_t planes, int H,
                                    int W, int factor, int dtype, void *stream);

/* The photometric loss's image pyramid.  Replaces
 *   F.interpolate(image, (out_h, out_w), mode='area')
 * (nnet_training/loss_functions/UnFlowLoss.py:279-280: the target images resized to every flow
 * scale) = ATen adaptive_avg_pool2d: output (oy, ox) is the mean over rows
 * [floor(oy*H/out_h), ceil((oy+1)*H/out_h)) x the same in x, summed in fp32 in row-major order
 * and divided by the window height, then width (bit-identical to torch's CPU kernel in fp32).
 *   src (planes, H, W) -> dst (planes, out_h, out_w); any sizes >= 1; fp32 / fp16 / bf16.
 * Forward only: the reference applies it to target images, which carry no gradient. */
int cerberus_area_resize(const void *src, void *dst, int64_t planes, int H, int W, int out_h,
                         int out_w, int dtype, void *stream);

/* All scales of that pyramid in one call (round 5): dsts[i] (planes, out_h[i], out_w[i]) for i < n_scales
 * (dsts, out_h, out_w are HOST arrays; dsts[i] device pointers).  When every scale is an integer ratio r in
 * {2, 4, 8, 16, 32, 64} of the source (and n_scales <= 4) ONE launch reads the source once and writes every
 * scale (unFlowLoss resizes each 25 MB target image to every flow scale: UnFlowLoss.py:279-280); otherwise
 * the scales are resized one by one.  Results are bit-identical to cerberus_area_resize either way. */
int cerberus_area_pyramid(const void *src, void *const *dsts, const int *out_h, const int *out_w,
                          int n_scales, int64_t planes, int H, int W, int dtype, void *stream);

/* unFlowLoss's photometric term as ONE differentiable scalar (no ABI bump: additions only).  Replaces, per call,
 * loss_photometric with its all-ones mask (nnet_training/loss_functions/UnFlowLoss.py:236-255) over SSIM
 * (loss_functions.py:47-77): 2 reflection pads, 5 average pools, ~20 elementwise launches and two whole-tensor means.
 *   loss[0] = mean over all B*C*H*W elements of
 *             l1_weight * |im_orig - im_recons| + ssim_weight * clamp((1 - SSIM(im_recons, im_orig)) / 2, 0, 1)
 * SSIM per channel on 3 x 3 windows behind a reflection padding of 1 (row -1 is row 1), C1 = 0.01^2, C2 = 0.03^2.
 * A weight of 0 skips its term (it is not multiplied: a NaN pixel then does not reach the result through it).
 *   im_orig, im_recons : (B,C,H,W) fp32, H, W >= 2        loss : ONE float in device memory, overwritten
 *   workspace          : cerberus_photometric_loss_workspace_bytes(B,C,H,W) bytes (one partial sum per 16 x 64 tile;
 *                        0 for a non-positive size), fully overwritten; no zero-fill needed
 * Forward: a tile kernel (both images + 1-pixel halo in LDS, one partial per workgroup) and a single-workgroup launch
 * that adds the partials in a fixed order: no floating-point atomics, bit-reproducible for a given shape.
 * Backward: grad_recons (B,C,H,W) = grad_loss[0] * d loss / d im_recons, every element written exactly once (no
 * zero-fill, no atomics), recomputed from the two images alone.  grad_loss points to ONE float in DEVICE memory (no
 * host synchronisation: the call can be captured in a graph).  clamp passes the gradient where its argument lies in
 * [0, 1] (bounds included), |.| has gradient 0 at equality (ATen's rules).  The loss is symmetric in the two images:
 * the gradient with respect to im_orig is the same call with the two image pointers exchanged.
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; empty tensors, H or W < 2, a null pointer,
 * a workspace that is too small CERB_EINVAL; C*H*W >= 2^31 CERB_ETOOLARGE -- all before any launch. */
int64_t cerberus_photometric_loss_workspace_bytes(int B, int C, int H, int W);
int cerberus_photometric_loss_forward(const void *im_orig, const void *im_recons, void *loss,
                                      void *workspace, int64_t workspace_bytes, int B, int C, int H,
                                      int W, float l1_weight, float ssim_weight, int dtype,
                                      void *stream);
int cerberus_photometric_loss_backward(const void *im_orig, const void *im_recons,
                                       const void *grad_loss, void *grad_recons, int B, int C, int H,
                                       int W, float l1_weight, float ssim_weight, int dtype,
                                       void *stream);

/* unFlowLoss's edge-aware smoothness term as one differentiable scalar.  Replaces _edge_aware_smoothness
 * (UnFlowLoss.py:162-187), ~15 launches per call:
 *   wx = exp(-alpha * mean_c |image[..., 1:] - image[..., :-1]|), wy likewise along rows
 *   degree 1: loss = (mean(wx * |dx flow| / 2) + mean(wy * |dy flow| / 2)) / 2
 *   degree 2: loss = (mean(wx[..., 1:] * |dx dx flow|) + mean(wy[..., 1:, :] * |dy dy flow|)) / 2
 * (the x and the y term are means over DIFFERENT element counts, then averaged).
 *   flow (B,flow_channels,H,W), image (B,image_channels,H,W), fp32; H, W > degree
 *   workspace : cerberus_edge_smoothness_workspace_bytes(B,H,W) bytes (an x and a y partial per 4 x 64 tile)
 * Same reduction scheme as above.  Backward: grad_flow = grad_loss[0] * d loss / d flow, a pure gather per flow element
 * (it appears in at most degree + 1 differences per axis), every element written once; there is no gradient for the
 * image (a target image).  Errors as above; a degree other than 1 or 2 is CERB_EINVAL. */
int64_t cerberus_edge_smoothness_workspace_bytes(int B, int H, int W);
int cerberus_edge_smoothness_forward(const void *flow, const void *image, void *loss, void *workspace,
                                     int64_t workspace_bytes, int B, int flow_channels,
                                     int image_channels, int H, int W, float alpha, int degree,
                                     int dtype, void *stream);
int cerberus_edge_smoothness_backward(const void *flow, const void *image, const void *grad_loss,
                                      void *grad_flow, int B, int flow_channels, int image_channels,
                                      int H, int W, float alpha, int degree, int dtype, void *stream);

/* unFlowLoss's census ("ternary") term as one differentiable scalar (additions only: no ABI bump).  Replaces
 * TernaryLoss(im, im_warp, max_distance).mean() (UnFlowLoss.py:119-156 and :237-239 with its all-ones mask): a grayscale
 * conversion, an identity-kernel conv2d into K = (2 max_distance + 1)^2 planes, ~10 elementwise launches per image over
 * those planes, a channel mean, a mask multiply and a whole-tensor mean.
 *   gray = 255 (0.2989 R + 0.5870 G + 0.1140 B);  for every offset o of the window  x_o(q) = gray(q + o) - gray(q),
 *   t_o = x_o / sqrt(0.81 + x_o^2);  D_o = (t_o(im) - t_o(im_warp))^2;  dist(q) = (1 / K) sum_o D_o / (0.1 + D_o)
 *   loss[0] = sum of dist(q) over max_distance <= y < H - max_distance, max_distance <= x < W - max_distance, / (B*H*W)
 * (the mean keeps the masked border in its denominator, as the reference's does).
 *   im, im_warp : (B,3,H,W) fp32; max_distance 1, 2 or 3; H, W >= 2 max_distance + 1
 *   loss        : ONE float in device memory, overwritten
 *   workspace   : cerberus_census_loss_workspace_bytes(B,H,W) bytes (one partial sum per 16 x 64 tile of every batch
 *                 item; 0 for a non-positive size), fully overwritten; no zero-fill needed
 * Forward: a tile kernel (the GRAY planes of both images + a halo of max_distance in LDS, one partial per workgroup) and
 * the single-workgroup fixed-order sum of the photometric op: no floating-point atomics, bit-reproducible for a given
 * shape.  The mask selects: a NaN in any pixel reaches the result through an interior neighbour, a masked pixel adds 0.
 * Backward: grad_warp (B,3,H,W) = grad_loss[0] * d loss / d im_warp, every element written exactly once (no zero-fill,
 * no atomics), recomputed from the two images; grad_loss points to ONE float in DEVICE memory (no host synchronisation:
 * capturable).  The loss is symmetric in the two images: the gradient with respect to im is the same call with the two
 * image pointers exchanged.
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; max_distance outside 1..3, B <= 0, H or W
 * < 2 max_distance + 1, a null pointer, a workspace that is too small CERB_EINVAL; 3*H*W >= 2^31 CERB_ETOOLARGE -- all
 * before any launch. */
int64_t cerberus_census_loss_workspace_bytes(int B, int H, int W);
int cerberus_census_loss_forward(const void *im, const void *im_warp, void *loss, void *workspace,
                                 int64_t workspace_bytes, int B, int H, int W, int max_distance,
                                 int dtype, void *stream);
int cerberus_census_loss_backward(const void *im, const void *im_warp, const void *grad_loss,
                                  void *grad_warp, int B, int H, int W, int max_distance, int dtype,
                                  void *stream);

/* unFlowLoss's occlusion masks (additions only: no ABI bump): forward-only ops, fp32, no gradient of any kind (the masks
 * are constants of the loss).
 *
 * cerberus_corresponding_map: get_corresponding_map (UnFlowLoss.py:34-81), the bilinear forward splat of ones.
 *   data : (B,2,H,W) fp32.  is_flow = 0: absolute target coordinates (channel 0 = x, 1 = y), the reference's argument;
 *          is_flow = 1: a flow; the target is pixel + flow, formed in fp32 by the kernel (get_occu_mask_backward, :108-117)
 *   map  : (B,1,H,W) fp32, overwritten: for every source pixel the taps floor / floor + 1 of its target (x, y) receive
 *          (1 - |x - xt|)(1 - |y - yt|); a tap outside the map is dropped, judged on the unclamped integer.
 *   workspace : cerberus_corresponding_map_workspace_bytes(B,H,W) = 8 B H W bytes (0 for a non-positive size), zeroed on
 *          the stream by the call itself (a kernel: capturable, no host synchronisation).
 * Sums are 64-bit integers of weights scaled by the constant 2^33 and rounded (a weight lies in [0, 1]; at most 2^-34
 * per tap, nothing for weights >= 2^-10): integer adds commute, so two runs give the same bits, eager or replayed from a
 * graph; there are no floating-point atomics.  A pixel that receives every source holds less than H*W * 2^33 < 2^63: no
 * wrap (H*W < 2^30 is enforced).  NaN and +-Inf positions contribute nothing (in the reference +-Inf contributes nothing and NaN is undefined
 * behaviour); positions of any magnitude are dropped by a range test in fp32 before any index is formed.
 *
 * cerberus_occlusion_mask_bidirection: get_occu_mask_bidirection (:96-106) in one launch.
 *   flow12, flow21 : (B,2,H,W) fp32;  mask : (B,1,H,W) fp32 of 0 / 1, overwritten
 *   w = flow21 sampled where cerberus_flow_warp_forward(flow21, flow12, CERB_PAD_ZEROS, CERB_INTERP_BILINEAR) samples it
 *   (the same bits; the warped flow is never written);  mask = |flow12 + w|^2 > scale (|flow12|^2 + |w|^2) + bias.
 *   An IEEE comparison: a NaN in any of a pixel's terms gives 0 there.
 *
 * Errors (both): unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; B, H or W <= 0, a null pointer, an
 * is_flow other than 0 / 1, a workspace that is too small CERB_EINVAL; H or W > 2^24 or 2*H*W >= 2^31 CERB_ETOOLARGE --
 * all before any launch. */
int64_t cerberus_corresponding_map_workspace_bytes(int B, int H, int W);
int cerberus_corresponding_map(const void *data, void *map, void *workspace, int64_t workspace_bytes,
                               int B, int H, int W, int is_flow, int dtype, void *stream);
int cerberus_occlusion_mask_bidirection(const void *flow12, const void *flow21, void *mask, int B, int H,
                                        int W, float scale, float bias, int dtype, void *stream);

/* The stereo reprojection warp of the depth reconstruction loss (additions only: no ABI bump): BackprojectDepth, Project3D
 * and F.grid_sample(l_img, pix_coords, padding_mode="border") of DepthReconstructionLossV1 (depth_losses.py:112-206) as one
 * launch each way, fp32.
 *   image : (B,C,H,W), any C >= 1; a target image: it gets no gradient
 *   depth : (B,1,H,W)
 *   inv_K : (B,3,3) row-major, the upper-left 3 x 3 of the inverse intrinsics;  proj : (B,3,4) row-major, (K @ T)[:, :3, :].
 *           Both in DEVICE memory, read by the kernels (no host copy, no synchronisation: capturable).
 *   out   : (B,C,H,W), overwritten.  Pixel (x, y) samples the image at the position
 *             u = inv_K . (x, y, 1);  p = proj . (depth * u, 1);  px = p.x / (p.z + eps),  py = p.y / (p.z + eps)
 *           normalised as (px / (W - 1) - 0.5) * 2 and sampled with align_corners=False, border padding, bilinear: the sampling
 *           rule of cerberus_flow_warp_forward(.., CERB_PAD_BORDER, CERB_INTERP_BILINEAR) at the flow (px - x, py - y).
 *           Each step is rounded on its own, in the reference's order.  Positions are never written.
 *   grad_depth : (B,1,H,W), every element written exactly once = sum_c grad_out[c] * d out[c] / d depth; a gather that
 *           recomputes the positions: no atomics, no workspace, the same bits from run to run.  0 where the border clip holds
 *           the position (ATen's rule).
 * A NaN position gives NaN at that pixel only (the warp's rule); +-Inf positions are clipped to the border.  Nothing outside
 * the tensors is read or written whatever the depth holds.
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; B or C <= 0, H or W < 2, B*C*H*W >= 2^31, a null
 * pointer CERB_EINVAL -- all before any launch. */
int cerberus_reproject_warp_forward(const void *image, const void *depth, const void *inv_K, const void *proj,
                                    void *out, int B, int C, int H, int W, float eps, int dtype, void *stream);
int cerberus_reproject_warp_backward(const void *image, const void *depth, const void *inv_K, const void *proj,
                                     const void *grad_out, void *grad_depth, int B, int C, int H, int W, float eps,
                                     int dtype, void *stream);

/* The segmentation head's loss as one differentiable scalar (additions only: no ABI bump): FocalLoss2D / SegCrossEntropy
 * (seg_losses.py:121-190), that is F.cross_entropy(logits, target, weight=w, ignore_index=i) reduced to a mean, times the
 * focal factor of that MEAN (the reference applies it to the scalar, :150-154).
 *   logits : (B,C,H,W) fp32, C >= 2, any C (the kernels stream over the classes);  target : (B,H,W) int64;
 *   weight : (C,) fp32, in DEVICE memory;  ignore_index : any integer;  gamma >= 0
 *   valid(p) = target(p) != ignore_index;  lse(p) = log sum_c exp(x_c(p)) (max-subtracted, expf / logf)
 *   num = sum_{valid p} w[t(p)] (lse(p) - x_t(p));  den = sum_{valid p} w[t(p)];  ce = num / den
 *   loss[0] = ce for gamma == 0 (exactly), else (1 - exp(-ce))^gamma * ce
 *   lse    : (B,H,W) fp32, overwritten (every pixel, ignored ones too): the backward reads it instead of a second pass
 *   state  : 4 floats, overwritten: [ce, den, (dloss/dce) / den, 0], read by the backward on the device
 *   workspace : cerberus_seg_cross_entropy_workspace_bytes(B,H,W) bytes (a num and a den partial per 1024 pixels; 0 for a
 *            non-positive or too large size), fully overwritten; no zero-fill needed
 * Forward: one pass over the logits (a lane owns 4 consecutive pixels and loads 16 bytes per class plane when H*W % 4 == 0
 * and logits, target and lse are 16-byte aligned; one pixel per lane otherwise -- both routes give the same bits) and a
 * single-workgroup fixed-order sum: no floating-point atomics, bit-reproducible for a given shape.
 * Backward: grad_logits (B,C,H,W) = grad_loss[0] * state[2] * w[t] * (softmax - onehot), every element written exactly once
 * (no zero-fill); exactly 0.0f at ignored pixels, at out-of-range labels and at pixels of weight 0 (a select: also when
 * state[2] is NaN).  grad_loss points to ONE float in DEVICE memory (no host synchronisation: capturable).
 * Every valid pixel ignored, or den == 0: loss NaN (0 / 0, as stock), gradient all zeros.  A NaN logit at a valid pixel
 * gives a NaN loss; at an ignored pixel it changes nothing.  A label outside [0, C) that is not ignore_index never forms
 * an address: it adds NaN to num (stock PyTorch raises a device-side assertion) and its gradient is zeros.
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; B < 0, C < 2, H or W <= 0, gamma < 0 or NaN
 * CERB_EINVAL; B*H*W > 2^31 - 1025 CERB_ETOOLARGE; then B == 0 returns 0 without a launch; a null pointer, a workspace that
 * is too small CERB_EINVAL -- all before any launch.
 *
 * cerberus_class_histogram: counts[c] = the number of labels equal to c, for c in [0, num_classes) other than ignore_index
 * (the counts of the reference's dynamic class weights, :144-147, without unique()).
 *   target : `count` int64 labels;  counts : num_classes int64, zeroed on the stream by the call itself (a kernel: capturable) and
 *   added to with integer adds (LDS per workgroup, then global): any order, the same result.  Labels outside
 *   [0, num_classes) are not counted.
 * Errors: count < 0, num_classes < 1 CERB_EINVAL; num_classes > 2048 CERB_EUNSUPPORTED; count > 2^40 CERB_ETOOLARGE; then
 * count == 0 returns 0 and touches nothing; a null pointer CERB_EINVAL. */
int64_t cerberus_seg_cross_entropy_workspace_bytes(int B, int H, int W);
int cerberus_seg_cross_entropy_forward(const void *logits, const void *target, const void *weight, void *loss,
                                       void *lse, void *state, void *workspace, int64_t workspace_bytes, int B,
                                       int C, int H, int W, int64_t ignore_index, float gamma, int dtype,
                                       void *stream);
int cerberus_seg_cross_entropy_backward(const void *logits, const void *target, const void *weight,
                                        const void *lse, const void *state, const void *grad_loss,
                                        void *grad_logits, int B, int C, int H, int W, int64_t ignore_index,
                                        int dtype, void *stream);
int cerberus_class_histogram(const void *target, void *counts, int64_t count, int num_classes,
                             int64_t ignore_index, void *stream);

/* Cross-entropy with online hard example mining (OHEM) as one differentiable scalar (additions only: no ABI bump):
 * SoftmaxCrossEntropyOHEMLoss (seg_losses.py:40-95) with the selection on the device.  Tensors as for
 * cerberus_seg_cross_entropy_*; thresh is compared in fp32; min_kept is any integer.
 *   valid(p) = target(p) != ignore_index && 0 <= target(p) < C;  prob(p) = exp(x_t(p) - lse(p))
 *   num_valid = #valid.  min_kept >= num_valid: every valid pixel is kept (a NaN prob too), threshold = +inf.  Else
 *   min_kept > 0: kth = the min_kept-th smallest prob of the valid pixels (a NaN orders above every number), threshold =
 *   kth > thresh ? kth : thresh, and thresh for a NaN kth.  Else threshold = thresh.
 *   kept(p) = valid(p) && prob(p) <= threshold (every pixel tied at kth is kept)
 *   loss[0] = sum_kept w[t] (lse - x_t) / sum_kept w[t]  (0 / 0 = NaN when nothing is kept)
 *   prob   : (B,H,W) fp32, overwritten: -1 where the pixel is not valid;   lse : (B,H,W) fp32, overwritten (every pixel)
 *   state  : 8 floats, overwritten: [ce, den, 1 / den, threshold, keep_all (1 or 0), the rank left among the pixels tied at
 *            kth (exact below 2^24), 0, 0], read by the backward on the device
 *   counts : 2 int64, overwritten: [num_valid, num_kept]
 *   workspace : cerberus_seg_ohem_workspace_bytes(B,H,W) bytes, 16-byte aligned (lse - x_t per pixel, three partials per 1024
 *            pixels, 3 x 2048 bins, 8 words of select state; 0 for a non-positive or too large size); the call zeroes what it
 *            adds to with a kernel of its own (capturable)
 * kth is exact: a radix select over the bits of prob, 11 / 11 / 10 bits from the top (cerberus_seg_ohem_digit_bits(0..2),
 * cerberus_seg_ohem_bins() bins per digit).  Counts are integer adds, floating-point sums go through per-workgroup partials in
 * a fixed order: the same bits on every run, on both routes (16-byte vector loads when H*W % 4 == 0 and the pointers are
 * aligned; scalar otherwise) and in a replayed graph.  The forward reads the logits once; nothing is read on the host.
 * A label outside [0, C) that is not ignore_index never forms an address and takes no part in the selection: it adds NaN to
 * the numerator, as in cerberus_seg_cross_entropy_forward, and its gradient is zeros.
 * Backward: grad_logits = grad_loss[0] * state[2] * w[t] * (softmax - onehot) at kept pixels (re-derived from prob and
 * state[3], state[4]), exactly 0.0f elsewhere; every element is written once.
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; B < 0, C < 1, H or W <= 0 CERB_EINVAL; C < 2 or
 * B*H*W > 2^31 - 1025 CERB_EUNSUPPORTED; a NaN thresh CERB_EINVAL; then B == 0 returns 0 without a launch; a null pointer, a
 * workspace that is too small or misaligned CERB_EINVAL -- all before any launch. */
int64_t cerberus_seg_ohem_workspace_bytes(int B, int H, int W);
int cerberus_seg_ohem_forward(const void *logits, const void *target, const void *weight, void *loss, void *prob,
                              void *lse, void *state, void *counts, void *workspace, int64_t workspace_bytes, int B,
                              int C, int H, int W, int64_t ignore_index, float thresh, int64_t min_kept, int dtype,
                              void *stream);
int cerberus_seg_ohem_backward(const void *logits, const void *target, const void *weight, const void *prob,
                               const void *lse, const void *state, const void *grad_loss, void *grad_logits, int B,
                               int C, int H, int W, int64_t ignore_index, int dtype, void *stream);
int cerberus_seg_ohem_digit_bits(int digit);
int cerberus_seg_ohem_bins(void);

/* The supervised depth loss InvHuberLoss (berHu) as one differentiable scalar (additions only: no ABI bump): the reference's
 * InvHuberLoss.forward (depth_losses.py:64-88) without `weight`, fp32.
 *   pred : (B,h,w) (a (B,1,h,w) prediction is the same memory);  gt : (B,H,W) with H % h == 0 and W % w == 0.  Pixel (y, x) of
 *          the prediction is compared with gt[b, y * (H / h), x * (W / w)]: for H == h, W == w the same pixel, otherwise the
 *          pixel F.interpolate(gt, (h, w), mode='nearest') picks (a pyramid level without a resized map).
 *   valid = g > 0 (false for a NaN g);  d = max(p, 0) - g;  err = valid ? |d| : 0;  m = max err;  c = 0.2 m;  N = B h w
 *   loss[0] = sum(err > c ? (d d + c c) / (2 c) : err) / N  -- N counts ALL pixels, as the reference's mean
 *   S = sum over {err > c} of (1/2 - d d / (2 c c));  ties = #{err == m}
 *   state : 4 floats, overwritten: [c, 0.2 S / ties, 1 / N, m], read by the backward on the device
 *   workspace : cerberus_inv_huber_workspace_bytes(B,h,w) bytes (1024 partial maxima and three partials per 1024 pixels; 0 for
 *          a non-positive or too large size), 16-byte aligned; no zero-fill needed
 * Forward: a max pass (at most 1024 workgroups, one partial maximum each; maxima are taken on the bit pattern, where a
 * positive NaN sorts above infinity), a sum pass that folds those partials itself, and a single-workgroup fixed-order finish:
 * no atomics, nothing zeroed, no workgroup waits for another, bit-reproducible for a given shape.  A lane owns 4 consecutive
 * pixels and loads 16 bytes of each map when h*w % 4 == 0, H == h, W == w and pred and gt are 16-byte aligned; one pixel per
 * lane otherwise -- both routes give the same bits.
 * Backward: grad_pred (B,h,w) = grad_loss[0] / N * [valid and p > 0] ((err > c ? d / c : sign(d)) + [err == m] state[1] sign(d)),
 * every element written exactly once (no zero-fill).  The second summand is the gradient through the data-dependent cutoff c,
 * split evenly over the pixels that hold the maximum.  grad_loss points to ONE float in DEVICE memory (capturable).
 * Decided by selection: an invalid pixel adds nothing whatever pred holds there and its gradient is 0.0f; a NaN at a valid
 * pixel gives a NaN loss; c == 0 (no valid pixel, or every valid pixel exact) gives loss 0.0f and a gradient of zeros (the
 * reference divides by 2 c and returns NaN); p <= 0 has gradient 0.0f.
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; B < 0 or a size <= 0 CERB_EINVAL; H % h != 0 or
 * W % w != 0 CERB_EUNSUPPORTED; B*h*w > 2^31 - 1025 CERB_ETOOLARGE; then B == 0 returns 0 without a launch; a null pointer, a
 * workspace that is misaligned or too small CERB_EINVAL -- all before any launch. */
int64_t cerberus_inv_huber_workspace_bytes(int B, int h, int w);
int cerberus_inv_huber_forward(const void *pred, const void *gt, void *loss, void *state, void *workspace,
                               int64_t workspace_bytes, int B, int h, int w, int H, int W, int dtype, void *stream);
int cerberus_inv_huber_backward(const void *pred, const void *gt, const void *state, const void *grad_loss,
                                void *grad_pred, int B, int h, int w, int H, int W, int dtype, void *stream);

/* The per-image statistics of the training metrics (additions only: no ABI bump): what the reference's metric loggers
 * (nnet_training/statistics/semantic.py, depth.py, optical_flow.py) compute from the model's outputs after every step.  Forward
 * only, fp32 inputs, everything reduced PER IMAGE.  A workgroup owns 1024 consecutive pixels of one image and a lane 4 of them:
 * 16-byte loads when H*W % 4 == 0 and the pointers are 16-byte aligned, guarded 4-byte loads otherwise -- both routes give the
 * same bits.  Terms are fp32 as the reference's element-wise ops and accumulated in float64 from the lane upward; per-workgroup
 * partials go to `workspace` (8-byte aligned, no zero-fill; its size comes from the *_workspace_bytes function, 0 for a
 * non-positive or too large size) and one workgroup per image adds them in a fixed order: no floating-point atomics, no host
 * round trip, capturable, bit-reproducible for a given shape.
 *
 * cerberus_seg_confusion: logits (B,C,H,W) fp32, target (B,H,W) int64 -> confusion (B,C,C) int64, [b, t, p] = the pixels of image
 *   b with label t whose argmax over the class planes is p (torch.argmax's rule: the first maximal class wins, a NaN logit counts
 *   as the maximum and the first NaN wins).  No index map is written.  A pixel whose label equals ignore_index or lies outside
 *   [0, C) is skipped by selection and never forms an address.  `confusion` is zeroed on the stream by the call itself (a kernel)
 *   and added to with integer adds (32-bit LDS bins per workgroup, one 64-bit global add per non-empty bin): any order, the same
 *   matrix.  2 <= C <= 64 (16 KiB of LDS bins); more classes: CERB_EUNSUPPORTED.
 *
 * cerberus_depth_metric_sums: pred, gt (B,h,w) fp32 (a (B,1,h,w) prediction is the same memory).  A pixel is valid if
 *   min_depth < gt < max_depth.  p = pred == 0 ? 1e-7f : pred (the input is not written);  d = p - gt;  l = logf(p) - logf(gt);
 *   r = max(p / gt, gt / p).
 *   sums   : (B,5) float64, over the valid pixels: |d| / gt, d d / gt, d d, l l, |l|
 *   counts : (B,4) int64, over the valid pixels: 1, r < 1.25, r < 1.5625, r < 1.953125
 *   An invalid pixel adds nothing whatever pred holds there; a valid pixel with pred < 0 makes the log sums NaN, as the reference.
 *
 * cerberus_flow_metric_sums: flow_pred, flow_gt (B,2,H,W), mask (B,H,W) fp32.  epe = sqrtf(dx dx + dy dy), e = epe * mask.
 *   sums   : (B,2) float64: sum e, sum mask
 *   counts : (B,1) int64: the pixels with e > 3 and e / max(|flow_gt|, 1e-10f) > 0.05f
 *
 * cerberus_warp_sad: image, source (B,C,H,W), flow (B,2,H,W) fp32 -> sad (B,) float64 = sum over c, y, x of
 *   |image - flow_warp(source, flow)| with border padding and bilinear sampling: each sample is the element
 *   cerberus_flow_warp_forward would have written (the same positions, weights and order of products); the warped image is
 *   never stored.  Any C >= 1.
 *
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; B < 0, a size <= 0, C < 2 (seg_confusion) or < 1
 * (warp_sad), min_depth >= max_depth or NaN CERB_EINVAL; H*W > 2^31 - 1025 or B > 65535 CERB_ETOOLARGE; C > 64 (seg_confusion)
 * CERB_EUNSUPPORTED; then B == 0 returns 0 without a launch; a null pointer, a workspace that is misaligned or too small
 * CERB_EINVAL -- all before any launch. */
int cerberus_seg_confusion(const void *logits, const void *target, void *confusion, int B, int C, int H, int W,
                           int64_t ignore_index, int dtype, void *stream);
int64_t cerberus_depth_metric_workspace_bytes(int B, int h, int w);
int cerberus_depth_metric_sums(const void *pred, const void *gt, void *sums, void *counts, void *workspace,
                               int64_t workspace_bytes, int B, int h, int w, float min_depth, float max_depth,
                               int dtype, void *stream);
int64_t cerberus_flow_metric_workspace_bytes(int B, int H, int W);
int cerberus_flow_metric_sums(const void *flow_pred, const void *flow_gt, const void *mask, void *sums, void *counts,
                              void *workspace, int64_t workspace_bytes, int B, int H, int W, int dtype, void *stream);
int64_t cerberus_warp_sad_workspace_bytes(int B, int H, int W);
int cerberus_warp_sad(const void *image, const void *source, const void *flow, void *sad, void *workspace,
                      int64_t workspace_bytes, int B, int C, int H, int W, int dtype, void *stream);

/* The region mutual information loss (additions only: no ABI bump): the heavy part of RMILoss (rmi.py:33-207) for
 * rmi_radius 3 and average pooling -- everything up to the three covariance matrices, and the backward from their gradients.
 * The 9 x 9 algebra between the two (inverse, Cholesky, log) is the caller's.
 *   logits : (B,C,H,W) fp32, C >= 1;  target : (B,H,W) int64;  pool = rmi_pool_size = rmi_pool_stride in 1..8 (1: no pooling)
 *   valid = 0 <= target < C (a negative label is ignored like one >= C);  o_c = valid and target == c;  s = sigmoid(x)
 *   bce[0] = sum_{valid pixels, all classes} (max(x,0) - x o + log1p(exp(-|x|))) / (n_valid + 1)
 *   prob = valid ? s + 1e-6 : 1e-6;  la_map, pr_map : (B,C,h,w) fp32 = avg_pool2d(o / prob, pool, pool, pool / 2),
 *          h = (H + 2 (pool / 2) - pool) / pool + 1 (the windows are disjoint and divide by pool^2 everywhere)
 *   means  : (B,C,2,9) float64: the means of the 9 shifted (h-2) x (w-2) slices of la_map ([..,0,:]) and pr_map ([..,1,:])
 *   la_cov, pr_cov, la_pr_cov : (B,C,9,9) float64 = L L^T, Pr Pr^T, L Pr^T of the slices minus their means
 *   state  : 4 floats, overwritten: [bce, n_valid, 1 / (n_valid + 1), 0], read by the backward on the device
 *   workspace : cerberus_rmi_workspace_bytes(B,C,H,W,pool) bytes (float64 partials; 0 for a size the calls reject), 8-byte
 *          aligned, fully overwritten; no zero-fill needed
 *   do_rmi == 0: only bce and state are written; the maps, means and matrices may be null.
 * Forward: one pass over the logits (a lane owns one pooling window for 8 class planes; 8-byte loads when pool is 4 or 8, W is
 * even, the logits are 8-byte and the labels 16-byte aligned; 4-byte loads otherwise -- both routes give the same bits), then the
 * means and the centred products from the pooled maps in float64.  Every sum has a fixed order and no floating-point atomics:
 * bit-reproducible for a given shape.
 * Backward: grad_logits (B,C,H,W) = valid ? s (1 - s) g_pool / pool^2 + grad_bce[0] state[2] (s - o) : 0.0f, where g_pool is
 * the gradient of the pooled probability gathered from grad_pr_cov = dloss/dpr_cov and grad_la_pr_cov = dloss/dla_pr_cov
 * (float64 (B,C,9,9)); every element written exactly once (no zero-fill), one launch.  grad_bce points to ONE float in DEVICE
 * memory (no host synchronisation: capturable).  la_cov carries no gradient (it depends on the labels only).
 * Labels never form an address.  An ignored pixel is skipped by selection: a NaN logit there changes nothing.
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; B < 0, C < 1, H or W <= 0, radius or pool < 1
 * CERB_EINVAL; radius != 3, pool > 8, a pooled side < 3 CERB_EUNSUPPORTED; H*W > 2^31 - 1025, B > 65535, C > 32767
 * CERB_ETOOLARGE; then B == 0 returns 0 without a launch; a null pointer, a workspace that is misaligned or too small
 * CERB_EINVAL -- all before any launch. */
int64_t cerberus_rmi_workspace_bytes(int B, int C, int H, int W, int pool);
int cerberus_rmi_forward(const void *logits, const void *target, void *bce, void *state, void *la_map, void *pr_map,
                         void *means, void *la_cov, void *pr_cov, void *la_pr_cov, void *workspace,
                         int64_t workspace_bytes, int B, int C, int H, int W, int radius, int pool, int do_rmi, int dtype,
                         void *stream);
int cerberus_rmi_backward(const void *logits, const void *target, const void *state, const void *la_map,
                          const void *pr_map, const void *means, const void *grad_bce, const void *grad_pr_cov,
                          const void *grad_la_pr_cov, void *grad_logits, int B, int C, int H, int W, int radius, int pool,
                          int do_rmi, int dtype, void *stream);

/* The OCR segmentation head's two own steps (additions only: no ABI bump): SpatialGather_Module and the core of
 * ObjectAttentionBlock (nnet_models/ocr_utils.py), fp32, forward and backward.  HW = H * W; R (K for the gather) in 1..32.
 *
 * Spatial gather:  p[b,k,:] = softmax over the HW pixels of scale * logits[b,k,:];  context[b,c,k] = sum_p p[b,k,p] feats[b,c,p]
 *   feats (B,C,HW), logits (B,K,HW) -> context (B,C,K), lse (B,K) = log sum_p exp(scale * logits[b,k,p])
 *   backward: grad_feats[b,c,p] = sum_k p[b,k,p] g[b,c,k];
 *             grad_logits[b,k,p] = scale p[b,k,p] (sum_c g[b,c,k] feats[b,c,p] - sum_c g[b,c,k] context[b,c,k]),  g = grad_context
 *   The backward forms p from the plane's maximum and sum, which it computes again from the logits (a pass over K / C of the bytes
 *   of the features): exp(x - lse) would carry the rounding of lse, half an ulp of a number near log(HW) + max, into every
 *   probability of the plane.
 * Object attention:  a[b,:,p] = softmax over r of scale * sum_c query[b,c,p] key[b,c,r];  context[b,c,p] = sum_r a[b,r,p] value[b,c,r]
 *   query (B,C,HW), key / value (B,C,R) -> context (B,C,HW), attn (B,R,HW)
 *   backward: da[r] = sum_c g[b,c,p] value[b,c,r];  dsim = a (da - sum_r a da), written to the caller's (B,R,HW) buffer `dsim`;
 *             grad_query[b,c,p] = scale sum_r dsim[b,r,p] key[b,c,r];  grad_key[b,c,r] = scale sum_p dsim[b,r,p] query[b,c,p];
 *             grad_value[b,c,r] = sum_p a[b,r,p] g[b,c,p]
 * Every sum over pixels is one partial per chunk of 256 pixels, added in chunk order by a second launch: no floating-point
 * atomics, the same bits on every run and for any alignment of the base pointers (no alignment is required).  Every output
 * element is written (no zero-fill needed); no host synchronisation: capturable.
 *   workspace : cerberus_ocr_workspace_bytes(B,C,R,HW) bytes (0 for sizes the calls reject), 16-byte aligned, fully overwritten;
 *               the gather forward and backward and the attention backward take it, the attention forward needs none.
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; B, C, R or HW <= 0 CERB_EINVAL; R > 32
 * CERB_EUNSUPPORTED; HW > 2^31 - 1025, or C R, B ceil(HW / 256), B ceil(C R / 256) past 2^31 - 1 CERB_ETOOLARGE; a null pointer, a
 * workspace that is misaligned or too small CERB_EINVAL -- all before any launch. */
int64_t cerberus_ocr_workspace_bytes(int B, int C, int R, int HW);
int cerberus_ocr_gather_forward(const void *feats, const void *logits, void *context, void *lse, void *workspace,
                                int64_t workspace_bytes, int B, int C, int K, int HW, float scale, int dtype, void *stream);
int cerberus_ocr_gather_backward(const void *feats, const void *logits, const void *context, const void *grad_context,
                                 void *grad_feats, void *grad_logits, void *workspace, int64_t workspace_bytes, int B, int C, int K,
                                 int HW, float scale, int dtype, void *stream);
int cerberus_ocr_attention_forward(const void *query, const void *key, const void *value, void *context, void *attn, int B, int C,
                                   int R, int HW, float scale, int dtype, void *stream);
int cerberus_ocr_attention_backward(const void *grad_context, const void *query, const void *key, const void *value, const void *attn,
                                    void *grad_query, void *grad_key, void *grad_value, void *dsim, void *workspace,
                                    int64_t workspace_bytes, int B, int C, int R, int HW, float scale, int dtype, void *stream);

/* The DETR set criterion (additions only: no ABI bump): the Hungarian matcher's cost matrix, the rectangular linear sum assignment
 * and the matched loss terms of the reference's DetrLoss / HungarianMatcher, for all L decoder layers of a step at once, fp32.
 *
 *   logits (N,Q,C1), boxes (N,Q,4) cxcywh, N = L B with the layers stacked layer-major over a batch of B
 *   tgt_labels (B,Tmax) int64, tgt_boxes (B,Tmax,4) fp32, tgt_count (B,) int32: the targets padded per image of the batch; image n
 *   reads row n % B; a count is clamped to 0..Tmax; a slot at or past the count is never read into a result
 *   fused limits: 1 <= Q <= 256, 0 <= Tmax <= 128, Q Tmax <= 16384, 2 <= C1 <= 256: cerberus_detr_fused_ok(Q, Tmax, C1) is 1 inside
 *
 * Matching cost of query q and target t:  w_bbox |p - t|_1 - w_class softmax(logits[q])[label t] - w_giou GIoU(xyxy(p), xyxy(t)).
 *   A non-finite entry becomes 1e9 and sets bit 0 of status[n]; a label outside [0, C1) among the counted targets is costed the
 *   same way and sets bit 1 (the loss counts a query matched to it as no-object).
 *   match_cost      : cost (N,Q,Tmax) fp32, padding columns zeroed; status (N,) int32 or null
 *   lsap            : solves a caller-given (N,Q,Tmax) fp32 matrix (non-finite entries as above); status (N,) int32 or null
 *   hungarian_match : the matrix is formed in LDS and solved there; bit for bit the result of lsap on match_cost's matrix
 *   match (N,Q) int32: the target of a query, or -1; min(Q, count) queries are matched, every target at most once.  The solver is
 *   the shortest-augmenting-path algorithm (Jonker-Volgenant, rectangular after Crouse), one wavefront per image with float64 duals:
 *   optimal for the fp32 matrix as given; the lowest column index wins a tie.  Every loop has a trip count fixed by Q and the count.
 *
 * Set loss, per layer l:  losses (L,4) fp32 = [loss_ce, loss_bbox, loss_giou, cardinality_error]
 *   loss_ce = sum w[c_q] nll_q / sum w[c_q] over the B Q queries of the layer, c_q = tgt_labels[match] or the no-object class C1 - 1,
 *   weight (C1,) fp32;  loss_bbox = sum over matched |p - t|_1 / num_boxes;  loss_giou = sum over matched (1 - GIoU) / num_boxes;
 *   cardinality_error = mean_b |#{q: argmax != C1 - 1} - count_b|.  num_boxes: ONE float in device memory.  A match outside
 *   [0, count) counts as unmatched.  wsum (L,) float64 = sum w[c_q], kept for the backward.
 *   One workgroup per image writes float64 partial sums, one workgroup adds them in index order: no floating-point atomics.
 *   workspace : cerberus_detr_workspace_bytes(N) bytes, 8-byte aligned, fully overwritten.
 *   backward  : grad_losses (L,4) fp32 -> grad_logits (N,Q,C1), grad_boxes (N,Q,4), every element written in one launch; unmatched
 *   queries get zeros in grad_boxes; the cardinality column carries no gradient.
 * Box rows are read with 16-byte loads where the base pointer allows and with scalar loads otherwise: no alignment beyond the
 * element's is required.  No host synchronisation: capturable.
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; N < 0, B or Q <= 0, C1 < 2, Tmax < 0, N % B != 0
 * CERB_EINVAL; a size past the fused limits CERB_EUNSUPPORTED; then N == 0 returns 0 without a launch; a null pointer (the targets
 * and the matrix may be null when Tmax == 0), a workspace that is misaligned or too small CERB_EINVAL -- all before any launch. */
int cerberus_detr_fused_ok(int Q, int Tmax, int C1);
int64_t cerberus_detr_workspace_bytes(int N);
int cerberus_detr_match_cost(const void *logits, const void *boxes, const void *tgt_labels, const void *tgt_boxes, const void *tgt_count,
                             void *cost, void *status, int N, int B, int Q, int C1, int Tmax, float w_class, float w_bbox,
                             float w_giou, int dtype, void *stream);
int cerberus_detr_lsap(const void *cost, const void *tgt_count, void *match, void *status, int N, int B, int Q, int Tmax, void *stream);
int cerberus_detr_hungarian_match(const void *logits, const void *boxes, const void *tgt_labels, const void *tgt_boxes,
                                  const void *tgt_count, void *match, void *status, int N, int B, int Q, int C1, int Tmax,
                                  float w_class, float w_bbox, float w_giou, int dtype, void *stream);
int cerberus_detr_set_loss_forward(const void *logits, const void *boxes, const void *match, const void *tgt_labels,
                                   const void *tgt_boxes, const void *tgt_count, const void *weight, const void *num_boxes, void *losses,
                                   void *wsum, void *workspace, int64_t workspace_bytes, int N, int B, int Q, int C1, int Tmax,
                                   int dtype, void *stream);
int cerberus_detr_set_loss_backward(const void *logits, const void *boxes, const void *match, const void *tgt_labels,
                                    const void *tgt_boxes, const void *tgt_count, const void *weight, const void *num_boxes,
                                    const void *wsum, const void *grad_losses, void *grad_logits, void *grad_boxes, int N, int B, int Q,
                                    int C1, int Tmax, int dtype, void *stream);

/* The Panoptic-DeepLab decoder head's own step (additions only: no ABI bump): the depthwise 5x5 convolution (cross-correlation,
 * stride 1, zero padding 2, no bias) of nnet_models/deeplab_panoptic.py, fp32 NCHW, over the virtual tensor
 *     in = cat(interpolate(low, (H,W), bilinear, align_corners=True), skip)        (B,Ca+Cb,H,W)
 * which is never written to memory.  Ca == 0 is the plain convolution of `skip` (low, h, w and grad_low are ignored).
 *   low (B,Ca,h,w), skip (B,Cb,H,W), weight (Ca+Cb,1,5,5) -> out (B,Ca+Cb,H,W);  Ca >= 0, Cb >= 1; h == H, h == 1 and
 *   non-integer ratios are legal.  The upsample uses ATen's fp32 operation order: scale = (float)(h-1)/(H-1) (0 when H == 1),
 *   src = scale * y, i0 = (int)src, i1 = min(i0+1, h-1), lambda = src - i0; the same for x.
 * Backward: any of grad_low (B,Ca,h,w), grad_skip (B,Cb,H,W), grad_weight (Ca+Cb,1,5,5) may be NULL: that gradient is not
 * computed and its launch is skipped (at least one must be asked for).  At most three launches: the stencil with the flipped
 * weights over grad_out, which also leaves one float64 partial of every grad_weight element per tile of 32 x 64 pixels (the input
 * window is built again from low / skip); grad_low as a gather (a low-res pixel sums the high-res pixels that sampled it, rows then
 * columns ascending); the fold of the partials.  No floating-point atomics: the same bits on every run, in a replayed graph and
 * for any alignment of the tensor pointers (4 bytes are required; rows that start on 16 bytes take 16-byte loads and stores).
 * Every element of every output asked for is written (no zero-fill needed); no host synchronisation: capturable.
 *   workspace : cerberus_pdl_workspace_bytes(B,Ca,Cb,H,W) bytes (0 for sizes the calls reject), 16-byte aligned: the gradient of
 *               the upsampled channels, B Ca H W floats padded to 16 bytes, then (Ca+Cb) x 25 x B x tiles float64 partials,
 *               tiles = ceil(H/32) ceil(W/64).  The forward needs none.
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; B, Cb, H or W <= 0, Ca < 0, h or w <= 0 with Ca > 0
 * CERB_EINVAL; H W > 2^31 - 1025, more than 65535 tiles, or B (Ca+Cb), B tiles, h w past 2^31 - 1 CERB_ETOOLARGE; a null pointer
 * (but for the optional ones above) or one that is not 4-byte aligned, a workspace that is misaligned or too small CERB_EINVAL --
 * all before any launch. */
int64_t cerberus_pdl_workspace_bytes(int B, int Ca, int Cb, int H, int W);
int cerberus_pdl_dwconv_forward(const void *low, const void *skip, const void *weight, void *out, int B, int Ca, int Cb, int h, int w,
                                int H, int W, int dtype, void *stream);
int cerberus_pdl_dwconv_backward(const void *grad_out, const void *low, const void *skip, const void *weight, void *grad_low,
                                 void *grad_skip, void *grad_weight, void *workspace, int64_t workspace_bytes, int B, int Ca, int Cb,
                                 int h, int w, int H, int W, int dtype, void *stream);

/* The DETR head's multi-head attention core (additions only: no ABI bump), csrc/detr_attn.hip: per batch entry b and head h, with
 * D = 32 channels per head,
 *     out = dropout(softmax(scale q k^T + key_padding_mask)) v
 * fp32, flash-style: nothing of size Lq x Lk is written.  The tensors are read where F.linear leaves them:
 *   q (Lq,B,H*D), k and v (Lk,B,H*D) -> out (Lq,B,H*D), lse (B,H,Lq): the log-sum-exp of every row of scale q k^T + mask, and
 *   stats (B,H,Lq,2): that row's maximum and its sum of exp(. - maximum), which the backward recomputes the probabilities from
 *   (exp(s - max) / sum as in the forward: exp(s - lse) would carry the rounding of lse and of s - lse, 2^-22 for a hundred keys).
 *   key_padding_mask : (B,Lk) bytes or NULL; non-zero means the key is ignored.  A row whose keys are all ignored gives out = 0,
 *                      lse = -inf and zero gradients (the stock chain gives NaN there).
 *   seed             : ONE int64 in device memory (8-byte aligned), read by the kernels: no host read, capturable.  May be NULL
 *                      when dropout_p == 0.  The keep decision is the stateless hash of csrc/attn_dropout.h over (seed, b H + h,
 *                      query, key); kept probabilities are multiplied by 1 / (1 - dropout_p).
 * Backward: any of grad_q (Lq,B,H*D), grad_k, grad_v (Lk,B,H*D) may be NULL (at least one must be asked for): grad_q NULL skips
 * the query-owning launch, grad_k and grad_v both NULL skip the key-owning one.  At most three launches: delta = rowsum(grad_out *
 * out), the key-owning kernel (grad_k, grad_v), the query-owning kernel (grad_q).  No atomics: the same bits on every run, in a
 * replayed graph, whatever else is asked for, and for any 4-byte alignment of the tensor pointers.  Every element of every output
 * asked for is written.
 *   delta : scratch, B*H*Lq floats.
 * cerberus_attn_dropout_keep writes the keep decisions as (B,H,Lq,Lk) bytes (1 = kept); dropout_p == 0 keeps everything.
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; Lq, Lk, B, H or D <= 0, dropout_p outside [0,1), a
 * scale that is not finite CERB_EINVAL; D != 32 CERB_EUNSUPPORTED; B H or max(Lq,Lk) B H D past 2^31 - 1, or a launch of 2^32 threads or more
 * CERB_ETOOLARGE; a null pointer (but for the optional ones above) or a misaligned one CERB_EINVAL -- all before any launch. */
int cerberus_attn_forward(const void *q, const void *k, const void *v, const void *key_padding_mask, const void *seed, void *out,
                          void *lse, void *stats, int Lq, int Lk, int B, int H, int D, float scale, float dropout_p, int dtype, void *stream);
int cerberus_attn_backward(const void *grad_out, const void *q, const void *k, const void *v, const void *key_padding_mask,
                           const void *seed, const void *out, const void *stats, void *grad_q, void *grad_k, void *grad_v, void *delta,
                           int Lq, int Lk, int B, int H, int D, float scale, float dropout_p, int dtype, void *stream);
int cerberus_attn_dropout_keep(const void *seed, void *keep, int B, int H, int Lq, int Lk, float dropout_p, void *stream);

/* The device side of the panoptic metric (additions only: no ABI bump): what the reference's PanopticMetric
 * (nnet_training/statistics/panoptic.py) and utilities/panoptic_post_processing.py do to the centre heat map, the offset map and
 * the id / class maps of every image.  Forward only, no host synchronisation, no floating-point atomics: capturable and
 * bit-reproducible.
 *
 * cerberus_center_peaks: heatmap (B,H,W) fp32 (a (B,1,H,W) map is the same memory) -> out (B,H,W) fp32, every element written.
 *   v = x <= threshold ? -1 : x;  out = v where v equals the maximum of v over the nms_kernel x nms_kernel window clipped to the
 *   image, else -1: the map that F.threshold(.., -1), max_pool2d(nms_kernel, 1, (nms_kernel-1)/2) and `hmp[hmp != pooled] = -1`
 *   leave behind.  Compares only: exact.  As in that chain a NaN passes the threshold and is the maximum of every window that
 *   holds it: the NaN pixel and every pixel within the window's reach of it give -1.  The input is not written.  nms_kernel is
 *   odd and at most cerberus_center_peaks_max_kernel() (15).
 *
 * cerberus_group_pixels: offsets (B,2,H,W) fp32 in (dy, dx) order, centers (B,max_centers,2) int64 (y, x), counts (B,) int64
 *   (the valid rows of each image; clamped to [0, max_centers]), sem (B,H,W) int64 or NULL -> out (B,H,W) int64 =
 *   1 + argmin_k sqrtf(dy dy + dx dx), dy = float(cy_k) - (float(y) + off_y), dx = float(cx_k) - (float(x) + off_x), all fp32
 *   without contraction; the first minimal index wins, a NaN distance counts as the minimum (torch.argmin's rule).  With sem,
 *   the id is kept where 0 <= sem < 64 and bit sem of thing_mask is set, else 0.  An image with no centre gives zeros.  Centres
 *   are walked through LDS in chunks of 256; max_centers is at most cerberus_group_pixels_max_centers() (4096).
 *
 * cerberus_instance_overlap: pred_inst, tgt_inst, pred_seg, tgt_seg (B,H,W) int64 -> inter (B,M,M), pred_cls (B,M,C), tgt_cls
 *   (B,M,C) int64, M = max_ids, C = num_classes: inter[b,i,j] = the pixels of image b with predicted id i and target id j;
 *   pred_cls[b,i,c] = those of predicted id i with predicted class c; tgt_cls[b,j,c] likewise for the target.  A pixel with
 *   either id outside [0, M) is skipped in all three; a class outside [0, C) is skipped in its class histogram only.  The
 *   outputs are zeroed on the stream by the call itself (a kernel) and added to with integer adds (32-bit LDS bins per
 *   workgroup, one 64-bit global add per non-empty bin).  M (M + 2 C) is at most cerberus_instance_overlap_max_bins() (16128:
 *   63 KiB of LDS; M = 101 with C = 19 fits).
 *
 * Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; B < 0, a size <= 0, an even nms_kernel or one outside
 * 1..15, max_centers, max_ids or num_classes < 1 CERB_EINVAL; H*W > 2^31 - 1025, B > 65535 or H > 16 * 65535 (center_peaks)
 * CERB_ETOOLARGE; max_centers or the bin count above its limit CERB_EUNSUPPORTED; then B == 0 returns 0 without a launch; a null
 * pointer (other than sem) CERB_EINVAL -- all before any launch. */
int cerberus_center_peaks_max_kernel(void);
int cerberus_group_pixels_max_centers(void);
int cerberus_instance_overlap_max_bins(void);
int cerberus_center_peaks(const void *heatmap, void *out, int B, int H, int W, float threshold, int nms_kernel, int dtype,
                          void *stream);
int cerberus_group_pixels(const void *offsets, const void *centers, const void *counts, const void *sem, void *out, int B,
                          int H, int W, int max_centers, uint64_t thing_mask, int dtype, void *stream);
int cerberus_instance_overlap(const void *pred_inst, const void *tgt_inst, const void *pred_seg, const void *tgt_seg,
                              void *inter, void *pred_cls, void *tgt_cls, int B, int H, int W, int max_ids, int num_classes,
                              void *stream);

/* The training side of the panoptic branch (additions only: no ABI bump): the Panoptic-DeepLab targets of the reference's
 * PanopticTargetGenerator (datasets/cityscapes_panoptic_transform.py) from an id map on the device, and the centre / offset
 * regression loss of its DeeplabPanopticLoss (loss_functions/panoptic_loss.py) as one differentiable scalar.  No host
 * synchronisation, no floating-point atomics: capturable and bit-reproducible.  A workgroup owns 1024 consecutive pixels
 * (elements); 16-byte loads and stores when H*W % 4 == 0 and the pointers are 16-byte aligned, 4-byte ones otherwise -- both
 * routes give the same bits.
 *
 * cerberus_panoptic_targets: ids (B,H,W) int32 (ids_int64 == 0) or int64 (1), the decoded panoptic id map; seg_ids, seg_category
 *   (B,S) int64; seg_flags (B,S) int32, bit 0 "thing", bit 1 "iscrowd"; seg_count (B,) int64, the live rows of each image's
 *   table (clamped to [0,S]; rows past it are ignored whatever they hold); gauss ((6 sigma + 3)^2) fp32, the caller's table of
 *   exp(-((x - x0)^2 + (y - y0)^2) / (2 sigma^2)), x0 = y0 = 3 sigma + 1.  S is at most
 *   cerberus_panoptic_targets_max_segments() (256).  Ids among an image's live rows must be distinct: the result is otherwise
 *   unspecified.  A pixel's row is the live row whose id it holds, if any.
 *   Per live row: n, sum y, sum x over its pixels as 64-bit INTEGERS (any order, the same sums); cy = double(sum y) / double(n),
 *   cx likewise; it has a centre if it is a thing and n > 0, and is small if it has a centre and n < small_instance_area.
 *   center_points : (B,S,2) float64 (cy, cx), NaN for a row without a centre
 *   semantic      : (B,H,W) int64: the row's category; ignore_label without a row, or for a crowd row if ignore_crowd_in_semantic
 *   foreground    : (B,H,W) int64: 1 on things
 *   center        : (B,H,W) fp32: max over the image's centres (Y,X) = ((int)cy, (int)cx) with 0 <= y - (Y - 3 sigma - 1) <
 *                   6 sigma + 3 and likewise in x of gauss[y - (Y - 3 sigma - 1)][x - (X - 3 sigma - 1)], else 0
 *   offset        : (B,2,H,W) fp32: float(cy - double(y)), float(cx - double(x)) on things, else 0
 *   semantic_mask : (B,H,W) fp32: small_instance_weight on small things, else 1
 *   center_mask   : (B,H,W) fp32: 1 on a row that is not crowd
 *   offset_mask   : (B,H,W) fp32: 1 on a row that is not crowd and, if ignore_stuff_in_offset, is a thing
 *   workspace : cerberus_panoptic_targets_workspace_bytes(B,H,W,S) bytes (the moments, a 32-bit row map, the rows' attributes; 0
 *               for a size the call rejects), 16-byte aligned; the call zeroes what it adds to (a kernel).
 *   Every output element is written exactly once.  Launches: zero, moments, finish (one workgroup per image), fill.
 *   Errors: B < 0, a size <= 0, S <= 0, sigma < 1, ids_int64 not 0 / 1 CERB_EINVAL; S > 256 CERB_EUNSUPPORTED; H*W > 2^31 - 1025,
 *   B > 65535 or sigma > 4096 CERB_ETOOLARGE; then B == 0 returns 0 without a launch; a null pointer, a workspace that is
 *   misaligned or too small CERB_EINVAL -- all before any launch.
 *
 * cerberus_panoptic_loss_forward: center_pred, center_tgt (B,1,H,W), offset_pred, offset_tgt (B,2,H,W), center_mask, offset_mask
 *   (B,H,W) or NULL, all fp32; masks are weights (any float), shared by the planes of their term.  With d = pred - tgt,
 *   f = d d (centre) or |d| (offset), N the term's elements, and sums over the term's ELEMENTS (the offset mask counts twice):
 *   mode 0 (reference): term = weight * sum f / N if the mask is NULL or sum m > 0, else 0 (the reference's `mean * mask` summed
 *                       and divided by the mask's sum, with its gate evaluated on the device)
 *   mode 1 (pixel)    : term = weight * sum_{m != 0} m f / sum m if sum m > 0, else 0; without a mask as mode 0.  An element
 *                       with m == 0 is skipped by selection: a NaN there changes nothing.
 *   loss[0] = centre term + offset term;  state : 2 floats, overwritten: the scales weight / N or weight / sum m (0 when a term
 *   is gated off), read by the backward on the device.  In mode 0 a NaN anywhere gives NaN.
 *   workspace : cerberus_panoptic_loss_workspace_bytes(B,H,W) bytes (three partials per 1024 elements of each term; 0 for a size
 *               the calls reject), 16-byte aligned; no zero-fill needed.
 *   Launches: one pass per term, then one workgroup that adds the partials in a fixed order.
 * cerberus_panoptic_loss_backward: grad_center (B,1,H,W), grad_offset (B,2,H,W), every element written exactly once by ONE
 *   launch: grad_loss[0] * scale * (2 d or sign(d), sign(0) = 0), times m in mode 1 with a mask; exactly 0.0f where m == 0 in
 *   mode 1 and everywhere when the term's scale is 0.  grad_loss points to ONE float in DEVICE memory.
 *   Errors: unknown dtype CERB_EDTYPE; fp16 / bf16 / fp64 CERB_EUNSUPPORTED; B < 0, a size <= 0, a mode other than 0 / 1
 *   CERB_EINVAL; 2*B*H*W > 2^31 - 1025 CERB_ETOOLARGE; then B == 0 returns 0 without a launch; a null pointer (other than a
 *   mask), a workspace that is misaligned or too small CERB_EINVAL -- all before any launch. */
int cerberus_panoptic_targets_max_segments(void);
int64_t cerberus_panoptic_targets_workspace_bytes(int B, int H, int W, int S);
int cerberus_panoptic_targets(const void *ids, int ids_int64, const void *seg_ids, const void *seg_category,
                              const void *seg_flags, const void *seg_count, const void *gauss, void *semantic,
                              void *foreground, void *center, void *offset, void *semantic_mask, void *center_mask,
                              void *offset_mask, void *center_points, void *workspace, int64_t workspace_bytes, int B, int H,
                              int W, int S, int sigma, int64_t ignore_label, int ignore_stuff_in_offset,
                              int64_t small_instance_area, float small_instance_weight, int ignore_crowd_in_semantic,
                              void *stream);
int64_t cerberus_panoptic_loss_workspace_bytes(int B, int H, int W);
int cerberus_panoptic_loss_forward(const void *center_pred, const void *center_tgt, const void *center_mask,
                                   const void *offset_pred, const void *offset_tgt, const void *offset_mask, void *loss,
                                   void *state, void *workspace, int64_t workspace_bytes, int B, int H, int W,
                                   float center_weight, float offset_weight, int mode, int dtype, void *stream);
int cerberus_panoptic_loss_backward(const void *center_pred, const void *center_tgt, const void *center_mask,
                                    const void *offset_pred, const void *offset_tgt, const void *offset_mask,
                                    const void *state, const void *grad_loss, void *grad_center, void *grad_offset, int B,
                                    int H, int W, int mode, int dtype, void *stream);

/* Diagnostics / tuning knobs (process-wide, read at launch time, default 0):
 *   "corr_force_generic" : 1 = always use the generic kernels (testing)
 *   "corr_fwd_variant"   : 0 = auto, 1..8 = force one register-staged forward variant,
 *                          9..13 = the LDS-DMA variants (fp32, W % 4 == 0) with 1, 2, 4, 8,
 *                          16 channel groups, 14 = the matrix-core kernel (fp16 / bf16 storage,
 *                          C <= 128; auto uses it for 16 < C <= 128), 15 = the coarse-level kernel (fp32, and
 *                          fp16 / bf16 storage with C > 128; any even W up to 64 -- round 6 -- and a channel count its lane
 *                          layout divides: corr_coarse.hip; auto uses it there up to 2560 (row, displacement
 *                          row) workgroups), 16 = auto without it, 17 = the persistent, cross-item pipelined forward
 *                          (fp32, C % 8 == 0: corr_fwd_pipe.hip; built and measured in round 5, slower than the tile
 *                          kernels: -DCERB_EXPERIMENTS builds only since round 6; with it, "corr_bwd_cslice" > 0 sets
 *                          its number of workgroups); round 6, 16-bit storage with W % 8 == 0: 16 < C <= 64 take the
 *                          column-walk form of the matrix-core forward (LDS-DMA tiles, ds_read_b64_tr_b16 operands;
 *                          corr_mfma.hip) -- 20 = the register-staged form of rounds 4-5 instead (what other widths and
 *                          65 .. 128 channels use), 26 = the walk's stand-still form (4 x 64 tiles, C <= 32); all three
 *                          give identical bits; with them "corr_bwd_cslice" > 0 sets the tiles per walk
 *   "corr_bwd_variant"   : 0 = auto, 1 = all 81 displacements per lane (register-staged),
 *                          3 = three displacement groups, 4 / 5 = LDS-DMA with the 8x64 /
 *                          16x32 tile (fp32, W % 4 == 0), 8 = displacement-row streaming,
 *                          11 = the matrix-core kernel in its row-per-wave form of rounds 2-4 (fp16 / bf16 storage; auto
 *                          uses the segment-per-wave form of round 5: same bits, 8-12 % faster),
 *                          12 = whole image rows per wavefront (fp32; round 6: any W % 4 == 0 up to 256, any
 *                          H and C -- widths between 64 / 128 / 256 run on the lanes of the next one; auto uses
 *                          it on maps wider than 64 with enough workgroups for the chip and on exact 64-wide
 *                          ones; 13 = auto, but not on 64-wide maps), 14 = the coarse-level kernel (fp32, round 6:
 *                          any W % 4 == 0 up to 64, corr_coarse.hip; auto uses it there up to 4096 workgroups), 15 = auto without
 *                          it; 2, 6, 7, 9, 10 (and forward
 *                          1, 2, 8) are measured-and-rejected variants that exist only in
 *                          -DCERB_EXPERIMENTS test builds (otherwise: auto)
 *                          NOTE on batch invariance: auto picks kernels from WORKGROUP COUNTS (the 2560 /
 *                          4096 / 192-workgroup thresholds above), which include the batch size, and the
 *                          kernels differ in summation order: a batch item's correlation values (and
 *                          forward of a stacked batch vs two separate calls) agree to fp32 rounding
 *                          (<= 1e-6 relative), not bit for bit, across batch sizes that change the kernel.
 *                          The warp ops choose from one image's shape only, except the grad_image tile
 *                          height (8 rows up to 32768 pixels per call, else 16), which moves the
 *                          fixed-point scale by <= 2^-29 of a tile's largest gradient.
 *   "experiments_build"  : read-only (cerberus_get_option): 1 in a -DCERB_EXPERIMENTS build
 *   "corr_bwd_cslice"    : 0 = auto, else channels per backward workgroup (the matrix-core
 *                          backward reads it as the number of tiles a workgroup walks down)
 *   "corr_no_mfma"       : 1 = fp16 / bf16 storage never takes the matrix-core kernels: the vector
 *                          kernels, selected as for fp32 (the fp32 path uses no MFMA either way)
 *   "warp_pair_taps"     : warp gather variant (0 default, 1 paired everywhere, 2 unpaired)
 *   "warp_tile_ranges"   : channel ranges per warp-backward tile (0 auto)
 *   "warp_tile_h"        : rows per warp-backward tile (0 auto, 8, 16)
 *   "warp_force_scatter" : 1 = warp backward by global atomics even when a context exists
 *   "warp_staged"        : 0 = auto (the forward gather goes through an LDS copy of the source
 *                          window on large maps with 16-byte aligned rows), 2 = always gather
 *                          from global memory, >= 4 = always staged where possible, with that
 *                          many channels per workgroup
 *   "warp_stagger"       : phase shift of the warp backward's co-resident workgroups (round 4): 0 = auto (when
 *                          the whole launch is resident at once: the second 16-row tile workgroup of every CU
 *                          starts 6 k cycles late, or, with one tile workgroup per CU, the two halves of the
 *                          grad_flow workgroups 6 k and 2 k cycles late), -1 = off, else the delays of the 2nd / 3rd / 4th
 *                          256 workgroups in units of 1024 cycles, one byte each.  Speed only: same results.
 *   "warp_fewc"          : 0 = auto (a warp of <= 4 channels takes the lane-per-pixel kernels when no context /
 *                          no grad_image is asked for: the photometric loss's RGB warps), -1 = off.  Same bits.
 *   "warp_pair16"        : (round 6) 0 = auto: fp16 / bf16 images with W % 8 == 0 take the kernels of warp16.hip --
 *                          forward and the backward's grad_flow role with two pixels per lane and a raw 16-bit LDS
 *                          window filled by LDS-DMA, the backward's tile role with its sources as pairs (W % 2 == 0);
 *                          -1 = off (the general kernels); 1 = additionally the fp32 forward through the same
 *                          window kernel (measured slower than the staged one: for A/B only).  Same bits in every case.
 * Returns CERB_EINVAL for an unknown key. */
int cerberus_set_option(const char *key, int value);
int cerberus_get_option(const char *key, int *value);

/* Name of the kernel variant the most recent correlation forward / backward of this PROCESS
 * dispatched to, whichever thread issued it (autograd runs backward on its own thread); for
 * tests and the bench's roofline report. */
const char *cerberus_last_kernel(int which /*0 = forward, 1 = backward*/);

#ifdef __cplusplus
}
#endif
#endif /* CERBERUS_HIP_H */
