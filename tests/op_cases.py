"""One sample call of every ``cerberus::`` op (tests/test_op_contract_cpu.py, tests/test_op_contract_gpu.py).

``CASES[name](device)`` returns ``(args, differentiable)``: the positional arguments of ``torch.ops.cerberus.<name>`` as
contiguous tensors on ``device``, and the indices of the tensor arguments the op has a real gradient for.  ``case(name, device,
layout)`` puts the arguments in ``layout`` (``LAYOUTS``).  ``OUTPUTS[name]`` states the shape and dtype of every tensor the call
returns: written out here, not taken from the Meta functions.

Values come from ``hash_uniform`` seeds; labels, ids and tables from the smallest case of the op's own ``*_cases.py``.  The
shapes are the smallest at which the op is defined and does real work (nothing exceeds 64 x 128 pixels).  A ``*_backward`` op
takes what its forward leaves (``lse``, ``state``, ``prob``, the warp context, ``la_map`` ...) from a contiguous forward call
made inside the builder when the device is a GPU; without one (the Meta run of the CPU test) the tensors a forward would have
produced are zeros of the shapes ``OUTPUTS`` states for that forward.

No layout shifts a tensor's start address: every view begins at offset 0 of its own buffer, so the binding's ``.contiguous()``
copies are the only thing between a layout and the kernels, and the kernels see the pointers the rest of the suite gives them.
Misaligned and offset views are not part of this table: tests/alignment_cases.py puts its arguments into such views
(``test_same_bits_from_an_offset_view``), and tests/test_alignment_gpu.py holds the hot-path kernels at every alignment gate."""
import numpy as np
import torch

import panoptic_cases
import panoptic_train_cases
import rmi_cases
import seg_loss_cases
import seg_ohem_cases
from cerberusnet_amd.synth import hash_uniform, stereo_camera, stereo_depth

LAYOUTS = ("contiguous", "channels_last", "sliced")

F32, F64, I64 = torch.float32, torch.float64, torch.int64
CORR_P = (4, 1, 4, 1, 1, 1)             # pad, kernel, max displacement, stride1, stride2, multiply: the model's d = 4 volume
CORR = (2, 6, 9, 12)                    # the correlation family and the warps
CORR_OUT = (2, 81, 9, 12)
CONCAT = (2, 90, 9, 12)                 # the caller-owned buffer of correlation_leaky_into: 3 + 81 + 6 channels
CONCAT_AT = 3
FLOW = (2, 2, 9, 12)
IMG = (2, 3, 9, 12)                     # photometric / census / smoothness / reproject
MAP4 = (2, 1, 9, 12)
MAP3 = (2, 9, 12)
SEG = (2, 5, 9, 12)                     # the segmentation losses
RMI = (2, 5, 13, 22)                    # pool 4 with its padding of 2: a 4 x 6 pooled map, 2 x 4 positions of the 3 x 3 slices
RMI_MAP = (2, 5, 4, 6)
HUBER_PRED, HUBER_GT = (2, 1, 8, 12), (2, 16, 24)
WARP_CONTEXT = 236                      # int64 words: 2 images x (5 strips x 16 B + 2 planes x 9 x 12 x 4 B) = 1888 B
OHEM_MIN_KEPT = 50                      # below the valid pixels (about 0.85 x 216): the select branch runs
PANOPTIC = (2, 8, 64)                   # panoptic_train_cases.target_case("vector"): 3 table rows, sigma 2
IGNORE = 255

# name -> [(shape, dtype) of every returned tensor, in order]
OUTPUTS = {
    "correlation": [(CORR_OUT, F32)],
    "correlation_backward": [(CORR, F32), (CORR, F32)],
    "correlation_leaky": [(CORR_OUT, F32)],
    "correlation_leaky_into": [],
    "correlation_backward_leaky": [(CORR, F32), (CORR, F32)],
    "warp_correlation_leaky": [(CORR_OUT, F32)],
    "area_pyramid": [(IMG, F32), ((2, 3, 3, 4), F32), ((2, 3, 4, 5), F32)],
    "flow_upsample": [((2, 2, 18, 24), F32)],
    "flow_upsample_backward": [(FLOW, F32)],
    "area_resize": [((2, 3, 4, 5), F32)],
    "flow_warp": [(CORR, F32)],
    "flow_warp_ctx": [(CORR, F32), ((WARP_CONTEXT,), I64)],
    "flow_warp_backward_ctx": [(CORR, F32), (FLOW, F32)],
    "flow_warp_backward": [(CORR, F32), (FLOW, F32)],
    "photometric_loss": [((), F32)],
    "photometric_loss_backward": [(IMG, F32), (IMG, F32)],
    "census_loss": [((), F32)],
    "census_loss_backward": [(IMG, F32), (IMG, F32)],
    "corresponding_map": [(MAP4, F32)],
    "occlusion_mask_bidirection": [(MAP4, F32)],
    "reproject_warp": [(IMG, F32)],
    "reproject_warp_backward": [(MAP4, F32)],
    "seg_cross_entropy": [((), F32), (MAP3, F32), ((4,), F32)],
    "seg_cross_entropy_backward": [(SEG, F32)],
    "class_histogram": [((5,), I64)],
    "seg_ohem_cross_entropy": [((), F32), (MAP3, F32), (MAP3, F32), ((8,), F32), ((2,), I64)],
    "seg_ohem_cross_entropy_backward": [(SEG, F32)],
    "inv_huber": [((), F32), ((4,), F32)],
    "inv_huber_backward": [(HUBER_PRED, F32)],
    "seg_confusion": [((2, 5, 5), I64)],
    "depth_metric_sums": [((2, 5), F64), ((2, 4), I64)],
    "flow_metric_sums": [((2, 2), F64), ((2, 1), I64)],
    "warp_sad": [((2,), F64)],
    "center_peaks": [(MAP4, F32)],
    "group_pixels": [(MAP3, I64)],
    "instance_overlap": [((2, 4, 4), I64), ((2, 4, 5), I64), ((2, 4, 5), I64)],
    "rmi_moments": [((), F32), ((2, 5, 9, 9), F64), ((2, 5, 9, 9), F64), ((2, 5, 9, 9), F64), (RMI_MAP, F32), (RMI_MAP, F32),
                    ((2, 5, 2, 9), F64), ((4,), F32)],
    "rmi_moments_backward": [(RMI, F32)],
    "edge_smoothness": [((), F32)],
    "edge_smoothness_backward": [(FLOW, F32)],
    "panoptic_targets": [(PANOPTIC, I64), (PANOPTIC, I64), ((2, 1, 8, 64), F32), ((2, 2, 8, 64), F32), (PANOPTIC, F32),
                         (PANOPTIC, F32), (PANOPTIC, F32), ((2, 3, 2), F64)],
    "panoptic_loss": [((), F32), ((2,), F32)],
    "panoptic_loss_backward": [(MAP4, F32), (FLOW, F32)],
}

# arguments the bindings require in the form the forward returned: they never take a layout
NO_LAYOUT = {"correlation_leaky_into": (0,), "correlation_backward_leaky": (2, 3), "flow_warp_backward_ctx": (2,)}
# arguments the op writes (its schema says so): what a call leaves in them is compared like an output
MUTATED = {"correlation_leaky_into": (0,)}


def on(device, a):
    return torch.from_numpy(np.array(a, order="C")).to(device)         # a fresh C-ordered copy (0-dim stays 0-dim; the shared inputs stay unwritten)


def uniform(device, shape, seed, lo=-1.0, hi=1.0):
    return on(device, hash_uniform(shape, seed, lo, hi))


def scalar(device, seed):
    """A 0-dim upstream gradient of a scalar loss."""
    return on(device, hash_uniform((), seed, 0.5, 2.0))


def same_bits(a, b):
    """Two tensors hold the same bits (NaNs and the sign of zero included), whatever their strides."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def forward(device, name, args):
    """What the contiguous forward call leaves for its backward: the real outputs on a GPU, zeros of the stated shapes elsewhere."""
    if torch.device(device).type == "cuda":
        out = getattr(torch.ops.cerberus, name)(*args)
        return [out] if isinstance(out, torch.Tensor) else list(out)
    return [torch.zeros(shape, dtype=dtype, device=device) for shape, dtype in OUTPUTS[name]]


def lay(t, layout):
    """``t`` (contiguous) in ``layout``: the same values, other strides, storage offset 0."""
    if layout == "contiguous" or t.dim() == 0:
        return t
    if layout == "channels_last":
        if t.dim() == 4:
            return t.to(memory_format=torch.channels_last)
        if t.dim() == 3:
            return t.transpose(1, 2).contiguous().transpose(1, 2)
        return t
    if layout == "sliced":
        wide = t.new_zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],))
        wide[..., ::2] = t
        return wide[..., ::2]
    raise ValueError(layout)


def case(name, device, layout):
    """(args, differentiable) of ``name`` with every tensor argument in ``layout`` (but for ``NO_LAYOUT``)."""
    args, differentiable = CASES[name](device)
    keep = NO_LAYOUT.get(name, ())
    args = [lay(a, layout) if isinstance(a, torch.Tensor) and i not in keep else a for i, a in enumerate(args)]
    return args, tuple(differentiable)


# ---- the correlation family ----------------------------------------------------------------------------------------------------
def _features(d):
    return uniform(d, CORR, 11), uniform(d, CORR, 12)


def _correlation(d):
    return [*_features(d), *CORR_P], (0, 1)


def _correlation_backward(d):
    return [*_features(d), uniform(d, CORR_OUT, 13), *CORR_P], ()


def _correlation_leaky(d):
    return [*_features(d), *CORR_P, 0.1], (0, 1)


def _correlation_leaky_into(d):
    return [uniform(d, CONCAT, 14), *_features(d), CONCAT_AT, *CORR_P, 0.1], ()


def _correlation_backward_leaky(d):
    x1, x2 = _features(d)
    fwd = uniform(d, CONCAT, 14)
    if torch.device(d).type == "cuda":
        torch.ops.cerberus.correlation_leaky_into(fwd, x1, x2, CONCAT_AT, *CORR_P, 0.1)
    return [x1, x2, uniform(d, CONCAT, 15), fwd, CONCAT_AT, *CORR_P, 0.1], ()


def _warp_inputs(d):
    return uniform(d, CORR, 21), uniform(d, FLOW, 22, -3.0, 3.0)


def _warp_correlation_leaky(d):
    x2, flow = _warp_inputs(d)
    return [uniform(d, CORR, 11), x2, flow, 1, 0.1], (0, 1, 2)


# ---- resampling and the warps ----------------------------------------------------------------------------------------------------
def _area_pyramid(d):
    return [uniform(d, IMG, 31, 0.0, 1.0), [9, 12, 3, 4, 4, 5]], ()      # the image's own size, an integer ratio, a ragged one


def _flow_upsample(d):
    return [uniform(d, FLOW, 32, -3.0, 3.0), 2], (0,)


def _flow_upsample_backward(d):
    return [uniform(d, (2, 2, 18, 24), 33), 2], (0,)                      # linear: its gradient is the forward


def _area_resize(d):
    return [uniform(d, IMG, 31, 0.0, 1.0), 4, 5], ()


def _flow_warp(d):
    return [*_warp_inputs(d), 1, 0], (0, 1)


def _flow_warp_backward_ctx(d):
    image, flow = _warp_inputs(d)
    context = forward(d, "flow_warp_ctx", [image, flow, 1, 0])[1]
    return [image, flow, context, uniform(d, CORR, 23), 1, 0, True, True], ()


def _flow_warp_backward(d):
    return [*_warp_inputs(d), uniform(d, CORR, 23), 1, 0, True, True], ()


# ---- unFlowLoss's terms ------------------------------------------------------------------------------------------------------------
def _images(d):
    return uniform(d, IMG, 41, 0.0, 1.0), uniform(d, IMG, 42, 0.0, 1.0)


def _photometric_loss(d):
    return [*_images(d), 0.15, 0.85], (0, 1)


def _photometric_loss_backward(d):
    return [*_images(d), scalar(d, 43), 0.15, 0.85, True, True], ()


def _census_loss(d):
    return [*_images(d), 1], (0, 1)


def _census_loss_backward(d):
    return [*_images(d), scalar(d, 44), 1, True, True], ()


def _corresponding_map(d):
    return [uniform(d, FLOW, 45, -3.0, 3.0), True], ()


def _occlusion_mask_bidirection(d):
    return [uniform(d, FLOW, 45, -3.0, 3.0), uniform(d, FLOW, 46, -3.0, 3.0), 0.01, 0.5], ()


def _edge_smoothness(d):
    return [uniform(d, FLOW, 47, -3.0, 3.0), uniform(d, IMG, 41, 0.0, 1.0), 10.0, 1], (0,)


def _edge_smoothness_backward(d):
    return [uniform(d, FLOW, 47, -3.0, 3.0), uniform(d, IMG, 41, 0.0, 1.0), scalar(d, 48), 10.0, 1], ()


def _reproject_inputs(d):
    B, _, H, W = IMG
    inv_K, K, T = stereo_camera(B, H, W, "rotated")
    proj = np.matmul(K, T)[:, :3, :]
    return [uniform(d, IMG, 51, 0.0, 1.0), on(d, stereo_depth(B, H, W, 52)), on(d, inv_K[:, :3, :3]), on(d, proj)]


def _reproject_warp(d):
    return [*_reproject_inputs(d), 1e-7], (1,)


def _reproject_warp_backward(d):
    return [*_reproject_inputs(d), uniform(d, IMG, 53), 1e-7], ()


# ---- the segmentation losses ---------------------------------------------------------------------------------------------------------
def _seg_inputs(d):
    x, t = seg_ohem_cases.inputs(SEG)
    return [on(d, x), on(d, t), on(d, seg_ohem_cases.class_weights(SEG[1]))]


def _seg_cross_entropy(d):
    return [*_seg_inputs(d), IGNORE, 2.0], (0,)


def _seg_cross_entropy_backward(d):
    x, t, w = _seg_inputs(d)
    _, lse, state = forward(d, "seg_cross_entropy", [x, t, w, IGNORE, 2.0])
    return [x, t, w, lse, state, scalar(d, 61), IGNORE], ()


def _class_histogram(d):
    return [on(d, seg_ohem_cases.inputs(SEG)[1]), SEG[1], IGNORE], ()


def _seg_ohem_cross_entropy(d):
    return [*_seg_inputs(d), IGNORE, 0.7, OHEM_MIN_KEPT], (0,)


def _seg_ohem_cross_entropy_backward(d):
    x, t, w = _seg_inputs(d)
    _, prob, lse, state, _ = forward(d, "seg_ohem_cross_entropy", [x, t, w, IGNORE, 0.7, OHEM_MIN_KEPT])
    return [x, t, w, prob, lse, state, scalar(d, 62), IGNORE], ()


def _rmi_inputs(d):
    return [on(d, rmi_cases.logits(RMI, 71)), on(d, rmi_cases.labels(RMI, 72))]


def _rmi_moments(d):
    return [*_rmi_inputs(d), 3, 4, True], (0,)


def _rmi_moments_backward(d):
    x, t = _rmi_inputs(d)
    _, _, _, _, la_map, pr_map, means, state = forward(d, "rmi_moments", [x, t, 3, 4, True])
    cov = (2, 5, 9, 9)
    return [x, t, la_map, pr_map, means, state, scalar(d, 73), on(d, hash_uniform(cov, 74, dtype=np.float64)),
            on(d, hash_uniform(cov, 75, dtype=np.float64)), 3, 4, True], ()


# ---- depth ---------------------------------------------------------------------------------------------------------------------------
def _huber_inputs(d):
    gt = hash_uniform(HUBER_GT, 82, 0.01, 5.0)
    gt[hash_uniform(HUBER_GT, 83, 0.0, 1.0) < 0.4] = 0.0                 # no measurement
    return [uniform(d, HUBER_PRED, 81, -1.0, 6.0), on(d, gt)]


def _inv_huber(d):
    return _huber_inputs(d), (0,)


def _inv_huber_backward(d):
    pred, gt = _huber_inputs(d)
    return [pred, gt, forward(d, "inv_huber", [pred, gt])[1], scalar(d, 84)], ()


# ---- the metrics ---------------------------------------------------------------------------------------------------------------------
def _seg_confusion(d):
    x, t, _ = _seg_inputs(d)
    return [x, t, IGNORE], ()


def _depth_metric_sums(d):
    gt = hash_uniform(MAP3, 91, 0.5, 100.0)
    pred = (gt * np.exp(hash_uniform(MAP3, 92, -1.0, 1.0))).astype(np.float32)[:, None]
    gt[hash_uniform(MAP3, 93, 0.0, 1.0) < 0.1] = 0.0
    return [on(d, pred), on(d, gt), 0.001, 80.0], ()


def _flow_metric_sums(d):
    gt = hash_uniform(FLOW, 94, -20.0, 20.0)
    pred = (gt + 8.0 * hash_uniform(FLOW, 95) ** 3).astype(np.float32)
    mask = (hash_uniform(MAP3, 96, 0.0, 1.0) < 0.8).astype(np.float32)
    return [on(d, pred), on(d, gt), on(d, mask)], ()


def _warp_sad(d):
    return [uniform(d, IMG, 97, 0.0, 1.0), uniform(d, IMG, 98, 0.0, 1.0), uniform(d, FLOW, 99, -3.0, 3.0)], ()


def _center_peaks(d):
    return [on(d, panoptic_cases.heatmap(MAP4, 100)), 0.1, 3], ()


def _group_pixels(d):
    centers, counts, offsets = panoptic_cases.group_gpu_inputs(MAP3, [5, 2], "quarter")
    sem = panoptic_cases.labels(MAP3, 401)
    return [on(d, offsets), on(d, centers), on(d, counts), on(d, sem), sum(1 << c for c in panoptic_cases.THINGS)], ()


def _instance_overlap(d):
    return [*(on(d, m) for m in panoptic_cases.id_maps(MAP3, 402, 4, 5)), 4, 5], ()


# ---- panoptic training ---------------------------------------------------------------------------------------------------------------
def _panoptic_targets(d):
    from cerberusnet_amd.utilities.panoptic_targets import gaussian_table
    ids, sid, cat, crowd, count, _segs, kwargs = panoptic_train_cases.target_case("vector")
    flags = (np.isin(cat, kwargs["thing_list"]).astype(np.int32) | ((crowd != 0).astype(np.int32) << 1)).astype(np.int32)
    sigma = kwargs["sigma"]
    gauss = gaussian_table(sigma).clone().to(d)
    return [on(d, ids), on(d, sid), on(d, cat), on(d, flags), on(d, count), gauss, kwargs["ignore_label"], sigma,
            kwargs["ignore_stuff_in_offset"], kwargs["small_instance_area"], float(kwargs["small_instance_weight"]),
            kwargs["ignore_crowd_in_semantic"]], ()


def _panoptic_loss_inputs(d):
    return [on(d, a) for a in panoptic_train_cases.loss_inputs(MAP3)]


def _panoptic_loss(d):
    return [*_panoptic_loss_inputs(d), 200.0, 0.01, 0], (0, 3)


def _panoptic_loss_backward(d):
    ts = _panoptic_loss_inputs(d)
    state = forward(d, "panoptic_loss", [*ts, 200.0, 0.01, 0])[1]
    return [*ts, state, scalar(d, 111), 0], ()


CASES = {
    "correlation": _correlation,
    "correlation_backward": _correlation_backward,
    "correlation_leaky": _correlation_leaky,
    "correlation_leaky_into": _correlation_leaky_into,
    "correlation_backward_leaky": _correlation_backward_leaky,
    "warp_correlation_leaky": _warp_correlation_leaky,
    "area_pyramid": _area_pyramid,
    "flow_upsample": _flow_upsample,
    "flow_upsample_backward": _flow_upsample_backward,
    "area_resize": _area_resize,
    "flow_warp": _flow_warp,
    "flow_warp_ctx": _flow_warp,
    "flow_warp_backward_ctx": _flow_warp_backward_ctx,
    "flow_warp_backward": _flow_warp_backward,
    "photometric_loss": _photometric_loss,
    "photometric_loss_backward": _photometric_loss_backward,
    "census_loss": _census_loss,
    "census_loss_backward": _census_loss_backward,
    "corresponding_map": _corresponding_map,
    "occlusion_mask_bidirection": _occlusion_mask_bidirection,
    "reproject_warp": _reproject_warp,
    "reproject_warp_backward": _reproject_warp_backward,
    "seg_cross_entropy": _seg_cross_entropy,
    "seg_cross_entropy_backward": _seg_cross_entropy_backward,
    "class_histogram": _class_histogram,
    "seg_ohem_cross_entropy": _seg_ohem_cross_entropy,
    "seg_ohem_cross_entropy_backward": _seg_ohem_cross_entropy_backward,
    "inv_huber": _inv_huber,
    "inv_huber_backward": _inv_huber_backward,
    "seg_confusion": _seg_confusion,
    "depth_metric_sums": _depth_metric_sums,
    "flow_metric_sums": _flow_metric_sums,
    "warp_sad": _warp_sad,
    "center_peaks": _center_peaks,
    "group_pixels": _group_pixels,
    "instance_overlap": _instance_overlap,
    "rmi_moments": _rmi_moments,
    "rmi_moments_backward": _rmi_moments_backward,
    "edge_smoothness": _edge_smoothness,
    "edge_smoothness_backward": _edge_smoothness_backward,
    "panoptic_targets": _panoptic_targets,
    "panoptic_loss": _panoptic_loss,
    "panoptic_loss_backward": _panoptic_loss_backward,
}
