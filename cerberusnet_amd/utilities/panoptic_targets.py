"""Panoptic-DeepLab training targets, generated on the device from the id map the augmentation left behind.

Drop-in for ``nnet_training/datasets/cityscapes_panoptic_transform.py``: ``PanopticTargetGenerator`` keeps its name, its
constructor arguments, ``generated_items``, ``rgb2id`` and ``__call__(panoptic, segments)``; ``panoptic_targets`` is the
batched function under it.  The reference is a host numpy loop in the data loader that runs BEFORE the synchronised crop,
flip and scale: a cropped instance keeps the centre of its uncropped mask and a flipped image keeps offsets that point the
wrong way.  Called on the already augmented id map, this module has neither problem.

For every image, from its id map and a table of segments (id, category, iscrowd; ``seg_count[b]`` live rows, rows past it are
ignored whatever they hold):

* a pixel's row is the live row whose id it holds, if any.  Ids among an image's live rows must be distinct; the result is
  otherwise unspecified.
* per row: the pixel count n and the centre ``(mean y, mean x)`` in float64 -- exactly ``double(sum y) / double(n)``, the sums
  being integers; a row has a centre if its category is in ``thing_list`` and n > 0, and is small if n < ``small_instance_area``
* ``semantic`` (int64): the row's category, ``ignore_label`` without a row (or on crowd rows with ``ignore_crowd_in_semantic``);
  ``foreground`` (int64): things; ``center`` (B,1,H,W): the maximum over the image's centres of the (6 sigma + 3)^2 Gaussian
  window around ``(int(cy), int(cx))``; ``offset`` (B,2,H,W): ``float32(cy - y), float32(cx - x)`` on things (a float64
  subtraction rounded once, as numpy 2 evaluates the reference); ``semantic_mask``: ``small_instance_weight`` on small things,
  else 1; ``center_mask``: rows that are not crowd; ``offset_mask``: the same, things only with ``ignore_stuff_in_offset``
* ``center_points`` (B,S,2) float64: ``(cy, cx)`` per row, NaN for a row without a centre

The reference keeps ``semantic`` and the masks in uint8 arrays; here a category or a weight is stored as given (nothing wraps
at 256, a fractional ``small_instance_weight`` is not truncated).

``backend='hip'`` (default): CUDA id maps with at most ``ops.PANOPTIC_TARGETS_MAX_SEGMENTS`` (256) table rows take
``cerberus::panoptic_targets`` (``csrc/panoptic_train.hip``: a zero-fill and three launches, integer moments, no host read).
CPU tensors, more rows and ``backend='torch'`` take the stock route below: the same arithmetic restated in device-agnostic
torch ops (float64 centres, no numpy, no host read), one pass per table row.  Both give the same bits.
"""
import functools

import numpy as np
import torch

from .. import ops

__all__ = ["panoptic_targets", "PanopticTargetGenerator", "gaussian_table"]

GENERATED_ITEMS = ['semantic', 'foreground', 'center', 'offset', 'semantic_mask', 'center_mask', 'offset_mask']


def _int_sigma(sigma):
    if isinstance(sigma, bool) or int(sigma) != sigma or sigma < 1:
        raise ValueError("sigma must be a positive integer (the Gaussian window has 6 sigma + 3 pixels a side), got %r" % (sigma,))
    return int(sigma)


@functools.lru_cache(maxsize=16)
def _gaussian_numpy(sigma):
    size = 6 * sigma + 3
    x = np.arange(0, size, 1, np.float64)
    y = x[:, np.newaxis]
    c = 3 * sigma + 1
    return np.exp(-((x - c) ** 2 + (y - c) ** 2) / (2 * sigma ** 2)).astype(np.float32)


@functools.lru_cache(maxsize=16)
def _gaussian_on(sigma, device):
    return torch.from_numpy(_gaussian_numpy(sigma)).to(device)


@functools.lru_cache(maxsize=16)
def _things_on(things, device):
    return torch.as_tensor(list(things), dtype=torch.int64, device=device)


def gaussian_table(sigma, device="cpu"):
    """The (6 sigma + 3, 6 sigma + 3) float32 window the centre heat map is made of: the reference's float64 formula, rounded
    once.  Made once per sigma and device; the kernels never call exp."""
    return _gaussian_on(_int_sigma(sigma), torch.device(device))


def _stock(ids, seg_ids, seg_category, flags, seg_count, gauss, ignore_label, sigma, ignore_stuff_in_offset, small_instance_area,
           small_instance_weight, ignore_crowd_in_semantic):
    B, H, W = ids.shape
    S = seg_ids.shape[1]
    dev = ids.device
    live = torch.arange(S, device=dev)[None, :] < seg_count[:, None]                      # (B,S)
    row = torch.full((B, H, W), -1, dtype=torch.int64, device=dev)
    for s in range(S):          # the first live row that holds the pixel's id
        hit = (ids == seg_ids[:, s, None, None]) & live[:, s, None, None] & (row < 0)
        row = torch.where(hit, torch.full_like(row, s), row)
    has_row = row >= 0
    r = row.clamp(min=0).reshape(B, -1)
    ys = torch.arange(H, device=dev, dtype=torch.int64)[:, None].expand(H, W)
    xs = torch.arange(W, device=dev, dtype=torch.int64)[None, :].expand(H, W)
    bin_ = (row + 1).reshape(B, -1)                                                          # bin 0: no row
    zeros = lambda: torch.zeros((B, S + 1), dtype=torch.int64, device=dev)
    n = zeros().scatter_add_(1, bin_, torch.ones_like(bin_))[:, 1:]                          # integer sums: exact in any order
    sy = zeros().scatter_add_(1, bin_, ys.reshape(1, -1).expand(B, -1))[:, 1:]
    sx = zeros().scatter_add_(1, bin_, xs.reshape(1, -1).expand(B, -1))[:, 1:]
    thing = live & ((flags & 1) != 0)
    crowd = live & ((flags & 2) != 0)
    has = thing & (n > 0)
    small = has & (n < small_instance_area)
    safe = n.clamp(min=1).double()
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    cy = torch.where(has, sy.double() / safe, nan)
    cx = torch.where(has, sx.double() / safe, nan)
    iy = torch.where(has, cy, torch.zeros_like(cy)).long()
    ix = torch.where(has, cx, torch.zeros_like(cx)).long()

    at = lambda t: t.gather(1, r).reshape(B, H, W)                                            # a row's attribute at every pixel
    p_thing, p_crowd = has_row & at(thing), has_row & at(crowd)
    ignore = torch.full((), ignore_label, dtype=torch.int64, device=dev)
    drop = ~has_row | (p_crowd if ignore_crowd_in_semantic else torch.zeros_like(has_row))
    semantic = torch.where(drop, ignore, at(seg_category))
    foreground = p_thing.long()
    one = torch.ones((), dtype=torch.float32, device=dev)
    semantic_mask = torch.where(has_row & at(small), torch.full((), float(small_instance_weight), dtype=torch.float32, device=dev), one)
    center_mask = (has_row & ~p_crowd).float()
    offset_mask = (has_row & ~p_crowd & (p_thing if ignore_stuff_in_offset else torch.ones_like(has_row))).float()
    zero64 = torch.zeros((), dtype=torch.float64, device=dev)
    off_y = torch.where(p_thing, at(cy) - ys.double(), zero64).float()                       # float64, rounded once
    off_x = torch.where(p_thing, at(cx) - xs.double(), zero64).float()
    offset = torch.stack([off_y, off_x], 1)

    size, reach = 6 * sigma + 3, 3 * sigma + 1
    center = torch.zeros((B, H, W), dtype=torch.float32, device=dev)
    yy = torch.arange(H, device=dev)[None, :]
    xx = torch.arange(W, device=dev)[None, :]
    for s in range(S):          # a maximum: any order
        gy = yy - (iy[:, s, None] - reach)                                                   # (B,H)
        gx = xx - (ix[:, s, None] - reach)                                                   # (B,W)
        ok = (has[:, s, None, None] & ((gy >= 0) & (gy < size))[:, :, None] & ((gx >= 0) & (gx < size))[:, None, :])
        window = gauss[gy.clamp(0, size - 1)[:, :, None], gx.clamp(0, size - 1)[:, None, :]]
        center = torch.maximum(center, torch.where(ok, window, torch.zeros_like(window)))
    return (semantic, foreground, center[:, None], offset, semantic_mask, center_mask, offset_mask, torch.stack([cy, cx], 2))


def panoptic_targets(ids, seg_ids, seg_category, seg_iscrowd, seg_count=None, *, ignore_label, thing_list, sigma=8,
                     ignore_stuff_in_offset=False, small_instance_area=0, small_instance_weight=1, ignore_crowd_in_semantic=False,
                     backend="hip"):
    """The training targets of a batch.  ``ids`` (B,H,W) int32 or int64: the decoded panoptic id map (after the augmentation);
    ``seg_ids``, ``seg_category``, ``seg_iscrowd`` (B,S): the padded segment tables; ``seg_count`` (B,): the live rows of each
    image (default: all S).  Returns a dict of ``semantic``, ``foreground`` (int64 (B,H,W)), ``center`` (B,1,H,W), ``offset``
    (B,2,H,W), ``semantic_mask``, ``center_mask``, ``offset_mask`` (float32 (B,H,W)) and ``center_points`` (B,S,2) float64 (NaN
    for a row without a centre).  Nothing is read back to the host."""
    if backend not in ("hip", "torch"):
        raise ValueError("backend must be 'hip' or 'torch'")
    sigma = _int_sigma(sigma)
    if ids.dim() != 3 or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError("ids must be a (B,H,W) int32 or int64 tensor, got %s %s" % (tuple(ids.shape), ids.dtype))
    B = ids.shape[0]
    if seg_ids.dim() != 2 or seg_ids.shape[0] != B or seg_category.shape != seg_ids.shape or seg_iscrowd.shape != seg_ids.shape:
        raise ValueError("seg_ids, seg_category and seg_iscrowd must be (B,S) with B = %d, got %s, %s, %s"
                         % (B, tuple(seg_ids.shape), tuple(seg_category.shape), tuple(seg_iscrowd.shape)))
    dev = ids.device
    S = seg_ids.shape[1]
    seg_ids, seg_category = seg_ids.to(dev, torch.int64), seg_category.to(dev, torch.int64)
    if seg_count is None:
        seg_count = torch.full((B,), S, dtype=torch.int64, device=dev)
    elif tuple(seg_count.shape) != (B,):
        raise ValueError("seg_count must be (B,) with B = %d, got %s" % (B, tuple(seg_count.shape)))
    seg_count = seg_count.to(dev, torch.int64)
    things = _things_on(tuple(int(c) for c in thing_list), dev)       # made once: no upload in a captured call
    flags = (torch.isin(seg_category, things).to(torch.int32) | ((seg_iscrowd.to(dev) != 0).to(torch.int32) << 1))
    gauss = gaussian_table(sigma, dev)
    args = (int(ignore_label), sigma, bool(ignore_stuff_in_offset), int(small_instance_area), float(small_instance_weight),
            bool(ignore_crowd_in_semantic))
    if S == 0 or ids.numel() == 0:
        raise ValueError("needs at least one pixel and one table row (an image without segments has seg_count 0), got ids %s and "
                         "S = %d" % (tuple(ids.shape), S))
    if backend == "hip" and ids.is_cuda and S <= ops.PANOPTIC_TARGETS_MAX_SEGMENTS:
        out = torch.ops.cerberus.panoptic_targets(ids, seg_ids, seg_category, flags, seg_count, gauss, *args)
    else:
        out = _stock(ids, seg_ids, seg_category, flags, seg_count, gauss, *args)
    return dict(zip(GENERATED_ITEMS + ["center_points"], out))


class PanopticTargetGenerator:
    """The reference's generator, one image at a time: ``__call__(panoptic, segments)`` takes the colour-coded (H,W,3) array and
    the list of segment dicts (``id``, ``category_id``, ``iscrowd``) and returns the reference's dict -- every map with a
    leading dimension of 1, on ``device``, and ``center_points`` as a list of ``[y, x]`` in table order.  That list is the one
    host read of this class; ``panoptic_targets`` has none."""

    generated_items = list(GENERATED_ITEMS)

    def __init__(self, ignore_label, thing_list, sigma=8, ignore_stuff_in_offset=False, small_instance_area=0,
                 small_instance_weight=1, ignore_crowd_in_semantic=False, backend="hip", device=None):
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        self.ignore_label = ignore_label
        self.thing_list = thing_list
        self.ignore_stuff_in_offset = ignore_stuff_in_offset
        self.small_instance_area = small_instance_area
        self.small_instance_weight = small_instance_weight
        self.ignore_crowd_in_semantic = ignore_crowd_in_semantic
        self.sigma = _int_sigma(sigma)
        self.backend = backend
        if device is None:
            device = "cuda" if backend == "hip" and torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.g = gaussian_table(self.sigma, self.device)

    @staticmethod
    def rgb2id(color):
        """The panoptic id of a colour ``[id % 256, id // 256 % 256, id // 65536]``: an (H,W,3) array gives an (H,W) map, a
        triple gives an int."""
        if isinstance(color, np.ndarray) and color.ndim == 3:
            c = color.astype(np.int32) if color.dtype == np.uint8 else color
            return c[:, :, 0] + 256 * c[:, :, 1] + 256 * 256 * c[:, :, 2]
        return int(color[0] + 256 * color[1] + 256 * 256 * color[2])

    def __call__(self, panoptic, segments):
        ids = torch.as_tensor(np.ascontiguousarray(self.rgb2id(np.asarray(panoptic)))).to(self.device)
        if ids.dtype not in (torch.int32, torch.int64):
            ids = ids.long()
        rows = max(len(segments), 1)
        table = torch.zeros((3, 1, rows), dtype=torch.int64)
        for i, seg in enumerate(segments):
            table[0, 0, i], table[1, 0, i], table[2, 0, i] = int(seg["id"]), int(seg["category_id"]), int(bool(seg["iscrowd"]))
        table = table.to(self.device)
        count = torch.full((1,), len(segments), dtype=torch.int64, device=self.device)
        out = panoptic_targets(ids[None], table[0], table[1], table[2], count, ignore_label=self.ignore_label, thing_list=self.thing_list,
                               sigma=self.sigma, ignore_stuff_in_offset=self.ignore_stuff_in_offset,
                               small_instance_area=self.small_instance_area, small_instance_weight=self.small_instance_weight,
                               ignore_crowd_in_semantic=self.ignore_crowd_in_semantic, backend=self.backend)
        points = out["center_points"][0]
        out["center_points"] = points[~torch.isnan(points[:, 0])].tolist()         # the one host read
        return out
