#!/usr/bin/env python3
"""Generate tests/golden/photometric.npz by running the REFERENCE's own SSIM module, smooth_grad_1st, smooth_grad_2nd and
unFlowLoss on the CPU with one thread, once in float32 and once in float64 (its Python is dtype-agnostic here).

Runs only where the reference tree lies (as tools/gen_golden.py, whose import recipe it uses); nothing of the reference is
copied: its modules are imported from where they lie and only results are saved.  Inputs come from
``cerberusnet_amd.synth.hash_uniform`` (tests/photometric_cases.py names the seeds), so the file holds results, not inputs:

  * per photometric case ``p<i>_``: shape, family, and per dtype (``f32_`` / ``f64_``) the map
    ``SSIM(im_recons, im_orig)`` (the module's output: ``clamp((1 - SSIM) / 2, 0, 1)``), the L1 and the SSIM mean
    (``unFlowLoss(weights={"l1": 1})`` / ``{"ssim": 1}`` ``.loss_photometric`` with the all-ones mask ``forward`` passes)
    and the gradients of each mean with respect to both images; in float32 also ``mix``, the same for the summed loss
    with the weights ``cases.WEIGHT_PAIRS[0]`` (in float64 it is the weighted sum of the two terms to 1e-14, in float32
    only to the rounding of an SSIM gradient, up to 2e-5 of its maximum); ``ssim_margin``: the smallest ``|arg - 1|`` over the
    float64 windows, ``arg`` the clamp's argument, taken from the module's own ``torch.clamp`` call;
  * per smoothness case ``s<i>_``: shape, image channels, degree, alpha, family, and per dtype the value and its
    gradients with respect to the flow and to the image;
  * per whole-loss configuration ``l<name>_``: the value in both dtypes, the indices (into forward + backward flows) of
    the flows the loss uses and the float64 gradient of each of them saved as a float32 array; every other flow is
    asserted to get no gradient (None, or the zeros ``torch.cat`` hands to a backward flow without consistency);
    ``ldefault_``: the value with the default keywords on the same inputs.

The inputs are conditioned, not filtered: ``ssim_margin >= cases.SSIM_MARGIN`` is asserted for every photometric case (the
clamp's corner at SSIM = -1 is nowhere near), so the tests never leave an element out of a comparison.

Size: the per-element float32 and float64 results of the listed cases are about 46 800 values of 12 bytes, mostly
incompressible mantissas, which alone exceed tests/golden/depth_recon.npz (208 058 bytes); dropping the whole-loss
gradients of the coarse scales would save about 5 KB of that and is therefore not done: all of them are stored.  (The L1
gradients, sign / N, compress to 12 KB in all.)
"""
import contextlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import photometric_cases as cases        # noqa: E402
from gen_golden import import_reference  # noqa: E402


@contextlib.contextmanager
def recorded_clamp(seen):
    """Keep the argument of every ``torch.clamp`` call made inside the block."""
    real = torch.clamp

    def clamp(x, *a, **k):
        seen.append(x.detach().clone())
        return real(x, *a, **k)
    torch.clamp = clamp
    try:
        yield
    finally:
        torch.clamp = real


def photometric(unflow, rec):
    ssim = unflow.SSIM()
    for i, (shape, family) in enumerate(cases.PHOTO_CASES):
        orig, recons = cases.photo_images(i)
        rec.update({"p%d_shape" % i: np.array(shape), "p%d_family" % i: np.array(family)})
        for tag, dtype in cases.DTYPES:
            o = torch.from_numpy(orig).to(dtype).requires_grad_(True)
            r = torch.from_numpy(recons).to(dtype).requires_grad_(True)
            seen = []
            with recorded_clamp(seen):
                rec["p%d_%s_map" % (i, tag)] = ssim(r, o).detach().numpy()
            assert len(seen) == 1 and seen[0].shape == tuple(shape)
            if dtype == torch.float64:
                margin = float((seen[0] - 1).abs().min())
                rec["p%d_ssim_margin" % i] = np.float64(margin)
                assert margin >= cases.SSIM_MARGIN, "case %d: ssim_margin %.3e: advance PHOTO_SEED" % (i, margin)
            ones = torch.ones_like(o)
            terms = {"l1": {"l1": 1.0}, "ssim": {"ssim": 1.0}}
            if dtype == torch.float32:        # the summed loss is linear in its terms only up to float32 rounding
                terms["mix"] = dict(zip(("l1", "ssim"), cases.WEIGHT_PAIRS[0]))
            for term, weights in terms.items():
                v = unflow.unFlowLoss(weights=weights).loss_photometric(o, r, ones)
                go, gr = torch.autograd.grad(v, (o, r))
                assert v.dtype == dtype and go.dtype == dtype
                rec.update({"p%d_%s_%s" % (i, tag, term): v.detach().numpy(), "p%d_%s_%s_grad_orig" % (i, tag, term): go.numpy(),
                            "p%d_%s_%s_grad_recons" % (i, tag, term): gr.numpy()})
        print("photometric %d %s %s: L1 %.9g SSIM %.9g ssim_margin %.3e map range [%.3e, %.3e]" % (
            i, shape, family, float(rec["p%d_f64_l1" % i]), float(rec["p%d_f64_ssim" % i]), float(rec["p%d_ssim_margin" % i]),
            rec["p%d_f64_map" % i].min(), rec["p%d_f64_map" % i].max()))


def smoothness(unflow, rec):
    for i, (shape, channels, degree, alpha, family) in enumerate(cases.SMOOTH_CASES):
        flow, image = cases.smooth_inputs(i)
        rec.update({"s%d_shape" % i: np.array(shape), "s%d_channels" % i: np.int64(channels), "s%d_degree" % i: np.int64(degree),
                    "s%d_alpha" % i: np.float64(alpha), "s%d_family" % i: np.array(family)})
        fn = {1: unflow.smooth_grad_1st, 2: unflow.smooth_grad_2nd}[degree]
        for tag, dtype in cases.DTYPES:
            f = torch.from_numpy(flow).to(dtype).requires_grad_(True)
            im = torch.from_numpy(image).to(dtype).requires_grad_(True)
            v = fn(f, im, alpha)
            gf, gi = torch.autograd.grad(v, (f, im))
            assert v.dtype == dtype and gf.dtype == dtype
            rec.update({"s%d_%s_value" % (i, tag): v.detach().numpy(), "s%d_%s_grad_flow" % (i, tag): gf.numpy(),
                        "s%d_%s_grad_image" % (i, tag): gi.numpy()})
        print("smoothness %d %s degree %d alpha %g %s: %.9g" % (i, shape, degree, alpha, family, float(rec["s%d_f64_value" % i])))


def whole_loss(unflow, rec):
    for name, cfg in list(cases.LOSS_CONFIGS.items()) + [("default", {"weights": {"l1": 0.15, "ssim": 0.85}})]:
        for tag, dtype in cases.DTYPES:
            l_img, l_seq, fw, bw = cases.loss_inputs(dtype)
            loss = unflow.unFlowLoss(**cfg)({"flow": fw, "flow_b": bw}, {"l_img": l_img, "l_seq": l_seq})
            assert loss.dtype == dtype
            rec["l%s_%s_value" % (name, tag)] = loss.detach().numpy()
            if dtype != torch.float64 or name == "default":
                continue
            grads = torch.autograd.grad(loss, fw + bw, allow_unused=True)
            used = cases.loss_used(name)
            rec["l%s_used" % name] = np.array(used)
            for j, g in enumerate(grads):
                if j in used:
                    assert float(g.abs().max()) > 0
                    rec["l%s_grad%d" % (name, j)] = g.numpy().astype(np.float32)
                else:
                    assert g is None or not bool(g.any()), (name, j)
        print("unFlowLoss %s: float64 %.12g float32 %.9g" % (name, float(rec["l%s_f64_value" % name]),
                                                             float(rec["l%s_f32_value" % name])))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    _, unflow = import_reference()
    rec = {"n_photo": np.int64(len(cases.PHOTO_CASES)), "n_smooth": np.int64(len(cases.SMOOTH_CASES)),
           "loss_configs": np.array(sorted(cases.LOSS_CONFIGS))}
    photometric(unflow, rec)
    smoothness(unflow, rec)
    whole_loss(unflow, rec)
    out = os.path.join(REPO, "tests", "golden", "photometric.npz")
    np.savez_compressed(out, **rec)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
