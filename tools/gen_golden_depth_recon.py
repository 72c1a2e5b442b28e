#!/usr/bin/env python3
"""Generate tests/golden/depth_recon.npz by running the REFERENCE's DepthReconstructionLossV1 on the CPU.

Runs only where the reference tree is present; the fixture it writes is committed.  Nothing from the reference is copied:
its modules are imported from where they lie (gen_golden.py's load-by-path recipe) and only inputs / outputs are saved.
The reference calls ``.cuda()`` on the camera matrices; ``torch.Tensor.cuda`` is a no-op for the duration of the run.

Per case (a: 2x3x37x53, b: 1x3x16x40): the two images, the camera, a depth and a disparity prediction; and for ssim on /
off and pred_type depth / disparity the loss value, the gradient of the prediction and 64 sampled pixels of the warped image
(the output of the reference's grid_sample call).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

CASES = {"a": (2, 3, 37, 53), "b": (1, 3, 16, 40)}


def inputs(shape, seed):
    from cerberusnet_amd.synth import hash_uniform, stereo_camera, stereo_depth
    B, C, H, W = shape
    coarse = torch.from_numpy(hash_uniform((B, C, max(2, H // 4), max(2, (W + 8) // 4)), seed, 0.0, 1.0))
    field = torch.nn.functional.interpolate(coarse, size=(H, W + 8), mode="bilinear", align_corners=True).numpy()
    rec = {"l_img": (field[..., 4:-4] + hash_uniform(shape, seed + 1, -0.02, 0.02)).astype(np.float32),
           "r_img": (field[..., 8:] + hash_uniform(shape, seed + 2, -0.02, 0.02)).astype(np.float32)}
    rec["inv_K"], rec["K"], rec["T"] = stereo_camera(B, H, W, "cityscapes")
    for pred_type in ("depth", "disparity"):
        rec["pred_" + pred_type] = stereo_depth(B, H, W, seed + 3, 1.0, 6.0, pred_type)
    return rec


def main():
    gen_golden.import_reference()
    mod = gen_golden._load("nnet_training.loss_functions.depth_losses",
                           os.path.join(gen_golden.REF, "loss_functions", "depth_losses.py"))
    torch.set_num_threads(8)
    real_cuda, real_sample = torch.Tensor.cuda, torch.nn.functional.grid_sample
    warped = []

    def sample(*args, **kwargs):
        warped.append(real_sample(*args, **kwargs))
        return warped[-1]

    torch.Tensor.cuda = lambda self, *_a, **_k: self
    torch.nn.functional.grid_sample = sample
    out = {}
    try:
        for tag, shape in CASES.items():
            rec = inputs(shape, 500 + ord(tag))
            B, _, H, W = shape
            targets = {"l_img": torch.from_numpy(rec["l_img"]), "r_img": torch.from_numpy(rec["r_img"]),
                       "camera": {"inv_K": torch.from_numpy(rec["inv_K"]), "K": torch.from_numpy(rec["K"]),
                                  "baseline_T": torch.from_numpy(rec["T"])}}
            for ssim in (True, False):
                for pred_type in ("depth", "disparity"):
                    key = "%s_%d" % (pred_type, int(ssim))
                    pred = torch.from_numpy(rec["pred_" + pred_type]).requires_grad_(True)
                    loss = mod.DepthReconstructionLossV1(B, H, W, pred_type=pred_type, ssim=ssim)({"depth": pred}, targets)
                    grad, = torch.autograd.grad(loss, pred)
                    rec["loss_" + key] = np.float32(loss.item())
                    rec["grad_" + key] = grad.numpy()
                    rec["widx_" + key], rec["wval_" + key] = gen_golden.sampled(warped[-1].detach().numpy())
            out.update({"%s_%s" % (tag, k): v for k, v in rec.items()})
    finally:
        torch.Tensor.cuda, torch.nn.functional.grid_sample = real_cuda, real_sample
    path = os.path.join(gen_golden.OUT, "depth_recon.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
