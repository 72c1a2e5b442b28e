#!/usr/bin/env python3
"""Generate tests/golden/ocr_head.npz by running the REFERENCE's own OCR_block on the CPU.

Runs only where the reference tree is present; the fixture it writes is committed.  Nothing from the reference is copied:
``nnet_models/ocr_utils.py``, ``nnet_models/nnet_ops.py`` and ``nnet_models/ocrnet.py`` are imported from where they lie (the
load-by-path recipe of gen_golden_panoptic.py) and only the seeded input of tests/ocr_cases.py and the reference's outputs are
saved.  ``ocrnet.py`` imports the backbone module, which OCR_block never touches: it gets an empty stand-in.

The block (24 -> 16 mid, 8 key channels, 5 classes, input (2,24,9,12)) runs in train mode with its one Dropout2d set to p = 0 after
construction (tests/ocr_cases.make_block): the BatchNorm layers use their batch statistics and nothing is random.
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

sys.path.insert(0, os.path.join(gen_golden.REPO, "tests"))
import ocr_cases as cases  # noqa: E402


def load_reference():
    models = os.path.join(gen_golden.REF, "nnet_models")
    for name, path in (("nnet_training", gen_golden.REF), ("nnet_training.nnet_models", models)):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    backbone = types.ModuleType("nnet_training.nnet_models.hrnetv2")
    backbone.get_seg_model = None
    sys.modules[backbone.__name__] = backbone
    for name in ("nnet_ops", "ocr_utils"):
        gen_golden._load("nnet_training.nnet_models." + name, os.path.join(models, name + ".py"))
    return gen_golden._load("nnet_training.nnet_models.ocrnet", os.path.join(models, "ocrnet.py")).OCR_block


def main():
    OCR_block = load_reference()
    torch.set_num_threads(8)
    block = cases.make_block(OCR_block)
    x = cases.block_input().requires_grad_(True)
    cls_out, aux_out, ocr_feats = block(x)
    loss = cases.block_loss(cls_out, aux_out, ocr_feats)
    loss.backward()
    state = block.state_dict()
    out = {
        "keys": np.array(list(state.keys())),
        "shapes": np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in state.values()], dtype=np.int64),
        "input": x.detach().numpy(),
        "cls_out": cls_out.detach().numpy(), "aux_out": aux_out.detach().numpy(), "ocr_feats": ocr_feats.detach().numpy(),
        "loss": np.float64(loss.item()),
        "grad_input": x.grad.numpy(),
        "grad_names": np.array([n for n, _ in block.named_parameters()]),
        "grad_norms": np.array([float(p.grad.double().norm()) for _, p in block.named_parameters()], dtype=np.float64),
    }
    path = os.path.join(gen_golden.OUT, "ocr_head.npz")
    np.savez_compressed(path, **out)
    print("loss %.9g, %d state entries, %d parameters" % (loss.item(), len(state), len(out["grad_names"])))
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
