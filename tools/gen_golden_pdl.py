#!/usr/bin/env python3
"""Generate tests/golden/pdl_head.npz by running the REFERENCE's own PanopticDeepLabDecoder on the CPU.

Runs only where the reference tree is present; the fixture it writes is committed.  Nothing from the reference is copied:
``nnet_models/aspp.py`` and ``nnet_models/deeplab_panoptic.py`` are imported from where they lie (the load-by-path recipe of
gen_golden_ocr.py) and only the seeded inputs of tests/pdl_cases.py and what the reference computes from them are saved.

The tiny decoder (tests/pdl_cases.CONFIG) runs twice with the same seeded parameters: in ``eval()`` for the three outputs, and in
``train()`` with only its Dropout modules in ``eval()`` (BatchNorm uses its batch statistics, nothing is random) for the loss, the
norms of the gradients of the three feature maps and the norm of every parameter's gradient.
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

sys.path.insert(0, os.path.join(gen_golden.REPO, "tests"))
import pdl_cases as cases  # noqa: E402


def load_reference():
    models = os.path.join(gen_golden.REF, "nnet_models")
    for name, path in (("nnet_training", gen_golden.REF), ("nnet_training.nnet_models", models)):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    gen_golden._load("nnet_training.nnet_models.aspp", os.path.join(models, "aspp.py"))
    return gen_golden._load("nnet_training.nnet_models.deeplab_panoptic", os.path.join(models, "deeplab_panoptic.py")).PanopticDeepLabDecoder


def main():
    decoder_cls = load_reference()
    torch.set_num_threads(8)
    feats = cases.features()
    with torch.no_grad():
        evaluated = cases.make_decoder(decoder_cls, mode="eval")((None, feats))
    net = cases.make_decoder(decoder_cls, mode="train")
    _, loss, grads, norms = cases.run_decoder(net, feats)
    state = net.state_dict()
    out = {
        "keys": np.array(list(state.keys())),
        "shapes": np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in state.values()], dtype=np.int64),
        "loss": np.float64(loss.item()),
        "grad_input_norms": np.array([float(g.double().norm()) for g in grads], dtype=np.float64),
        "grad_names": np.array(list(norms)),
        "grad_norms": np.array(list(norms.values()), dtype=np.float64),
    }
    for i, f in enumerate(feats):
        out["feature%d" % i] = f.numpy()
    for key in cases.OUTPUTS:
        out[key] = evaluated[key].numpy()
    path = os.path.join(gen_golden.OUT, "pdl_head.npz")
    np.savez_compressed(path, **out)
    print("loss %.9g, %d state entries, %d parameters" % (loss.item(), len(state), len(out["grad_names"])))
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
