#!/usr/bin/env python3
"""Generate tests/golden/detr_head.npz by running the REFERENCE's own DETR head on the CPU.

Runs only where the reference tree is present; the fixture it writes is committed.  Nothing from the reference is copied:
``nnet_models/detr/transformer.py``, ``nnet_models/detr/position_encoding.py``, ``nnet_models/detr/detr.py`` (for ``MLP``) and
``nnet_models/detr_sfd.py`` (for ``DetrSegmHead``) are imported from where they lie (the load-by-path recipe of gen_golden_ocr.py).
What they import and the head never uses -- ``misc``, the backbone, the matcher, the mask head (torchvision), the criterion, the
correlation package, the warp, the other heads -- gets empty stand-in modules whose every attribute is an empty class.

The reference's head runs with the sine encoding only: its learned encoding reads ``.tensors`` of a NestedTensor and the head passes
it a plain tensor, so that encoding is compared on its own, through a one-attribute wrapper.

Only outputs and the list of state-dict key names are stored: weights and inputs are regenerated from the seeds of
tests/attn_cases.py on both sides.  Everything runs in ``eval()``: nothing is random.
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

sys.path.insert(0, os.path.join(gen_golden.REPO, "tests"))
import attn_cases as cases  # noqa: E402


class _StandIn(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


class _Tensors:
    """What the reference's learned encoding reads of a NestedTensor."""

    def __init__(self, tensors):
        self.tensors = tensors


def load_reference():
    models = os.path.join(gen_golden.REF, "nnet_models")
    detr = os.path.join(models, "detr")
    for name, path in (("nnet_training", gen_golden.REF), ("nnet_training.nnet_models", models), ("nnet_training.nnet_models.detr", detr),
                       ("nnet_training.loss_functions", None), ("nnet_training.correlation_package", None)):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path] if path else []
        sys.modules[name] = pkg
    for name in ("nnet_models.detr.misc", "nnet_models.detr.box_ops", "nnet_models.detr.backbone", "nnet_models.detr.matcher",
                 "nnet_models.detr.segmentation", "loss_functions.detr_loss", "loss_functions.UnFlowLoss",
                 "correlation_package.correlation", "nnet_models.hrnetv2", "nnet_models.pwcnet_modules", "nnet_models.ocrnet_sfd"):
        full = "nnet_training." + name
        sys.modules[full] = _StandIn(full)
        parent, _, leaf = full.rpartition(".")
        setattr(sys.modules[parent], leaf, sys.modules[full])
    loaded = {}
    for leaf in ("transformer", "position_encoding", "detr"):
        loaded[leaf] = gen_golden._load("nnet_training.nnet_models.detr." + leaf, os.path.join(detr, leaf + ".py"))
    loaded["detr_sfd"] = gen_golden._load("nnet_training.nnet_models.detr_sfd", os.path.join(models, "detr_sfd.py"))
    return loaded


def main():
    ref = load_reference()
    torch.set_num_threads(8)
    out = {}
    x = cases.features()
    with torch.no_grad():
        for tag, pre in (("post", False), ("pre", True)):
            hs, memory = cases.make_transformer(ref["transformer"].Transformer, pre)(*cases.transformer_inputs())
            out["transformer_%s_hs" % tag], out["transformer_%s_memory" % tag] = hs.numpy(), memory.numpy()
        out["pos_sine"] = ref["position_encoding"].PositionEmbeddingSine(32, normalize=True)(x).numpy()
        learned = cases.seed_parameters(ref["position_encoding"].PositionEmbeddingLearned(32), cases.POSITION_SEED)
        out["pos_learned"] = learned(_Tensors(x)).numpy()
        for tag, pre, pos in (("post_sine", False, "sine"), ("pre_sine", True, "sine")):
            head = cases.make_head(ref["detr_sfd"].DetrSegmHead, pre, pos)
            res = head(x)
            assert set(res) == {"logits", "bboxes", "detr_aux"}
            out["head_%s_logits" % tag], out["head_%s_bboxes" % tag] = res["logits"].numpy(), res["bboxes"].numpy()
            out["head_%s_aux_logits" % tag] = torch.stack([a["pred_logits"] for a in res["detr_aux"]]).numpy()
            out["head_%s_aux_bboxes" % tag] = torch.stack([a["pred_boxes"] for a in res["detr_aux"]]).numpy()
            out["head_%s_keys" % tag] = np.array(list(head.state_dict().keys()))
    path = os.path.join(gen_golden.OUT, "detr_head.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays, %d state entries" % (path, os.path.getsize(path), len(out), len(out["head_post_sine_keys"])))


if __name__ == "__main__":
    main()
