"""The DETR head without a GPU: the modules of nnet_models/detr against the reference's own run (tests/golden/detr_head.npz, written
by tools/gen_golden_detr_head.py from the seeds of tests/attn_cases.py), the routes the fused core does not take, and the C entry
points' argument checks."""
import copy
import inspect
import os

import pytest
import torch

import attn_cases as cases
import cerberusnet_amd as ca
import detr_cases as dcase
from cerberusnet_amd import _lib, build, nnet_models, ops_attn
from cerberusnet_amd.nnet_models.detr import transformer as tr
from conftest import rel_err

NEW_NAMES = ["Transformer", "TransformerEncoder", "TransformerDecoder", "TransformerEncoderLayer", "TransformerDecoderLayer",
             "PositionEmbeddingSine", "PositionEmbeddingLearned", "build_position_encoding", "MLP", "DetrSegmHead"]
TOL = 1e-5          # the golden tolerance of test_ocr_head_cpu.py


@pytest.fixture(scope="module")
def gold(golden):
    return golden("detr_head")


def test_state_dict_keys_equal_the_reference(gold):
    for tag, pre in (("post_sine", False), ("pre_sine", True)):
        assert list(cases.make_head(ca.DetrSegmHead, pre, backend="torch").state_dict()) == [str(k) for k in gold["head_%s_keys" % tag]]
    keys = [str(k) for k in gold["head_post_sine_keys"]]
    assert "transformer.encoder.layers.0.self_attn.in_proj_weight" in keys and "transformer.decoder.layers.1.multihead_attn.out_proj.bias" in keys
    assert "transformer.encoder.norm.weight" not in keys and "transformer.encoder.norm.weight" in [str(k) for k in gold["head_pre_sine_keys"]]
    # the backend adds no state
    assert list(cases.make_head(ca.DetrSegmHead, backend="hip").state_dict()) == keys


def test_constructor_defaults_are_the_references():
    d = {k: p.default for k, p in inspect.signature(ca.Transformer.__init__).parameters.items()}
    assert (d["d_model"], d["nhead"], d["encoder_layers"], d["decoder_layers"], d["dim_feedforward"], d["dropout"], d["activation"],
            d["normalize_before"], d["return_intermediate_dec"]) == (512, 8, 6, 6, 2048, 0.1, "relu", False, False)
    assert d["backend"] == tr.DEFAULT_ATTENTION_BACKEND
    # the reference config's misspelt keys are swallowed: 8 heads and 6 + 6 layers are what it really builds
    t = ca.Transformer(d_model=256, dim_feedforward=32, n_heads=4, enc_layers=2, dec_layers=2, hidden_dim=256)
    assert t.nhead == 8 and len(t.encoder.layers) == 6 and len(t.decoder.layers) == 6
    s = {k: p.default for k, p in inspect.signature(ca.DetrSegmHead.__init__).parameters.items()}
    assert list(s)[1:] == ["num_channels", "num_classes", "num_queries", "position_embedding_config", "transformer_config", "aux_loss",
                           "seg_enable", "backend"]
    assert s["aux_loss"] is False and s["seg_enable"] is False
    p = {k: q.default for k, q in inspect.signature(ca.PositionEmbeddingSine.__init__).parameters.items()}
    assert (p["num_pos_feats"], p["temperature"], p["normalize"], p["scale"]) == (64, 10000, False, None)
    with pytest.raises(ValueError, match="normalize should be True"):
        ca.PositionEmbeddingSine(8, scale=1.0)
    with pytest.raises(ValueError, match="not supported"):
        ca.build_position_encoding(type="v9", hidden_dim=8)
    with pytest.raises(ValueError, match="backend"):
        ca.Transformer(d_model=64, nhead=2, backend="triton")


@pytest.mark.parametrize("backend", ["torch", "hip"])
def test_eval_outputs_match_the_reference_run(gold, backend):
    """On CPU tensors 'hip' takes the stock route: the same numbers."""
    x = cases.features()
    with torch.no_grad():
        for tag, pre in (("post", False), ("pre", True)):
            hs, memory = cases.make_transformer(ca.Transformer, pre, backend=backend)(*cases.transformer_inputs())
            assert hs.shape == gold["transformer_%s_hs" % tag].shape == (2, 2, 10, 64)
            assert rel_err(hs.numpy(), gold["transformer_%s_hs" % tag]) < TOL, tag
            assert rel_err(memory.numpy(), gold["transformer_%s_memory" % tag]) < TOL, tag
        for tag, pre in (("post_sine", False), ("pre_sine", True)):
            out = cases.make_head(ca.DetrSegmHead, pre, backend=backend)(x)
            assert set(out) == {"logits", "bboxes", "aux_outputs", "detr_aux"}
            assert out["logits"].shape == (2, 10, 6) and out["bboxes"].shape == (2, 10, 4)
            assert rel_err(out["logits"].numpy(), gold["head_%s_logits" % tag]) < TOL, tag
            assert rel_err(out["bboxes"].numpy(), gold["head_%s_bboxes" % tag]) < TOL, tag
            assert len(out["aux_outputs"]) == len(out["detr_aux"]) == 1
            for i, (mine, theirs) in enumerate(zip(out["aux_outputs"], out["detr_aux"])):
                assert set(mine) == {"logits", "bboxes"} and set(theirs) == {"pred_logits", "pred_boxes"}
                assert mine["logits"] is theirs["pred_logits"] and mine["bboxes"] is theirs["pred_boxes"]
                assert rel_err(mine["logits"].numpy(), gold["head_%s_aux_logits" % tag][i]) < TOL, tag
                assert rel_err(mine["bboxes"].numpy(), gold["head_%s_aux_bboxes" % tag][i]) < TOL, tag
    assert set(cases.make_head(ca.DetrSegmHead, aux_loss=False, backend=backend)(x)) == {"logits", "bboxes"}


def test_position_encodings_match_the_reference_run(gold):
    x = cases.features()
    with torch.no_grad():
        sine = ca.PositionEmbeddingSine(32, normalize=True)(x)
        learned = cases.seed_parameters(ca.PositionEmbeddingLearned(32), cases.POSITION_SEED)(x)
    assert sine.shape == learned.shape == (2, 64, 9, 13)
    assert rel_err(sine.numpy(), gold["pos_sine"]) < TOL and rel_err(learned.numpy(), gold["pos_learned"]) < TOL
    assert isinstance(ca.build_position_encoding(type="sine", hidden_dim=64, d_model=64), ca.PositionEmbeddingSine)
    built = ca.build_position_encoding(type="learned", hidden_dim=64)
    assert isinstance(built, ca.PositionEmbeddingLearned) and built.row_embed.weight.shape == (50, 32)
    # the head with the learned encoding (the reference's own head cannot run it: it hands the encoding a plain tensor)
    out = cases.make_head(ca.DetrSegmHead, pos_type="learned", backend="torch")(x)
    assert out["logits"].shape == (2, 10, 6) and bool(torch.isfinite(out["logits"]).all())


def test_aux_outputs_feed_the_criterion_and_a_backward_reaches_every_parameter():
    head = cases.make_head(ca.DetrSegmHead, backend="torch")
    out = head(cases.features())
    weights = {"loss_ce": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0, "loss_ce_0": 1.0, "loss_bbox_0": 5.0, "loss_giou_0": 2.0}
    crit = ca.DetrLoss(cases.HEAD["num_classes"], weights, 0.1, ["labels", "boxes", "cardinality"], backend="torch",
                       matcher_cfg={"cost_class": 1.0, "cost_bbox": 5.0, "cost_giou": 2.0})
    targets = {"labels": [torch.tensor([1, 3, 0]), torch.tensor([2])],
               "bboxes": [torch.from_numpy(dcase.make_boxes((3,), 11)), torch.from_numpy(dcase.make_boxes((1,), 12))]}
    loss = crit(out, targets)
    loss = sum(loss.values()) if isinstance(loss, dict) else loss
    assert bool(torch.isfinite(loss))
    loss.backward()
    for name, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert float(p.grad.abs().max()) > 0.0 or name.endswith("in_proj_bias"), name


def test_seg_enable_raises():
    with pytest.raises(NotImplementedError, match="mask head"):
        ca.DetrSegmHead(8, 3, 4, dict(type="sine"), cases.transformer_config(), seg_enable=True)


def test_cpu_and_16_bit_tensors_take_the_stock_route_without_touching_the_library(monkeypatch):
    def boom(*_a, **_k):
        raise AssertionError("the fused route was taken")
    monkeypatch.setattr(ops_attn, "detr_attention", boom)
    monkeypatch.setattr(_lib, "get", boom)
    x = cases.features()
    head = cases.make_head(ca.DetrSegmHead, backend="hip")
    want = cases.make_head(ca.DetrSegmHead, backend="torch")(x)
    got = head(x)
    assert torch.equal(got["logits"], want["logits"]) and torch.equal(got["bboxes"], want["bboxes"])
    layer = ca.TransformerEncoderLayer(64, 2, 32, backend="hip").eval()
    src = cases.tensor((7, 2, 64), 5)
    half = copy.deepcopy(layer).to(torch.bfloat16)(src.to(torch.bfloat16), pos=src.to(torch.bfloat16))
    assert half.dtype == torch.bfloat16 and bool(torch.isfinite(half.float()).all())
    # what else the fused route leaves to the module: an attn_mask, a head width other than 32
    assert layer(src, src_mask=torch.zeros(7, 7, dtype=torch.bool)).shape == (7, 2, 64)
    assert ca.TransformerEncoderLayer(64, 4, 32, backend="hip").eval()(src).shape == (7, 2, 64)
    assert not ops_attn.attn_fused_ok(src, src, src, 2) and not ops_attn.attn_fused_ok(src.to("meta"), src, src, 4)


def test_meta_shapes_and_refusals():
    m = lambda *s: torch.empty(s, device="meta")
    out, lse, stats = torch.ops.cerberus_attn.attention(m(5, 2, 64), m(7, 2, 64), m(7, 2, 64), 2, None, 0.5, 0.0, None)
    assert out.shape == (5, 2, 64) and lse.shape == (2, 2, 5) and stats.shape == (2, 2, 5, 2) and out.dtype == lse.dtype == torch.float32
    gq, gk, gv = torch.ops.cerberus_attn.attention_backward(m(5, 2, 64), m(5, 2, 64), m(7, 2, 64), m(7, 2, 64), out, stats, 2, None, 0.5, 0.0,
                                                            None, [True, False, True])
    assert gq.shape == (5, 2, 64) and gk.shape == (0,) and gv.shape == (7, 2, 64)
    q = torch.zeros(5, 2, 64)
    with pytest.raises(RuntimeError, match="cerberus_attn::attention has no CPU implementation"):
        ca.detr_attention(q, q, q, 2)


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.get()
    p = 1 << 20                                   # a non-null, 16-byte aligned address that is never dereferenced
    ok = dict(Lq=5, Lk=7, B=2, H=3, D=32)

    def fwd(scale=1.0, drop=0.0, dtype=0, ptrs=None, **over):
        d = dict(ok, **over)
        return lib.cerberus_attn_forward(*(ptrs or [p] * 8), d["Lq"], d["Lk"], d["B"], d["H"], d["D"], scale, drop, dtype, None)

    def bwd(scale=1.0, drop=0.0, dtype=0, ptrs=None, **over):
        d = dict(ok, **over)
        return lib.cerberus_attn_backward(*(ptrs or [p] * 12), d["Lq"], d["Lk"], d["B"], d["H"], d["D"], scale, drop, dtype, None)

    for over, code in ((dict(Lq=0), -1), (dict(Lk=0), -1), (dict(B=-1), -1), (dict(H=0), -1), (dict(D=0), -1), (dict(D=16), -5),
                       (dict(D=64), -5), (dict(Lk=1 << 30), -6), (dict(B=1 << 16, H=1 << 16), -6), (dict(Lq=1, Lk=1, B=1 << 12, H=1 << 13), -6), (dict(drop=1.0), -1),
                       (dict(drop=-0.1), -1), (dict(scale=float("inf")), -1), (dict(dtype=9), -2), (dict(dtype=1), -5)):
        assert fwd(**over) == code and bwd(**over) == code, over
    for i in (0, 1, 2, 5, 6, 7):                  # q, k, v, out, lse, stats; the mask and (at p = 0) the seed are optional
        ptrs = [p] * 8
        ptrs[i] = None
        assert fwd(ptrs=ptrs) == -1, i
    ptrs = [p] * 8
    ptrs[4] = None
    assert fwd(ptrs=ptrs, drop=0.1) == -1         # dropout needs the seed
    ptrs[0], ptrs[4] = p + 2, p
    assert fwd(ptrs=ptrs) == -1                   # a float pointer that is not 4-byte aligned
    ptrs[0], ptrs[4] = p, p + 4
    assert fwd(ptrs=ptrs, drop=0.1) == -1         # a seed that is not 8-byte aligned
    for i in (0, 1, 2, 3, 6, 7, 11):              # grad_out, q, k, v, out, stats, delta
        ptrs = [p] * 12
        ptrs[i] = None
        assert bwd(ptrs=ptrs) == -1, i
    ptrs = [p] * 12
    ptrs[8] = ptrs[9] = ptrs[10] = None
    assert bwd(ptrs=ptrs) == -1                   # no gradient asked for
    assert lib.cerberus_attn_dropout_keep(p, p, 0, 1, 1, 1, 0.5, None) == -1
    assert lib.cerberus_attn_dropout_keep(None, p, 1, 1, 1, 1, 0.5, None) == -1
    assert lib.cerberus_attn_dropout_keep(p, p, 1, 1, 1, 1, 1.0, None) == -1
    assert lib.cerberus_attn_dropout_keep(p, p, 1 << 15, 1 << 15, 1 << 20, 1 << 20, 0.5, None) == -6
    assert lib.cerberus_attn_dropout_keep(p, p, 1, 1, 1 << 16, 1 << 16, 0.5, None) == -6          # 2^32 elements: one thread each
    assert lib.cerberus_abi_version() == 7


def test_the_source_is_in_both_source_lists_and_the_names_are_exported():
    assert "detr_attn.hip" in build.SOURCES and "detr_attn.hip" in build.EXPERIMENT_SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "detr_attn.hip")) and os.path.exists(os.path.join(build.CSRC, "attn_dropout.h"))
    for name in NEW_NAMES:
        assert name in ca.__all__ and name in nnet_models.__all__, name
        assert getattr(ca, name) is getattr(nnet_models, name)
    assert "detr_attention" in ca.__all__ and ca.detr_attention is ops_attn.detr_attention
    assert ops_attn.HEAD_DIM == 32
    head = ca.DetrSegmHead(8, 3, 4, dict(type="sine"), cases.transformer_config())
    assert head.backend == tr.DEFAULT_ATTENTION_BACKEND
    assert all(layer.backend == tr.DEFAULT_ATTENTION_BACKEND for layer in list(head.transformer.encoder.layers) + list(head.transformer.decoder.layers))
    # the hash restated in Python has the threshold the C side computes
    assert cases.keep_threshold(0.0) == 0 and cases.keep_threshold(0.5) == 1 << 31 and cases.keep_threshold(0.1) == 429496736
