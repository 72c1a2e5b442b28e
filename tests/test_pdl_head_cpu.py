"""The Panoptic-DeepLab head without a GPU: the modules against the reference's own run (tests/golden/pdl_head.npz, written by
tools/gen_golden_pdl.py), the ``cerberus_pdl::`` ops' fake implementations and refusals, and the C entry points' argument checks."""
import os

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import pdl_cases as cases
from cerberusnet_amd import _lib, build, nnet_models, ops_pdl
from cerberusnet_amd.nnet_models import deeplab_panoptic
from conftest import rel_err

NEW_NAMES = ["ASPP", "SinglePanopticDeepLabDecoder", "SinglePanopticDeepLabHead", "PanopticDeepLabDecoder"]
OPS = {"dwconv5x5", "dwconv5x5_backward", "upcat_dwconv5x5", "upcat_dwconv5x5_backward"}


@pytest.fixture(scope="module")
def gold(golden):
    return golden("pdl_head")


def test_state_dict_keys_and_shapes_equal_the_reference(gold):
    state = cases.make_decoder(ca.PanopticDeepLabDecoder, "torch").state_dict()
    assert len(state) == 176 and list(state.keys()) == [str(k) for k in gold["keys"]]
    for (name, v), shape in zip(state.items(), gold["shapes"]):
        assert list(v.shape) == [int(s) for s in shape if s >= 0], name
    assert list(cases.make_decoder(ca.PanopticDeepLabDecoder, "hip").state_dict().keys()) == list(state.keys())


def test_torch_backend_matches_the_reference_run(gold):
    feats = cases.features()
    for i, f in enumerate(feats):
        assert f.numpy().tobytes() == gold["feature%d" % i].tobytes()
    with torch.no_grad():
        pred = cases.make_decoder(ca.PanopticDeepLabDecoder, "torch", mode="eval")((None, feats))
    assert list(pred) == ["seg", "center", "offset"]
    for key, shape in cases.OUTPUTS.items():
        assert tuple(pred[key].shape) == shape == gold[key].shape
        assert rel_err(pred[key].numpy(), gold[key]) < 1e-5, key
    _, loss, grads, norms = cases.run_decoder(cases.make_decoder(ca.PanopticDeepLabDecoder, "torch"), feats)
    assert abs(loss.item() - float(gold["loss"])) <= 1e-5 * abs(float(gold["loss"]))
    np.testing.assert_allclose([float(g.double().norm()) for g in grads], gold["grad_input_norms"], rtol=1e-3)
    assert list(norms) == [str(n) for n in gold["grad_names"]]
    np.testing.assert_allclose(np.array(list(norms.values())), gold["grad_norms"], rtol=1e-3)


def test_hip_backend_on_cpu_tensors_gives_the_bits_of_torch():
    feats = cases.features()
    a = cases.run_decoder(cases.make_decoder(ca.PanopticDeepLabDecoder, "hip"), feats)
    b = cases.run_decoder(cases.make_decoder(ca.PanopticDeepLabDecoder, "torch"), feats)
    for key in cases.OUTPUTS:
        assert torch.equal(a[0][key], b[0][key]), key
    assert torch.equal(a[1], b[1]) and all(torch.equal(u, v) for u, v in zip(a[2], b[2])) and a[3] == b[3]


def test_backends_and_image_pooling():
    with pytest.raises(ValueError, match="backend"):
        ca.PanopticDeepLabDecoder(**cases.CONFIG, backend="triton")
    with pytest.raises(ValueError, match="backend"):
        ca.SinglePanopticDeepLabHead(8, 8, [3], ["seg"], backend="cuda")
    net = cases.make_decoder(ca.PanopticDeepLabDecoder, "hip", mode="eval")
    assert net.semantic_decoder.backend == net.semantic_head.backend == net.instance_decoder.backend == net.instance_head.backend == "hip"
    plain = ca.PanopticDeepLabDecoder(**dict(cases.CONFIG, has_instance=False))
    assert plain.instance_decoder is None and plain.instance_head is None
    assert plain.semantic_decoder.backend == deeplab_panoptic.DEFAULT_UPCAT_BACKEND
    assert plain.semantic_head.backend == deeplab_panoptic.DEFAULT_DWCONV_BACKEND
    net.set_image_pooling((3, 4))
    for decoder in (net.semantic_decoder, net.instance_decoder):
        pool = decoder.aspp.convs[-1].aspp_pooling[0]
        assert isinstance(pool, torch.nn.AvgPool2d) and pool.kernel_size == (3, 4)
    with torch.no_grad():
        pred = net((None, cases.features()))
    assert {k: tuple(v.shape) for k, v in pred.items()} == cases.OUTPUTS


def test_integration_backbone_decoder_losses():
    """Tiny HighResolutionNet -> decoder -> DeeplabPanopticLoss(backend='torch') + cross-entropy on seg: shapes, and a gradient for
    every parameter."""
    torch.manual_seed(0)
    widths = [8, 16, 24, 32]
    cfg = ca.nnet_models.hrnet_config(widths)
    for stage in cfg.values():
        stage["NUM_MODULES"] = 1
        stage["NUM_BLOCKS"] = [1] * stage["NUM_BRANCHES"]
    backbone = ca.nnet_models.HighResolutionNet(**cfg)
    head = ca.PanopticDeepLabDecoder(in_channels=backbone.output_ch, low_level_channels_project=[12, 8, 6], decoder_channels=16,
                                     atrous_rates=[1, 2, 3], num_classes=5, has_instance=True,
                                     instance_low_level_channels_project=[8, 6, 4], instance_decoder_channels=8, instance_aspp_channels=12,
                                     instance_head_channels=8, instance_num_classes=[1, 2], instance_class_key=["center", "offset"])
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    B, H, W = 2, 64, 96
    pred = head(backbone(torch.randn(B, 3, H, W)))
    h, w = H // 4, W // 4
    assert {k: tuple(v.shape) for k, v in pred.items()} == {"seg": (B, 5, h, w), "center": (B, 1, h, w), "offset": (B, 2, h, w)}
    targets = {"center": torch.rand(B, 1, h, w), "offset": torch.randn(B, 2, h, w), "center_mask": torch.ones(B, h, w),
               "offset_mask": torch.ones(B, h, w)}
    loss = ca.DeeplabPanopticLoss(backend="torch")(pred, targets)
    loss = loss + torch.nn.functional.cross_entropy(pred["seg"], torch.randint(0, 5, (B, h, w)))
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    loss.backward()
    for name, p in list(backbone.named_parameters()) + list(head.named_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


def test_meta_shapes_dtypes_and_strides():
    m = lambda *s: torch.empty(s, device="meta")
    x, wt = m(2, 6, 9, 12).to(memory_format=torch.channels_last), m(6, 1, 5, 5)
    y = torch.ops.cerberus_pdl.dwconv5x5(x, wt)
    assert y.shape == (2, 6, 9, 12) and y.stride() == (648, 108, 12, 1)
    gx, gw = torch.ops.cerberus_pdl.dwconv5x5_backward(m(2, 6, 9, 12), x, wt, [True, True])
    assert gx.shape == (2, 6, 9, 12) and gx.stride() == (648, 108, 12, 1) and gw.shape == (6, 1, 5, 5)
    gx, gw = torch.ops.cerberus_pdl.dwconv5x5_backward(m(2, 6, 9, 12), x, wt, [False, True])
    assert gx.shape == (0,) and gw.shape == (6, 1, 5, 5)
    low, skip, wt = m(2, 4, 5, 7), m(2, 3, 9, 12), m(7, 1, 5, 5)
    y2 = torch.ops.cerberus_pdl.upcat_dwconv5x5(low, skip, wt)
    assert y2.shape == (2, 7, 9, 12) and y2.is_contiguous()
    gl, gs, gw2 = torch.ops.cerberus_pdl.upcat_dwconv5x5_backward(m(2, 7, 9, 12), low, skip, wt, [True, True, True])
    assert gl.shape == (2, 4, 5, 7) and gs.shape == (2, 3, 9, 12) and gw2.shape == (7, 1, 5, 5)
    masked = torch.ops.cerberus_pdl.upcat_dwconv5x5_backward(m(2, 7, 9, 12), low, skip, wt, [True, False, False])
    assert masked[0].shape == (2, 4, 5, 7) and masked[1].shape == (0,) and masked[2].shape == (0,)
    for t in (y, gx, gw, y2, gl, gs, gw2) + tuple(masked):
        assert t.dtype == torch.float32 and t.device.type == "meta" and t.storage_offset() == 0 and t.is_contiguous()


def test_raw_ops_raise_on_cpu_tensors():
    x, wt = torch.randn(1, 3, 4, 5), torch.randn(3, 1, 5, 5)
    low, wt2 = torch.randn(1, 2, 2, 3), torch.randn(5, 1, 5, 5)
    with pytest.raises(RuntimeError, match="cerberus_pdl::dwconv5x5 has no CPU implementation"):
        torch.ops.cerberus_pdl.dwconv5x5(x, wt)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ca.dwconv5x5(x.clone().requires_grad_(True), wt)
    with pytest.raises(RuntimeError, match="cerberus_pdl::dwconv5x5_backward has no CPU implementation"):
        torch.ops.cerberus_pdl.dwconv5x5_backward(x, x, wt, [True, True])
    with pytest.raises(RuntimeError, match="cerberus_pdl::upcat_dwconv5x5 has no CPU implementation"):
        ca.upcat_dwconv5x5(low, x, wt2)
    with pytest.raises(RuntimeError, match="cerberus_pdl::upcat_dwconv5x5_backward has no CPU implementation"):
        torch.ops.cerberus_pdl.upcat_dwconv5x5_backward(torch.randn(1, 5, 4, 5), low, x, wt2, [True, True, True])


FWD_OK = dict(B=1, Ca=2, Cb=3, h=3, w=4, H=5, W=9)


def _sizes(**over):
    d = dict(FWD_OK, **over)
    return d["B"], d["Ca"], d["Cb"], d["h"], d["w"], d["H"], d["W"]


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.get()
    p = 1 << 20                                   # a non-null, 16-byte aligned address that is never dereferenced
    big = 1 << 40
    fwd = lambda s, dtype=0, ptrs=None: lib.cerberus_pdl_dwconv_forward(*(ptrs or [p] * 4), *s, dtype, None)
    bwd = lambda s, dtype=0, ptrs=None, nbytes=big: lib.cerberus_pdl_dwconv_backward(*(ptrs or [p] * 8), nbytes, *s, dtype, None)
    for over, code in ((dict(B=0), -1), (dict(B=-2), -1), (dict(Cb=0), -1), (dict(Ca=-1), -1), (dict(H=0), -1), (dict(W=0), -1),
                       (dict(W=-5), -1), (dict(h=0), -1), (dict(w=-1), -1),
                       (dict(H=1 << 16, W=1 << 15), -6),                # H W past 2^31 - 1025
                       (dict(H=1 << 15, W=1 << 14), -6),                # 1024 x 256 tiles: past the 65535 of grid.y
                       (dict(B=1 << 20, Cb=1 << 12), -6),               # B (Ca + Cb) past 2^31 - 1
                       (dict(h=1 << 16, w=1 << 16), -6)):               # h w past 2^31 - 1
        s = _sizes(**over)
        assert fwd(s) == code, over
        assert bwd(s) == code, over
        if "h" not in over and "w" not in over:
            assert lib.cerberus_pdl_workspace_bytes(s[0], s[1], s[2], s[5], s[6]) == 0, over
    s = _sizes()
    for dtype, code in ((9, -2), (-1, -2), (1, -5), (2, -5), (3, -5)):       # unknown; fp16, bf16, fp64
        assert fwd(s, dtype) == code and bwd(s, dtype) == code, dtype
    need = lib.cerberus_pdl_workspace_bytes(1, 2, 3, 5, 9)
    assert need > 0
    for i in range(4):                                                         # a null pointer, a pointer off its 4 bytes
        for bad in (None, p + 2):
            ptrs = [p] * 4
            ptrs[i] = bad
            assert fwd(s, ptrs=ptrs) == -1, (i, bad)
    for i in (0, 1, 2, 3, 7):                                                  # grad_out, low, skip, weight, the workspace
        ptrs = [p] * 8
        ptrs[i] = None
        assert bwd(s, ptrs=ptrs) == -1, i
    assert bwd(s, ptrs=[p, p, p, p, None, None, None, p]) == -1               # no gradient asked for
    for i in (4, 5, 6):
        ptrs = [p] * 8
        ptrs[i] = p + 2
        assert bwd(s, ptrs=ptrs) == -1, i
    assert bwd(s, nbytes=need - 1) == -1                                      # one byte short
    for off in (4, 8):
        assert bwd(s, ptrs=[p] * 7 + [p + off]) == -1                         # misaligned workspace
    assert lib.cerberus_abi_version() == 7


def test_python_and_c_workspace_sizes_are_equal():
    lib = _lib.get()
    for s in ((1, 0, 1, 1, 1), (1, 2, 3, 5, 9), (2, 5, 3, 9, 13), (4, 256, 32, 128, 256), (4, 0, 256, 128, 256), (3, 1, 1, 33, 65),
              (256, 1, 1, 3, 3), (0, 1, 1, 3, 3), (1, -1, 1, 3, 3), (1, 1, 0, 3, 3), (1, 1, 1, 0, 3), (1, 1, 1, 1 << 16, 1 << 15),
              (1, 1, 1, 1 << 15, 1 << 14), (1 << 20, 0, 1 << 12, 3, 3)):
        assert ops_pdl._pdl_workspace_bytes(*s) == lib.cerberus_pdl_workspace_bytes(*s), s
    # (3, 1, 1, 33, 65): 3 x 33 x 65 = 6435 floats padded to 6436, then 2 channels x 25 taps x 3 images x (2 x 2) tiles doubles
    assert lib.cerberus_pdl_workspace_bytes(3, 1, 1, 33, 65) == 4 * 6436 + 8 * 2 * 25 * 3 * 4
    assert (ops_pdl.PDL_TILE_H, ops_pdl.PDL_TILE_W, ops_pdl.PDL_FOLD) == (32, 64, 256)
    for name, rounds in (("fold_one_round", 1.0), ("fold_two_rounds", 260 / 256)):
        B, _, _, _, _, H, W = cases.SHAPES[name]
        assert B * -(-H // 32) * -(-W // 64) == rounds * ops_pdl.PDL_FOLD, name


def test_the_source_is_in_both_source_lists():
    assert "pdl_head.hip" in build.SOURCES and "pdl_head.hip" in build.EXPERIMENT_SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "pdl_head.hip"))


def test_the_names_are_exported_and_the_op_set_is_the_four():
    for name in NEW_NAMES:
        assert name in ca.__all__ and name in nnet_models.__all__, name
        assert getattr(ca, name) is getattr(nnet_models, name)
    for name in ("dwconv5x5", "upcat_dwconv5x5", "ops_pdl"):
        assert name in ca.__all__ and hasattr(ca, name), name
    ops = {n.split("::", 1)[1].split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("cerberus_pdl::")}
    assert ops == OPS
