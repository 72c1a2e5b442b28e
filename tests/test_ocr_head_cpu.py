"""The OCR segmentation head without a GPU: the modules against the reference's own run (tests/golden/ocr_head.npz, written by
tools/gen_golden_ocr.py), the ``cerberus_ocr::`` ops' fake implementations and refusals, and the C entry points' argument checks."""
import os

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import ocr_cases as cases
from cerberusnet_amd import _lib, build, nnet_models, ops_ocr
from cerberusnet_amd.nnet_models import ocr_utils
from conftest import l2_err, rel_err

NEW_NAMES = ["BNReLU", "scale_as", "SpatialGather_Module", "ObjectAttentionBlock", "SpatialOCR_Module", "OCR_block", "OCRNetHead"]


@pytest.fixture(scope="module")
def gold(golden):
    return golden("ocr_head")


def _run(block, x):
    x = x.clone().requires_grad_(True)
    outs = block(x)
    loss = cases.block_loss(*outs)
    loss.backward()
    return outs, loss, x.grad, {n: float(p.grad.double().norm()) for n, p in block.named_parameters()}


def test_state_dict_keys_and_shapes_equal_the_reference(gold):
    state = cases.make_block(ca.OCR_block, "torch").state_dict()
    assert list(state.keys()) == [str(k) for k in gold["keys"]]
    for (name, v), shape in zip(state.items(), gold["shapes"]):
        assert list(v.shape) == [int(s) for s in shape if s >= 0], name
    head = ca.OCRNetHead([8, 16], mid_channels=16, key_channels=8, classes=5).state_dict()
    assert list(head.keys()) == ["ocr." + str(k) for k in gold["keys"]]


def test_torch_backend_matches_the_reference_run(gold):
    assert cases.block_input().numpy().tobytes() == gold["input"].tobytes()
    outs, loss, grad, norms = _run(cases.make_block(ca.OCR_block, "torch"), torch.from_numpy(gold["input"]))
    for name, o in zip(("cls_out", "aux_out", "ocr_feats"), outs):
        assert o.shape == gold[name].shape
        assert rel_err(o.detach().numpy(), gold[name]) < 1e-5, name
    assert abs(loss.item() - float(gold["loss"])) <= 1e-5 * abs(float(gold["loss"]))
    assert l2_err(grad.numpy(), gold["grad_input"]) < 1e-3
    assert list(norms) == [str(n) for n in gold["grad_names"]]
    np.testing.assert_allclose(np.array(list(norms.values())), gold["grad_norms"], rtol=1e-3)


def test_hip_backend_on_cpu_tensors_gives_the_bits_of_torch():
    x = cases.block_input()
    a = _run(cases.make_block(ca.OCR_block, "hip"), x)
    b = _run(cases.make_block(ca.OCR_block, "torch"), x)
    for u, v in zip(a[0], b[0]):
        assert torch.equal(u, v)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]
    head = ca.OCRNetHead([8, 16], mid_channels=16, key_channels=8, classes=5, backend="hip").eval()
    out = head((x, None))
    assert set(out) == {"seg", "seg_aux"} and out["seg"].shape == (2, 5, 9, 12) and out["seg_aux"].shape == (2, 5, 9, 12)


def test_attention_scale_above_one_pools_and_resizes_around_the_core():
    torch.manual_seed(0)
    x, proxy = torch.randn(2, 6, 8, 10), torch.randn(2, 6, 5, 1)
    a, b = ca.ObjectAttentionBlock(6, 4, scale=2, backend="hip"), ca.ObjectAttentionBlock(6, 4, scale=2, backend="torch")
    b.load_state_dict(a.state_dict())
    ya, yb = a(x, proxy), b(x, proxy)
    assert ya.shape == x.shape and torch.equal(ya, yb)


def test_meta_shapes_dtypes_and_strides():
    m = lambda *s: torch.empty(s, device="meta")
    ctx, lse = torch.ops.cerberus_ocr.spatial_gather(m(2, 6, 9, 12), m(2, 5, 9, 12), 1.0)
    assert ctx.shape == (2, 6, 5) and lse.shape == (2, 5) and ctx.is_contiguous() and lse.is_contiguous()
    gf, gl = torch.ops.cerberus_ocr.spatial_gather_backward(m(2, 6, 9, 12), m(2, 5, 9, 12), m(2, 6, 5), m(2, 6, 5), 1.0)
    assert gf.shape == (2, 6, 9, 12) and gl.shape == (2, 5, 9, 12)
    out, attn = torch.ops.cerberus_ocr.object_attention(m(2, 6, 9, 12).to(memory_format=torch.channels_last), m(2, 6, 5), m(2, 6, 5), 0.5)
    assert out.shape == (2, 6, 9, 12) and attn.shape == (2, 5, 9, 12)
    assert out.stride() == (648, 108, 12, 1) and attn.stride() == (540, 108, 12, 1)
    gq, gk, gv = torch.ops.cerberus_ocr.object_attention_backward(m(2, 6, 9, 12), m(2, 6, 9, 12), m(2, 6, 5), m(2, 6, 5),
                                                                  m(2, 5, 9, 12), 0.5)
    assert gq.shape == (2, 6, 9, 12) and gk.shape == (2, 6, 5) and gv.shape == (2, 6, 5)
    for t in (ctx, lse, gf, gl, out, attn, gq, gk, gv):
        assert t.dtype == torch.float32 and t.device.type == "meta" and t.storage_offset() == 0


def test_raw_ops_raise_on_cpu_tensors():
    f, x = torch.randn(1, 3, 4, 5), torch.randn(1, 2, 4, 5)
    with pytest.raises(RuntimeError, match="cerberus_ocr::spatial_gather has no CPU implementation"):
        torch.ops.cerberus_ocr.spatial_gather(f, x, 1.0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ca.spatial_gather(f.requires_grad_(True), x)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus_ocr.spatial_gather_backward(f, x, torch.randn(1, 3, 2), torch.randn(1, 3, 2), 1.0)
    k = torch.randn(1, 3, 2)
    with pytest.raises(RuntimeError, match="cerberus_ocr::object_attention has no CPU implementation"):
        ca.object_attention(f, k, k, 0.5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus_ocr.object_attention_backward(f, f, k, k, x, 0.5)


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.get()
    p = 1 << 20                                   # a non-null, 16-byte aligned address that is never dereferenced
    ok = dict(B=1, C=4, R=5, HW=63)

    def sizes(**over):
        d = dict(ok, **over)
        return d["B"], d["C"], d["R"], d["HW"]

    big = 1 << 30
    for over, code in ((dict(B=0), -1), (dict(C=0), -1), (dict(R=0), -1), (dict(HW=0), -1), (dict(HW=-3), -1), (dict(R=33), -5),
                       (dict(HW=0x7fffffff), -6), (dict(C=1 << 28, R=32), -6)):
        s = sizes(**over)
        assert lib.cerberus_ocr_gather_forward(p, p, p, p, p, big, *s, 1.0, 0, None) == code, over
        assert lib.cerberus_ocr_gather_backward(p, p, p, p, p, p, p, big, *s, 1.0, 0, None) == code, over
        assert lib.cerberus_ocr_attention_forward(p, p, p, p, p, *s, 1.0, 0, None) == code, over
        assert lib.cerberus_ocr_attention_backward(p, p, p, p, p, p, p, p, p, p, big, *s, 1.0, 0, None) == code, over
        assert lib.cerberus_ocr_workspace_bytes(*s) == 0, over
    s = sizes()
    assert lib.cerberus_ocr_gather_forward(p, p, p, p, p, big, *s, 1.0, 9, None) == -2          # unknown dtype
    assert lib.cerberus_ocr_gather_forward(p, p, p, p, p, big, *s, 1.0, 1, None) == -5          # fp16
    need = lib.cerberus_ocr_workspace_bytes(*s)
    assert need > 0
    for i in range(5):                                                                           # a null pointer, the workspace too
        args = [p] * 5
        args[i] = None
        assert lib.cerberus_ocr_gather_forward(*args, big, *s, 1.0, 0, None) == -1, i
    assert lib.cerberus_ocr_gather_forward(p, p, p, p, p, need - 1, *s, 1.0, 0, None) == -1     # too small
    assert lib.cerberus_ocr_gather_forward(p, p, p, p, p + 4, big, *s, 1.0, 0, None) == -1      # misaligned
    for i in range(7):
        args = [p] * 7
        args[i] = None
        assert lib.cerberus_ocr_gather_backward(*args, big, *s, 1.0, 0, None) == -1, i
    for i in range(5):
        args = [p] * 5
        args[i] = None
        assert lib.cerberus_ocr_attention_forward(*args, *s, 1.0, 0, None) == -1, i
    for i in range(10):
        args = [p] * 10
        args[i] = None
        assert lib.cerberus_ocr_attention_backward(*args, big, *s, 1.0, 0, None) == -1, i
    assert lib.cerberus_ocr_attention_backward(*([p] * 10), need - 1, *s, 1.0, 0, None) == -1
    assert lib.cerberus_abi_version() == 7


def test_python_and_c_workspace_sizes_are_equal():
    lib = _lib.get()
    for s in ((1, 1, 1, 1), (1, 3, 1, 35), (2, 19, 19, 37 * 53), (1, 17, 32, 22500), (4, 512, 19, 128 * 256), (3, 65, 2, 257),
              (2, 256, 19, 2048), (0, 4, 5, 6), (1, 4, 33, 6), (1, 4, 0, 6), (1, 1 << 28, 32, 6), (1, 4, 5, 0x7fffffff), (-1, 4, 5, 6)):
        assert ops_ocr._ocr_workspace_bytes(*s) == lib.cerberus_ocr_workspace_bytes(*s), s
    # (2, 256, 19, 2048): 3 x 38 floats of statistics padded to 116, 2 x 8 chunks x 256 x 19 partials
    assert lib.cerberus_ocr_workspace_bytes(2, 256, 19, 2048) == 4 * (116 + 2 * 8 * 256 * 19)
    assert ops_ocr.OCR_CHUNK == 256 and ops_ocr.OCR_MAX_REGIONS == 32


def test_the_source_is_in_both_source_lists():
    assert "ocr_head.hip" in build.SOURCES and "ocr_head.hip" in build.EXPERIMENT_SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "ocr_head.hip"))


def test_ocr_aspp_is_refused():
    with pytest.raises(NotImplementedError):
        ca.SpatialOCR_Module(8, 4, 8, OCR_ASPP=True, kwargs={"bott_ch": 4})
    with pytest.raises(ValueError, match="backend"):
        ca.OCR_block(8, mid_channels=8, key_channels=4, classes=3, backend="triton")


def test_the_names_are_exported():
    for name in NEW_NAMES:
        assert name in ca.__all__ and name in nnet_models.__all__, name
        assert getattr(ca, name) is getattr(nnet_models, name)
    # the measured defaults (profiles/ocr_head_fused.txt): the attention's fused route won at both shapes, the gather's did not
    block = ca.OCR_block(8, mid_channels=8, key_channels=4, classes=3)
    assert block.ocr_gather_head.backend == ocr_utils.DEFAULT_GATHER_BACKEND == "torch"
    assert block.ocr_distri_head.object_context_block.backend == ocr_utils.DEFAULT_ATTENTION_BACKEND == "hip"
    both = ca.OCRNetHead([8], mid_channels=8, key_channels=4, classes=3, backend="hip").ocr
    assert both.ocr_gather_head.backend == both.ocr_distri_head.object_context_block.backend == "hip"
    ops = {n for n in torch._C._dispatch_get_all_op_names() if n.startswith("cerberus_ocr::")}
    assert {n.split(".")[0] for n in ops} == {"cerberus_ocr::spatial_gather", "cerberus_ocr::spatial_gather_backward",
                                              "cerberus_ocr::object_attention", "cerberus_ocr::object_attention_backward"}
