"""The Panoptic-DeepLab head's fused ops and modules on the GPU (csrc/pdl_head.hip).

The yardstick of the ops is the stock chain in float64 on the CPU (tests/pdl_cases.reference): the forward and every gradient must
have rel_err < 1e-5.  The stock chain in fp32 stays at or below 4e-7 of it, so the bound leaves room for another summation order
and none for a wrong tap.  The kernel's tile is 32 rows x 64 columns: "x2_tile_edge" (33 x 65) puts one row and one column past the
first tile, "two_tile_rows" (40 x 40) a second tile row, "wide" (5 x 139) three tiles in x with a ragged last one.
"""
import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import pdl_cases as cases
from op_cases import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("low", "skip", "weight")


def on_gpu(name):
    return [None if t is None else t.to(DEV) for t in cases.op_inputs(name)]


@pytest.mark.parametrize("name", cases.PARITY)
def test_forward_and_gradients_against_the_float64_chain(name):
    low, skip, weight, gy = on_gpu(name)
    y, grads = cases.run_fused(low, skip, weight, gy)
    ref = cases.reference(name)
    assert set(grads) == set(ref) - {"y"}
    figures = {"y": cases.rel_err(y.cpu().numpy(), ref["y"])}
    figures.update({k: cases.rel_err(g.cpu().numpy(), ref[k]) for k, g in grads.items()})
    print(name, figures)
    for k, e in figures.items():
        assert y.shape == ref["y"].shape and e < cases.BOUND, (name, k, e)


def test_two_runs_give_the_same_bits():
    args = on_gpu("x2_tile_edge")
    y0, g0 = cases.run_fused(*args)
    y1, g1 = cases.run_fused(*args)
    assert same_bits(y0, y1)
    for k in NAMES:
        assert same_bits(g0[k], g1[k]), k


def test_graph_replay_gives_the_same_bits():
    low, skip, weight, gy = on_gpu("x2_tile_edge")
    eager = torch.ops.cerberus_pdl.upcat_dwconv5x5(low, skip, weight)
    eager_grads = torch.ops.cerberus_pdl.upcat_dwconv5x5_backward(gy, low, skip, weight, [True, True, True])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):      # warm-up on the side stream: the library is loaded and the allocator primed before the capture
            torch.ops.cerberus_pdl.upcat_dwconv5x5(low, skip, weight)
            torch.ops.cerberus_pdl.upcat_dwconv5x5_backward(gy, low, skip, weight, [True, True, True])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = torch.ops.cerberus_pdl.upcat_dwconv5x5(low, skip, weight)
        grads = torch.ops.cerberus_pdl.upcat_dwconv5x5_backward(gy, low, skip, weight, [True, True, True])
    for _ in range(2):
        out.zero_()
        for g in grads:
            g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, eager)
        for g, e in zip(grads, eager_grads):
            assert same_bits(g, e)


@pytest.mark.parametrize("name", ["ratios", "x2_tile_edge"])
def test_same_bits_from_an_offset_view_of_every_argument(name):
    """Every tensor in turn starts one element past its buffer: the wide loads and stores of that tensor are off, the values are
    not."""
    low, skip, weight, gy = on_gpu(name)
    y0 = torch.ops.cerberus_pdl.upcat_dwconv5x5(low, skip, weight)
    g0 = torch.ops.cerberus_pdl.upcat_dwconv5x5_backward(gy, low, skip, weight, [True, True, True])
    p0 = torch.ops.cerberus_pdl.dwconv5x5(skip, weight[:skip.shape[1]])
    q0 = torch.ops.cerberus_pdl.dwconv5x5_backward(gy[:, :skip.shape[1]], skip, weight[:skip.shape[1]], [True, True])
    for i in range(4):
        args = [gy, low, skip, weight]
        args[i] = cases.offset_view(args[i])
        assert args[i].data_ptr() % 16 == 4
        g = torch.ops.cerberus_pdl.upcat_dwconv5x5_backward(*args, [True, True, True])
        for k in range(3):
            assert same_bits(g[k], g0[k]), (name, i, k)
        if i > 0:
            assert same_bits(torch.ops.cerberus_pdl.upcat_dwconv5x5(*args[1:]), y0), (name, i)
    pw, pg = weight[:skip.shape[1]].contiguous(), gy[:, :skip.shape[1]].contiguous()
    for i in range(3):
        args = [pg, skip, pw]
        args[i] = cases.offset_view(args[i])
        q = torch.ops.cerberus_pdl.dwconv5x5_backward(*args, [True, True])
        assert same_bits(q[0], q0[0]) and same_bits(q[1], q0[1]), (name, i)
        if i > 0:
            assert same_bits(torch.ops.cerberus_pdl.dwconv5x5(*args[1:]), p0), (name, i)


@pytest.mark.parametrize("name", ["x2_tile_edge", "plain"])
def test_needs_input_grad_skips_launches_and_keeps_the_bits(name):
    args = on_gpu(name)
    _, full = cases.run_fused(*args)
    _, frozen = cases.run_fused(*args, need=(True, True, False))             # the weights frozen
    _, only_w = cases.run_fused(*args, need=(False, False, True))            # only the weights trainable
    assert set(only_w) == {"weight"} and same_bits(only_w["weight"], full["weight"])
    assert set(frozen) == set(full) - {"weight"}
    for k in frozen:
        assert same_bits(frozen[k], full[k]), k
    if name != "plain":
        _, only_low = cases.run_fused(*args, need=(True, False, False))
        assert set(only_low) == {"low"} and same_bits(only_low["low"], full["low"])
        low, skip, weight, gy = args
        masked = torch.ops.cerberus_pdl.upcat_dwconv5x5_backward(gy, low, skip, weight, [False, True, False])
        assert masked[0].shape == (0,) and masked[2].shape == (0,) and same_bits(masked[1], full["skip"])


def test_other_dtypes_and_shapes_are_rejected_with_the_stock_route_named():
    low, skip, weight, gy = on_gpu("ratios")
    with pytest.raises(RuntimeError, match="must be float32.*F.conv2d"):
        torch.ops.cerberus_pdl.upcat_dwconv5x5(low.half(), skip.half(), weight.half())
    with pytest.raises(RuntimeError, match="must be float32.*F.conv2d"):
        torch.ops.cerberus_pdl.dwconv5x5_backward(gy[:, :3].double(), skip.double(), weight[:3].double(), [True, True])
    with pytest.raises(RuntimeError, match="weight must be"):
        torch.ops.cerberus_pdl.upcat_dwconv5x5(low, skip, weight[:-1])
    with pytest.raises(RuntimeError, match="grad_y must be"):
        torch.ops.cerberus_pdl.upcat_dwconv5x5_backward(gy[:, 1:], low, skip, weight, [True, True, True])


# ---- the modules -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden):
    return golden("pdl_head")


def test_hip_decoder_against_the_torch_decoder_on_the_same_device():
    feats = cases.features(DEV)
    hip = cases.run_decoder(cases.make_decoder(ca.PanopticDeepLabDecoder, "hip").to(DEV), feats)
    ref = cases.run_decoder(cases.make_decoder(ca.PanopticDeepLabDecoder, "torch").to(DEV), feats)
    for key in cases.OUTPUTS:
        assert cases.rel_err(hip[0][key].detach().cpu().numpy(), ref[0][key].detach().cpu().numpy()) < 1e-5, key
    for i, (a, b) in enumerate(zip(hip[2], ref[2])):
        assert cases.l2_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-4, i
    assert list(hip[3]) == list(ref[3])
    np.testing.assert_allclose(np.array(list(hip[3].values())), np.array(list(ref[3].values())), rtol=1e-3)


def test_hip_decoder_takes_the_fused_ops(monkeypatch):
    calls = []
    for name in ("dwconv5x5", "upcat_dwconv5x5"):
        real = getattr(ca.ops_pdl, name)
        monkeypatch.setattr(ca.ops_pdl, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    net = cases.make_decoder(ca.PanopticDeepLabDecoder, "hip", mode="eval").to(DEV)
    with torch.no_grad():
        net((None, cases.features(DEV)))
    assert sorted(calls) == ["dwconv5x5"] * 3 + ["upcat_dwconv5x5"] * 4        # 3 classifiers, 2 decoders x 2 stages
    del calls[:]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        net((None, cases.features(DEV)))
    assert calls == []                                                          # autocast: the stock ops


def test_eval_outputs_against_the_fixture(gold):
    net = cases.make_decoder(ca.PanopticDeepLabDecoder, "hip", mode="eval").to(DEV)
    with torch.no_grad():
        pred = net((None, cases.features(DEV)))
    for key in cases.OUTPUTS:
        assert cases.rel_err(pred[key].cpu().numpy(), gold[key]) < 1e-5, key


def test_one_training_step_end_to_end():
    net = cases.make_decoder(ca.PanopticDeepLabDecoder, "hip").to(DEV)
    pred = net((None, cases.features(DEV)))
    B, _, H, W = cases.OUTPUTS["seg"]
    targets = {"center": cases.tensor((B, 1, H, W), 81, 0.0, 1.0).to(DEV), "offset": cases.tensor((B, 2, H, W), 82, -4.0, 4.0).to(DEV),
               "center_mask": torch.ones(B, H, W, device=DEV), "offset_mask": torch.ones(B, H, W, device=DEV)}
    labels = (cases.tensor((B, H, W), 83, 0.0, 4.999).floor().long()).to(DEV)
    loss = ca.DeeplabPanopticLoss(backend="hip")(pred, targets) + ca.seg_cross_entropy(pred["seg"], labels)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
