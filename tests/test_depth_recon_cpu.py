"""CPU tests of the depth reconstruction loss (loss_functions/depth_losses.py): the stock-op formulation against the
reference's own results (tests/golden/depth_recon.npz, written by tools/gen_golden_depth_recon.py), and the op layer of
cerberus::reproject_warp as far as it goes without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
from cerberusnet_amd import _lib
from cerberusnet_amd import build as cbuild
from cerberusnet_amd.loss_functions import depth_losses as D
from conftest import REPO, l2_err

CASES = {"a": (2, 3, 37, 53), "b": (1, 3, 16, 40)}
VALUE_TOL = 1e-6
GRAD_TOL = 1e-5


def _targets(g, tag, dtype=torch.float32):
    t = lambda k: torch.from_numpy(g["%s_%s" % (tag, k)]).to(dtype)
    return {"l_img": t("l_img"), "r_img": t("r_img"), "camera": {"inv_K": t("inv_K"), "K": t("K"), "baseline_T": t("T")}}


@pytest.mark.parametrize("backend", ["torch", "hip"])       # on CPU tensors 'hip' falls back to stock ops
@pytest.mark.parametrize("pred_type", ["depth", "disparity"])
@pytest.mark.parametrize("ssim", [True, False])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_stock_formulation_reproduces_the_reference(golden, tag, ssim, pred_type, backend):
    g = golden("depth_recon")
    B, _, H, W = CASES[tag]
    key = "%s_%d" % (pred_type, int(ssim))
    pred = torch.from_numpy(g["%s_pred_%s" % (tag, pred_type)]).requires_grad_(True)
    fn = ca.DepthReconstructionLossV1(B, H, W, pred_type=pred_type, ssim=ssim, backend=backend)
    loss = fn({"depth": pred}, _targets(g, tag))
    grad, = torch.autograd.grad(loss, pred)
    ref_v, ref_g = float(g["%s_loss_%s" % (tag, key)]), g["%s_grad_%s" % (tag, key)]
    print("%s %s %s: value rel %.3e grad l2_err %.3e" % (tag, key, backend, abs(loss.item() - ref_v) / abs(ref_v), l2_err(grad.numpy(), ref_g)))
    assert abs(loss.item() - ref_v) <= VALUE_TOL * abs(ref_v)
    assert l2_err(grad.numpy(), ref_g) <= GRAD_TOL
    assert float(np.abs(ref_g).max()) > 0


@pytest.mark.parametrize("tag", sorted(CASES))
def test_stock_warp_reproduces_the_reference_pixels(golden, tag):
    g = golden("depth_recon")
    t = _targets(g, tag)
    cam = t["camera"]
    for pred_type in ("depth", "disparity"):
        pred = torch.from_numpy(g["%s_pred_%s" % (tag, pred_type)])
        depth = pred if pred_type == "depth" else ca.DepthReconstructionLossV1.depth_from_disparity(pred)
        warped = ca.reproject_warp(t["l_img"], depth, cam["inv_K"], cam["K"], cam["baseline_T"]).numpy().reshape(-1)
        idx, val = g["%s_widx_%s_1" % (tag, pred_type)], g["%s_wval_%s_1" % (tag, pred_type)]
        assert l2_err(warped[idx], val) <= 1e-6


def test_module_surface():
    fn = ca.DepthReconstructionLossV1(2, 8, 12)
    assert fn.pred_type == "disparity" and fn.backend == "hip" and fn.use_ssim
    assert isinstance(fn.back_proj_depth, ca.BackprojectDepth) and isinstance(fn.project_3d, ca.Project3D)
    assert fn.project_3d.eps == 1e-7
    d = torch.tensor([257.0])
    assert float(fn.depth_from_disparity(d)) == pytest.approx(0.209313 * 2262.52)
    with pytest.raises(ValueError):
        ca.DepthReconstructionLossV1(2, 8, 12, backend="cuda")
    with pytest.raises(NotImplementedError):
        ca.DepthReconstructionLossV1(1, 8, 12, pred_type="inverse")({"depth": torch.ones(1, 1, 8, 12)},
                                                                    {"camera": {}, "l_img": None, "r_img": None})
    points = ca.BackprojectDepth(2, 8, 12)(torch.full((2, 1, 8, 12), 3.0), torch.eye(4).expand(2, 4, 4))
    assert points.shape == (2, 4, 96)
    assert points[1, :, 13].tolist() == [3.0, 3.0, 3.0, 1.0]           # pixel (x, y) = (1, 1)
    grid = ca.Project3D(2, 8, 12)(points, torch.eye(4).expand(2, 4, 4), torch.eye(4).expand(2, 4, 4))
    assert grid.shape == (2, 8, 12, 2)
    assert grid[0, 7, 11].tolist() == pytest.approx([1.0, 1.0], abs=1e-6) and grid[0, 0, 0].tolist() == pytest.approx([-1.0, -1.0])
    # float64 flows through the stock path untouched
    assert ca.reproject_warp(torch.rand(1, 2, 8, 12).double(), torch.ones(1, 1, 8, 12).double(), *(torch.eye(4)[None].double(),) * 3).dtype == torch.float64


def test_meta_implementations_give_the_shapes():
    m = lambda *s: torch.empty(*s, device="meta")
    out = torch.ops.cerberus.reproject_warp(m(2, 5, 7, 9), m(2, 1, 7, 9), m(2, 3, 3), m(2, 3, 4), 1e-7)
    assert out.shape == (2, 5, 7, 9) and out.dtype == torch.float32 and out.device.type == "meta"
    gd = torch.ops.cerberus.reproject_warp_backward(m(2, 5, 7, 9), m(2, 1, 7, 9), m(2, 3, 3), m(2, 3, 4), m(2, 5, 7, 9), 1e-7)
    assert gd.shape == (2, 1, 7, 9) and gd.device.type == "meta"


def test_cpu_tensors_through_the_raw_ops_raise():
    img, depth = torch.rand(1, 3, 4, 6), torch.ones(1, 1, 4, 6)
    k, p = torch.eye(3)[None], torch.eye(4)[None, :3]
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.reproject_warp(img, depth, k, p, 1e-7)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.cerberus.reproject_warp_backward(img, depth, k, p, img, 1e-7)


def test_header_and_binding_declare_the_symbols():
    with open(os.path.join(REPO, "include", "cerberus_hip.h")) as f:
        header = f.read()
    for name, nargs in (("cerberus_reproject_warp_forward", 12), ("cerberus_reproject_warp_backward", 13)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1])
    assert "#define CERBERUS_HIP_ABI_VERSION 7 " in header            # additions only
    assert "reproject.hip" in cbuild.SOURCES
    assert set(D.__all__) <= set(ca.loss_functions.__all__)
