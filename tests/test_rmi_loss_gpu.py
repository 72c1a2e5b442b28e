"""GPU tests of the fused RMI loss (csrc/rmi_loss.hip, cerberus::rmi_moments, loss_functions/rmi.py).

Yardstick: ``rmi_cases.restate`` in float64 on the CPU.  The stock chain (``backend='torch'``, and for the covariance matrices
the same restatement with its front end in fp32) runs on the GPU in the same test; its own error against float64 is ``e_stock``.
Bounds: the loss value within 1e-5 S (S = |lambda bce| + |(1 - lambda) rmi|, the project's VALUE_TOL); ``l2_err`` and ``rel_err`` of
the three covariance matrices and of grad_logits each at most 4 x max(e_stock, 2^-23) (test_seg_loss_gpu.py's bound and floor).

Shapes beyond the table of the design, chosen for the folds (p = 1, so a cell is a pixel):
  (1,17,150,150): 22500 cells = 88 front-end workgroups x 3 class groups = 264 BCE partials: threads 0..7 of the one-workgroup
                  final sum add two (second round); 148 x 148 = 21904 positions = 22 moment chunks per (n, c), added in index
                  order by the fold (the table's largest shape has 2); the mean kernel's lanes walk 88 rounds.
  (2,17,150,150): 528 partials: threads 0..15 add three (third round).
At (1,17,150,150) also ONE valid pixel, in the first, a middle and the last front-end workgroup / moment chunk.

Measured on an MI355X (worst over the 14 shapes and the label variants; fused / stock): value error 9.2e-8 S / 9.2e-8 S at
(1,17,150,150); grad_logits rel_err 3.4e-6 / 4.1e-6 at (1,19,15,23), l2_err 1.3e-6 / 1.7e-6 there, worst ratio to
max(e_stock, 2^-23) 1.10 (rel_err 1.48e-6 / 1.35e-6 at (1,19,13,22)); la_cov 8.3e-8 / 8.3e-8 at p = 3 (k / 9 is rounded; 1e-16
elsewhere), ratio 0.70; pr_cov l2_err 1.3e-7 / 1.5e-7, ratio 0.90; la_pr_cov l2_err 1.5e-7 / 1.7e-7, ratio 0.86.  BCE alone:
gradient l2_err 4.8e-8 / 4.7e-8.  Every label ignored: loss -36.1042786 against 0.25 C log(5e-4) = -36.1042867.  Peak memory at
(2,19,128,256): 1.285 x the logits' bytes fused, 8.76 x stock.  The classes, hip / torch: 0.809456408 / 0.809456229,
0.576281905 / 0.576281786, 3.58192015 / 3.58191991, 1.61891282 / 1.61891246.
"""
import functools

import numpy as np
import pytest
import torch

import cerberusnet_amd as ca
import rmi_cases as cases
from cerberusnet_amd import ops
from conftest import l2_err, rel_err

pytestmark = pytest.mark.gpu

VALUE_TOL = 1e-5
FLOOR = 2.0 ** -23
DEV = "cuda"

# (shape, pool)
TABLE = [((1, 2, 8, 8), 4), ((1, 19, 13, 22), 4), ((1, 19, 15, 23), 4), ((2, 5, 24, 40), 4), ((2, 19, 37, 53), 4),
         ((3, 5, 16, 33), 4), ((2, 150, 9, 20), 4), ((2, 4, 11, 13), 2), ((2, 3, 17, 19), 3), ((1, 3, 7, 9), 1),
         ((2, 19, 128, 256), 4), ((2, 5, 40, 56), 8), ((1, 17, 150, 150), 1), ((2, 17, 150, 150), 1)]


def _inputs(shape, seed=1000):
    return cases.logits(shape, seed + 7 * shape[1] + shape[3]), cases.labels(shape, seed + 3 + 7 * shape[1] + shape[3])


@functools.lru_cache(maxsize=None)
def _yardstick(shape, pool, variant="table"):
    """float64 on the CPU, computed once per case and left unchanged: value, S, the matrices, the gradient."""
    x, t = _inputs(shape)
    t = _variant(t, shape, variant)
    leaf = torch.from_numpy(x).double().requires_grad_(True)
    out = cases.restate(leaf, torch.from_numpy(t), shape[1], p=pool)
    grad, = torch.autograd.grad(out["loss"], leaf)
    return {"x": x, "t": t, "loss": float(out["loss"].detach()), "S": out["S"], "bce": float(out["bce"].detach()), "grad": grad.numpy(),
            "cov": [out[k].detach().numpy() for k in ("la_cov", "pr_cov", "la_pr_cov")]}


def _variant(t, shape, variant):
    N, C, H, W = shape
    if variant == "table":
        return t
    t = t.copy()
    if variant == "image_ignored":
        t[-1] = cases.IGNORE
        t[t == 3] = 0                       # and a class absent from the batch
    elif variant.startswith("one_pixel"):
        pixel = {"first": 3, "middle": (H * W // 2 // 256) * 256 + 130, "last": H * W - 2}[variant.split(":")[1]]
        keep = t.reshape(-1)[pixel]
        t[:] = cases.IGNORE
        t.reshape(-1)[pixel] = keep if keep != cases.IGNORE else 2
    return t


def _fused(x, t, C, pool, **kw):
    leaf = x.detach().requires_grad_(True)
    loss = ca.rmi_loss(leaf, t, num_classes=C, rmi_pool_size=pool, rmi_pool_stride=pool, backend="hip", **kw)
    grad, = torch.autograd.grad(loss, leaf)
    return loss, grad


def _stock(x, t, C, pool, **kw):
    leaf = x.detach().requires_grad_(True)
    loss = ca.rmi_loss(leaf, t, num_classes=C, rmi_pool_size=pool, rmi_pool_stride=pool, backend="torch", **kw)
    grad, = torch.autograd.grad(loss, leaf)
    return loss, grad


def _check_against_the_yardstick(shape, pool, variant="table"):
    y = _yardstick(shape, pool, variant)
    C = shape[1]
    x, t = torch.from_numpy(y["x"]).to(DEV), torch.from_numpy(y["t"]).to(DEV)
    loss, grad = _fused(x, t, C, pool)
    cov = torch.ops.cerberus.rmi_moments(x, t, 3, pool, True)[1:4]
    s_loss, s_grad = _stock(x, t, C, pool)
    s_out = cases.restate(x, t, C, p=pool, front=torch.float32)
    s_cov = [s_out[k] for k in ("la_cov", "pr_cov", "la_pr_cov")]
    print("%s p=%d %s: value %.9g ref %.9g: |diff| / S fused %.3e stock %.3e" % (
        shape, pool, variant, loss.item(), y["loss"], abs(loss.item() - y["loss"]) / y["S"], abs(s_loss.item() - y["loss"]) / y["S"]))
    assert loss.dtype == torch.float32 and loss.shape == () and bool(torch.isfinite(loss))
    assert abs(loss.item() - y["loss"]) <= VALUE_TOL * y["S"]
    pairs = [("grad", grad, s_grad, y["grad"])] + [(n, c, sc, r) for n, c, sc, r in zip(("la_cov", "pr_cov", "la_pr_cov"), cov, s_cov,
                                                                                       y["cov"])]
    failed = []
    for name, got, stock, ref in pairs:
        got, stock = got.detach().cpu().numpy(), stock.detach().cpu().numpy()
        for metric in (l2_err, rel_err):
            e, e_stock = metric(got, ref), metric(stock, ref)
            print("   %-9s %s fused %.3e stock %.3e" % (name, metric.__name__, e, e_stock))
            if not e <= 4 * max(e_stock, FLOOR):
                failed.append((name, metric.__name__, e, e_stock))
    assert not failed, failed
    return y, loss, grad, cov


@pytest.mark.parametrize("shape,pool", TABLE)
def test_fused_route_against_float64(shape, pool):
    """Measured on the MI355X: the module docstring and DESIGN.md 3.19."""
    y, loss, grad, cov = _check_against_the_yardstick(shape, pool)
    ignored = torch.from_numpy((y["t"] < 0) | (y["t"] >= shape[1])).to(DEV)[:, None]
    assert float(grad.abs().mul(ignored).max()) == 0.0
    for m in cov[:2]:                                               # entry (k,q) and (q,k) are the same products in the same order
        assert torch.equal(m, m.mT)
    if shape == (1, 2, 8, 8):                                       # one position: the centred points are exactly zero
        assert all(float(m.abs().max()) == 0.0 for m in cov)
        _, bce_grad = _fused(torch.from_numpy(y["x"]).to(DEV), torch.from_numpy(y["t"]).to(DEV), 2, pool, do_rmi=False)
        assert torch.equal(grad, 0.5 * bce_grad)                   # lambda bce alone carries the gradient
    if shape == (1, 19, 15, 23):                                    # row 14 and column 22 lie in no window: BCE gradient only
        x, t = torch.from_numpy(y["x"]).to(DEV), torch.from_numpy(y["t"]).to(DEV)
        _, bce_grad = _fused(x, t, 19, pool, do_rmi=False)
        assert torch.equal(grad[:, :, 14], 0.5 * bce_grad[:, :, 14]) and torch.equal(grad[..., 22], 0.5 * bce_grad[..., 22])
        assert not torch.equal(grad[:, :, 13], 0.5 * bce_grad[:, :, 13])


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_valid_pixel_in_the_first_a_middle_and_the_last_chunk(where):
    """(1,17,150,150), p = 1: the pixel's workgroup is 0, 43 or 87 of 88 and its position's chunk 0, 10 / 11 or 21 of 22: a
    partial read from the wrong slot changes the value (the BCE is this pixel's alone) and the matrices."""
    shape, pool = (1, 17, 150, 150), 1
    y, loss, grad, cov = _check_against_the_yardstick(shape, pool, "one_pixel:" + where)
    valid = (y["t"] != cases.IGNORE)
    assert int(valid.sum()) == 1
    live = torch.from_numpy(valid).to(DEV)[:, None].expand_as(grad)
    assert float(grad[~live].abs().max()) == 0.0 and float(grad[live].abs().min()) > 0.0
    state = torch.ops.cerberus.rmi_moments(torch.from_numpy(y["x"]).to(DEV), torch.from_numpy(y["t"]).to(DEV), 3, pool, True)[7]
    assert state[1].item() == 1.0 and state[2].item() == 0.5


def test_labels_that_are_ignored():
    shape, pool = (2, 19, 37, 53), 4
    C = shape[1]
    y, *_ = _check_against_the_yardstick(shape, pool, "image_ignored")           # an image with every label ignored, class 3 absent
    assert (y["t"][-1] == cases.IGNORE).all() and not (y["t"] == 3).any() and (y["t"] == 4).any()
    t0 = _yardstick(shape, pool)["t"]
    x = torch.from_numpy(y["x"]).to(DEV)
    # negative labels and labels >= C other than 255: the same bits as 255
    t = torch.from_numpy(t0).to(DEV)
    odd = t.clone()
    n_ign = int((t == cases.IGNORE).sum())
    odd[t == cases.IGNORE] = torch.tensor([-1, -7, C, 99, 1 << 40, -(1 << 40)], device=DEV)[torch.arange(n_ign, device=DEV) % 6]
    a, b = _fused(x, t, C, pool), _fused(x, odd, C, pool)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for u, v in zip(torch.ops.cerberus.rmi_moments(x, t, 3, pool, True), torch.ops.cerberus.rmi_moments(x, odd, 3, pool, True)):
        assert torch.equal(u, v)
    # every label ignored everywhere: bce = 0, a finite loss (0.5 logdet(5e-4 I) per class), a gradient of zeros
    none = torch.full_like(t, cases.IGNORE)
    loss, grad = _fused(x, none, C, pool)
    out = torch.ops.cerberus.rmi_moments(x, none, 3, pool, True)
    want = 0.5 * C * 0.5 * np.log(5e-4)
    print("all ignored: loss %.9g, 0.25 C log(5e-4) = %.9g" % (loss.item(), want))
    assert out[0].item() == 0.0 and bool(torch.isfinite(loss)) and abs(loss.item() - want) <= VALUE_TOL * abs(want)
    # the probability map is 1e-6 times the share of a window that lies inside the image: not constant at the border
    assert float(grad.abs().max()) == 0.0 and float(out[1].abs().max()) == 0.0 and float(out[3].abs().max()) == 0.0
    assert 0.0 < float(out[2].abs().max()) < 1e-9
    # a NaN logit under an ignored label changes nothing
    poisoned = x.clone()
    poisoned[0][:, t[0] == cases.IGNORE] = float("nan")
    assert bool(torch.isnan(poisoned).any())
    c = _fused(poisoned, t, C, pool)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_do_rmi_off_is_the_bce_part_and_writes_no_maps():
    shape, pool = (2, 19, 37, 53), 4
    y = _yardstick(shape, pool)
    x, t = torch.from_numpy(y["x"]).to(DEV), torch.from_numpy(y["t"]).to(DEV)
    off = torch.ops.cerberus.rmi_moments(x, t, 3, pool, False)
    on = torch.ops.cerberus.rmi_moments(x, t, 3, pool, True)
    assert all(o.numel() == 0 for o in off[1:7]) and torch.equal(off[0], on[0]) and torch.equal(off[7], on[7])
    loss, grad = _fused(x, t, 19, pool, do_rmi=False)
    s_loss, s_grad = _stock(x, t, 19, pool, do_rmi=False)
    leaf = torch.from_numpy(y["x"]).double().requires_grad_(True)
    ref = cases.restate(leaf, torch.from_numpy(y["t"]), 19, p=pool, do_rmi=False)["loss"]
    ref_grad, = torch.autograd.grad(ref, leaf)
    assert torch.equal(loss, off[0]) and abs(loss.item() - y["bce"]) <= VALUE_TOL * y["bce"] and float(ref.detach()) == y["bce"]
    for metric in (l2_err, rel_err):
        e, e_stock = metric(grad.cpu().numpy(), ref_grad.numpy()), metric(s_grad.cpu().numpy(), ref_grad.numpy())
        print("bce only: grad %s fused %.3e stock %.3e" % (metric.__name__, e, e_stock))
        assert e <= 4 * max(e_stock, FLOOR)
    assert int(on[7][1].item()) == int((y["t"] != cases.IGNORE).sum())


def test_two_calls_and_a_misaligned_view_give_the_same_bits():
    """(2,19,37,53) (scalar loads either way) and (2,5,24,40) (p = 4 and W even: the 8-byte route when aligned, the scalar route
    4 bytes into a buffer): loss, matrices, maps and gradient bit for bit."""
    for shape, pool in (((2, 19, 37, 53), 4), ((2, 5, 24, 40), 4), ((2, 5, 40, 56), 8)):
        y = _yardstick(shape, pool)
        C = shape[1]
        x, t = torch.from_numpy(y["x"]).to(DEV), torch.from_numpy(y["t"]).to(DEV)
        buf = torch.zeros(x.numel() + 1, dtype=torch.float32, device=DEV)
        tbuf = torch.zeros(t.numel() + 1, dtype=torch.int64, device=DEV)
        xv, tv = buf[1:].view(shape), tbuf[1:].view(t.shape)
        xv.copy_(x)
        tv.copy_(t)
        assert xv.data_ptr() % 16 == 4 and tv.data_ptr() % 16 == 8 and xv.is_contiguous()
        runs = [(_fused(a, b, C, pool), torch.ops.cerberus.rmi_moments(a, b, 3, pool, True)) for a, b in ((x, t), (x, t), (xv, tv))]
        for (l, g), outs in runs[1:]:
            assert torch.equal(l, runs[0][0][0]) and torch.equal(g, runs[0][0][1])
            for u, v in zip(outs, runs[0][1]):
                assert torch.equal(u, v)


def test_peak_memory_is_the_gradient_two_pooled_maps_and_the_workspace():
    """(2,19,128,256): the excess of torch.cuda.max_memory_allocated over the level before the call (the inputs are allocated by
    then) is at most 1.25 x the logits' bytes + 1 MB: the gradient (1.0), two pooled maps (33 x 65 / (128 x 256) = 0.065 each), the
    145 KB workspace and the 9 x 9 algebra.  The stock chain's two float64 stacks alone are 2 x 9 x 31 x 63 x 8 / (128 x 256 x 4) =
    2.15 x; its figure is printed beside the fused one."""
    shape, pool = (2, 19, 128, 256), 4
    y = _yardstick(shape, pool)
    x, t = torch.from_numpy(y["x"]).to(DEV), torch.from_numpy(y["t"]).to(DEV)
    _fused(x, t, 19, pool)                                                      # warm: the library, the solver's handles
    torch.cuda.synchronize()
    results = {}
    for name, fn in (("fused", _fused), ("stock", _stock)):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss, grad = fn(x, t, 19, pool)
        torch.cuda.synchronize()
        results[name] = (torch.cuda.max_memory_allocated() - before) / (x.numel() * 4)
        del loss, grad
    print("peak excess / logits bytes: fused %.3f stock %.3f" % (results["fused"], results["stock"]))
    assert results["fused"] * x.numel() * 4 <= 1.25 * x.numel() * 4 + (1 << 20)
    assert ops._rmi_workspace_bytes(2, 19, 128, 256, 4) == 148608


def test_the_classes_on_both_backends():
    shape = (2, 5, 24, 40)
    x1, t_np = _inputs(shape, 1100)
    x2, _ = _inputs(shape, 1200)
    x1, x2, t = torch.from_numpy(x1).to(DEV), torch.from_numpy(x2).to(DEV), torch.from_numpy(t_np).to(DEV)

    def run(make, call):
        out = []
        for backend in ("hip", "torch"):
            a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
            loss = call(make(backend), a, b)
            out.append((loss, torch.autograd.grad(loss, [v for v in (a, b)], allow_unused=True)))
        return out

    def close(pair, scale):
        (lh, gh), (lt, gt) = pair
        print("   hip %.9g torch %.9g" % (lh.item(), lt.item()))
        assert abs(lh.item() - lt.item()) <= 2 * VALUE_TOL * scale
        for u, v in zip(gh, gt):
            assert (u is None) == (v is None)
            if u is not None:
                assert l2_err(u.cpu().numpy(), v.cpu().numpy()) <= 1e-5

    outs = [cases.restate(torch.from_numpy(v.cpu().numpy()).double(), torch.from_numpy(t_np), 5) for v in (x1, x2)]
    parts = [(float(o["bce"]), float(o["rmi"])) for o in outs]
    S1 = outs[0]["S"]
    kw = dict(num_classes=5, weight=0.5, aux_weight=0.4)
    aux = lambda backend: ca.RMILossAux(backend=backend, **kw)
    close(run(aux, lambda m, a, b: m({"seg": a, "seg_aux": b}, {"seg": t})), cases.golden_scale("RMILossAux", kw, {"aux": True}, parts))
    close(run(aux, lambda m, a, b: m({"seg": a}, {"seg": t[:, None]})), cases.golden_scale("RMILossAux", kw, {"aux": False}, parts))
    for ocr in (False, True):
        kw = dict(num_classes=5, ocr_aux_rmi=ocr)
        ms = lambda backend: ca.MultiScaleRMILoss(backend=backend, **kw)
        close(run(ms, lambda m, a, b: m({"pred": a, "aux": b}, t)), cases.golden_scale("MultiScaleRMILoss", kw, {}, parts))
    # the two fallbacks of backend='hip' are the stock chain itself: max pooling, and fp16 logits
    mx = lambda backend: ca.RMILoss(num_classes=5, rmi_pool_way=0, backend=backend)
    (lh, gh), (lt, gt) = run(mx, lambda m, a, b: m(a, t))
    assert torch.equal(lh, lt) and torch.equal(gh[0], gt[0])
    half = lambda backend: ca.RMILoss(num_classes=5, backend=backend)
    (lh, gh), (lt, gt) = run(half, lambda m, a, b: m(a.half(), t))
    assert torch.equal(lh, lt) and torch.equal(gh[0], gt[0]) and lh.dtype == torch.float32
    # and the fused route really is another one: same value to rounding, not the same bits
    (lh, _), (lt, _) = run(half, lambda m, a, b: m(a, t))
    assert abs(lh.item() - lt.item()) <= 2 * VALUE_TOL * S1


def test_raw_op_rejects_what_the_wrapper_routes_elsewhere():
    x, t = torch.zeros(1, 3, 16, 16, device=DEV), torch.zeros(1, 16, 16, dtype=torch.int64, device=DEV)
    for args in ((x, t, 2, 4, True), (x, t, 3, 9, True), (x[..., :7, :], t[:, :7], 3, 4, True), (x.half(), t, 3, 4, True),
                 (x, t.int(), 3, 4, True), (x, t[:, :8], 3, 4, True)):
        with pytest.raises(RuntimeError, match="cerberus::rmi_moments"):
            torch.ops.cerberus.rmi_moments(*args)
    leaf = x.clone().requires_grad_(True)
    out = torch.ops.cerberus.rmi_moments(leaf, t, 3, 4, True)
    assert not out[1].requires_grad and out[2].requires_grad and out[3].requires_grad and not out[4].requires_grad
    g, = torch.autograd.grad(out[0] + out[2].sum() + out[3].sum(), leaf, create_graph=True)
    with pytest.raises(RuntimeError, match="no double backward"):
        g.sum().backward()
