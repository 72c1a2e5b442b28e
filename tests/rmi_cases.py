"""Inputs and the yardstick of the RMI-loss tests, shared by tests/test_rmi_loss_cpu.py, tests/test_rmi_loss_gpu.py and the
generator of tests/golden/rmi_loss.npz (tools/gen_golden_rmi.py).

Inputs come from ``hash_uniform`` seeds as in seg_loss_cases.py: logits uniform in [-4, 4), labels skewed as
``min(floor(u * u * C), C - 1)`` and about 15 % of them set to the ignore value 255.

``restate`` is the test-owned float64 statement of the loss (steps 1-8 of the design): it shares no code with
the package and returns the parts the tests compare; the yardstick is its float64 run on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

from cerberusnet_amd.synth import hash_uniform

IGNORE_SHARE = 0.15
IGNORE = 255

# the golden cases: (class name, shape (N,C,H,W), constructor keywords, forward keywords, target given as (N,1,H,W))
GOLDEN_CASES = [
    ("RMILoss", (2, 5, 24, 40), dict(num_classes=5), dict(), False),
    ("RMILoss", (2, 5, 24, 40), dict(num_classes=5), dict(do_rmi=False), False),
    ("RMILoss", (1, 19, 13, 22), dict(num_classes=19, lambda_way=0, loss_weight_lambda=0.3), dict(), True),
    ("RMILoss", (2, 4, 11, 13), dict(num_classes=4, rmi_pool_size=2, rmi_pool_stride=2), dict(), False),
    ("RMILoss", (1, 3, 7, 9), dict(num_classes=3, rmi_pool_size=1, rmi_pool_stride=1), dict(), False),
    ("RMILoss", (2, 3, 19, 20), dict(num_classes=3, rmi_pool_way=0), dict(), False),
    ("RMILoss", (2, 3, 19, 20), dict(num_classes=3, rmi_pool_way=2, lambda_way=0), dict(), False),
    ("RMILoss", (2, 3, 19, 20), dict(num_classes=3, rmi_radius=2), dict(), False),
    ("RMILoss", (2, 3, 19, 20), dict(num_classes=3, rmi_radius=1, rmi_pool_size=2, rmi_pool_stride=2), dict(), False),
    ("RMILossAux", (2, 5, 24, 40), dict(num_classes=5, weight=0.5, aux_weight=0.4), dict(aux=True), False),
    ("RMILossAux", (1, 19, 15, 23), dict(num_classes=19), dict(aux=False), False),
    ("MultiScaleRMILoss", (2, 5, 24, 40), dict(num_classes=5, ocr_aux_rmi=False), dict(), False),
    ("MultiScaleRMILoss", (2, 5, 24, 40), dict(num_classes=5, ocr_aux_rmi=True, alpha=0.3), dict(), False),
]


def logits(shape, seed):
    return hash_uniform(shape, seed, -4.0, 4.0)


def labels(shape, seed, ignore_share=IGNORE_SHARE, ignore=IGNORE):
    """(N,H,W) int64 labels for logits of ``shape`` = (N,C,H,W)."""
    N, C, H, W = shape
    u = hash_uniform((N, H, W), seed, 0.0, 1.0, dtype=np.float64)
    t = np.minimum(np.floor(u * u * C), C - 1).astype(np.int64)
    drop = hash_uniform((N, H, W), seed + 1, 0.0, 1.0) < ignore_share
    t[drop] = ignore
    return t


def golden_inputs(i):
    """The logits of golden case ``i`` -- one (N,C,H,W) float32 array per prediction the class reads -- and its target."""
    name, shape, _, fwd, four_d = GOLDEN_CASES[i]
    heads = 2 if name == "MultiScaleRMILoss" or fwd.get("aux") else 1
    xs = [logits(shape, 900 + 10 * i + k) for k in range(heads)]
    t = labels(shape, 905 + 10 * i)
    return xs, (t[:, None] if four_d else t)


def golden_call(module, name, fwd, xs, t):
    """Run golden case's class (of ``module``: the reference's or the package's) on tensors ``xs`` and ``t``."""
    if name == "RMILoss":
        return module(xs[0], t, **fwd)
    if name == "RMILossAux":
        preds = {"seg": xs[0]}
        if fwd["aux"]:
            preds["seg_aux"] = xs[1]
        return module(preds, {"seg": t})
    return module({"pred": xs[0], "aux": xs[1]}, t)


def golden_scale(name, kwargs, fwd, parts):
    """S of a golden case: the sum of the absolute values of the weighted bce and rmi terms the loss is made of; ``parts`` holds
    (bce, rmi) of every prediction."""
    lam, way = kwargs.get("loss_weight_lambda", 0.5), kwargs.get("lambda_way", 1)
    term = lambda bce, rmi, on: (abs(lam * bce) + abs((1 - lam) * rmi) if way else abs(bce) + abs(lam * rmi)) if on else abs(bce)
    if name == "RMILoss":
        return term(*parts[0], fwd.get("do_rmi", True))
    if name == "RMILossAux":
        s = term(*parts[0], True) + (kwargs.get("aux_weight", 0.4) * term(*parts[1], True) if fwd["aux"] else 0.0)
        return kwargs.get("weight", 1.0) * s
    return term(*parts[0], True) + kwargs.get("alpha", 0.4) * term(*parts[1], kwargs["ocr_aux_rmi"])


def restate(x, y, C, R=3, p=4, lam=0.5, lambda_way=1, do_rmi=True, front=torch.float64):
    """Steps 1-8 in float64, on the device of ``x``.  ``x``: (N,C,H,W) tensor (a leaf that requires grad gives the gradient),
    ``y``: (N,H,W) int64.  Returns a dict: loss, bce, rmi, S, and with ``do_rmi`` la_cov, pr_cov, la_pr_cov.
    ``front=torch.float32`` runs steps 1-4 (up to the pooled maps) in fp32 as the stock chain does: its covariance matrices are
    what the stock ops would give."""
    x = x.to(front)
    valid = (y >= 0) & (y < C)
    onehot = F.one_hot(torch.where(valid, y, torch.zeros_like(y)), C).permute(0, 3, 1, 2).to(front) * valid[:, None]
    vf = valid[:, None].to(front)
    bce = (F.binary_cross_entropy_with_logits(x, onehot, reduction="none") * vf).sum() / (valid.sum().to(front) + 1.0)
    out = {"bce": bce, "loss": bce, "S": abs(float(bce.detach())), "rmi": None}
    if not do_rmi:
        return out
    prob = torch.sigmoid(x) * vf + 1e-6
    if p > 1:
        onehot, prob = F.avg_pool2d(onehot, p, p, p // 2), F.avg_pool2d(prob, p, p, p // 2)
    h, w = onehot.shape[2:]
    nh, nw = h - R + 1, w - R + 1
    slices = lambda m: torch.stack([m[:, :, a:a + nh, b:b + nw] for a in range(R) for b in range(R)], 2).flatten(3)
    L, P = slices(onehot).double(), slices(prob).double()
    L, P = L - L.mean(3, keepdim=True), P - P.mean(3, keepdim=True)
    eye = torch.eye(R * R, dtype=torch.float64, device=x.device) * 5e-4
    la_cov, pr_cov, la_pr_cov = L @ L.mT, P @ P.mT, L @ P.mT
    appro = la_cov - la_pr_cov @ torch.linalg.inv(pr_cov + eye) @ la_pr_cov.mT
    chol = torch.linalg.cholesky(appro + eye)
    logdet = 2.0 * torch.log(torch.diagonal(chol, dim1=-2, dim2=-1) + 1e-8).sum(-1)
    rmi = ((0.5 * logdet).mean(0) / (R * R)).sum()
    if lambda_way:
        loss, S = lam * bce.double() + (1 - lam) * rmi, abs(lam * float(bce.detach())) + abs((1 - lam) * float(rmi.detach()))
    else:
        loss, S = bce.double() + lam * rmi, abs(float(bce.detach())) + abs(lam * float(rmi.detach()))
    out.update(loss=loss, rmi=rmi, S=S, la_cov=la_cov, pr_cov=pr_cov, la_pr_cov=la_pr_cov)
    return out
