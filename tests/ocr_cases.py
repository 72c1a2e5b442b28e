"""Seeded inputs of the OCR head's two steps and their float64 restatement in the reference's operation order
(nnet_models/ocr_utils.py: SpatialGather_Module.forward, ObjectAttentionBlock.forward between f_pixel / f_object / f_down and f_up).
The GPU tests take the float64 run on the CPU as their yardstick and the same chain in fp32 on the GPU as the error to compare with.
"""
import numpy as np
import torch

from cerberusnet_amd.synth import hash_uniform
from conftest import l2_err, rel_err  # noqa: F401  (the two metrics of every comparison here)


def tensor(shape, seed, lo=-1.0, hi=1.0):
    return torch.from_numpy(np.array(hash_uniform(tuple(shape), seed, lo, hi), order="C"))


def gather_inputs(B, C, K, H, W, seed, logit_range=3.0):
    """feats (B,C,H,W), logits (B,K,H,W), the upstream gradient of the context (B,C,K,1)."""
    return (tensor((B, C, H, W), seed), tensor((B, K, H, W), seed + 1, -logit_range, logit_range), tensor((B, C, K, 1), seed + 2))


def attention_inputs(B, C, R, H, W, seed, query_range=1.0):
    """query (B,C,H,W), key and value (B,C,R), the upstream gradient of the context (B,C,H,W)."""
    return (tensor((B, C, H, W), seed, -query_range, query_range), tensor((B, C, R), seed + 1), tensor((B, C, R), seed + 2),
            tensor((B, C, H, W), seed + 3))


def gather_chain(feats, probs, scale=1.0):
    """SpatialGather_Module.forward in stock ops: (B,C,K,1)."""
    batch_size, c = probs.size(0), probs.size(1)
    probs = probs.reshape(batch_size, c, -1)
    feats = feats.reshape(batch_size, feats.size(1), -1).permute(0, 2, 1)
    probs = torch.softmax(scale * probs, dim=2)
    return torch.matmul(probs, feats).permute(0, 2, 1).unsqueeze(3)


def attention_chain(query, key, value, scale):
    """The core of ObjectAttentionBlock.forward in stock ops: (B,C,H,W)."""
    B, C, H, W = query.shape
    q = query.reshape(B, C, -1).permute(0, 2, 1)
    sim_map = torch.matmul(q, key)
    sim_map = scale * sim_map
    sim_map = torch.softmax(sim_map, dim=-1)
    context = torch.matmul(sim_map, value.permute(0, 2, 1))
    return context.permute(0, 2, 1).contiguous().view(B, C, H, W)


BLOCK = dict(high_level_ch=24, mid_channels=16, key_channels=8, classes=5)       # the golden's OCR_block (tests/golden/ocr_head.npz)
BLOCK_INPUT = (2, 24, 9, 12)
BLOCK_SEED = 1000


def block_input(shape=BLOCK_INPUT, seed=41):
    return tensor(shape, seed)


def block_loss(cls_out, aux_out, ocr_feats):
    """One scalar that every output feeds."""
    return (cls_out * cls_out).mean() + (aux_out * aux_out).mean() + (ocr_feats * ocr_feats).mean()


def make_block(cls, backend=None, **sizes):
    """An ``OCR_block`` of ``cls`` with seeded parameters, in train mode with its one Dropout2d at p = 0: the BatchNorm layers use
    their batch statistics and nothing is random."""
    from cerberusnet_amd.synth import fill_parameters
    sizes = dict(BLOCK, **sizes)
    kwargs = {} if backend is None else {"backend": backend}
    block = cls(sizes["high_level_ch"], mid_channels=sizes["mid_channels"], key_channels=sizes["key_channels"], classes=sizes["classes"],
                **kwargs)
    fill_parameters(block, BLOCK_SEED)
    drops = [m for m in block.modules() if isinstance(m, torch.nn.Dropout2d)]
    assert len(drops) == 1
    drops[0].p = 0.0
    return block.train()


def run(fn, inputs, upstream, device, dtype):
    """(output, gradients of the inputs) of ``fn(*inputs)`` under ``upstream``, computed on ``device`` in ``dtype``, returned as
    float64 CPU tensors."""
    leaves = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    grads = torch.autograd.grad(out, leaves, grad_outputs=upstream.to(device=device, dtype=dtype))
    return [out.detach().double().cpu()] + [g.double().cpu() for g in grads]


FLOOR = 2.0 ** -23


def bound(e_stock):
    """4 x max(the stock chain's own error, one fp32 ulp of 1): the rule of test_seg_loss_gpu.py and test_rmi_loss_gpu.py."""
    return 4.0 * max(e_stock, FLOOR)
