"""Seeded inputs of the DETR attention core (csrc/detr_attn.hip), its float64 restatement in stock ops with the reference's reshape of
the (L,B,E) tensors into heads (``nn.MultiheadAttention`` as nnet_models/detr/transformer.py calls it: ``softmax(scale q k^T + mask)``,
times ``keep / (1 - p)``, times ``v``), and the dropout keep hash of csrc/attn_dropout.h restated in torch integer ops.  The GPU tests
take the float64 run on the CPU as their yardstick and the same chain in fp32 on the GPU as the error to compare with."""
import math

import numpy as np
import torch

from cerberusnet_amd.synth import hash_uniform
from conftest import l2_err, rel_err  # noqa: F401  (the two metrics of every comparison here)
from ocr_cases import FLOOR, bound  # noqa: F401  (4 x max(e_stock, 2^-23))

HEAD_DIM = 32


def tensor(shape, seed, lo=-1.0, hi=1.0):
    return torch.from_numpy(np.array(hash_uniform(tuple(shape), seed, lo, hi), order="C"))


def inputs(Lq, Lk, B, H, seed, query_range=1.0):
    """q (Lq,B,E), k and v (Lk,B,E), the upstream gradient of the output (Lq,B,E); E = 32 H."""
    E = H * HEAD_DIM
    return (tensor((Lq, B, E), seed, -query_range, query_range), tensor((Lk, B, E), seed + 1), tensor((Lk, B, E), seed + 2),
            tensor((Lq, B, E), seed + 3))


def padding_mask(B, Lk, head, tail):
    """(B,Lk) bool: entry b ignores its first ``head[b]`` and its last ``tail[b]`` keys."""
    mask = torch.zeros(B, Lk, dtype=torch.bool)
    for b in range(B):
        mask[b, :head[b]] = True
        if tail[b]:
            mask[b, Lk - tail[b]:] = True
    return mask


def chain(q, k, v, n_heads, scale, key_padding_mask=None, keep=None, p=0.0):
    """The attention core in stock ops, in the dtype and on the device of ``q``: (Lq,B,E)."""
    Lq, B, E = q.shape
    Lk, D = k.shape[0], E // n_heads
    qh = q.contiguous().view(Lq, B * n_heads, D).transpose(0, 1)
    kh = k.contiguous().view(Lk, B * n_heads, D).transpose(0, 1)
    vh = v.contiguous().view(Lk, B * n_heads, D).transpose(0, 1)
    attn = scale * torch.bmm(qh, kh.transpose(1, 2))
    if key_padding_mask is not None:
        attn = attn.view(B, n_heads, Lq, Lk).masked_fill(key_padding_mask.to(q.device)[:, None, None, :], float("-inf")).view(B * n_heads, Lq, Lk)
    attn = torch.softmax(attn, dim=-1)
    if keep is not None:
        attn = attn * (keep.to(device=q.device, dtype=q.dtype).view(B * n_heads, Lq, Lk) / (1.0 - p))
    out = torch.bmm(attn, vh)
    return out.transpose(0, 1).contiguous().view(Lq, B, E)


def lse_chain(q, k, n_heads, scale, key_padding_mask=None):
    """The log-sum-exp of every row of ``scale q k^T + mask``: (B,H,Lq)."""
    Lq, B, E = q.shape
    Lk, D = k.shape[0], E // n_heads
    qh = q.contiguous().view(Lq, B * n_heads, D).transpose(0, 1)
    kh = k.contiguous().view(Lk, B * n_heads, D).transpose(0, 1)
    attn = (scale * torch.bmm(qh, kh.transpose(1, 2))).view(B, n_heads, Lq, Lk)
    if key_padding_mask is not None:
        attn = attn.masked_fill(key_padding_mask.to(q.device)[:, None, None, :], float("-inf"))
    return torch.logsumexp(attn, dim=-1)


def run(fn, tensors, upstream, device, dtype):
    """(output, gradients of ``tensors``) of ``fn(*tensors)`` under ``upstream``, computed on ``device`` in ``dtype``, returned as
    float64 CPU tensors."""
    leaves = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    grads = torch.autograd.grad(out, leaves, grad_outputs=upstream.to(device=device, dtype=dtype))
    return [out.detach().double().cpu()] + [g.double().cpu() for g in grads]


# ---- the keep hash (csrc/attn_dropout.h), in int64 tensors holding 32-bit values ---------------------------------------------------
M32 = 0xFFFFFFFF


def _mul32(x, c):
    """(x * c) mod 2^32 for an int64 tensor (or int) x < 2^32 and a constant c < 2^32, without leaving 63 bits."""
    lo, hi = x & 0xFFFF, x >> 16
    return (lo * c + (((hi * c) & 0xFFFF) << 16)) & M32


def _mix(x):
    x = x ^ (x >> 16)
    x = _mul32(x, 0x85EBCA6B)
    x = x ^ (x >> 13)
    x = _mul32(x, 0xC2B2AE35)
    return x ^ (x >> 16)


def keep_threshold(p):
    """min(2^32 - 1, floor(p 2^32)) for the fp32 value of p."""
    return int(min(4294967295.0, math.floor(float(np.float32(p)) * 4294967296.0)))


def keep_reference(seed, B, H, Lq, Lk, p):
    """(B,H,Lq,Lk) bool: the keep decision of every (plane, query, key) for the integer ``seed``."""
    if keep_threshold(p) == 0:
        return torch.ones(B, H, Lq, Lk, dtype=torch.bool)
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = s & M32, s >> 32
    plane = torch.arange(B * H, dtype=torch.int64)
    plane_key = _mix(lo ^ _mix((hi + _mul32(plane + 1, 0x9E3779B9)) & M32))                     # (B H,)
    i = torch.arange(Lq, dtype=torch.int64)
    row_key = _mix((plane_key[:, None] + _mul32(i, 0x85EBCA77)[None, :]) & M32)                 # (B H, Lq)
    j = torch.arange(Lk, dtype=torch.int64)
    h = _mix(row_key[:, :, None] ^ _mul32(j, 0xC2B2AE3D)[None, None, :])                        # (B H, Lq, Lk)
    return (h >= keep_threshold(p)).view(B, H, Lq, Lk)


# ---- the head (nnet_models/detr): seeded modules and inputs, the same on the reference's side (tools/gen_golden_detr_head.py) --------
HEAD = dict(num_channels=24, num_classes=5, num_queries=10)
FEATURES = (2, 24, 9, 13)
D_MODEL = 64
HEAD_SEED, TRANSFORMER_SEED, POSITION_SEED = 2000, 3000, 3500


def transformer_config(normalize_before=False, dropout=0.1):
    """d_model 64, 2 heads (width 32), feed-forward 64, 2 + 2 layers; 'hidden_dim' is the position encoding's; 'n_heads' and
    'enc_layers' are the reference config's misspelt keys, which the transformer swallows."""
    return dict(hidden_dim=D_MODEL, d_model=D_MODEL, nhead=2, encoder_layers=2, decoder_layers=2, dim_feedforward=64, dropout=dropout,
                normalize_before=normalize_before, return_intermediate_dec=True, n_heads=4, enc_layers=3)


def seed_parameters(module, seed):
    """``fill_parameters``, then 1 added to every LayerNorm weight: the seeded weights are small, and a norm that scales by about
    0.05 would leave every output next to its bias."""
    from cerberusnet_amd.synth import fill_parameters
    fill_parameters(module, seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.add_(1.0)
    return module


def make_head(cls, normalize_before=False, pos_type="sine", aux_loss=True, dropout=0.1, **kwargs):
    head = cls(HEAD["num_channels"], HEAD["num_classes"], HEAD["num_queries"], dict(type=pos_type),
               transformer_config(normalize_before, dropout), aux_loss=aux_loss, **kwargs)
    return seed_parameters(head, HEAD_SEED).eval()


def make_transformer(cls, normalize_before=False, **kwargs):
    return seed_parameters(cls(**transformer_config(normalize_before), **kwargs), TRANSFORMER_SEED).eval()


def features(shape=FEATURES, seed=71):
    return tensor(shape, seed)


def transformer_inputs():
    """src (2,64,9,13), a padding mask (entry 1 ignores its last three columns), query_embed (10,64), pos_embed like src."""
    B, _, H, W = FEATURES
    mask = torch.zeros(B, H, W, dtype=torch.bool)
    mask[1, :, -3:] = True
    return tensor((B, D_MODEL, H, W), 72), mask, tensor((HEAD["num_queries"], D_MODEL), 73), tensor((B, D_MODEL, H, W), 74)


def head_loss(out):
    """One scalar that every output of the head feeds."""
    terms = [out["logits"], out["bboxes"]] + [t for aux in out.get("aux_outputs", []) for t in (aux["logits"], aux["bboxes"])]
    return sum((t * t).mean() for t in terms)
