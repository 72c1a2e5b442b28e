"""The DETR head's transformer: the reference's nnet_models/detr/transformer.py (constructor arguments, ``forward`` signatures and
``state_dict`` keys, so the ``detr.transformer.*`` entries of a reference checkpoint load) in stock ops around ONE fused step, the
attention core of csrc/detr_attn.hip.

Every layer keeps its ``nn.MultiheadAttention`` submodules: they own ``in_proj_weight``, ``in_proj_bias`` and ``out_proj.*``.  With
``backend='hip'`` a layer does what that module does around its core itself -- ``F.linear`` with the three slices of
``in_proj_weight``, ``ops_attn.detr_attention`` (with the module's dropout when training), ``out_proj`` -- and never forms the
(B H, Lq, Lk) probability tensor that the module's default ``need_weights=True`` materialises.  Everything the core does not take
calls the module as the reference does: ``backend='torch'``, CPU tensors, 16-bit tensors, autocast, head widths other than 32, an
``attn_mask``, a key-padding mask that is not bool.

A query whose keys are all masked gives the out_proj bias on the fused route and NaN on the stock one.
"""
import copy

import torch
import torch.nn.functional as F
from torch import nn

from ... import ops_attn

# Opt-in (profiles/detr_attn_fused.txt): against nn.MultiheadAttention as the reference calls it the fused route is
# 1.36 x faster at (Lq, Lk, B, H) = (2048, 2048, 2, 8) and 0.72 x at the decoder's (100, 2048, 2, 8); the rule asks for "not slower"
# at both.  At the workload's own 32768 tokens only backend='hip' can run at all.
DEFAULT_ATTENTION_BACKEND = "torch"


def _check_backend(backend):
    if backend not in ("hip", "torch"):
        raise ValueError("backend must be 'hip' or 'torch', got %r" % (backend,))
    return backend


def _takes_fused_route(mha, query, key, value, key_padding_mask, attn_mask):
    if attn_mask is not None or not mha._qkv_same_embed_dim or mha.batch_first or mha.bias_k is not None or mha.add_zero_attn:
        return False
    if key_padding_mask is not None and key_padding_mask.dtype != torch.bool:
        return False
    if mha.in_proj_weight.dtype != torch.float32 or query.dim() != 3:
        return False
    return ops_attn.attn_fused_ok(query, key, value, mha.num_heads)


def attend(mha, query, key, value, key_padding_mask=None, attn_mask=None, backend="torch"):
    """``mha(query, key, value, attn_mask=..., key_padding_mask=...)[0]`` for an ``nn.MultiheadAttention`` and (L,B,E) tensors; with
    ``backend='hip'`` through the fused core where it applies."""
    if backend == "hip" and _takes_fused_route(mha, query, key, value, key_padding_mask, attn_mask):
        e = mha.embed_dim
        w, b = mha.in_proj_weight, mha.in_proj_bias
        bias = (None, None, None) if b is None else (b[:e], b[e:2 * e], b[2 * e:])
        q = F.linear(query, w[:e], bias[0])
        k = F.linear(key, w[e:2 * e], bias[1])
        v = F.linear(value, w[2 * e:], bias[2])
        out = ops_attn.detr_attention(q, k, v, mha.num_heads, key_padding_mask, mha.dropout if mha.training else 0.0)
        return mha.out_proj(out)
    return mha(query, key, value=value, attn_mask=attn_mask, key_padding_mask=key_padding_mask)[0]


def _activation(name):
    fns = {"relu": F.relu, "gelu": F.gelu, "glu": F.glu}
    if name not in fns:
        raise RuntimeError("activation should be relu/gelu, not %s." % name)
    return fns[name]


def _clones(module, count):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(count)])


def _add(tensor, pos):
    return tensor if pos is None else tensor + pos


class TransformerEncoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", normalize_before=False,
                 backend=DEFAULT_ATTENTION_BACKEND):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.activation = _activation(activation)
        self.normalize_before = normalize_before
        self.backend = _check_backend(backend)

    def with_pos_embed(self, tensor, pos):
        return _add(tensor, pos)

    def _attention(self, x, src_mask, src_key_padding_mask, pos):
        qk = _add(x, pos)
        return attend(self.self_attn, qk, qk, x, src_key_padding_mask, src_mask, self.backend)

    def _feed_forward(self, x):
        return self.linear2(self.dropout(self.activation(self.linear1(x))))

    def forward_post(self, src, src_mask=None, src_key_padding_mask=None, pos=None):
        src = self.norm1(src + self.dropout1(self._attention(src, src_mask, src_key_padding_mask, pos)))
        return self.norm2(src + self.dropout2(self._feed_forward(src)))

    def forward_pre(self, src, src_mask=None, src_key_padding_mask=None, pos=None):
        src = src + self.dropout1(self._attention(self.norm1(src), src_mask, src_key_padding_mask, pos))
        return src + self.dropout2(self._feed_forward(self.norm2(src)))

    def forward(self, src, src_mask=None, src_key_padding_mask=None, pos=None):
        if self.normalize_before:
            return self.forward_pre(src, src_mask, src_key_padding_mask, pos)
        return self.forward_post(src, src_mask, src_key_padding_mask, pos)


class TransformerDecoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", normalize_before=False,
                 backend=DEFAULT_ATTENTION_BACKEND):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.norm3 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.dropout3 = nn.Dropout(dropout)
        self.activation = _activation(activation)
        self.normalize_before = normalize_before
        self.backend = _check_backend(backend)

    def with_pos_embed(self, tensor, pos):
        return _add(tensor, pos)

    def _self_attention(self, x, tgt_mask, tgt_key_padding_mask, query_pos):
        qk = _add(x, query_pos)
        return attend(self.self_attn, qk, qk, x, tgt_key_padding_mask, tgt_mask, self.backend)

    def _cross_attention(self, x, memory, memory_mask, memory_key_padding_mask, pos, query_pos):
        return attend(self.multihead_attn, _add(x, query_pos), _add(memory, pos), memory, memory_key_padding_mask, memory_mask,
                      self.backend)

    def _feed_forward(self, x):
        return self.linear2(self.dropout(self.activation(self.linear1(x))))

    def forward_post(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None,
                     pos=None, query_pos=None):
        tgt = self.norm1(tgt + self.dropout1(self._self_attention(tgt, tgt_mask, tgt_key_padding_mask, query_pos)))
        tgt = self.norm2(tgt + self.dropout2(self._cross_attention(tgt, memory, memory_mask, memory_key_padding_mask, pos, query_pos)))
        return self.norm3(tgt + self.dropout3(self._feed_forward(tgt)))

    def forward_pre(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None,
                    pos=None, query_pos=None):
        tgt = tgt + self.dropout1(self._self_attention(self.norm1(tgt), tgt_mask, tgt_key_padding_mask, query_pos))
        tgt = tgt + self.dropout2(self._cross_attention(self.norm2(tgt), memory, memory_mask, memory_key_padding_mask, pos, query_pos))
        return tgt + self.dropout3(self._feed_forward(self.norm3(tgt)))

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None, pos=None,
                query_pos=None):
        step = self.forward_pre if self.normalize_before else self.forward_post
        return step(tgt, memory, tgt_mask, memory_mask, tgt_key_padding_mask, memory_key_padding_mask, pos, query_pos)


class TransformerEncoder(nn.Module):
    def __init__(self, encoder_layer, num_layers, norm=None):
        super().__init__()
        self.layers = _clones(encoder_layer, num_layers)
        self.num_layers = num_layers
        self.norm = norm

    def forward(self, src, mask=None, src_key_padding_mask=None, pos=None):
        for layer in self.layers:
            src = layer(src, src_mask=mask, src_key_padding_mask=src_key_padding_mask, pos=pos)
        return src if self.norm is None else self.norm(src)


class TransformerDecoder(nn.Module):
    def __init__(self, decoder_layer, num_layers, norm=None, return_intermediate=False):
        super().__init__()
        self.layers = _clones(decoder_layer, num_layers)
        self.num_layers = num_layers
        self.norm = norm
        self.return_intermediate = return_intermediate

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None, pos=None,
                query_pos=None):
        """(layers or 1, Q, B, E): every layer's normalised output with ``return_intermediate``, else the last one's."""
        outputs = []
        for layer in self.layers:
            tgt = layer(tgt, memory, tgt_mask=tgt_mask, memory_mask=memory_mask, tgt_key_padding_mask=tgt_key_padding_mask,
                        memory_key_padding_mask=memory_key_padding_mask, pos=pos, query_pos=query_pos)
            if self.return_intermediate:
                outputs.append(self.norm(tgt))          # the reference applies the norm without asking whether there is one
        if not self.return_intermediate:
            return (tgt if self.norm is None else self.norm(tgt)).unsqueeze(0)
        return torch.stack(outputs)


class Transformer(nn.Module):
    def __init__(self, d_model=512, nhead=8, encoder_layers=6, decoder_layers=6, dim_feedforward=2048, dropout=0.1, activation="relu",
                 normalize_before=False, return_intermediate_dec=False, backend=DEFAULT_ATTENTION_BACKEND, **kwargs):
        super().__init__()
        encoder_layer = TransformerEncoderLayer(d_model, nhead, dim_feedforward, dropout, activation, normalize_before, backend)
        self.encoder = TransformerEncoder(encoder_layer, encoder_layers, nn.LayerNorm(d_model) if normalize_before else None)
        decoder_layer = TransformerDecoderLayer(d_model, nhead, dim_feedforward, dropout, activation, normalize_before, backend)
        self.decoder = TransformerDecoder(decoder_layer, decoder_layers, nn.LayerNorm(d_model), return_intermediate=return_intermediate_dec)
        self._reset_parameters()
        self.d_model = d_model
        self.nhead = nhead
        self.backend = backend

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, src, mask, query_embed, pos_embed):
        """``src``, ``pos_embed`` (B,E,H,W), ``mask`` (B,H,W) bool with True = padding, ``query_embed`` (Q,E) ->
        (layers or 1, B, Q, E) decoder states and the (B,E,H,W) encoder memory."""
        bs, c, h, w = src.shape
        src = src.flatten(2).permute(2, 0, 1)
        pos_embed = pos_embed.flatten(2).permute(2, 0, 1)
        query_embed = query_embed.unsqueeze(1).repeat(1, bs, 1)
        mask = mask.flatten(1)
        memory = self.encoder(src, src_key_padding_mask=mask, pos=pos_embed)
        hs = self.decoder(torch.zeros_like(query_embed), memory, memory_key_padding_mask=mask, pos=pos_embed, query_pos=query_embed)
        return hs.transpose(1, 2), memory.permute(1, 2, 0).view(bs, c, h, w)
