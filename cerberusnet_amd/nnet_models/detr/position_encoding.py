"""Positional encodings of the DETR head (the reference's nnet_models/detr/position_encoding.py), in stock ops.  Both take the plain
(B,C,H,W) feature tensor the head passes and return (B, 2 num_pos_feats, H, W); there is no padding mask (every pixel is valid)."""
import math

import torch
from torch import nn

__all__ = ["PositionEmbeddingSine", "PositionEmbeddingLearned", "build_position_encoding"]


class PositionEmbeddingSine(nn.Module):
    """Sine / cosine of the 1-based row and column index at ``num_pos_feats`` wavelengths each: channels [rows | columns]."""

    def __init__(self, num_pos_feats=64, temperature=10000, normalize=False, scale=None):
        super().__init__()
        if scale is not None and normalize is False:
            raise ValueError("normalize should be True if scale is passed")
        self.num_pos_feats = num_pos_feats
        self.temperature = temperature
        self.normalize = normalize
        self.scale = 2 * math.pi if scale is None else scale

    def forward(self, features):
        b, _, h, w = features.shape
        valid = torch.ones((b, h, w), dtype=torch.bool, device=features.device)
        y_embed = valid.cumsum(1, dtype=torch.float32)
        x_embed = valid.cumsum(2, dtype=torch.float32)
        if self.normalize:
            eps = 1e-6
            y_embed = y_embed / (y_embed[:, -1:, :] + eps) * self.scale
            x_embed = x_embed / (x_embed[:, :, -1:] + eps) * self.scale
        dim_t = torch.arange(self.num_pos_feats, dtype=torch.float32, device=features.device)
        dim_t = self.temperature ** (2 * (dim_t // 2) / self.num_pos_feats)

        def waves(embed):
            phase = embed[:, :, :, None] / dim_t
            return torch.stack((phase[:, :, :, 0::2].sin(), phase[:, :, :, 1::2].cos()), dim=4).flatten(3)

        return torch.cat((waves(y_embed), waves(x_embed)), dim=3).permute(0, 3, 1, 2)


class PositionEmbeddingLearned(nn.Module):
    """A learned embedding per column and per row (up to 50 each): channels [columns | rows]."""

    def __init__(self, num_pos_feats=256):
        super().__init__()
        self.row_embed = nn.Embedding(50, num_pos_feats)
        self.col_embed = nn.Embedding(50, num_pos_feats)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.uniform_(self.row_embed.weight)
        nn.init.uniform_(self.col_embed.weight)

    def forward(self, features):
        h, w = features.shape[-2:]
        x_emb = self.col_embed(torch.arange(w, device=features.device))
        y_emb = self.row_embed(torch.arange(h, device=features.device))
        pos = torch.cat([x_emb.unsqueeze(0).repeat(h, 1, 1), y_emb.unsqueeze(1).repeat(1, w, 1)], dim=-1)
        return pos.permute(2, 0, 1).unsqueeze(0).repeat(features.shape[0], 1, 1, 1)


def build_position_encoding(**kwargs):
    """``type`` 'v2' / 'sine' or 'v3' / 'learned', ``hidden_dim`` channels in all; other keys are ignored."""
    n_steps = kwargs["hidden_dim"] // 2
    if kwargs["type"] in ("v2", "sine"):
        return PositionEmbeddingSine(n_steps, normalize=True)
    if kwargs["type"] in ("v3", "learned"):
        return PositionEmbeddingLearned(n_steps)
    raise ValueError("not supported %s" % kwargs["type"])
