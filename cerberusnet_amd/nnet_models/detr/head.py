"""The DETR detection head (the reference's ``DetrSegmHead`` of nnet_models/detr_sfd.py and ``MLP`` of nnet_models/detr/detr.py):
a 1x1 projection of the backbone's map, the transformer of transformer.py over its pixels, a class and a box predictor per object
query.  Constructor arguments, ``forward`` signature and ``state_dict`` keys are the reference's; ``backend`` selects the fused
attention core ('hip') or ``nn.MultiheadAttention`` as the reference calls it ('torch')."""
import torch
import torch.nn.functional as F
from torch import nn

from .position_encoding import build_position_encoding
from .transformer import DEFAULT_ATTENTION_BACKEND, Transformer


class MLP(nn.Module):
    """``num_layers`` linear layers with a ReLU between them."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        dims = [input_dim] + [hidden_dim] * (num_layers - 1) + [output_dim]
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip(dims[:-1], dims[1:]))

    def forward(self, x):
        for layer in self.layers[:-1]:
            x = F.relu(layer(x))
        return self.layers[-1](x)


class DetrSegmHead(nn.Module):
    """``forward(features)`` with features (B,num_channels,H,W) returns 'logits' (B,Q,num_classes+1) and 'bboxes' (B,Q,4) in [0,1]
    (cx, cy, w, h).  With ``aux_loss`` (and ``return_intermediate_dec=True`` in ``transformer_config``) the earlier decoder layers'
    predictions come too: as 'aux_outputs', a list of {'logits','bboxes'} dicts (what ``DetrLoss`` reads), and the same tensors
    under the reference's name 'detr_aux' with its inner keys 'pred_logits' / 'pred_boxes'.

    ``position_embedding_config`` needs 'type'; ``transformer_config`` needs 'hidden_dim' (the position encoding's width) beside the
    transformer's own arguments, which ignores the keys it does not know."""

    def __init__(self, num_channels, num_classes, num_queries, position_embedding_config, transformer_config, aux_loss=False,
                 seg_enable=False, backend=DEFAULT_ATTENTION_BACKEND):
        super().__init__()
        if seg_enable:
            raise NotImplementedError("DetrSegmHead(seg_enable=True): the mask head (MHAttentionMap, MaskHeadSmallConv) is not part of this package")
        self.pos_embed = build_position_encoding(**position_embedding_config, **transformer_config)
        self.transformer = Transformer(**dict(transformer_config, backend=backend))
        hidden_dim = self.transformer.d_model
        self.class_embed = nn.Linear(hidden_dim, num_classes + 1)
        self.bbox_embed = MLP(hidden_dim, hidden_dim, 4, 3)
        self.query_embed = nn.Embedding(num_queries, hidden_dim)
        self.input_proj = nn.Conv2d(num_channels, hidden_dim, kernel_size=1)
        self.aux_loss = aux_loss
        self.backend = backend

    def forward(self, features):
        b, _, h, w = features.shape
        mask = torch.zeros((b, h, w), dtype=torch.bool, device=features.device)         # no pixel is padding
        pos = self.pos_embed(features)
        hs, _memory = self.transformer(self.input_proj(features), mask, self.query_embed.weight, pos)
        logits = self.class_embed(hs)
        boxes = self.bbox_embed(hs).sigmoid()
        out = {"logits": logits[-1], "bboxes": boxes[-1]}
        if self.aux_loss:
            layers = list(zip(logits[:-1], boxes[:-1]))
            out["aux_outputs"] = [{"logits": a, "bboxes": c} for a, c in layers]
            out["detr_aux"] = [{"pred_logits": a, "pred_boxes": c} for a, c in layers]
        return out
