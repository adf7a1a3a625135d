"""ColBERT's encoder (reference: dpr_scale/models/citadel_models/colbert_model.py): one vector per token behind the first position,
no routing and no CLS vector.  Same constructor kwargs, same `forward(tokens, **kwargs)`, same key and shape in the returned dict, same
sub-module names (`transformer`, `project`: they are checkpoint keys).  The transformer and the projection stay on PyTorch-ROCm; the
token vectors are scored by the MaxSim kernels (hotpath.expert_sim_score in training, dpr_scale_amd.colbert in retrieval).

`model_path`: a directory / hub id (AutoModel.from_pretrained, as the reference), or a dict of BertConfig fields for a random-init model
of that architecture (what the tests use: nothing is downloaded).
"""
from typing import Optional, Union

import torch.nn as nn

from .hf_model import _backbone


class ColBERTEncoder(nn.Module):
    def __init__(self, model_path: Union[str, dict] = "roberta-base", dropout: float = 0.1, projection_dim: Optional[int] = None):
        super().__init__()
        self.transformer, cfg = _backbone(model_path, dropout)
        width = cfg.hidden_size if projection_dim == -1 else projection_dim
        self.project = nn.Identity()
        if width:
            dense = nn.Linear(cfg.hidden_size, width)
            nn.init.normal_(dense.weight, mean=0.0, std=0.02)
            self.project = nn.Sequential(dense)

    def forward(self, tokens, **kwargs):
        """{"expert_repr": [B, T - 1, width]}: the projected last hidden states of positions 1 .. T - 1, zero at padded positions."""
        last = self.transformer(**tokens, output_hidden_states=True, return_dict=True).hidden_states[-1]
        keep = tokens["attention_mask"][:, 1:].unsqueeze(-1)
        return {"expert_repr": (keep * self.project(last[:, 1:, :])).clone()}
