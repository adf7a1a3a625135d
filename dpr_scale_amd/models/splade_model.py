"""SPLADE's encoder (reference: dpr_scale/models/citadel_models/splade_model.py:12-32): max over tokens of log(1 + relu(MLM logits)).
Same constructor kwargs and `forward(tokens) -> [B, V]`; the pooling is hotpath.router_head with no routing and no softmax (one HIP
launch forward, one backward; the reference's [B, T, V] product is never formed).  `model_path` as in citadel_model.py."""
from typing import Union

import torch.nn as nn

from ..hotpath import router_head
from .citadel_model import _mlm_backbone


class SPLADEEncoder(nn.Module):
    def __init__(self, model_path: Union[str, dict] = "roberta-base", dropout: float = 0.1):
        super().__init__()
        self.transformer, _ = _mlm_backbone(model_path, dropout)

    def forward(self, tokens):
        outputs = self.transformer(**tokens, return_dict=True)  # B x T x C
        return router_head(outputs.logits, tokens["attention_mask"], topk=0, skip_first=1, want_softmax=False)["router_repr"]
