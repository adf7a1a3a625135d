"""CITADEL's encoder (reference: dpr_scale/models/citadel_models/citadel_model.py:12-82): a masked-LM transformer whose logits route
every token to its top-k vocabulary "experts".  Same constructor kwargs, same `forward(tokens, topk=1, add_cls=False)`, same keys and
shapes in the returned dict, same sub-module names (`transformer`, `tok_project`, `cls_project`: they are checkpoint keys).  The
transformer and the two projections stay on PyTorch-ROCm; everything the reference derives from the logits (:55-73, four [B, T, V]
tensors there) is hotpath.router_head -- HIP kernels that stream the logits once more forward and once backward and keep only
[B, V] / [B, T, k] results.  There is no CPU fallback: logits on the CPU raise.

`model_path`: a directory / hub id (AutoModelForMaskedLM.from_pretrained, as the reference), or a dict of BertConfig fields for a
random-init model of that architecture (what the tests use: nothing is downloaded).
"""
from typing import Optional, Union

import torch.nn as nn

from ..hotpath import router_head
from .hf_model import _with_dropout


def _mlm_backbone(model_path, dropout, **extra):
    import transformers as tf

    if isinstance(model_path, dict):  # architecture only: random weights
        config = _with_dropout(tf.BertConfig(**model_path), dropout)
        for k, v in extra.items():
            setattr(config, k, v)
        return tf.AutoModelForMaskedLM.from_config(config), config
    config = _with_dropout(tf.AutoConfig.from_pretrained(model_path), dropout)
    for k, v in extra.items():
        setattr(config, k, v)
    return tf.AutoModelForMaskedLM.from_pretrained(model_path, config=config), config


def _projection(hidden_size, dim):
    """citadel_model.py:30-44: Identity, or Sequential(Linear) with N(0, 0.02) weights."""
    if not dim:
        return nn.Identity()
    linear = nn.Linear(hidden_size, dim)
    linear.weight.data.normal_(mean=0.0, std=0.02)
    return nn.Sequential(linear)


class CITADELEncoder(nn.Module):
    def __init__(
        self,
        model_path: Union[str, dict] = "bert-base-uncased",
        dropout: float = 0.1,
        tok_projection_dim: Optional[int] = None,
        cls_projection_dim: Optional[int] = None,
    ):
        super().__init__()
        self.transformer, cfg = _mlm_backbone(model_path, dropout, output_hidden_states=True, tok_projection_dim=tok_projection_dim)
        self.cls_project = _projection(cfg.hidden_size, cls_projection_dim)
        self.tok_project = _projection(cfg.hidden_size, tok_projection_dim)

    def forward(self, tokens, topk=1, add_cls=False):
        outputs = self.transformer(**tokens, return_dict=True)
        last = outputs.hidden_states[-1]
        attention_mask = tokens["attention_mask"][:, 1:]
        # :52-73 -- the [:, 1:, :] slice is the head's skip_first = 1: the logits are read in place
        ret = router_head(outputs.logits, tokens["attention_mask"], topk=topk, skip_first=1, want_softmax=True)
        ret["attention_mask"] = attention_mask.clone()
        if add_cls:
            ret["cls_repr"] = self.cls_project(last[:, 0, :]).clone()
        ret["expert_repr"] = (self.tok_project(last[:, 1:, :]) * attention_mask.unsqueeze(-1)).clone()
        return ret
