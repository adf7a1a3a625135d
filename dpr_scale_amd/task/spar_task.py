"""Drop-in for dpr_scale/task/spar_task.py: a task that holds a dense retriever and a lexical model Lambda, both restored from their own
checkpoints (saved with hyperparameters), and embeds a text with both -- [dense | lexical], the query's lexical half scaled by
`lexical_weight`.  Torch only: nothing here is a hot path.  dpr_scale_amd/spar.py searches the two halves as two indexes and applies
the weight to the fp32 partial score instead; encode with lexical_weight = 1 (or split the vector at the dense width) to feed it."""
import torch

from .dpr_task import DenseRetrieverTask


class SalientPhraseAwareDenseRetrieverTask(DenseRetrieverTask):
    def __init__(
        self,
        pretrained_checkpoint_path: str = "",
        lexical_model_checkpoint_path: str = "",
        lexical_weight: float = 0,
        **kwargs,
    ):
        super().__init__(**kwargs)
        self.pretrained_checkpoint_path = pretrained_checkpoint_path
        self.lexical_model_checkpoint_path = lexical_model_checkpoint_path
        self.lexical_weight = lexical_weight

    def setup(self, stage: str):
        if stage == "test" and self.setup_done:
            return  # keep the restored models
        # each model is a whole DenseRetrieverTask restored from its own checkpoint (saved with hyperparameters); Lambda first, as the
        # reference loads them
        for name, path in (("lexical_model", self.lexical_model_checkpoint_path), ("dense_model", self.pretrained_checkpoint_path)):
            setattr(self, name, DenseRetrieverTask.load_from_checkpoint(path, map_location=self.device))
        self.setup_done = True

    def encode_queries(self, query_ids):
        dense = self._encode_sequence(query_ids, self.dense_model.query_encoder)  # bs x d1
        lexical = self.dense_model._encode_sequence(query_ids, self.lexical_model.query_encoder)  # bs x d2
        return torch.cat([dense, lexical * self.lexical_weight], dim=-1)

    def encode_contexts(self, contexts_ids):
        dense = self._encode_sequence(contexts_ids, self.dense_model.context_encoder)  # ctx_cnt x d1
        lexical = self._encode_sequence(contexts_ids, self.lexical_model.context_encoder)  # the weight is applied to the queries only
        return torch.cat([dense, lexical], dim=-1)
