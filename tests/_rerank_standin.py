"""TEST-ONLY CPU stand-in for HipKernels.maxsim_score (next to maxsim_fwd / maxsim_bwd of tests/_multivec_standin.py), built on the
float64 oracle, so that the CPU suite can drive hotpath.expert_score_only / rerank_score and the drop-in rerank tasks."""
from _multivec_oracle import expert_sim_score as oracle_score
from _multivec_standin import MultiVecKernels


class RerankKernels(MultiVecKernels):
    name = "rerank-test-standin"

    def __init__(self):
        super().__init__()
        self.score_calls = []  # (Nq, Nc, M, pool) of every maxsim_score call

    def maxsim_score(self, Qb, Cb, qids, cids, qw, cw, KQ, KD, pool, M, m8):
        assert M >= 1 and Cb.shape[0] == Qb.shape[0] * M and Qb.shape[-1] % 32 == 0
        self.score_calls.append((Qb.shape[0], Cb.shape[0], M, pool))
        qr, cr = self._reprs(Qb, Cb, qids, cids, qw, cw, KQ, KD)
        mask = None if m8 is None else m8.bool()
        return oracle_score(qr, cr, mask, True, ("sum", "max")[pool]).float()

    def maxsim_fwd(self, *a, **k):
        raise AssertionError("the score-only path must not build the training tables")
