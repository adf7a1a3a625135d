"""TEST-ONLY CPU stand-in for HipKernels.maxsim_fwd / maxsim_bwd, built on the float64 oracle, so that the CPU suite can drive the
orchestration of hotpath.expert_sim_score and the drop-in MultiVecRetrieverTask (the pattern of tests/_oracle_kernels.py)."""
import torch

from _multivec_oracle import expert_sim_score as oracle_score
from _oracle_kernels import OracleKernels


class MultiVecKernels(OracleKernels):
    name = "multivec-test-standin"

    @staticmethod
    def _reprs(Qb, Cb, qids, cids, qw, cw, KQ, KD, grad=False):
        q, c = Qb.double(), Cb.double()
        if grad:
            q.requires_grad_(True)
            c.requires_grad_(True)
        qr, cr = {"expert_repr": q}, {"expert_repr": c}
        if qids is not None:
            Nq, LQ, Nc, LD = Qb.shape[0], Qb.shape[1], Cb.shape[0], Cb.shape[1]
            qr["expert_ids"], cr["expert_ids"] = qids.long().view(Nq, LQ, KQ), cids.long().view(Nc, LD, KD)
            if qw is not None:
                a, b = qw.double().view(Nq, LQ, KQ), cw.double().view(Nc, LD, KD)
                if grad:
                    a.requires_grad_(True)
                    b.requires_grad_(True)
                qr["expert_weights"], cr["expert_weights"] = a, b
        return qr, cr

    def maxsim_fwd(self, Qb, Cb, qids, cids, qw, cw, KQ, KD, pool, M, m8):
        qr, cr = self._reprs(Qb, Cb, qids, cids, qw, cw, KQ, KD)
        mask = None if m8 is None else m8.bool()
        S = oracle_score(qr, cr, mask, M > 0, ("sum", "max")[pool]).float()
        return S, torch.zeros(1)

    def maxsim_bwd(self, dS, Qb, Cb, qids, cids, qw, cw, KQ, KD, pool, M, m8, state, need_dq=True, need_dc=True, need_dw=False):
        with torch.enable_grad():  # (called from inside an autograd backward)
            qr, cr = self._reprs(Qb, Cb, qids, cids, qw, cw, KQ, KD, grad=True)
            mask = None if m8 is None else m8.bool()
            S = oracle_score(qr, cr, mask, M > 0, ("sum", "max")[pool])
            fin = torch.isfinite(S)
            (S.masked_fill(~fin, 0.0) * dS.double().masked_fill(~fin, 0.0)).sum().backward()
        f = lambda t: None if t is None else t.float()
        dw = qw is not None and need_dw
        return (f(qr["expert_repr"].grad) if need_dq else None, f(cr["expert_repr"].grad) if need_dc else None,
                f(qr["expert_weights"].grad) if dw else None, f(cr["expert_weights"].grad) if dw else None)
