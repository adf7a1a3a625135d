"""TEST-ONLY torch stand-in for HipKernels.ivf_compact / ivf_gather on CPU tensors (on top of the search stand-in of _ivf_standin.py),
so that the CPU suite can drive ivf.pack_queries_device, ivf.IndexBuilder and the writer drop-ins, and the reference the GPU suite
compares the kernels with.  Compaction is `mask.nonzero()` (row-major, i.e. (b, t, k) order); the gather is the rounding chain written
as explicit torch casts in the operands' own dtypes."""
import torch

from _ivf_standin import IvfKernels


class IvfPackKernels(IvfKernels):
    name = "ivf-pack-test-standin"

    def ivf_compact(self, expert_ids, weights, att, row_ids, test_weight, min_weight=0.0, capacity=None):
        B, L, K = expert_ids.shape
        keep = (att > 0).reshape(B, L, 1).expand(B, L, K)
        w32 = torch.ones((B, L, K), dtype=torch.float32) if weights is None else weights.to(torch.float32)
        if test_weight:
            keep = keep & (w32 > torch.tensor(float(min_weight), dtype=torch.float32))
        slot = keep.reshape(-1).nonzero().flatten()
        counts = keep.reshape(B, -1).sum(1)
        seq_off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)]).to(torch.int32)
        n = int(slot.shape[0])
        m = n if capacity is None else min(n, int(capacity))
        slot = slot[:m]
        b = slot // (L * K)
        return (n, int(counts.max()), seq_off, expert_ids.reshape(-1)[slot].to(torch.int32), row_ids.to(torch.int32)[b],
                slot.to(torch.int32), w32.reshape(-1)[slot])

    def ivf_gather(self, expert_repr, weights, slot, perm, K, entry_fp16, out_dtype, out_ld=None):
        d = expert_repr.shape[-1]
        x = expert_repr.reshape(-1, d)
        r = (slot if perm is None else slot[perm]).long()
        v = x[r // K]
        if weights is not None:
            # the host loops multiply ONE weight (a 0-dim tensor) with one row: the result has the row's dtype and torch casts the
            # weight to it first (test_rounding_chain_of_the_standin checks this against such products)
            prod = torch.result_type(weights.new_zeros(()), x)
            v = weights.to(prod).reshape(-1)[r].unsqueeze(1) * v
            assert v.dtype == prod
        if entry_fp16:
            v = v.to(torch.float16)
        v = v.to(torch.float32)
        out_ld = d if out_ld is None else out_ld
        if out_ld > d:
            v = torch.cat([v, torch.zeros((v.shape[0], out_ld - d))], 1)
        return v.to(out_dtype).contiguous()
