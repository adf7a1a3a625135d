"""The fp32 pairwise stream kernels (pairwise_fwd_kernel / pairwise_bwd_kernel, csrc/rowwise.h) on the MI355X, through
hotpath.pairwise_score and through kernels.pairwise_fwd / pairwise_bwd, against float64.

Grid inputs (q, c multiples of 1/4 in [-1, 1], g multiples of 1/8 in [-2, 2]) make every product and every partial sum exact in fp32
(|S| <= d in units of 1/16: 30522 * 16 < 2^24; |dq| <= 2 M in units of 1/32), so S, dq and dc must equal float64 bit for bit in any
summation order.  Gaussian inputs get element-wise bounds derived from the arithmetic (one rounding per fused multiply-add)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DIMS = [1, 2, 3, 255, 256, 511, 512, 513, 1024, 1025, 30522]  # odd d (scalar path), d < 512, the 512-column slab edge, vocabulary width
U = 2.0**-24


def _gamma(n):
    return n * U / (1 - n * U)


def _grid(seed, B, M, d):
    g = np.random.default_rng(seed)
    q = torch.from_numpy((g.integers(-4, 5, size=(B, d)) / 4.0).astype(np.float32))
    c = torch.from_numpy((g.integers(-4, 5, size=(B * M, d)) / 4.0).astype(np.float32))
    gr = torch.from_numpy((g.integers(-16, 17, size=(B, M)) / 8.0).astype(np.float32))
    return q, c, gr


def _mask(seed, B, M):
    """[B, M] bool with at least one masked pair (and, when there is more than one pair, at least one live one)."""
    m = torch.from_numpy(np.random.default_rng(seed).random((B, M)) < 0.4)
    m.view(-1)[(seed * 7) % (B * M)] = True
    if B * M > 1:
        m.view(-1)[(seed * 7 + 1) % (B * M)] = False
    return m


def _ref(q, c, g, mask):
    """float64: S [B, M] (-inf at masked pairs), dq, dc for upstream g (no gradient through masked pairs)."""
    B, d = q.shape
    M = c.shape[0] // B
    qd, cd, gd = q.double(), c.double().view(B, M, d), g.double()
    S = torch.einsum("bk,bmk->bm", qd, cd)
    if mask is not None:
        S = S.masked_fill(mask, float("-inf"))
        gd = gd.masked_fill(mask, 0.0)
    return S, torch.einsum("bm,bmk->bk", gd, cd), (gd[:, :, None] * qd[:, None, :]).reshape(B * M, d)


def _score(q, c, g, mask):
    """hotpath.pairwise_score forward + backward on the device; (S, dq, dc) on the CPU."""
    from dpr_scale_amd import hotpath

    tq, tc = q.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
    S = hotpath.pairwise_score(tq, tc, None if mask is None else mask.to(DEV))
    fin = torch.isfinite(S)
    (S.masked_fill(~fin, 0.0) * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return S.detach().cpu(), tq.grad.cpu(), tc.grad.cpu()


def _exact(name, got, ref):
    ref32 = ref.float()
    assert torch.equal(ref32.double(), ref), f"{name}: the reference is not an fp32 number (the case is not exact)"
    if not torch.equal(got, ref32):
        bad = (got != ref32).nonzero()
        at = tuple(bad[0].tolist())
        raise AssertionError(f"{name}: {bad.shape[0]} of {got.numel()} elements differ, first at {at}: got {got[at].item()!r}, expected "
                             f"{ref32[at].item()!r}; differing indices span {bad.min(0).values.tolist()} .. {bad.max(0).values.tolist()}")


@pytest.mark.parametrize("d", DIMS)
def test_grid_inputs_are_exact(d):
    from dpr_scale_amd import hotpath

    kn = hotpath.default_kernels()
    for B in (1, 3):
        for M in (1, 2, 5):
            for masked in (False, True):
                tag = f"d={d} B={B} M={M} masked={masked}"
                q, c, g = _grid(d * 31 + B * 7 + M, B, M, d)
                mask = _mask(d + B + M, B, M) if masked else None
                S0, dq0, dc0 = _ref(q, c, g, mask)
                S, dq, dc = _score(q, c, g, mask)
                _exact("S " + tag, S, S0)
                _exact("dq " + tag, dq, dq0)
                _exact("dc " + tag, dc, dc0)
                if masked:
                    assert bool((S[mask] == float("-inf")).all()) and bool(torch.isfinite(S[~mask]).all()), tag
                    rows = mask.view(-1)
                    assert torch.equal(dc[rows], torch.zeros_like(dc[rows])), tag  # (-0.0 counts as 0)
                # the kernels object directly, and its gradient subsets (dq == nullptr, dc == nullptr)
                tq, tc = q.to(DEV), c.to(DEV)
                m8 = None if mask is None else mask.to(DEV, torch.uint8).view(-1).contiguous()
                gz = (g if mask is None else g.masked_fill(mask, 0.0)).to(DEV).contiguous()  # the caller zeroes masked pairs
                _exact("fwd " + tag, kn.pairwise_fwd(tq, tc, m8).cpu(), S0)
                both = kn.pairwise_bwd(gz, tq, tc)
                only_q = kn.pairwise_bwd(gz, tq, tc, need_dq=True, need_dc=False)
                only_c = kn.pairwise_bwd(gz, tq, tc, need_dq=False, need_dc=True)
                torch.cuda.synchronize()
                assert only_q[1] is None and only_c[0] is None, tag
                assert torch.equal(only_q[0], both[0]) and torch.equal(only_c[1], both[1]), tag
                _exact("bwd dq " + tag, both[0].cpu(), dq0)
                _exact("bwd dc " + tag, both[1].cpu(), dc0)


@pytest.mark.parametrize("d", [3, 512, 1025])
def test_masked_dummy_rows_take_no_part(d):
    """A masked context row full of inf and NaN: its score is -inf, dq is finite and what it is without that row, its dc is 0."""
    B, M = 2, 3
    q, c, g = _grid(d, B, M, d)
    mask = torch.zeros(B, M, dtype=torch.bool)
    mask[0, 1] = mask[1, 2] = True
    c[1] = float("inf")
    c[1, ::2] = float("nan")
    c[5, : d // 2 + 1] = float("-inf")
    c[5, d // 2 + 1:] = float("nan")
    S, dq, dc = _score(q, c, g, mask)
    clean = c.clone()
    clean[mask.view(-1)] = 0.0  # the oracle never sees the dummy rows
    S0, dq0, dc0 = _ref(q, clean, g, mask)
    _exact("S", S, S0)
    assert bool(torch.isfinite(dq).all())
    _exact("dq", dq, dq0)
    _exact("dc", dc, dc0)
    assert torch.equal(dc[mask.view(-1)], torch.zeros(2, d))


@pytest.mark.parametrize("d", [513, 30522])
def test_gaussian_inputs_within_derived_bounds(d):
    """u = 2^-24, gamma(n) = n u / (1 - n u).  S: at most d roundings on any path (the products inside the fused multiply-adds are
    not rounded), in any order: |S - ref| <= gamma(d) sum_k |q_k c_k|.  dq: M fused multiply-adds: gamma(M) sum_j |g_j c_jk|.
    dc: one rounded product: u |g q|."""
    B, M = 3, 5
    gen = torch.Generator().manual_seed(d)
    q, c, g = torch.randn(B, d, generator=gen), torch.randn(B * M, d, generator=gen), torch.randn(B, M, generator=gen)
    mask = _mask(d, B, M)
    for m in (None, mask):
        S0, dq0, dc0 = _ref(q, c, g, m)
        S, dq, dc = _score(q, c, g, m)
        qd, cd, gd = q.double(), c.double().view(B, M, d), g.double()
        if m is not None:
            gd = gd.masked_fill(m, 0.0)
        fin = torch.isfinite(S0)
        assert torch.equal(torch.isfinite(S), fin) and bool((S[~fin] == float("-inf")).all())
        bS = _gamma(d) * torch.einsum("bk,bmk->bm", qd.abs(), cd.abs())
        bq = _gamma(M) * torch.einsum("bm,bmk->bk", gd.abs(), cd.abs())
        bc = U * (gd[:, :, None] * qd[:, None, :]).abs().reshape(B * M, d)
        eS, eq, ec = (S.double() - S0)[fin].abs(), (dq.double() - dq0).abs(), (dc.double() - dc0).abs()
        print(f"d={d} masked={m is not None}: max err/bound S {float((eS / bS[fin]).max()):.3g} dq {float((eq / bq.clamp_min(1e-300)).max()):.3g} "
              f"dc {float((ec / bc.clamp_min(1e-300)).max()):.3g}")
        assert bool((eS <= bS[fin]).all()) and bool((eq <= bq).all()) and bool((ec <= bc).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_inputs_score_as_their_widened_values(dtype):
    from dpr_scale_amd import hotpath

    B, M, d = 3, 2, 1025
    gen = torch.Generator().manual_seed(9)
    q, c = torch.randn(B, d, generator=gen).to(dtype).to(DEV), torch.randn(B * M, d, generator=gen).to(dtype).to(DEV)
    mask = _mask(4, B, M).to(DEV)
    S = hotpath.pairwise_score(q, c, mask)
    S32 = hotpath.pairwise_score(q.float(), c.float(), mask)
    assert S.dtype == torch.float32 and torch.equal(S, S32) and bool(torch.isfinite(S).any())


def test_noncontiguous_query_gives_the_same_bits():
    from dpr_scale_amd import hotpath

    B, M, d = 3, 2, 513
    gen = torch.Generator().manual_seed(10)
    wide, c, g = torch.randn(B, 2 * d, generator=gen), torch.randn(B * M, d, generator=gen), torch.randn(B, M, generator=gen)
    out = []
    for contiguous in (False, True):
        tq = wide.to(DEV)[:, ::2]
        tq = (tq.contiguous() if contiguous else tq).requires_grad_(True)
        assert tq.is_contiguous() == contiguous
        tc = c.to(DEV).requires_grad_(True)
        S = hotpath.pairwise_score(tq, tc)
        (S * g.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        out.append((S.detach().cpu(), tq.grad.cpu(), tc.grad.cpu()))
    for x, y in zip(*out):
        assert torch.equal(x, y)
