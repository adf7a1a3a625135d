"""Capture and side-stream conformance on the MI355X.

Part A: every row of tests/_capture_cases.py -- every entry point of include/dprhot.h that takes a stream, the RCCL collectives
excepted -- is run eagerly on the default stream (ref_A, ref_B), then on ONE side stream, then captured there into a HIP graph and
replayed on input set B and again over a scribbled workspace.  The header's promise is what is tested: a call only enqueues on
`stream`, does not synchronise, and may be captured after one eager call at the same shape.

Part B: the autograd operator (the C++ node and the Python node) inside a whole-step graph, forward + backward, replayed on other
inputs and other grad_output scales, and replayed once more after the caches that fed it addresses (the expected-grad-scale scalar, the
step workspace) have been replaced and the freed memory has been handed to somebody else.

Everything is linear on one side stream: no fork, no second capture stream, no environment variable.  Equality is torch.equal on the
int32 / int16 / int8 view of every output, so NaN cells compare as bits; there is no tolerance.  The references are eager calls of code
paths the conformance suites hold to their oracles.  No test calls torch.cuda.empty_cache()."""
import gc
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import _capture_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = CC.DEV
REPLAYED = {}  # case name -> the symbols its fn() called while it was captured


FAULTS = ("illegal memory access", "unspecified launch failure", "hardware exception", "memory access fault")


def ends_the_session_on_a_device_fault(test):
    """A faulted device takes no more work: should a call here ever report a device fault, the session ends instead of going on to launch
    the remaining rows on it.  (A mismatch, a refused capture or a library status is an ordinary failure; the other rows still run.)"""
    import functools

    @functools.wraps(test)
    def run(*args, **kwargs):
        try:
            return test(*args, **kwargs)
        except RuntimeError as e:
            if any(f in str(e) for f in FAULTS):
                pytest.exit(f"device fault in {test.__name__}{args}{kwargs}: {e}", returncode=3)
            raise
    return run


def bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.int8, 2: torch.int16}.get(t.element_size(), torch.int32))


def _flat(outs):
    return [t for t in (outs or ()) if t is not None]


def _fill(tensors, byte):
    for t in tensors:
        if t.numel():
            t.view(torch.uint8).fill_(byte)


def _same(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, j)
        assert torch.equal(bits(g), bits(w)), f"{what}: output {j} {tuple(g.shape)} {g.dtype} differs in {int((bits(g) != bits(w)).sum())} words"


def helper(case):
    kn, L, _ = CC.kernels()
    built = case.build()
    x = [a.clone() for a in built.A]
    ws_of = built.ws if callable(built.ws) else (lambda: built.ws)

    def run(src, ws_byte=CC.SENTINEL):
        for t, s in zip(x, src):
            t.copy_(s)
        _fill(built.outs, CC.SENTINEL)
        _fill(ws_of(), ws_byte)
        return built.outs + _flat(built.fn(x))

    # 1. eager, default stream
    ref_A = [t.clone() for t in run(built.A)]
    ref_B = [t.clone() for t in run(built.B)]
    torch.cuda.synchronize()
    # 2. eager, the side stream: all lazy initialisation happens here
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run(built.A)
    torch.cuda.synchronize()
    _same(got, ref_A, f"{case.name}: side stream")
    del got
    # 3. capture: nothing runs
    with torch.cuda.stream(side):
        for t, s in zip(x, built.A):
            t.copy_(s)
        _fill(built.outs, CC.SENTINEL)
        _fill(ws_of(), CC.SENTINEL)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    L.called.clear()
    try:
        with torch.cuda.graph(g, stream=side):
            fresh = _flat(built.fn(x))
    except Exception:
        torch.cuda.synchronize()  # a refused capture: the library's error string is in the exception; nothing more runs on this graph
        raise
    torch.cuda.synchronize()
    REPLAYED[case.name] = set(L.called)
    for j, t in enumerate(built.outs):
        assert bool((t.view(torch.uint8) == CC.SENTINEL).all()), f"{case.name}: output {j} was written while capturing"
    # 4. replay on B; 5. replay on B over a scribbled workspace
    for ws_byte in (CC.SENTINEL, CC.SCRIBBLE):
        with torch.cuda.stream(side):
            for t, s in zip(x, built.B):
                t.copy_(s)
            _fill(built.outs + fresh, CC.SENTINEL)
            _fill(ws_of(), ws_byte)
            g.replay()
        torch.cuda.synchronize()
        _same(built.outs + fresh, ref_B, f"{case.name}: replay on B, workspace filled with {ws_byte:#x}")
        if built.after is not None:
            built.after()
    print(f"[capture] {case.name}: replayed {' '.join(sorted(REPLAYED[case.name]))}")
    del g, fresh  # 6.


@pytest.mark.parametrize("case", CC.CASES, ids=[c.name for c in CC.CASES])
@ends_the_session_on_a_device_fault
def test_side_stream_and_replay_equal_the_eager_call(case):
    helper(case)


# ---- B. the operator inside a whole-step graph ------------------------------------------------------------------------------------------
NODES = ("cpp", "py")
SCALES = (1.0, 8.0, 0.5)  # powers of two: the rescale by go / used is exact whatever `used` was


def _operator(node):
    from dpr_scale_amd import hotpath

    if node == "cpp":
        assert hotpath._OPX_NODE, "the C++ autograd node (csrc/opx.cpp) was not built"
        return lambda q, c, y, m, T: hotpath.inbatch_contrastive_loss(q, c, y, m, T)
    kn = hotpath.HipKernels()
    return lambda q, c, y, m, T: hotpath.InBatchContrastive.apply(q, c, y, m, T, False, kn, None, None)


def _op_sets(shape):
    """Three input sets (q, c, y, mask bool, scale): other labels and masks, grad_output scales 1, 8 and 0.5."""
    sets = []
    for j, s in enumerate(SCALES):
        q, c, y, m = CC._step_data(shape, 100 + j)
        sets.append((q, c, y, m.bool(), torch.tensor([s], device=DEV)))
    return sets


def _eager(op, data):
    """(loss, q.grad, c.grad) of one eager step on the default stream, fresh leaves."""
    q, c, y, m, scale = data
    q, c = q.clone().requires_grad_(True), c.clone().requires_grad_(True)
    loss = op(q, c, y, m, 1.0 / CC.INV_T)
    loss.backward(gradient=scale[0])
    torch.cuda.synchronize()
    return [loss.detach().clone(), q.grad.clone(), c.grad.clone()]


class _Captured:
    """A whole step -- loss = op(...); loss.backward(gradient=scale[0]) -- captured on a side stream after three warm-up iterations."""

    def __init__(self, op, first):
        self.static = [t.clone() for t in first]
        self.q, self.c, self.y, self.m, self.scale = self.static
        self.q.requires_grad_(True)
        self.c.requires_grad_(True)
        self.side = torch.cuda.Stream()
        self.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            for _ in range(3):
                op(self.q, self.c, self.y, self.m, 1.0 / CC.INV_T).backward(gradient=self.scale[0])
        torch.cuda.synchronize()
        self.q.grad = self.c.grad = None
        self.graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(self.graph, stream=self.side):
                self.loss = op(self.q, self.c, self.y, self.m, 1.0 / CC.INV_T)
                self.loss.backward(gradient=self.scale[0])
        except Exception:
            torch.cuda.synchronize()
            raise
        torch.cuda.synchronize()

    def replay(self, data):
        with torch.cuda.stream(self.side), torch.no_grad():
            for t, s in zip(self.static, data):
                t.copy_(s)
            self.graph.replay()
        torch.cuda.synchronize()
        return [self.loss.detach(), self.q.grad, self.c.grad]


@pytest.mark.parametrize("shape", [CC.SMALL, CC.FEW], ids=CC._tag)
@pytest.mark.parametrize("node", NODES)
@ends_the_session_on_a_device_fault
def test_whole_step_graph_replays_equal_the_eager_step(node, shape):
    op = _operator(node)
    sets = _op_sets(shape)
    cap = _Captured(op, sets[0])
    for j in (1, 2, 0):
        _same(cap.replay(sets[j]), _eager(op, sets[j]), f"{node} node {shape}: replay of set {j} (scale {SCALES[j]})")
    del cap


def _larger_shape(cached_bytes):
    """The smallest general-family shape (64, 512 k, 64) whose step workspace exceeds the cached buffer."""
    from dpr_scale_amd import _lib

    return next(s for s in ((64, 512 * k, 64) for k in range(1, 129)) if _lib.workspace_bytes(*s) > cached_bytes)


@pytest.mark.parametrize("node", NODES)
@ends_the_session_on_a_device_fault
def test_replay_after_the_caches_moved_on_scribbles_on_nobody(node):
    """After the capture the side stream's caches are replaced -- an eager step of a shape that needs a larger workspace, eager steps
    that publish new expected-grad-scale scalars -- and memory of the old sizes is handed to this test, filled with patterns.  The graph
    still owns what it was given: its replay equals the eager step bit for bit and every pattern byte is unchanged."""
    from dpr_scale_amd import _lib

    op = _operator(node)
    shape = CC.SMALL
    sets = _op_sets(shape)
    cap = _Captured(op, sets[0])
    gc.collect()
    old_bytes = max(_lib.workspace_bytes(*shape), 1 << 20)  # hotpath.py and csrc/opx.cpp floor the cached workspace at 1 MiB
    big = _larger_shape(old_bytes)
    with torch.cuda.stream(cap.side):
        zeros = [torch.zeros(1, dtype=torch.float32, device=DEV) for _ in range(4096)]
        for data in (_op_sets(big)[1], sets[1]):  # a larger workspace; a new scalar for the captured step's own site
            q, c, y, m, scale = data
            q, c = q.clone().requires_grad_(True), c.clone().requires_grad_(True)
            op(q, c, y, m, 1.0 / CC.INV_T).backward(gradient=scale[0])
        held = [torch.full((old_bytes,), 0x5A, dtype=torch.uint8, device=DEV) for _ in range(8)]
    torch.cuda.synchronize()
    got = cap.replay(sets[2])
    _same(got, _eager(op, sets[2]), f"{node} node: replay after the caches moved on")
    assert not bool(torch.cat(zeros).any()), "a replay wrote into memory the expected-grad-scale cache had given back"
    assert all(bool((h == 0x5A).all()) for h in held), "a replay wrote into memory the workspace cache had given back"
    del cap


# ---- the declared symbols are the ones that were replayed (last: it reads what the rows above recorded) ---------------------------------
def test_every_row_called_the_symbols_it_declares():
    if not REPLAYED:
        pytest.skip("no capture row ran in this session")
    for c in CC.CASES:
        if c.name in REPLAYED:
            assert set(c.symbols) <= REPLAYED[c.name], (c.name, sorted(set(c.symbols) - REPLAYED[c.name]))
