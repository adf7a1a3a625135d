"""A/B of the batch-32 step's softmax + backward launch: step_small_kernel (small_step_roles = 0) against the role-split forms of
csrc/step_small.h (1: 16-column dQ tiles, 2: 32-column dQ tiles, 3: form 2 with the outputs written by a workgroup of their own), in ONE
process, arms alternating.  --option NAME alternates another option of the library instead (small_sim_copy 0 / 1: the sim launch's bf16
copies on the compute waves / on waves of their own); a shape written p32x256x768 is the packed one-rank step (bf16 contexts, 256 rows
padded to the packed row count).
Each arm is a HIP graph of ten dprhot_inbatch_step_f32 calls (device-bound, like bench.py --driver graph10); a round times 200 replays
of every arm in turn with device events.  Prints one line per shape: us per step, min / median / max over the rounds.

  python scratch/small_step_ab.py [--rounds 7] [--option small_step_roles] [--arms 0,1,2,3] [--shapes 32x256x768,32x64x768,...]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpr_scale_amd import _lib  # noqa: E402
from dpr_scale_amd.hotpath import _ptr  # noqa: E402

DEFAULT_SHAPES = "32x256x768,32x64x768,32x528x768,32x256x1024"


def build_arm(B, Nc, d, arm, dev, option="small_step_roles", packed=False):
    if packed:
        return build_arm_packed(B, Nc, d, arm, dev, option)
    gen = torch.Generator(device="cpu").manual_seed(B + Nc + d)
    q = (torch.randn(B, d, generator=gen) * d ** -0.25).to(dev)
    c = (torch.randn(Nc, d, generator=gen) * d ** -0.25).to(dev)
    y = (torch.arange(B) * (Nc // B)).to(torch.int64).to(dev)
    f32, bf16 = torch.float32, torch.bfloat16
    Qb, Cb = torch.empty((B, d), dtype=bf16, device=dev), torch.empty((Nc, d), dtype=bf16, device=dev)
    rl, lse, ls = torch.empty(B, dtype=f32, device=dev), torch.empty(B, dtype=f32, device=dev), torch.empty(1, dtype=f32, device=dev)
    G = torch.empty((B, Nc), dtype=bf16, device=dev)
    dQ, dC = torch.empty((B, d), dtype=f32, device=dev), torch.empty((Nc, d), dtype=f32, device=dev)
    nbytes = _lib.workspace_bytes(B, Nc, d)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    keep = (q, c, y, Qb, Cb, rl, lse, ls, G, dQ, dC, ws)

    def step(stream):
        _lib.check(_lib.lib.dprhot_inbatch_step_f32(_ptr(q), _ptr(c), _ptr(Qb), _ptr(Cb), B, Nc, d, _ptr(y), 0, None, 1.0, 1.0 / B, 1.0, None,
                                                    None, _ptr(rl), _ptr(lse), _ptr(ls), _ptr(G), _ptr(dQ), _ptr(dC), _ptr(ws), nbytes, stream),
                   "dprhot_inbatch_step_f32")

    _lib.set_option(option, arm)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(ctypes.c_void_p(side.cuda_stream))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(10):
            step(ctypes.c_void_p(side.cuda_stream))
    torch.cuda.synchronize()
    return g, keep, (dQ, dC, ls, G, rl, lse)


def build_arm_packed(B, n_ctx, d, arm, dev, option):
    """dprhot_inbatch_step_packed_f32 at W = 1 through the Python wrapper (its outputs come from the graph's own pool)."""
    from dpr_scale_amd.hotpath import HipKernels

    kn = HipKernels()
    gen = torch.Generator(device="cpu").manual_seed(B + n_ctx + d)
    q = (torch.randn(B, d, generator=gen) * d ** -0.25).to(dev)
    c = (torch.randn(n_ctx, d, generator=gen) * d ** -0.25).to(dev)
    m = torch.zeros(n_ctx, dtype=torch.uint8, device=dev)
    Cb = torch.empty((kn.packed_rows(n_ctx, d), d), dtype=torch.bfloat16, device=dev)
    kn.pack_ctx(c, m, Cb)
    Qb = torch.empty((B, d), dtype=torch.bfloat16, device=dev)
    y = (torch.arange(B) * (n_ctx // B)).to(torch.int64).to(dev)
    _lib.set_option(option, arm)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        kn.inbatch_step_packed_f32(q, Cb, Qb, 1, 0, n_ctx, y, 1.0, 1.0 / B, want_G=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(10):
            out = kn.inbatch_step_packed_f32(q, Cb, Qb, 1, 0, n_ctx, y, 1.0, 1.0 / B, want_G=True)
    torch.cuda.synchronize()
    return g, (q, c, m, Cb, Qb, y, kn), tuple(o for o in out if o.element_size() in (2, 4)) + (Qb,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--option", default="small_step_roles")
    ap.add_argument("--arms", default="0,1,2,3")
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    arms = [int(x) for x in a.arms.split(",")]
    default = _lib.get_option(a.option)
    for shape in a.shapes.split(","):
        B, Nc, d = (int(x) for x in shape.lstrip("p").split("x"))
        graphs = {arm: build_arm(B, Nc, d, arm, dev, a.option, packed=shape.startswith("p")) for arm in arms}
        ref = None
        for arm in arms:  # same bits from every arm before any of them is timed
            graphs[arm][0].replay()
            torch.cuda.synchronize()
            out = [t.clone() for t in graphs[arm][2]]
            if ref is None:
                ref = out
            assert all(torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32), r.view(torch.int16 if r.element_size() == 2 else torch.int32)) for x, r in zip(out, ref)), f"{shape}: arm {arm} differs from arm {arms[0]}"
        us = {arm: [] for arm in arms}
        for _ in range(a.rounds):
            for arm in arms:
                g = graphs[arm][0]
                for _ in range(20):
                    g.replay()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.replays):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                us[arm].append(e0.elapsed_time(e1) * 1e3 / (a.replays * 10))
        print(shape + "  " + "  ".join(f"{a.option}={arm}: min {min(v):.3f} med {statistics.median(v):.3f} max {max(v):.3f}" for arm, v in us.items()), flush=True)
    _lib.set_option(a.option, default)


if __name__ == "__main__":
    main()
