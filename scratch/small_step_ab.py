"""A/B of the batch-32 step's softmax + backward launch: step_small_kernel (small_step_roles = 0) against the role-split forms of
csrc/step_small.h (1: 16-column dQ tiles, 2: 32-column dQ tiles, 3: form 2 with the outputs written by a workgroup of their own), in ONE
process, arms alternating.
Each arm is a HIP graph of ten dprhot_inbatch_step_f32 calls (device-bound, like bench.py --driver graph10); a round times 200 replays
of every arm in turn with device events.  Prints one line per shape: us per step, min / median / max over the rounds.

  python scratch/small_step_ab.py [--rounds 7] [--arms 0,1,2,3] [--shapes 32x256x768,32x64x768,...]
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


def build_arm(B, Nc, d, arm, dev):
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

    _lib.set_option("small_step_roles", arm)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--arms", default="0,1,2,3")
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    arms = [int(x) for x in a.arms.split(",")]
    default = _lib.get_option("small_step_roles")
    for shape in a.shapes.split(","):
        B, Nc, d = (int(x) for x in shape.split("x"))
        graphs = {arm: build_arm(B, Nc, d, arm, dev) for arm in arms}
        ref = None
        for arm in arms:  # same bits from every arm before any of them is timed
            graphs[arm][0].replay()
            torch.cuda.synchronize()
            out = [t.clone() for t in graphs[arm][2]]
            if ref is None:
                ref = out
            assert all(torch.equal(x.view(torch.int32), r.view(torch.int32)) for x, r in zip(out, ref)), f"{shape}: arm {arm} differs from arm {arms[0]}"
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
        print(shape + "  " + "  ".join(f"small_step_roles={arm}: min {min(v):.3f} med {statistics.median(v):.3f} max {max(v):.3f}" for arm, v in us.items()), flush=True)
    _lib.set_option("small_step_roles", default)


if __name__ == "__main__":
    main()
