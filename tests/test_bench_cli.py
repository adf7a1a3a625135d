"""bench.py's command line: a plain run times exactly --steps steps and measures nothing else; --full carries the extra
blocks; --dump-outputs writes the last step's outputs (float32, at most 64 MB, a fixed sample of an array above its share)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench():
    """bench.py as a module, without the environment default it sets for its own process (it would outlive this test)."""
    had = "HIP_FORCE_DEV_KERNARG" in os.environ
    import bench

    if not had:
        os.environ.pop("HIP_FORCE_DEV_KERNARG", None)
    return bench


def _parse(*argv):
    bench = _bench()
    saved = sys.argv
    sys.argv = ["bench.py", *argv]
    try:
        return bench.parse()
    finally:
        sys.argv = saved


def test_plain_run_has_no_extra_blocks_and_full_keeps_them():
    a = _parse("--steps", "20")
    assert (a.full, a.repeats, a.blocks) == (False, 1, set())
    a = _parse("--full")
    assert a.repeats == 31 and a.blocks == {"operator", "torch_gpu", "scale", "rank", "router", "grad_hook", "cpu", "e2e", "model"}
    a = _parse("--full", "--only", "operator,e2e5", "--repeats", "3")
    assert a.repeats == 3 and a.blocks == {"operator", "e2e5"}
    assert _parse("--full", "--no-cpu-baseline", "--no-e2e").blocks == {"operator", "torch_gpu", "scale", "rank", "router", "grad_hook", "model"}
    assert _parse("--only", "step").blocks == set()
    with pytest.raises(SystemExit):
        _parse("--only", "operator")  # the extra blocks need --full


def test_dump_outputs_is_float32_bounded_and_samples_the_same_positions(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(3)
    small = rng.standard_normal((32, 768)).astype(np.float32)
    big = rng.standard_normal((9000, 1024)).astype(np.float32)  # 36.9 MB: above its share of the 64 MB
    outs = {"loss": np.float32([1.5]), "row_loss": np.arange(32, dtype=np.float64), "dq": small, "dc": big}
    bench.dump_outputs(outs, str(tmp_path / "a"))
    bench.dump_outputs(outs, str(tmp_path / "b"))
    total = 0
    for name in outs:
        x = np.load(tmp_path / "a" / f"{name}.npy")
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
        assert x.dtype == np.float32 and np.array_equal(x, np.load(tmp_path / "b" / f"{name}.npy"))
    assert total <= bench.DUMP_BYTES
    assert np.array_equal(np.load(tmp_path / "a" / "dq.npy"), small)  # under its share: whole, shape kept
    d = np.load(tmp_path / "a" / "dc.npy")
    assert d.ndim == 1 and 0 < d.size < big.size and np.isin(d, big).all()


def _run_bench(args, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_last_step(tmp_path):
    """A plain run: one region of exactly --steps steps, no extra blocks; the dumped gradients are the step's (fp64 oracle on the
    same seeded inputs, the bf16 bars of the parity suite)."""
    from dpr_scale_amd.datamodule.synthetic import unit_logit_embeddings
    from oracle import inbatch_oracle as O

    out = tmp_path / "dump"
    line = _run_bench(["--gpus", "1", "--steps", "37", "--warmup", "5", "--dump-outputs", str(out)])
    assert line["steps"] == 37 and line["timing"]["repeats"] == 1 and line["timing"]["steps_per_repeat"] == 37
    assert line["ms_per_step"] > 0 and abs(line["value"] - 32 / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert key in line
    assert line["config"]["driver"] in ("eager", "graph", "graph10") and set(line["driver_probe"]) == {"eager", "graph", "graph10"}
    assert not {"cpu_baseline", "operator", "end_to_end", "roofline_at_scale"} & set(line) and line["roofline"] is None
    q, c, y, m = unit_logit_embeddings(1234, 32, 8, 768)
    ref = O.training_step_global(q, c, y, m, 1.0)
    got = {n: np.load(out / f"{n}.npy") for n in ("loss", "row_loss", "row_lse", "dq", "dc")}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert _rel(got["row_lse"], ref["lse"]) <= 1e-3 and _rel(got["row_loss"], ref["row_loss"]) <= 1e-3
    assert _rel(got["loss"], ref["row_loss"].sum()) <= 1e-3  # the loss numerator: the sum of the rows' losses
    assert _rel(got["dq"], ref["dQ"]) <= 1e-2 and _rel(got["dc"], ref["dC"]) <= 1e-2


@pytest.mark.gpu
def test_plain_run_time_per_step_does_not_follow_the_step_count():
    """--steps is the number of steps in the timed region: 100 times as many steps take ~100 times as long, so ms_per_step
    (region / steps) stays put -- a region of any other length would move it by up to that factor."""
    few, many = (_run_bench(["--gpus", "1", "--driver", "eager", "--steps", str(n), "--warmup", "20"]) for n in (200, 20000))
    assert (few["steps"], many["steps"]) == (200, 20000)
    assert 1 / 3 <= many["ms_per_step"] / few["ms_per_step"] <= 3, (few["ms_per_step"], many["ms_per_step"])


@pytest.mark.gpu
def test_plain_two_rank_run_on_one_device_prints_its_line_and_dumps_rank_0(tmp_path):
    """The plain N > 1 path (bench.py starts its own two ranks; gloo, both on device 0): the line comes out, without the N = 1
    driver probe, and rank 0's dump is its share of the global step (fp64 oracle on both ranks' seeded inputs)."""
    from dpr_scale_amd.datamodule.synthetic import unit_logit_embeddings
    from oracle import inbatch_oracle as O

    out = tmp_path / "dump"
    line = _run_bench(["--gpus", "2", "--steps", "30", "--warmup", "5", "--dump-outputs", str(out)],
                      env={"DPRHOT_DIST_BACKEND": "gloo", "DPRHOT_SAME_DEVICE": "1"})
    assert line["n_gpus"] == 2 and line["steps"] == 30 and line["timing"]["repeats"] == 1 and line["ms_per_step"] > 0
    assert "driver_probe" not in line and "variants" not in line and line["roofline"] is None
    B, K, d = 32, 8, 768
    parts = [unit_logit_embeddings(1234 + r, B, K, d) for r in range(2)]
    Q, C = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    y = np.concatenate([p[2] + r * B * K for r, p in enumerate(parts)])
    ref = O.training_step_global(Q, C, y, np.concatenate([p[3] for p in parts]), 1.0)
    got = {n: np.load(out / f"{n}.npy") for n in ("loss", "row_loss", "row_lse", "dq", "dc")}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert _rel(got["row_lse"], ref["lse"][:B]) <= 1e-3 and _rel(got["row_loss"], ref["row_loss"][:B]) <= 1e-3
    assert _rel(got["loss"], ref["row_loss"].sum()) <= 1e-3  # both ranks' loss numerators, summed by the reduce-scatter
    assert _rel(got["dq"], ref["dQ"][:B]) <= 1e-2 and _rel(got["dc"], ref["dC"][:B * K]) <= 1e-2
