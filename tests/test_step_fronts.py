"""The fronts of the batch-32 step's two launches, read from the compiled text (no GPU): step_small_kernel_out<1, 3, 32>
(csrc/step_small.h) and sim_small_kernel<true, SS_PATCH> (csrc/sim_small.h) are compiled alone to gfx950 assembly, as
scripts/small_step_isa_count.py does.  Both launches are chains of latencies, and a wait on memory in front of a role's operand loads
is a whole trip that the result does not need:
  second launch: in the dC, dQ, loss and row-store stretches -- each there twice, as the compile-time text of 32 x 256 and as the
                 run-time text -- no s_waitcnt on vmcnt stands between the stretch's first global load and its first
                 global_load_dwordx4 (the device-side scale used to be such a load and wait, in front of everything);
  sim launch:    no wait on vmcnt and at most one on lgkmcnt (the kernel arguments) precedes the first global_load_dwordx4.
Only loads and waits are named here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpr_scale_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
STEP = ('#include "step_small.h"\ntemplate __global__ void dprhot::step_small_kernel_out<1, 3, 32>(dprhot::StepSmallArgs);\n',
        "_ZN6dprhot21step_small_kernel_out")
SIM = ('#include "sim_small.h"\ntemplate __global__ void dprhot::sim_small_kernel<true, 2>(int, dprhot::GemmArgs, dprhot::EpiSim);\n',
       "_ZN6dprhot16sim_small_kernel")

pytestmark = pytest.mark.skipif(not (os.path.isfile(HIPCC) or shutil.which(HIPCC)), reason="no hipcc")


def _body(inst, symbol, tmp_path):
    """[(mnemonic, operands)] of the one kernel whose mangled name starts with `symbol`."""
    src, asm = tmp_path / "inst.hip", tmp_path / "inst.s"
    src.write_text(inst)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I" + CSRC, str(src), "-o", str(asm)],
                   check=True, stderr=subprocess.DEVNULL)
    body, on = [], False
    for ln in asm.read_text().splitlines():
        if re.match(r"^%s\S*:" % re.escape(symbol), ln):
            on = True
        elif on and ln.startswith(".Lfunc_end"):
            break
        elif on and ln.startswith("\t") and not ln.strip().startswith((".", ";")):
            t = ln.split(None, 1)
            body.append((t[0], t[1].strip() if len(t) > 1 else ""))
    assert body, f"no kernel {symbol} in the assembly"
    return body


def _stretches(body):
    """The text cut behind every s_barrier and s_endpgm and -- where a role's path runs on into the next role's text -- behind the last
    global store in front of a global load: [(closing mnemonic or "-", instructions)]."""
    out, cur, last_store = [], [], None
    for op, args in body:
        if op in ("s_barrier", "s_endpgm"):
            out.append((op, cur))
            cur, last_store = [], None
            continue
        if op.startswith("global_load") and last_store is not None:
            out.append(("-", cur[:last_store + 1]))
            cur, last_store = cur[last_store + 1:], None
        if op.startswith("global_store"):
            last_store = len(cur)
        cur.append((op, args))
    return out


def _role(end, ins):
    """Which role's front a stretch is, from what follows its first global_load_dwordx4 (CPT = 1, NS = 3: six slab loads per thread)."""
    first = next((k for k, (op, _) in enumerate(ins) if op == "global_load_dwordx4"), None)
    if first is None:
        return None
    tail = [op for op, _ in ins[first:]]
    x4, stores = tail.count("global_load_dwordx4"), sum(op.startswith("global_store") for op in tail)
    if x4 < 6:
        return None
    if end != "s_barrier":
        return "row-store" if stores else None
    return "loss" if stores else "dQ" if x4 >= 8 else "dC"  # dQ: the two C-tile loads of waves 8-15 as well; dC: the Q tile


def _vm_waits_in_front(ins):
    first_ld = next(k for k, (op, _) in enumerate(ins) if op.startswith("global_load"))
    first_x4 = next(k for k, (op, _) in enumerate(ins) if op == "global_load_dwordx4")
    return [(k, a) for k, (op, a) in enumerate(ins[first_ld:first_x4], first_ld) if op == "s_waitcnt" and "vmcnt" in a]


def test_second_launch_roles_wait_for_nothing_in_front_of_their_loads(tmp_path):
    seen = {}
    for end, ins in _stretches(_body(*STEP, tmp_path)):
        role = _role(end, ins)
        if role is None:
            continue
        seen[role] = seen.get(role, 0) + 1
        waits = _vm_waits_in_front(ins)
        assert not waits, f"{role} stretch #{seen[role]}: s_waitcnt {waits} between its first global load and its first global_load_dwordx4"
    # every role is there as the compile-time text and as the run-time text
    assert seen == {"dC": 2, "dQ": 2, "loss": 2, "row-store": 2}, seen


def test_sim_launch_front(tmp_path):
    body = _body(*SIM, tmp_path)
    first_x4 = next(k for k, (op, _) in enumerate(body) if op == "global_load_dwordx4")
    waits = [a for op, a in body[:first_x4] if op == "s_waitcnt"]
    assert not [a for a in waits if "vmcnt" in a], f"a wait on vmcnt in front of the first operand load: {waits}"
    assert len([a for a in waits if "lgkmcnt" in a]) <= 1, f"more than one wait on the kernel arguments in front of the first operand load: {waits}"
    assert sum(op == "global_load_dwordx4" for op, _ in body) == 32
