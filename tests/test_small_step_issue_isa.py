"""The issue cost of the batch-32 step's shared row softmax, read from the compiled text (no GPU): step_small_kernel_out<1, 3, 32>
(csrc/step_small.h) is compiled alone to gfx950 assembly, as tests/test_step_fronts.py and scripts/small_step_isa_count.py do, and
cut into stretches behind every barrier and program end.  The stretch in front of a role's first barrier is that role's loads and the
row softmax, which every workgroup of the launch repeats on four waves per SIMD: its vector instructions are the launch's critical
path.  In the dC, dQ and loss stretches -- each there twice, as the compile-time (FULL) text of 32 x 256 and as the run-time text, the
FULL one being the shorter: it has no -inf selects and no guards -- the number of v_* instructions must stay below what the text had
before the softmax was rewritten on two-element vectors with a one-statement row maximum.
Only loads, barriers and v_* counts are named here."""
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

# v_* instructions from a role's entry to its first barrier in the text of the parent of this change (commit 4a644fa, "Clear the fronts
# of both batch-32 launches, split form 3's output role"), as scripts/small_step_isa_count.py printed them there (the record, with the
# figures of this text next to them: profiles/small_step_issue_isa.txt): (FULL text, run-time text)
PARENT = {"dC": (171, 185), "dQ": (177, 207), "loss": (136, 150)}

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
    """Which role's front a stretch that ends in a barrier is, from what follows its first global_load_dwordx4 (CPT = 1, NS = 3: six
    slab loads per thread): stores in front of the barrier only in the loss role, eight or more wide loads in the dQ role (the two
    C-tile loads of waves 8-15), fewer in the dC role (the Q tile)."""
    first = next((k for k, (op, _) in enumerate(ins) if op == "global_load_dwordx4"), None)
    if first is None or end != "s_barrier":
        return None
    tail = [op for op, _ in ins[first:]]
    x4, stores = tail.count("global_load_dwordx4"), sum(op.startswith("global_store") for op in tail)
    if x4 < 6:
        return None
    return "loss" if stores else "dQ" if x4 >= 8 else "dC"


def test_vector_instructions_in_front_of_each_roles_first_barrier(tmp_path):
    counts = {}
    for end, ins in _stretches(_body(*STEP, tmp_path)):
        role = _role(end, ins)
        if role is not None:
            counts.setdefault(role, []).append(sum(op.startswith("v_") for op, _ in ins))
    assert {r: len(v) for r, v in counts.items()} == {"dC": 2, "dQ": 2, "loss": 2}, counts
    print({r: sorted(v) for r, v in counts.items()})
    for role, (full, run_time) in PARENT.items():
        new_full, new_run_time = sorted(counts[role])
        assert new_full < full, f"{role} role, FULL text: {new_full} vector instructions in front of the barrier, the parent had {full}"
        assert new_run_time < run_time, f"{role} role, run-time text: {new_run_time} vector instructions, the parent had {run_time}"
