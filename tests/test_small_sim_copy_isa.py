"""The two roles of sim_small_split_kernel (csrc/sim_small.h), read from the compiled text (no GPU): the kernel is compiled alone to
gfx950 assembly, as tests/test_step_fronts.py does with the launch it replaces.  One scalar compare on the block index behind the single
wait for the kernel arguments sends a wave into the compute role (32 operand loads, the MFMA chain, the slab stores) or the copy role (16
loads, 8-byte stores).  Either role's way from the kernel's first instruction to its first global_load_dwordx4 holds at most one wait on
lgkmcnt and none on vmcnt -- a wait on memory there is a whole trip in front of the role's only trip.  The ways are followed through the
text: the first conditional branch is the role branch, one role falls through it and the other starts at its target.
Only loads, waits and branches are named here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpr_scale_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INST = '#include "sim_small.h"\ntemplate __global__ void dprhot::sim_small_split_kernel<%s>(int, dprhot::GemmArgs, dprhot::EpiSim);\n'
SYMBOL = "_ZN6dprhot22sim_small_split_kernel"

pytestmark = pytest.mark.skipif(not (os.path.isfile(HIPCC) or shutil.which(HIPCC)), reason="no hipcc")


def _body(b_f32, tmp_path):
    """[(mnemonic, operands)] of the kernel, its local labels as ("label", name)."""
    src, asm = tmp_path / "inst.hip", tmp_path / "inst.s"
    src.write_text(INST % b_f32)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I" + CSRC, str(src), "-o", str(asm)],
                   check=True, stderr=subprocess.DEVNULL)
    body, on = [], False
    for ln in asm.read_text().splitlines():
        if re.match(r"^%s\S*:" % re.escape(SYMBOL), ln):
            on = True
        elif on and ln.startswith(".Lfunc_end"):
            break
        elif on and re.match(r"^\.LBB\w+:", ln):
            body.append(("label", ln.split(":")[0]))
        elif on and ln.startswith("\t") and not ln.strip().startswith((".", ";")):
            t = ln.split(None, 1)
            body.append((t[0], re.sub(r"\s*;.*", "", t[1]).strip() if len(t) > 1 else ""))
    assert body, f"no kernel {SYMBOL} in the assembly"
    return body


def _way_to_first_x4(body, start, taken):
    """The instructions from `start` up to the first global_load_dwordx4, straight through the text; a conditional branch on the way that
    would leave it (an early return, an empty-exec skip) is passed by, an unconditional one is followed."""
    way, k = list(taken), start
    while True:
        assert k < len(body), "no global_load_dwordx4 on this way"
        op, args = body[k]
        if op == "global_load_dwordx4":
            return way
        if op == "s_branch":
            k = body.index(("label", args))
            continue
        if op != "label":
            way.append((op, args))
        k += 1


def _roles(body):
    """(ways of the two roles to their first global_load_dwordx4, the number of global_load_dwordx4 in each role's text)"""
    br = next(k for k, (op, _) in enumerate(body) if op.startswith("s_cbranch"))
    assert body[br][0] in ("s_cbranch_scc0", "s_cbranch_scc1"), f"the role branch is a scalar compare's: {body[br]}"
    target = body.index(("label", body[br][1]))
    assert target > br
    head = [x for x in body[:br + 1] if x[0] != "label"]
    ways = [_way_to_first_x4(body, br + 1, head), _way_to_first_x4(body, target, head)]
    x4 = [sum(op == "global_load_dwordx4" for op, _ in body[br + 1:target]), sum(op == "global_load_dwordx4" for op, _ in body[target:])]
    return ways, x4


@pytest.mark.parametrize("b_f32", ["true", "false"])
def test_both_roles_reach_their_loads_behind_one_wait(b_f32, tmp_path):
    body = _body(b_f32, tmp_path)
    ways, x4 = _roles(body)
    # fp32 contexts: 32 operand loads in the compute role; bf16 contexts: the 16 of q (the fragments of C are 8 more, counted apart)
    assert sorted(x4) == ([16, 32] if b_f32 == "true" else [16, 24]), x4
    for way, n in zip(ways, x4):
        role = "copy" if n == 16 else "compute"
        waits = [a for op, a in way if op == "s_waitcnt"]
        assert not [a for a in waits if "vmcnt" in a], f"{role} role: a wait on vmcnt in front of its first operand load: {waits}"
        assert len([a for a in waits if "lgkmcnt" in a]) <= 1, f"{role} role: more than one wait on the kernel arguments in front of its first operand load: {waits}"
    # the role branch itself stands behind that one wait and in front of every load
    br = next(k for k, (op, _) in enumerate(body) if op.startswith("s_cbranch"))
    assert not [op for op, _ in body[:br] if op.startswith("global_load")]


def test_compute_role_holds_32_operand_loads(tmp_path):
    _, x4 = _roles(_body("true", tmp_path))
    assert max(x4) == 32 and sum(x4) == 48, x4
