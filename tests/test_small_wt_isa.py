"""The write-through stores of the batch-32 sim launch's copy waves (what option small_sim_copy = 1 launches), read from the compiled text (no GPU):
sim_small_split_kernel<true, 1> (csrc/sim_small.h) is compiled alone to gfx950 assembly, as tests/test_step_fronts.py does with
today's kernels.  The copy role has eight 16-byte stores carrying sc1 per lane and no narrower store, its sixteen whole-line loads
are as before, the compute role of the same kernel stores no write-through piece, and the kernel uses no scratch.
(The dC tiles of the second launch were to leave the same way; that form lost its A/B and is not in the library:
scratch/negative/README.md.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpr_scale_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SIM = ('#include "sim_small.h"\ntemplate __global__ void dprhot::sim_small_split_kernel<true, 1>(int, dprhot::GemmArgs, dprhot::EpiSim);\n',
       "_ZN6dprhot22sim_small_split_kernel")

pytestmark = pytest.mark.skipif(not (os.path.isfile(HIPCC) or shutil.which(HIPCC)), reason="no hipcc")


def _kernel(inst, symbol, tmp_path):
    """([(mnemonic, operands)], bytes of scratch) of the one kernel whose mangled name starts with `symbol`."""
    src, asm = tmp_path / "inst.hip", tmp_path / "inst.s"
    src.write_text(inst)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I" + CSRC, str(src), "-o", str(asm)],
                   check=True, stderr=subprocess.DEVNULL)
    text = asm.read_text()
    body, on = [], False
    for ln in text.splitlines():
        if re.match(r"^%s\S*:" % re.escape(symbol), ln):
            on = True
        elif on and ln.startswith(".Lfunc_end"):
            break
        elif on and ln.startswith("\t") and not ln.strip().startswith((".", ";")):
            t = ln.split(None, 1)
            body.append((t[0], t[1].strip() if len(t) > 1 else ""))
    assert body, f"no kernel {symbol} in the assembly"
    desc = re.search(r"\.amdhsa_kernel %s\S*\n(.*?)\.end_amdhsa_kernel" % re.escape(symbol), text, re.S)
    scratch = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc.group(1))
    return body, int(scratch.group(1))


def _is_store(op):
    return "_store" in op


def _is_wt16(op, args):
    return op == "buffer_store_dwordx4" and "sc1" in args.split()


def test_copy_role_eight_write_through_stores_and_no_narrower_one(tmp_path):
    body, scratch = _kernel(*SIM, tmp_path)
    assert scratch == 0, f"sim_small_split_kernel<true, 1> uses {scratch} bytes of scratch"
    wt = [k for k, (op, args) in enumerate(body) if _is_wt16(op, args)]
    assert len(wt) == 8, f"{len(wt)} 16-byte write-through stores in the kernel, expected the copy role's eight"
    # the copy role's text: the run of instructions around its stores that holds no MFMA -- from the kernel's first instruction (the
    # compiler lays this role in front) or the last MFMA in front of the stores, to the first load or MFMA behind them
    mf = [k for k, (op, _) in enumerate(body) if op.startswith("v_mfma")]
    assert mf, "the compute role's MFMA chain is in the same kernel"
    lo = max([k for k in mf if k < wt[0]], default=-1) + 1
    hi = next((k for k, (op, _) in enumerate(body) if k > wt[-1] and (op.startswith("v_mfma") or "_load" in op or op == "s_endpgm")), len(body))
    role = body[lo:hi]
    if lo > 0:  # laid behind the compute role: its text starts behind that role's last store
        last = max([k for k, (op, _) in enumerate(role) if _is_store(op) and k < wt[0] - lo], default=-1)
        role = role[last + 1:]
    loads = [op for op, _ in role if op.startswith("global_load")]
    assert loads == ["global_load_dwordx4"] * 16, f"the copy role's sixteen whole-line loads: {loads}"
    others = [(op, args) for op, args in role if _is_store(op) and not _is_wt16(op, args)]
    assert not others, f"copy role: stores other than 16-byte write-through ones: {others}"
    assert sum(_is_wt16(op, args) for op, args in role) == 8
