"""Static instruction counts of step_small_kernel_out<1, 3, 32> (csrc/step_small.h), the flagship instantiation of the batch-32 step's
second launch, and of sim_small_kernel<true, SS_PATCH> (csrc/sim_small.h), the first: each kernel alone is compiled to gfx950 assembly
(no GPU needed) and its vector instructions (v_*) are counted, in total and per stretch of program text that ends in a workgroup
barrier or at the end of a program path -- the stretch in front of a role's first barrier is that role's loads and shared row softmax.
Per stretch it also prints the front: the number of s_waitcnt lines ahead of the first global_load_dwordx4 (counted from the stretch's
start) and how many of them wait on vmcnt between the stretch's first global load and that first global_load_dwordx4 -- a wait there
is a trip to memory in front of the loads the role is about.  A record for profiles/small_step_lean_isa.txt and
profiles/step_fronts_isa.txt, not a test (tests/test_step_fronts.py asserts the fronts).
The role named next to a stretch is a GUESS from its loads and stores behind the first global_load_dwordx4, the kernel carrying each
role twice (the compile-time text of 32 x 256 and the run-time text): row-store role: stores and no barrier; loss role:
global stores in front of its barrier; dQ role: 8 or more global_load_dwordx4 (with the C-tile loads of waves 8-15); dC role: 7.  The
guess is fitted to this one instantiation as compiled for that record: after a change to the kernel, check the labels against the
assembly before quoting them.

  python scripts/small_step_isa_count.py [--csrc dpr_scale_amd/csrc] [--hipcc /opt/rocm/bin/hipcc]
"""
import argparse
import collections
import os
import re
import subprocess
import tempfile

INST = '#include "step_small.h"\ntemplate __global__ void dprhot::step_small_kernel_out<1, 3, 32>(dprhot::StepSmallArgs);\n'
INST_SIM = ('#include "sim_small.h"\ntemplate __global__ void dprhot::sim_small_kernel<true, dprhot::SS_PATCH>(int, dprhot::GemmArgs, '
            'dprhot::EpiSim);\n')


def kernel_body(hipcc, csrc, inst, symbol, tmp, quiet=False):
    """The instruction lines (mnemonic, operands) of the one kernel whose mangled name starts with `symbol`."""
    src, asm = os.path.join(tmp, "inst.hip"), os.path.join(tmp, "inst.s")
    open(src, "w").write(inst)
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I" + csrc, src, "-o", asm]
    if not quiet:
        print("# " + " ".join(cmd[:6]) + " -I<csrc> inst.hip -o inst.s")
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    body, on = [], False
    for ln in open(asm):
        if re.match(r"^%s\S*:" % re.escape(symbol), ln):
            on = True
        elif on and ln.startswith(".Lfunc_end"):
            break
        elif on and ln.startswith("\t") and not ln.strip().startswith((".", ";")):
            t = ln.split(None, 1)
            body.append((t[0], t[1].strip() if len(t) > 1 else ""))
    return body


def stretches(body):
    """The body cut behind every s_barrier and s_endpgm -- and, where a role's path runs on into the next role's text without ending the
    program, behind its last global store ("-"): [(closing mnemonic or "-", [(mnemonic, operands), ...]), ...]."""
    out, cur, last_store = [], [], None
    for op, args in body:
        if op in ("s_barrier", "s_endpgm"):
            out.append((op, cur))
            cur, last_store = [], None
            continue
        if op.startswith("global_load") and last_store is not None:  # loads behind stores: another role begins
            out.append(("-", cur[:last_store + 1]))
            cur, last_store = cur[last_store + 1:], None
        if op.startswith("global_store"):
            last_store = len(cur)
        cur.append((op, args))
    return out


def front(ins):
    """(s_waitcnt lines ahead of the first global_load_dwordx4, vmcnt waits among them behind the first global load, lgkmcnt waits among
    them), or None for a stretch without a global_load_dwordx4."""
    first_x4 = next((k for k, (op, _) in enumerate(ins) if op == "global_load_dwordx4"), None)
    if first_x4 is None:
        return None
    first_ld = next(k for k, (op, _) in enumerate(ins) if op.startswith("global_load"))
    waits = [(k, a) for k, (op, a) in enumerate(ins[:first_x4]) if op == "s_waitcnt"]
    return len(waits), sum(1 for k, a in waits if k > first_ld and "vmcnt" in a), sum(1 for k, a in waits if "lgkmcnt" in a)


def role_of(end, ins):
    first_x4 = next((k for k, (op, _) in enumerate(ins) if op == "global_load_dwordx4"), None)
    if first_x4 is None:
        return ""
    tail = [op for op, _ in ins[first_x4:]]
    x4, st = tail.count("global_load_dwordx4"), sum(op.startswith("global_store") for op in tail)
    if end != "s_barrier":
        return "row-store role" if x4 >= 6 and st else ""
    return "loss role" if st else "dQ role (with the C-tile loads of waves 8-15)" if x4 >= 8 else "dC role" if x4 >= 7 else "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dpr_scale_amd", "csrc"))
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        full = kernel_body(a.hipcc, a.csrc, INST, "_ZN6dprhot21step_small_kernel_out", tmp)
        sim = kernel_body(a.hipcc, a.csrc, INST_SIM, "_ZN6dprhot16sim_small_kernel", tmp, quiet=True)
    body = [op for op, _ in full]
    c = collections.Counter(body)

    def n(pred):
        return sum(v for k, v in c.items() if pred(k))

    print(f"instructions {len(body)}  vector (v_*) {n(lambda k: k.startswith('v_'))}  v_cndmask {n(lambda k: 'cndmask' in k)}  "
          f"v_cmp {n(lambda k: k.startswith('v_cmp'))}  v_lshl_add_u64 {c['v_lshl_add_u64']}  ds_bpermute_b32 {c['ds_bpermute_b32']}  "
          f"v_permlane16_swap {n(lambda k: 'permlane16' in k)}  v_div_scale_f32 {c['v_div_scale_f32']}  s_barrier {c['s_barrier']}")
    for end, ins in stretches(full):
        seg = collections.Counter()
        for op, _ in ins:
            seg["v"] += op.startswith("v_")
            seg["cnd"] += "cndmask" in op
            seg["cmp"] += op.startswith("v_cmp")
            seg["gload"] += op.startswith("global_load")
            seg["gstore"] += op.startswith("global_store")
            seg["mfma"] += "mfma" in op
        fr = front(ins)
        fr_txt = f"front: {fr[0]} s_waitcnt before the first dwordx4 load, {fr[1]} on vmcnt behind the first load" if fr else ""
        print(f"  up to {end:9s}: v_* {seg['v']:4d}  v_cndmask {seg['cnd']:3d}  v_cmp {seg['cmp']:3d}  global loads {seg['gload']:2d}  "
              f"global stores {seg['gstore']:2d}  mfma {seg['mfma']}   {role_of(end, ins)}  {fr_txt}")
    ops = [op for op, _ in sim]
    first_x4 = ops.index("global_load_dwordx4")
    fr = front(sim)
    print(f"sim_small_kernel<true, SS_PATCH>: instructions {len(ops)}, the first global_load_dwordx4 is instruction {first_x4 + 1}; "
          f"{fr[0]} s_waitcnt before it ({fr[2]} on lgkmcnt, {sum(1 for op, a in sim[:first_x4] if op == 's_waitcnt' and 'vmcnt' in a)} on vmcnt), "
          f"v_rcp_iflag_f32 before it {ops[:first_x4].count('v_rcp_iflag_f32_e32')}, branches before it "
          f"{sum(op.startswith('s_cbranch') for op in ops[:first_x4])}")


if __name__ == "__main__":
    main()
