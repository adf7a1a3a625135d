"""Static instruction counts of step_small_kernel_out<1, 3, 32> (csrc/step_small.h), the flagship instantiation of the batch-32 step's
second launch: the kernel alone is compiled to gfx950 assembly (no GPU needed) and its vector instructions (v_*) are counted, in total
and per stretch of program text that ends in a workgroup barrier -- the stretch in front of a role's first barrier is that role's loads
and shared row softmax.  A record for profiles/small_step_lean_isa.txt, not a test.
The role named next to a stretch is a GUESS from its global loads and stores (output role: 6 or more stores; dQ role: 10 or more loads;
dC role: 8 or more), fitted to this one instantiation as compiled for that record: after a change to the kernel, check the labels
against the assembly before quoting them.

  python scripts/small_step_isa_count.py [--csrc dpr_scale_amd/csrc] [--hipcc /opt/rocm/bin/hipcc]
"""
import argparse
import collections
import os
import re
import subprocess
import tempfile

INST = '#include "step_small.h"\ntemplate __global__ void dprhot::step_small_kernel_out<1, 3, 32>(dprhot::StepSmallArgs);\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dpr_scale_amd", "csrc"))
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        src, asm = os.path.join(tmp, "inst.hip"), os.path.join(tmp, "inst.s")
        open(src, "w").write(INST)
        cmd = [a.hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I" + a.csrc, src, "-o", asm]
        print("# " + " ".join(cmd[:6]) + " -I<csrc> inst.hip -o inst.s")
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        body, on = [], False
        for ln in open(asm):
            if re.match(r"^_ZN6dprhot21step_small_kernel_out\S*:", ln):
                on = True
            elif on and ln.startswith(".Lfunc_end"):
                break
            elif on and ln.startswith("\t") and not ln.strip().startswith((".", ";")):
                body.append(ln.split()[0])
    c = collections.Counter(body)

    def n(pred):
        return sum(v for k, v in c.items() if pred(k))

    print(f"instructions {len(body)}  vector (v_*) {n(lambda k: k.startswith('v_'))}  v_cndmask {n(lambda k: 'cndmask' in k)}  "
          f"v_cmp {n(lambda k: k.startswith('v_cmp'))}  v_lshl_add_u64 {c['v_lshl_add_u64']}  ds_bpermute_b32 {c['ds_bpermute_b32']}  "
          f"v_permlane16_swap {n(lambda k: 'permlane16' in k)}  v_div_scale_f32 {c['v_div_scale_f32']}  s_barrier {c['s_barrier']}")
    seg = collections.Counter()
    for op in body:
        if op in ("s_barrier", "s_endpgm"):
            role = "output role" if seg["gstore"] >= 6 else "dQ role (with the C-tile loads of waves 8-15)" if seg["gload"] >= 10 else \
                   "dC role" if seg["gload"] >= 8 else "-"
            print(f"  up to {op:9s}: v_* {seg['v']:4d}  v_cndmask {seg['cnd']:3d}  v_cmp {seg['cmp']:3d}  global loads {seg['gload']:2d}  "
                  f"global stores {seg['gstore']:2d}  mfma {seg['mfma']}   {role if op == 's_barrier' and seg['mfma'] + seg['gload'] and seg['v'] > 100 else ''}")
            seg = collections.Counter()
            continue
        seg["v"] += op.startswith("v_")
        seg["cnd"] += "cndmask" in op
        seg["cmp"] += op.startswith("v_cmp")
        seg["gload"] += op.startswith("global_load")
        seg["gstore"] += op.startswith("global_store")
        seg["mfma"] += "mfma" in op


if __name__ == "__main__":
    main()
