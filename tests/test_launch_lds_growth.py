"""A kernel whose dynamic-LDS request grows within one process (csrc/dprhot.hip: launch<Kern>).  The launch helper keeps, per kernel
instantiation and device, the largest size it has raised hipFuncAttributeMaxDynamicSharedMemorySize to, and raises it again when a
larger request follows a smaller one.  A helper that raised the limit only once would make the second call below return DPRHOT_E_HIP.

The batch-32 step at 32 x 320 x 768, then 32 x 512 x 768, then 32 x 320 x 768 again: fwd_plan gives both column counts three slabs
(256-deep K chunks of d = 768) and 256 < ncp <= 512, so both run the SAME instantiation -- step_small_kernel_out<CPT = 2, NS = 3,
QTW = 32> at the default small_step_roles, step_small_kernel<2, 16, 3, 1> at 0 -- with 52,480 then 73,984 bytes of LDS
(step_roles_lds) and 54,528 then 76,032 bytes (step_small_lds): all above the 48 KiB that need no attribute.

The high-water mark lives as long as the process, so the body runs in one fresh child process (this file run as a script)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, D, COLS = 32, 768, (320, 512, 320)


def _child():
    sys.path.insert(0, ROOT)
    import torch

    from dpr_scale_amd import _lib
    from test_small_step_out import NAMES, _inputs, _same, _step

    dev = torch.device("cuda", 0)
    default = _lib.get_option("small_step_roles")
    assert default != 0
    data = {Nc: _inputs(B, Nc, D, 0.05, dev, seed=Nc) for Nc in set(COLS)}
    out = {}
    for roles in (default, 0):
        _lib.set_option("small_step_roles", roles)
        # (_step raises unless the call returns DPRHOT_OK)
        out[roles] = [_step(B, Nc, D, 1.0, *data[Nc], dev) for Nc in COLS]
        _same(out[roles][2], out[roles][0], NAMES, f"small_step_roles={roles}, third call against first")
    for i, Nc in enumerate(COLS):
        _same(out[default][i], out[0][i], NAMES, f"call {i} ({Nc} columns), small_step_roles={default} against 0")
    print("lds growth ok")


@pytest.mark.gpu
def test_lds_request_grows_within_one_process():
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lds growth ok" in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


if __name__ == "__main__":
    _child()
