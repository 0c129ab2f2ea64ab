"""The discipline of the GPU tests that run their cases in a child process (tests/test_as_dims_gpu.py, tests/test_ipm_dims_gpu.py,
tests/test_dense_cons_gpu.py): one child, one time limit, no retry; a child that ends by a signal, at its time limit or with a HIP
error in its output fails the test, and nothing else is started."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

HIP_FAULT = ("illegal memory access", "HIP error", "hipError", "HSA_STATUS_ERROR", "Memory access fault")


def run_child(module, args, ok_token, timeout, env=None):
    """python -m `module` `args` from the repository root, with `env` added to the environment; the child must end with return code 0 and
    `ok_token` as the last thing it prints, and must have printed its worst error.  Returns its output."""
    cmd = [sys.executable, "-m", module, *args]
    try:
        r = subprocess.run(cmd, cwd=str(Path(__file__).resolve().parents[2]), env=dict(os.environ, **(env or {})), capture_output=True, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"the child was still running after {timeout} s\n" + out[-3000:])
    print(r.stdout)
    hip_fault = [w for w in HIP_FAULT if w in r.stderr or w in r.stdout]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or hip_fault:
        pytest.fail(f"the child ended with return code {r.returncode}" + (f" and {hip_fault[0]!r} in its output" if hip_fault else "") + "\n" + r.stdout[-3000:] + "\n" + r.stderr[-3000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith(ok_token), (r.returncode, r.stdout[-4000:], r.stderr[-3000:])
    assert "worst error" in r.stdout
    return r.stdout
