"""Every (xdim, udim) pair of the active-set sweeps, at the smallest shapes that reach each body of the sweeps, against the exact
oracle: M = 3, N in {2, 9}, Nc in {1, 2}, a cold solve and a warm one under prev_is_last_solution between which controls are held
and released, with and without the SENS forward sweeps (tests/support/as_dims.py holds the cases and the assertions).  What a cut
of the sweeps' vector instructions can break shows here: the row masks of pairs with udim < 4, the padding selects of pairs with
xdim % 4 != 0, the MAIN body next to the general body, restarts at the checkpoint rungs 4 and 8.

One child process, one time limit, no retry; a child that ends by a signal, at its time limit or with a HIP error fails the test
and nothing else is started."""
import subprocess
import sys
from pathlib import Path

import pytest

from tests.support.as_dims import OK_TOKEN

pytestmark = pytest.mark.gpu

# seconds: the oracle's share is 4 s on the CPU (python -m tests.support.as_dims --dry) + one more oracle solve per warm solve, start-up,
# and 400 device solves of 3 particles by <= 9 stages, milliseconds each — times a generous allowance for a slower or busier host
TIMEOUT = 300
_HIP_FAULT = ("illegal memory access", "HIP error", "hipError", "HSA_STATUS_ERROR", "Memory access fault")


def test_every_pair_cold_and_warm_matches_the_oracle():
    cmd = [sys.executable, "-m", "tests.support.as_dims"]
    try:
        r = subprocess.run(cmd, cwd=str(Path(__file__).resolve().parents[1]), capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"the child was still running after {TIMEOUT} s\n" + out[-3000:])
    print(r.stdout)
    hip_fault = [w for w in _HIP_FAULT if w in r.stderr or w in r.stdout]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or hip_fault:
        pytest.fail(f"the child ended with return code {r.returncode}" + (f" and {hip_fault[0]!r} in its output" if hip_fault else "") + "\n" + r.stdout[-3000:] + "\n" + r.stderr[-3000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith(OK_TOKEN), (r.returncode, r.stdout[-4000:], r.stderr[-3000:])
    assert "worst error" in r.stdout
