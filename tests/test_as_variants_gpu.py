"""What each selectable instantiation of the active-set sweeps computes (pmpc_amd/csrc/kernels_as.hip, selection in as_variant.h),
at small shapes against the exact oracles.  The rest of the suite reaches the lean (MODE 0) and deep (MODE 1) factor sweeps only
above 1024 particles — one pair, by properties — and never the one-stage forward ring or SKIP on MODE 1: the three process-wide
knobs PMPC_AS_DEEP2_MAXM / PMPC_AS_DEEP_MAXM / PMPC_AS_FWD_PF2_MAXM put them in front of every particle count.
They are read once per process, so every (family, setting) is a child process: tests/support/as_variants.py, which holds the
cases, the tolerances and the coverage assertion (launch counts of pmpc_as_sweep_launches against the selectors' expected set).

One child at a time, no retry.  A child that ends by a signal, at its time limit or with a HIP error in its output stops the
module: every later test fails at once and starts nothing on the device."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests.support.as_variants import CHILDREN, KNOB_ENV, OK_TOKEN, SETTINGS

pytestmark = pytest.mark.gpu

# Time limit per child in seconds: the oracle's share measured in a dry run on the CPU (python -m tests.support.as_variants FAMILY
# --dry: plain 20 s, cone 44 s, state box 9 s, fp32 11 s, ragged 62 s) + start-up + the device solves (a few hundred of <= 16 particles by <= 10
# stages, milliseconds each), times a generous allowance for a slower or busier host.
TIMEOUT = {"plain": 300, "cone": 400, "xbox": 200, "f32": 250, "ragged": 500}

_HIP_FAULT = ("illegal memory access", "HIP error", "hipError", "HSA_STATUS_ERROR", "Memory access fault")
_stopped = None  # why no further child may start


@pytest.mark.parametrize("family,setting", CHILDREN, ids=[f"{f}-{s}" for f, s in CHILDREN])
def test_sweep_variants_match_the_oracle_and_are_the_ones_launched(family, setting):
    global _stopped
    if _stopped:
        pytest.fail(f"not started: {_stopped}")
    env = dict(os.environ)
    env.update({k: str(v) for k, v in zip(KNOB_ENV, SETTINGS[setting])})
    cmd = [sys.executable, "-m", "tests.support.as_variants", family]
    try:
        r = subprocess.run(cmd, cwd=str(Path(__file__).resolve().parents[1]), env=env, capture_output=True, text=True, timeout=TIMEOUT[family])
    except subprocess.TimeoutExpired as e:
        _stopped = f"the child {family}-{setting} was still running after {TIMEOUT[family]} s"
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(_stopped + "\n" + out[-3000:])
    print(r.stdout)  # (pytest -s / a failure report show each case, the knobs, the worst error and the launched variants)
    hip_fault = [w for w in _HIP_FAULT if w in r.stderr or w in r.stdout]  # (a device fault that reached Python as an exception: return code 1)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or hip_fault:
        _stopped = f"the child {family}-{setting} ended with return code {r.returncode}" + (f" and {hip_fault[0]!r} in its output" if hip_fault else "")
        pytest.fail(_stopped + "\n" + r.stdout[-3000:] + "\n" + r.stderr[-3000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith(OK_TOKEN), (r.returncode, r.stdout[-4000:], r.stderr[-3000:])
    assert f"knobs {tuple(SETTINGS[setting])}" in r.stdout and "worst error" in r.stdout
