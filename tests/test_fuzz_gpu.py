"""The fuzzers of tools/fuzz/ as a bounded `-m gpu` test: fixed seeds, a few hundred random problems each against the oracle
(dims, consensus horizons, boxes, slew, state boxes that bind, stage cones, warm-start sequences).  Each script prints a summary
line; the bar is the north star's 1e-6 on every case, and no failed solve that the oracle could solve."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _run(script, *argv, timeout=900):
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "fuzz" / script), *map(str, argv)], cwd=str(ROOT), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return r.stdout.strip().splitlines()


def test_fuzz_parity_qp_path():
    last = _run("fuzz_parity.py", 11, 200)[-1]
    m = re.search(r"(\d+) cases, (\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(2)) == 0 and float(m.group(3)) <= 1e-6, last


def test_fuzz_parity_ragged_control_boxes():
    """Boxes drawn per entry — one-sided, pinned, excluding zero, different per particle on the consensus stages — where every other fuzzer
    draws +-b: QP path, slew and the hard cone objective."""
    last = _run("fuzz_parity.py", 111, 150, "ragged")[-1]
    m = re.search(r"(\d+) cases, (\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(1)) == 150 and int(m.group(2)) == 0 and float(m.group(3)) <= 1e-6, last


def test_fuzz_stage_cones():
    last = _run("fuzz_soc.py", 12, 120)[-1]
    m = re.search(r"(\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(1)) == 0 and float(m.group(2)) <= 1e-6, last


def test_fuzz_stage_cones_path_following_alone():
    """--path: cone_as = 0 and the draw widened to what only the path-following iteration serves (udim 1 and 5 .. 8, soc_q 4, uncompiled dims,
    undeclared symmetry, forced generic kernels); the script counts a case answered by another solver as a failure."""
    last = _run("fuzz_soc.py", 17, 10, "--path")[-1]
    m = re.search(r"(\d+) cases \((\d+) skipped\), (\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(1)) >= 7 and int(m.group(3)) == 0 and float(m.group(4)) <= 1e-6, last


def test_fuzz_warm_start_sequences():
    last = _run("fuzz_warm_as.py", 13, 60, 5)[-1]
    m = re.search(r"(\d+) sequences, (\d+) solves, (\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(3)) == 0 and float(m.group(4)) <= 1e-6, last


@pytest.mark.parametrize("mode", ["boxes", "cone"])
def test_fuzz_binding_state_boxes(mode):
    out = _run("fuzz_xbox.py", 60, 14, *(["cone"] if mode == "cone" else []))
    m = re.search(r"worst ([0-9.e+-]+)", out[-1])
    assert m and float(m.group(1)) <= 1e-6, out[-1]


def test_fuzz_state_rows_of_extra_cstrs():
    last = _run("fuzz_state_rows.py", 15, 50)[-1]
    m = re.search(r"(\d+) cases \((\d+) skipped\), (\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(3)) == 0 and int(m.group(2)) < 25 and float(m.group(4)) <= 1e-6, last


def test_fuzz_cone_objective_hard_and_smoothed():
    last = _run("fuzz_cone.py", 24, 40, 24, 5)[-1]  # (worst-k cases at M <= 5: the direct cone program is the slow part; the ties it found are tests/golden/worstk_ties.npz)
    m = re.search(r"(\d+) cases \((\d+) skipped\), (\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(3)) == 0 and int(m.group(2)) < 20 and float(m.group(4)) <= 1e-6, last


def test_fuzz_sharded_equals_one_rank():
    last = _run("fuzz_sharded.py", 31, 300)[-1]
    m = re.search(r"(\d+) cases \((\d+) skipped\), (\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(3)) == 0 and int(m.group(2)) < 60 and float(m.group(4)) <= 1e-8, last


def test_fuzz_sharded_smoothed_cone_objective_equals_one_rank():
    """Log-barrier / squareplus smoothing of the cone objective on 2 .. 4 mock ranks against one rank (the Newton iteration's host side runs on
    gathered per-particle data, identically on every rank)."""
    last = _run("fuzz_sharded.py", 61, 120, "smooth")[-1]
    m = re.search(r"(\d+) cases \((\d+) skipped\), (\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(3)) == 0 and int(m.group(2)) < 25 and float(m.group(4)) <= 1e-8, last


def test_fuzz_dense_consensus_systems():
    """17 .. 256 shared unknowns (the register-resident consensus factorisation and, at 256, the blocked one), held shared controls, cold and warm."""
    last = _run("fuzz_dense_cons.py", 71, 60)[-1]
    m = re.search(r"(\d+) cases \((\d+) with a shared control on its bound\), (\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(3)) == 0 and int(m.group(2)) >= 30 and float(m.group(4)) <= 1e-7, last


def test_fuzz_sequence_of_unrelated_problems_on_one_context():
    last = _run("fuzz_sequence.py", 41, 150)[-1]
    m = re.search(r"(\d+) calls \((\d+) skipped\), (\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(3)) == 0 and int(m.group(2)) < 30 and float(m.group(4)) <= 1e-6, last


def test_fuzz_state_rows_inside_the_cone_objective():
    last = _run("fuzz_state_rows_cone.py", 81, 24)[-1]
    m = re.search(r"(\d+) cases \((\d+) skipped\), (\d+) failures, worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(3)) == 0 and int(m.group(2)) < 15 and float(m.group(4)) <= 1e-6, last


def test_fuzz_library_scp_loop_against_python_driven_loop():
    last = _run("fuzz_scp_loop.py", 102, 150)[-1]
    m = re.search(r"(\d+) cases, (\d+) failures, worst difference ([0-9.e+-]+)", last)
    assert m and int(m.group(2)) == 0, last


def test_fuzz_freeze_of_the_shared_step_changes_no_answer():
    # (seed 7, sequence 36: a held shared control released in a late round while the free ones stand still — the ADVICE r04 case,
    #  4e-2 off with status 0 before the fix)
    last = _run("fuzz_freeze.py", 7, 45, 5)[-1]
    m = re.search(r"(\d+) solves, (\d+) failures, worst freeze on/off ([0-9.e+-]+), worst rel err ([0-9.e+-]+)", last)
    assert m and int(m.group(1)) > 150 and int(m.group(2)) == 0 and float(m.group(3)) <= 1e-7 and float(m.group(4)) <= 1e-6, last
