"""The dense consensus solves other than the register-resident one, and a second row of tiles in the condensing kernels, against the
oracle (cases and child process: tests/support/dense_cons.py).  tests/test_parity_gpu.py::test_dense_consensus_systems_of_every_panel_count
runs with the rounds on, which always re-factor — through k_cons_solve_reg; the vector-only solves (interior-point correctors only)
and the variants the launcher falls back to are what is here, each leg asserting from the launch counts (pmpc_fast_launches, kind 2)
that the variant it exists for ran.  Sizes: nc = 72 is the last the lds variant takes, 465 the last of the blocked one."""
import numpy as np
import pytest

from tests.support.child import run_child
from tests.support.dense_cons import CASES, OK_TOKEN, TOL, _rel, case_id, case_nc, case_problem, variant_for
from tests.test_slew_gpu import _solve

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_vector_only_consensus_solves_of_the_interior_point_correctors(case, oracle):
    """polish_mu = 0: the interior-point iteration alone, whose correctors issue vector-only dense solves — lds up to nc = 72, blocked
    up to 465, plain beyond; the condensing kernel is the grouped one, with a second row of tiles from nc = 65."""
    from pmpc_amd import _lib
    from pmpc_amd.device import DeviceSolver

    args, kw, Xo, Uo, k = case_problem(oracle, case)
    nc = case_nc(case)
    s = DeviceSolver(0)
    s.set_option("polish_mu", 0)
    for kind in ("cond", "cons"):
        _lib.fast_launches(kind, reset=True)
    X, U, status, info = _solve(s, args, kw, case[4])
    s.close()
    cond, cons = _lib.fast_launches("cond"), _lib.fast_launches("cons")
    ex, eu = _rel(X, Xo), _rel(U, Uo, 1.0)  # (the existing dense test's measure)
    print(f"nc {nc} ipm {info['ipm_iters']} errX {ex:.2e} errU {eu:.2e} cond {cond} cons (code: count) {dict((c, n) for c, n in enumerate(cons) if n)}")
    assert status == 0 and info["fast_path"] == 1 and info["active_set_rounds"] == 0 and info["ipm_iters"] > 0, info
    assert ex <= TOL and eu <= TOL, (ex, eu, info)
    assert np.all(U[:, :k] == U[0:1, :k])
    assert cons[_lib.cons_solve_code(variant_for(nc), False)] > 0, (variant_for(nc), cons)
    assert cond[1] > 0 and cond[0] == 0, cond


def _child(leg, env, timeout):
    run_child("tests.support.dense_cons", [leg], OK_TOKEN, timeout, env=env)


def test_factorisations_without_the_register_resident_solve():
    """PMPC_CONS_REG=0, rounds on, cold then warm: factorisations through lds (nc <= 72), blocked (73 .. 465) and plain (468).
    One child (the switch is read once per process), time limit 120 s: the oracle's share is about a second, 22 small device solves."""
    _child("reg_off", {"PMPC_CONS_REG": "0"}, 120)


def test_factorisations_where_neither_lds_variant_serves():
    """PMPC_CONS_REG=0 PMPC_CONS_LDS=0 — the order of fall-back where the runtime refuses the large LDS allocations: the blocked
    variant at nc = 72 and 18.  One child, time limit 120 s: three cases."""
    _child("lds_off", {"PMPC_CONS_REG": "0", "PMPC_CONS_LDS": "0"}, 120)
