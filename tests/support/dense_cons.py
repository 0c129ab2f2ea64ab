"""The dense consensus solves other than the register-resident one (pmpc_amd/csrc/kernels_generic.hip: k_cons_solve_lds up to nc = 72,
k_cons_solve_blocked up to nc = 465, the plain k_cons_solve beyond) — the cases of tests/test_dense_cons_gpu.py and the child process of
its legs that need PMPC_CONS_REG / PMPC_CONS_LDS (read once per process).

    PMPC_CONS_REG=0 python -m tests.support.dense_cons reg_off                  factorisations through lds (<= 72) and blocked (73 .. 465)
    PMPC_CONS_REG=0 PMPC_CONS_LDS=0 python -m tests.support.dense_cons lds_off  the order of fall-back where the runtime refuses the register-resident
                                                                                solve's 117 KB of LDS: blocked at small sizes too

Rounds on, cold then warm (the warm solve re-factors with the accepted set held), as tests/test_parity_gpu.py::
test_dense_consensus_systems_of_every_panel_count does; tolerance and conditions are that test's."""
from __future__ import annotations

import os
import sys

import numpy as np

from tests.support.problems import abi_args, rand_problem

OK_TOKEN = "DENSE_CONS_OK"
TOL = 1e-7
# (M, N, x, u, Nc, u-bound); nc = Nc u
CASES = [
    (2, 18, 4, 4, -1, 0.3), (2, 36, 4, 2, -1, 0.3),  # nc = 72: the last size the lds variant takes
    (2, 19, 8, 4, -1, 0.3), (3, 25, 5, 3, -1, 0.4),  # nc = 76, 75: just past it — blocked
    (2, 40, 12, 4, -1, 0.4),                         # nc = 160
    # a second row of tiles in k_cond_fast / k_cond_fast_grouped (blockIdx.y > 0 needs nc > 64), one per udim
    (2, 66, 4, 1, 65, 0.5), (2, 34, 10, 2, 33, 0.3), (2, 23, 7, 3, 22, 0.4), (2, 18, 9, 4, 17, 0.4),
    (2, 116, 4, 4, -1, 0.3), (2, 117, 4, 4, -1, 0.3),  # nc = 464, 468: either side of the blocked variant's 64 KB — the second is k_cons_solve's
]
LDS_OFF_CASES = [CASES[0], CASES[1], (3, 9, 4, 2, -1, 0.3)]  # nc = 72, 72, 18
LDS_MAX, BLOCKED_MAX = 72, 465  # launch_cons_solve's arithmetic


def case_nc(case):
    M, N, x, u, Nc, bu = case
    return (N if Nc < 0 else Nc) * u


def case_id(case):
    return f"nc={case_nc(case)}-{case}"


def variant_for(nc, lds_on=True):
    """Which kernel launch_cons_solve gives a system the register-resident solve does not take."""
    if nc <= 16:
        return "plain"
    return "lds" if lds_on and nc <= LDS_MAX else ("blocked" if nc <= BLOCKED_MAX else "plain")


def case_problem(orc, case):
    """(args, kw, Xo, Uo, k) with a shared control on its bound (the 1e30 diagonal of the consensus system) and one free."""
    M, N, x, u, Nc, bu = case
    args, kw = rand_problem(np.random.default_rng(7000 + N * u + M), M, N, x, u, bu)
    Xo, Uo = orc.lqp_solve_py(*args, Nc=Nc, **kw)
    k = N if Nc < 0 else Nc
    on = np.abs(np.abs(Uo[0, :k]) - bu) <= 1e-9
    assert on.any() and not on.all(), ("no shared control on its bound, or none free", case, int(on.sum()), on.size)
    return args, kw, Xo, Uo, k


def _rel(a, b, floor=1e-300):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), floor)


def run(leg):
    from oracle import lqp_oracle as orc
    from pmpc_amd import _lib, backend

    assert os.environ.get("PMPC_CONS_REG") == "0" and (os.environ.get("PMPC_CONS_LDS") == "0") == (leg == "lds_off"), leg
    worst = 0.0
    for case in (LDS_OFF_CASES if leg == "lds_off" else CASES):
        args, kw, Xo, Uo, k = case_problem(orc, case)
        _lib.fast_launches("cons", reset=True)
        for rep in ("cold", "warm"):
            X, U = backend.lqp_solve(*abi_args(args, kw, case[4]))
            ex, eu = _rel(X, Xo), _rel(U, Uo, 1.0)
            print(f"case {case_id(case)} {rep} errX {ex:.2e} errU {eu:.2e}", flush=True)
            assert ex <= TOL and eu <= TOL, ("parity", case, rep, ex, eu)
            assert np.all(U[:, :k] == U[0:1, :k]), (case, rep)
            worst = max(worst, ex, eu)
        cons = _lib.fast_launches("cons")
        want = variant_for(case_nc(case), lds_on=leg != "lds_off")
        print(f"  launches (code: count) {dict((c, n) for c, n in enumerate(cons) if n)}; factorisations expected in {want}", flush=True)
        assert cons[_lib.cons_solve_code(want, True)] > 0, ("no factorisation in the expected variant", case, want, cons)
        assert cons[_lib.cons_solve_code("reg12", True)] == 0 and cons[_lib.cons_solve_code("reg17", True)] == 0, (case, cons)
        if leg == "lds_off":
            assert cons[_lib.cons_solve_code("lds", True)] == 0 and cons[_lib.cons_solve_code("lds", False)] == 0, (case, cons)
    print(f"worst error {leg}: {worst:.3e}", flush=True)


if __name__ == "__main__":
    run(sys.argv[1])
    print(OK_TOKEN, flush=True)
