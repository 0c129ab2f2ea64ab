"""The stage-cone PATH-FOLLOWING iteration of `pmpc_lsoc_solve_device` where it alone answers (kernels_soc.hip, QpSolve::soc_interior_point and
run_cone_dispatch, the full u x u Hessian blocks `LQArgs.du_full` in the Riccati sweeps) against `oracle.lsoc_solve_py`, the primal barrier method
on the sparse joint KKT system.  Since the active-set rounds (kernels_cone.hip, option cone_as) answer every compiled symmetric case first, each
test here says through `last_info` which solver ran.  Ids: <k_soc_* instance>-<sweep family>-<Nc class>-<shape>-<boxes>; `socRT`: the run-time-size
instance (UDT = 0).  Bound: the north star's 1e-6 (tests/support/soc_path.py); the worst measured errors per leg are in CHANGELOG.md (1.6e-10
with the centring steps that end the iteration; 5e-7 on the cones with q >= 2 before them)."""
import numpy as np
import pytest

from tests.support import soc_path as sp
from tests.support.soc_path import TOL, Case

pytestmark = pytest.mark.gpu


def _solver(**options):
    from pmpc_amd.device import DeviceSolver

    s = DeviceSolver(0)
    for key, val in options.items():
        s.set_option(key, val)
    return s


def _assert_path_following_alone(info, fast):
    assert info["ipm_iters"] > 0 and info["active_set_rounds"] == 0 and info["fast_path"] == (1 if fast else 0), info


# ---- 1. path following alone on the MFMA sweeps: cone_as = 0, symmetric cost, compiled (xdim, udim) ---------------------------------------------
# Case(M, N, x, u, Nc, box, q, v0, seed, one_sided): every compiled (u, q) instance, the run-time-size one on (3,3,3) (4,2,2) (4,1,1) (12,4,4),
# Nc in {0, 1, 3, -1}, no boxes, one-sided boxes, and 48 x 11 = 528 (particle, stage) pairs = two full blocks of 256 and a ragged third
FAST_CASES = [
    Case(3, 6, 12, 4, 3, 0.8, 2, 0.3),
    Case(4, 7, 12, 4, 1, 0.5, 3, 0.3),
    Case(4, 6, 8, 4, -1, 0.6, 1, 0.3),
    Case(4, 7, 6, 3, 0, 0.6, 2, 0.3),
    Case(5, 8, 5, 3, 1, None, 1, 0.3),
    Case(3, 8, 4, 2, -1, 0.6, 1, 0.15),
    Case(5, 6, 3, 3, 1, 0.6, 3, 0.3),
    Case(6, 10, 4, 2, 3, 0.6, 2, 0.3, 0, True),
    Case(3, 6, 4, 1, 1, 0.3, 1, 0.3),
    Case(4, 6, 12, 4, 0, 0.8, 4, 0.3),
    Case(48, 11, 4, 2, 1, 0.6, 1, 0.3),
]


@pytest.mark.parametrize("case", FAST_CASES, ids=[c.id("fast") for c in FAST_CASES])
def test_path_following_alone_on_the_fast_sweeps(case, oracle):
    args, kw, soc, Xo, Uo = sp.reference(oracle, case)
    sp.assert_input_conditions(Uo, kw, case.Nc, soc)
    s = _solver(cone_as=0)
    try:
        X, U, status, info = sp.device_solve(s, args, kw, case.Nc, soc)
    finally:
        s.close()
    assert status == 0
    _assert_path_following_alone(info, fast=True)
    sp.assert_matches(X, U, Xo, Uo, kw, case.Nc, soc, label=f"leg 1 {case.id('fast')}")


# ---- 2. path following on the generic kernels (du_full in k_bwd_generic and its consensus rows): no option set, the rounds cannot run there ------
# how the solve gets there: "forced" = force_generic on a compiled pair, "undeclared" = the cost is not declared symmetric, "dims" = (xdim, udim) is
# not a compiled pair; udim 5 and 8 with q = 4: the run-time-size instance at its array limits UMAX = 8, QMAX = 4
GENERIC_CASES = [
    (Case(3, 6, 12, 4, 1, 0.8, 2, 0.3, 1), "forced"),
    (Case(4, 7, 4, 2, 2, 0.6, 1, 0.3, 1), "undeclared"),
    (Case(4, 6, 7, 2, 0, 0.6, 1, 0.3, 1), "dims"),
    (Case(3, 6, 13, 2, -1, 0.4, 2, 0.3, 1), "dims"),
    (Case(2, 5, 6, 5, 1, 0.4, 4, 0.5, 1), "dims"),
    (Case(2, 4, 8, 8, -1, 0.3, 4, 0.5, 1), "dims"),
]


@pytest.mark.parametrize("case,how", GENERIC_CASES, ids=[c.id("generic:" + how) for c, how in GENERIC_CASES])
def test_path_following_on_the_generic_sweeps(case, how, oracle):
    args, kw, soc, Xo, Uo = sp.reference(oracle, case)
    sp.assert_input_conditions(Uo, kw, case.Nc, soc)
    s = _solver(warn_slow_path=0)
    try:
        assert s.get_option("cone_as") == 1.0  # (the default stands: it is the path, not the switch, that keeps the rounds out)
        X, U, status, info = sp.device_solve(s, args, kw, case.Nc, soc, symmetric_cost=how != "undeclared", force_generic=how == "forced")
    finally:
        s.close()
    assert status == 0
    _assert_path_following_alone(info, fast=False)
    sp.assert_matches(X, U, Xo, Uo, kw, case.Nc, soc, label=f"leg 2 {case.id('generic:' + how)}")


# ---- 3. path following, then the rounds from its iterate (mode 5 of run_cone_dispatch) -------------------------------------------------------------
MODE5_CASES = [Case(4, 7, 12, 4, 1, 0.5, 3, 0.3), Case(3, 8, 4, 2, -1, 0.6, 1, 0.15), Case(5, 6, 3, 3, 1, 0.6, 2, 0.3, 2)]


def _perturbed(args, seed, rel=0.02):
    """A related problem: f, X_prev, U_prev moved by about 2 % of their spread."""
    rng = np.random.default_rng(seed)
    return tuple(a + rel * np.std(a) * rng.standard_normal(a.shape) if k in (1, 4, 5) else a for k, a in enumerate(args))


@pytest.mark.parametrize("case", MODE5_CASES, ids=[c.id("fast:then-rounds") for c in MODE5_CASES])
def test_rounds_started_from_the_path_following_iterate(case, oracle):
    """cone_cold_rounds = 0 and a cold start: the path-following iterate names the box statuses and cone multipliers of one more attempt of the
    rounds, which replace its last digits (mu == 0) and leave set and multipliers behind — a second, related solve is answered by the warm
    rounds alone."""
    args, kw, soc, Xo, Uo = sp.reference(oracle, case)
    sp.assert_input_conditions(Uo, kw, case.Nc, soc)
    args2 = _perturbed(args, 600 + case.x)
    Xo2, Uo2 = sp.oracle_solve(oracle, args2, kw, case.Nc, soc)
    sp.assert_input_conditions(Uo2, kw, case.Nc, soc)
    s = _solver(cone_as=1, cone_cold_rounds=0)
    try:
        X, U, status, info = sp.device_solve(s, args, kw, case.Nc, soc, cold_start=True)
        X2, U2, status2, info2 = sp.device_solve(s, args2, kw, case.Nc, soc, cold_start=False)
    finally:
        s.close()
    assert status == 0 and info["fast_path"] == 1 and info["ipm_iters"] > 0 and info["active_set_rounds"] >= 1 and info["mu"] == 0.0, info
    sp.assert_matches(X, U, Xo, Uo, kw, case.Nc, soc, label=f"leg 3 {case.id('then-rounds')}")
    assert status2 == 0 and info2["ipm_iters"] == 0 and info2["active_set_rounds"] >= 1, info2
    sp.assert_matches(X2, U2, Xo2, Uo2, kw, case.Nc, soc, label=f"leg 3 warm rounds {case.id('then-rounds')}")


# ---- 4. the iteration's own warm start (w.soc_key) ----------------------------------------------------------------------------------------------
def test_warm_start_of_the_path_following_iteration(oracle):
    """One context, cone_as = 0, five solves: cold; a related problem from the remembered early iterate (no more Newton steps than its cold
    solve); boxes tightened so that the remembered controls fall outside them (rejected by the prepare pass: exactly the cold solve's counts);
    warm again; warm_start = 0."""
    case = Case(5, 8, 4, 2, 1, 0.6, 1, 0.1, 3)
    args, kw, soc, Xo, Uo = sp.reference(oracle, case)
    sp.assert_input_conditions(Uo, kw, case.Nc, soc)
    args2 = _perturbed(args, 77)
    Xo2, Uo2 = sp.oracle_solve(oracle, args2, kw, case.Nc, soc)
    sp.assert_input_conditions(Uo2, kw, case.Nc, soc)
    kwT = dict(kw, u_l=-0.1 * np.ones_like(kw["u_l"]), u_u=0.1 * np.ones_like(kw["u_u"]))
    socT = dict(soc, u_interior=0.05 * np.eye(case.u)[0])  # (strictly inside the tighter boxes)
    XoT, UoT = sp.oracle_solve(oracle, args2, kwT, case.Nc, socT)
    sp.assert_input_conditions(UoT, kwT, case.Nc, socT)

    def check(s, a, k, c, ref, label, **flags):
        X, U, status, info = sp.device_solve(s, a, k, case.Nc, c, **flags)
        assert status == 0
        _assert_path_following_alone(info, fast=True)
        sp.assert_matches(X, U, *ref, k, case.Nc, c, label="leg 4 " + label)
        return info

    s, fresh = _solver(cone_as=0), _solver(cone_as=0)
    try:
        check(s, args, kw, soc, (Xo, Uo), "1 cold")
        warm = check(s, args2, kw, soc, (Xo2, Uo2), "2 warm, related problem")
        cold = check(fresh, args2, kw, soc, (Xo2, Uo2), "2 the same, cold", cold_start=True)
        assert warm["ipm_iters"] <= cold["ipm_iters"], (warm, cold)
        rejected = check(s, args2, kwT, socT, (XoT, UoT), "3 remembered controls outside the tighter boxes")
        coldT = check(fresh, args2, kwT, socT, (XoT, UoT), "3 the same, cold", cold_start=True)
        assert (rejected["ipm_iters"], rejected["structured_solves"]) == (coldT["ipm_iters"], coldT["structured_solves"]), (rejected, coldT)
        again = check(s, args2, kwT, socT, (XoT, UoT), "4 warm again")
        assert again["ipm_iters"] <= coldT["ipm_iters"], (again, coldT)
        s.set_option("warm_start", 0)
        off = check(s, args2, kwT, socT, (XoT, UoT), "5 warm_start = 0")
        assert off["ipm_iters"] == coldT["ipm_iters"], (off, coldT)
    finally:
        s.close()
        fresh.close()


# ---- 5. infeasible start: status 3, NaN outputs, and the context goes on ----------------------------------------------------------------------------
@pytest.mark.parametrize("case,fast", [(Case(3, 6, 4, 2, 1, 0.6, 1, 0.3, 4), True), (Case(3, 6, 7, 2, 1, 0.6, 1, 0.3, 4), False)],
                         ids=["soc2x1-fast-Nc1", "soc2x1-generic:dims-Nc1"])
def test_infeasible_start_returns_3_with_nan_outputs(case, fast, oracle):
    """soc_u_interior outside the cone, then exactly on a box side (inside the cone): status 3 of include/pmpc_abi.h with the failure convention
    of every solve (X_out, U_out filled with NaN); the next valid solve on the context matches the oracle."""
    args, kw, soc, Xo, Uo = sp.reference(oracle, case)
    sp.assert_input_conditions(Uo, kw, case.Nc, soc)
    outside = soc["u_interior"] + 0.5 * np.eye(case.u)[1]  # inside the boxes, |W u + w0| ~ 0.5 > v'u + v0 = 0.4
    on_side = np.array(soc["u_interior"], copy=True)
    on_side[0] = case.box                                  # the upper side of u_0; the cone holds there with room
    assert sp.cone_slack(outside, soc) < -1e-2 and np.all(np.abs(outside) < case.box) and sp.cone_slack(on_side, soc) > 1e-2
    s = _solver(cone_as=0, warn_slow_path=0)
    try:
        for bad in (outside, on_side):
            X, U, status, info = sp.device_solve(s, args, kw, case.Nc, soc, u_interior=bad)
            assert status == 3 and info["status"] == 3, (status, info)
            assert np.all(np.isnan(X)) and np.all(np.isnan(U))
        X, U, status, info = sp.device_solve(s, args, kw, case.Nc, soc)
    finally:
        s.close()
    assert status == 0
    _assert_path_following_alone(info, fast=fast)
    sp.assert_matches(X, U, Xo, Uo, kw, case.Nc, soc, label=f"leg 5 after two refused starts, fast {fast}")


# ---- 7. fp32-stored matrices: the widening leg (PMPC_NEEDS_F64) ------------------------------------------------------------------------------------
def test_path_following_on_fp32_stored_matrices(oracle):
    """float32 fx, fu, Q, R with cone_as = 0: the solve asks for widened copies and runs the same iteration on them — against the oracle on the
    fp32-ROUNDED data, so the bound stays the 1e-6 of the fp64 legs."""
    import torch

    case = Case(4, 7, 6, 3, 1, 0.6, 2, 0.3, 5)
    args, kw, soc = sp.make(case)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    args = tuple(r32(a) if k in (2, 3, 6, 7) else a for k, a in enumerate(args))
    Xo, Uo = sp.oracle_solve(oracle, args, kw, case.Nc, soc)
    sp.assert_input_conditions(Uo, kw, case.Nc, soc)
    s = _solver(cone_as=0)
    try:
        X, U, status, info = sp.device_solve(s, args, kw, case.Nc, soc, dtype=torch.float32)
    finally:
        s.close()
    assert status == 0
    _assert_path_following_alone(info, fast=True)
    sp.assert_matches(X, U, Xo, Uo, kw, case.Nc, soc, label="leg 7 fp32-stored matrices")
