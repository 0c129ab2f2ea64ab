"""Control boxes that are not one number — per entry, one-sided (+-inf), pinned (lo == hi), excluding zero, different per particle on the
consensus stages — on every solver path against the oracle.  The cases, and the conditions that make each of them able to tell a wrong
kernel from a right one, are tests/support/ragged_boxes.py's; tests/test_ragged_boxes.py certifies them on the CPU.  Tolerances are the
project's: 1e-7 (tests/test_parity_gpu.py, same relative measures), 1e-6 for the cone objective, stage cones and the log barrier
(tests/test_cone_gpu.py), 1e-8 sharded against one rank (tests/test_fuzz_gpu.py).  Every test prints its errors and the worst of its path."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.support import ragged_boxes as rb
from tests.support.problems import abi_args

pytestmark = pytest.mark.gpu
TOL, TOL_CONE, TOL_SHARD = 1e-7, 1e-6, 1e-8
T = rb.TABLES
_worst = {}


def _check(path, label, X, U, Xo, Uo, tol, N, Nc):
    ex, eu = rb.errors(X, U, Xo, Uo)
    _worst[path] = max(_worst.get(path, 0.0), ex, eu)
    print(f"{path} {label}: errX {ex:.2e} errU {eu:.2e} tol {tol:.0e}; worst error {path}: {_worst[path]:.3e}", flush=True)
    assert ex <= tol and eu <= tol, (path, label, ex, eu, tol)
    rb.assert_shared_exactly(U, N, Nc)


def _ids(table):
    return [rb.case_id(c) for c in T[table]]


def _device(s, case, args, kw, entry="lqp_solve", **extra):
    """One solve through the device API; (X, U, status, info)."""
    import torch

    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    Tr = lambda a: dev(np.swapaxes(a, -1, -2))
    x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref = args
    opt = dict(f=dev(f), fx=Tr(fx), fu=Tr(fu), X_prev=dev(X_prev), U_prev=dev(U_prev), Q=Tr(Q), R=Tr(R), X_ref=dev(X_ref), U_ref=dev(U_ref),
               reg_x=kw["reg_x"], reg_u=kw["reg_u"], Nc=case[5], symmetric_cost=True)
    if "u_l" in kw:
        opt.update(lu=dev(kw["u_l"]), uu=dev(kw["u_u"]))
    if "slew_reg" in kw:
        opt["slew_reg"] = dev(kw["slew_reg"])
    if "slew_reg0" in kw:
        opt.update(slew_reg0=dev(kw["slew_reg0"]), slew_um1=dev(kw["slew_um1"]))
    opt.update({k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in extra.items()})
    X, U, status = getattr(s, entry)(**opt)
    s.sync()
    return X.cpu().numpy(), U.cpu().numpy(), status, dict(s.last_info)


# ---- a. QP path through the C ABI, cold then warm -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T["qp"], ids=_ids("qp"))
def test_qp_path_cold_and_warm(case):
    from pmpc_amd import backend

    ref = rb.reference("qp", case)
    for rep in ("cold", "warm"):  # c_lqp_solve keeps its context: the same problem again starts from the stored statuses and multipliers
        X, U = backend.lqp_solve(*abi_args(ref["args"], ref["kw"], case[5]))
        _check("qp", f"{rb.case_id(case)} {rep}", X, U, ref["Xo"], ref["Uo"], TOL, case[2], case[5])


# ---- b. interior-point path alone -------------------------------------------------------------------------------------------------
def test_interior_point_path_alone():
    """PMPC_POLISH_MU=0 (read once per process: a child): no active-set use, the Mehrotra iteration to mu = 1e-12 on per_entry, one_sided,
    upper_only and offset boxes, cold and warm, to 1e-7.  A pinned entry has no interior, and the iteration answers it all the same: parity
    to the same 1e-7 is asserted (measured 6e-15), and the next call on the context."""
    env = dict(os.environ, PMPC_POLISH_MU="0")
    r = subprocess.run([sys.executable, "-m", "tests.support.ragged_boxes", "ipm_only"], cwd=str(Path(__file__).resolve().parents[1]), env=env,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith(rb.IPM_OK), (r.stdout[-3000:], r.stderr[-3000:])


@pytest.mark.parametrize("case", T["tie"], ids=_ids("tie"))
def test_finish_of_the_interior_point_iteration_labels_pinned_entries_by_their_multiplier(case):
    """The only finite sides are pins, the cold rounds are off (option as_cold_rounds = 0): the interior-point iteration runs, and at its
    handover every boxed entry has both sides active — lower multiplier above lower slack AND upper above upper.  k_as_setup resolves that by
    the larger multiplier, which is the sign of the pin's multiplier; then the finish's first check finds nothing to release or to activate
    and its first round is accepted.  Labelled the other way round every pin has the wrong sign, is released, leaves its point and comes
    back: the same answer after at least three rounds.  So: parity, and exactly one round."""
    from pmpc_amd.device import DeviceSolver

    ref = rb.reference("tie", case)
    s = DeviceSolver(0)
    try:
        s.set_option("as_cold_rounds", 0)
        X, U, status, info = _device(s, case, ref["args"], ref["kw"], cold_start=True)
        print(f"tie {rb.case_id(case)}: fast_path {info['fast_path']} ipm {info['ipm_iters']} rounds {info['active_set_rounds']}", flush=True)
        assert status == 0 and info["ipm_iters"] > 0, info
        _check("tie", rb.case_id(case), X, U, ref["Xo"], ref["Uo"], TOL, case[2], case[5])
        assert info["active_set_rounds"] == 1, info
    finally:
        s.close()


# ---- c. slew, increment form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T["slew"], ids=_ids("slew"))
def test_slew_increment_form(case):
    """The control boxes of a slew problem restated in increments are STATE boxes of [x; u] (kernels_slew.hip, kernels_xbox.hip); its
    consensus stages take particle 0's (cons_lo / cons_hi of solve_slew_increment_form)."""
    from pmpc_amd.device import DeviceSolver

    ref = rb.reference("slew", case)
    s = DeviceSolver(0)
    try:
        for rep in ("cold", "warm"):
            X, U, status, info = _device(s, case, ref["args"], ref["kw"])
            assert status == 0 and info["fast_path"] == 1, info  # (the increment form, not the generic kernels)
            _check("slew", f"{rb.case_id(case)} {rep}", X, U, ref["Xo"], ref["Uo"], TOL, case[2], case[5])
    finally:
        s.close()


# ---- d. dense consensus system ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T["dense"], ids=_ids("dense"))
def test_dense_consensus_system_with_held_and_pinned_shared_controls(case):
    """A shared control held by particle 0's box is the 1e30 diagonal of k_cons_solve_reg; a pinned one is held on both sides."""
    from pmpc_amd import backend

    ref = rb.reference("dense", case)
    for rep in ("cold", "warm"):
        X, U = backend.lqp_solve(*abi_args(ref["args"], ref["kw"], case[5]))
        _check("dense", f"{rb.case_id(case)} {rep}", X, U, ref["Xo"], ref["Uo"], TOL, case[2], case[5])


# ---- e. cone objective --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T["cone"], ids=_ids("cone"))
def test_cone_objective_hard_boxes(case, oracle):
    from pmpc_amd import backend

    ref = rb.reference("cone", case)
    args, kw = ref["args"], ref["kw"]
    X, U = backend.lcone_solve(*abi_args(args, kw, case[5]), smooth_alpha=float("nan"), solver="ecos")
    _check("cone", rb.case_id(case), X, U, ref["Xo"], ref["Uo"], TOL_CONE, case[2], case[5])
    J = oracle.particle_costs_py(X, U, *args[4:], reg_x=kw["reg_x"], reg_u=kw["reg_u"])  # the value of the reference's objective
    want = oracle.cone_objective(ref["info"]["J"])
    assert abs(oracle.cone_objective(J) - want) <= 1e-8 * abs(want)


@pytest.mark.parametrize("case", T["barrier"], ids=_ids("barrier"))
def test_cone_objective_log_barrier(case):
    from pmpc_amd import backend

    ref = rb.reference("barrier", case)
    X, U = backend.lcone_solve(*abi_args(ref["args"], ref["kw"], case[5]), smooth_alpha=dict(case[8])["alpha"], solver="ecos")
    _check("barrier", rb.case_id(case), X, U, ref["Xo"], ref["Uo"], TOL_CONE, case[2], case[5])


def test_log_barrier_refuses_a_pinned_entry_and_recovers():
    """-log(hi - u) - log(u - lo) with lo == hi has no finite value anywhere: NaN outputs, and the next call on the context answers."""
    from pmpc_amd import backend

    pinned = next(c for c in T["cone"] if c[1:6] == rb.CONE_SHAPES[0] and c[6] == "pinned")
    ref = rb.reference("cone", pinned)
    X, U = backend.lcone_solve(*abi_args(ref["args"], ref["kw"], pinned[5]), smooth_alpha=10.0, solver="ecos")
    assert np.isnan(X).all() and np.isnan(U).all(), "a finite answer under the log barrier with a pinned entry"
    nxt = next(c for c in T["barrier"] if c[1:6] == rb.CONE_SHAPES[0] and c[6] == "per_entry")
    ref = rb.reference("barrier", nxt)
    X, U = backend.lcone_solve(*abi_args(ref["args"], ref["kw"], nxt[5]), smooth_alpha=10.0, solver="ecos")
    _check("barrier", rb.case_id(nxt) + " after the refusal", X, U, ref["Xo"], ref["Uo"], TOL_CONE, nxt[2], nxt[5])


# ---- f. stage cone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T["soc"], ids=_ids("soc"))
def test_stage_cone_next_to_ragged_boxes(case):
    from pmpc_amd.device import DeviceSolver

    ref = rb.reference("soc", case)
    c = rb.soc_cone(case[4], case[7])
    s = DeviceSolver(0)
    try:
        X, U, status, info = _device(s, case, ref["args"], ref["kw"], entry="lsoc_solve", soc_W=c["W"], soc_w0=c["w0"], soc_v=c["v"], soc_v0=c["v0"],
                                     soc_u_interior=c["u_interior"])
        assert status == 0, info
        _check("soc", rb.case_id(case), X, U, ref["Xo"], ref["Uo"], TOL_CONE, case[2], case[5])
    finally:
        s.close()


# ---- g. state boxes with one-sided sides ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T["xbox"], ids=_ids("xbox"))
def test_one_sided_state_boxes_next_to_ragged_control_boxes(case):
    from pmpc_amd import backend

    ref = rb.reference("xbox", case)
    kw = ref["kw"]
    for rep in ("cold", "warm"):
        X, U = backend.lqp_solve(*abi_args(ref["args"], kw, case[5]))
        _check("xbox", f"{rb.case_id(case)} {rep}", X, U, ref["Xo"], ref["Uo"], TOL, case[2], case[5])
        assert np.all(X >= kw["x_l"] - 1e-8) and np.all(X <= kw["x_u"] + 1e-8)


# ---- h. sharded -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T["shard"] + T["shard_cone"], ids=_ids("shard") + _ids("shard_cone"))
def test_sharded_equals_one_rank_and_the_oracle(case):
    """Rank 0's boxes of the consensus stages are broadcast: a particle of ANOTHER rank whose own box the shared optimum violates (the
    CPU gate's condition) shows a rank that kept its own."""
    from tests.test_multirank_gpu import _solve_sharded

    cone = case[0] == "cone"
    ref = rb.reference("shard_cone" if cone else "shard", case)
    world, Nc, N = dict(case[8])["world"], case[5], case[2]
    X1, U1, _ = _solve_sharded(ref["args"], ref["kw"], Nc, 1, cone=cone)
    Xw, Uw, infos = _solve_sharded(ref["args"], ref["kw"], Nc, world, repeats=2, cone=cone)  # (the second solve: warm, static_cons_bounds)
    tol = TOL_CONE if cone else TOL
    _check("shard", f"{rb.case_id(case)} one rank", X1, U1, ref["Xo"], ref["Uo"], tol, N, Nc)
    _check("shard", f"{rb.case_id(case)} {world} ranks", Xw, Uw, ref["Xo"], ref["Uo"], tol, N, Nc)  # (shared controls bitwise equal across ranks)
    _check("shard-vs-1", rb.case_id(case), Xw, Uw, X1, U1, TOL_SHARD, N, Nc)


# ---- i. one context, the kinds in sequence --------------------------------------------------------------------------------------------
def test_one_context_meets_every_kind_in_sequence():
    """The warm state (statuses and multipliers per side, solver_qp.hip) of each call meets the next call's boxes: a side that is gone, a
    box that became a point, no boxes, boxes that exclude the previous answer, an empty box (NaN outputs, as
    test_empty_box_fails_like_the_reference requires), and the consensus boxes' cached working copy (static_cons_bounds) before and after
    particle 0's box changed in place."""
    import torch

    from pmpc_amd.device import DeviceSolver

    args, base, steps = rb.sequence()
    M, N, Nc = rb.SEQ["M"], rb.SEQ["N"], rb.SEQ["Nc"]
    case = (None,) * 5 + (Nc,)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    s = DeviceSolver(0)
    try:
        lu = uu = None
        for st in steps:
            name = st["name"]
            extra = {}
            if name in ("static_1", "static_2"):  # the SAME tensors as the per_entry step, untouched
                extra = dict(lu=lu, uu=uu, static_cons_bounds=True)
            elif name == "particle_0_moved":  # ... changed in place, flag off
                lu.copy_(dev(st["lo"]))
                uu.copy_(dev(st["hi"]))
                extra = dict(lu=lu, uu=uu)
            elif st["lo"] is not None:
                lu, uu = dev(st["lo"]), dev(st["hi"])
                extra = dict(lu=lu, uu=uu)
            X, U, status, info = _device(s, case, args, base, **extra)
            if st["Xo"] is None:
                print(f"sequence {name}: status {status}", flush=True)
                assert status != 0 and np.isnan(X).all() and np.isnan(U).all(), (name, status)
                continue
            assert status == 0, (name, info)
            _check("sequence", name, X, U, st["Xo"], st["Uo"], TOL, N, Nc)
    finally:
        s.close()


# ---- j. sentinels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["one_nan_in_u_l", "all_infinite"])
def test_sentinels_switch_the_control_boxes_off(how, oracle):
    """One NaN in a single entry of u_l alone switches ALL control boxes off (c_interface.jl:60); -inf / +inf everywhere bound nothing."""
    from pmpc_amd import backend

    case = T["qp"][0]
    ref = rb.reference("qp", case)
    args, kw, Nc = ref["args"], dict(ref["kw"]), case[5]
    Xo, Uo = oracle.lqp_solve_py(*args, Nc=Nc, reg_x=kw["reg_x"], reg_u=kw["reg_u"])
    assert rb.rel(Uo, ref["Uo"]) > 1e-3  # (the boxes mattered)
    if how == "one_nan_in_u_l":
        kw["u_l"] = kw["u_l"].copy()
        kw["u_l"][2, 3, 1] = np.nan
    else:
        kw["u_l"], kw["u_u"] = np.full_like(kw["u_l"], -np.inf), np.full_like(kw["u_u"], np.inf)
    X, U = backend.lqp_solve(*abi_args(args, kw, Nc))
    _check("sentinel", how, X, U, Xo, Uo, TOL, case[2], Nc)
