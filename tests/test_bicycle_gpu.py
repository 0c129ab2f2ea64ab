"""Kinematic bicycle (built-in model 2, pmpc_amd/csrc/dynamics.hip) on the GPU: the linearisation kernels against the numpy
specification, its compact Jacobian records, the library's SCP loop on them — next to the unicycle, which has the same dimensions
and another record layout — and the public `solve(..., builtin_model="bicycle")`."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _random_point(M, N, seed=3):
    """A bicycle problem moved off its start iterate: random states, accelerations and steering angles inside the boxes."""
    from pmpc_amd import dynamics as dyn

    rng = np.random.default_rng(seed)
    prob = dyn.make_bicycle_problem(M=M, N=N)
    prob["x0"] = prob["x0"] + 0.3 * rng.standard_normal(prob["x0"].shape)
    prob["X_prev"] = prob["X_prev"] + 0.3 * rng.standard_normal(prob["X_prev"].shape)
    prob["U_prev"] = rng.uniform(-1.0, 1.0, prob["U_prev"].shape) * np.array([2.0, 0.5])
    return prob


def _abi(a):  # py layout (row, col) -> ABI layout (col, row)
    return np.ascontiguousarray(np.swapaxes(a, -1, -2))


@pytest.mark.parametrize("M,N", [(37, 11), (3, 1)])
def test_dense_linearisation_equals_the_numpy_specification(M, N):
    """k_linearize<Bicycle> against pmpc_amd.dynamics.bicycle at X_ = [x0, X_prev[:-1]]: rtol = atol = 1e-12 (every entry is a
    product of a few factors, nothing cancels); (3, 1) is the x0 branch alone in a partial block.  The fp32-output kernel writes the
    fp64 values rounded."""
    import torch

    from pmpc_amd.device import MODEL_BICYCLE, DeviceSolver, to_device_problem

    prob = _random_point(M, N)
    d = to_device_problem(prob)
    X_lin = np.concatenate([prob["x0"][:, None, :], prob["X_prev"][:, :-1]], 1)
    f_np, fx_np, fu_np = prob["f_fx_fu_fn"](X_lin, prob["U_prev"])
    s = DeviceSolver(0)
    try:
        f, fx, fu = s.linearize(MODEL_BICYCLE, d["x0"], d["X_prev"], d["U_prev"], d["params"])
        fx32 = torch.empty((M, N, 4, 4), dtype=torch.float32, device="cuda")
        fu32 = torch.empty((M, N, 2, 4), dtype=torch.float32, device="cuda")
        f2, _, _ = s.linearize(MODEL_BICYCLE, d["x0"], d["X_prev"], d["U_prev"], d["params"], fx=fx32, fu=fu32)
        s.sync()
        for name, got, ref in (("f", f, f_np), ("fx", fx, _abi(fx_np)), ("fu", fu, _abi(fu_np))):
            err = float(np.abs(got.cpu().numpy() - ref).max())
            print(f"bicycle ({M}, {N}) {name}: max abs difference to numpy {err:.3e}")
            np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-12, atol=1e-12)
        assert torch.equal(f2, f) and torch.equal(fx32, fx.float()) and torch.equal(fu32, fu.float())
    finally:
        s.close()


@pytest.mark.parametrize("M,N", [(37, 11), (3, 1), (130, 50)])
def test_expanded_bicycle_records_equal_the_dense_linearisation(M, N):
    """Both orientations of the records and the per-particle constant pool (1, dt), expanded by k_expand_jac, against
    pmpc_linearize_device: exact equality."""
    import torch

    from pmpc_amd.device import MODEL_BICYCLE, DeviceSolver, to_device_problem

    d = to_device_problem(_random_point(M, N))
    s = DeviceSolver(0)
    try:
        f, fx, fu = s.linearize(MODEL_BICYCLE, d["x0"], d["X_prev"], d["U_prev"], d["params"])
        fc, jc = s.linearize_compact(MODEL_BICYCLE, d["x0"], d["X_prev"], d["U_prev"], d["params"])
        s.sync()
        assert jc.numel() == M * N * 11 + M * 3  # (record and pool sizes of the model's picture with KS = 1)
        assert torch.equal(f, fc)
        for orient in (0, 1):
            ex, eu = s.expand_jac(MODEL_BICYCLE, jc, M, N, 4, 2, orient)
            s.sync()
            assert torch.equal(ex, fx), (orient, (ex != fx).nonzero()[:5])
            assert torch.equal(eu, fu), (orient, (eu != fu).nonzero()[:5])
    finally:
        s.close()


def _loop(s, mid, prob, steps, **extra):
    """`steps` iterations of the library's loop from the problem's start iterate, cold first iteration."""
    import torch

    from pmpc_amd.device import to_device_problem

    d = to_device_problem(prob)
    M, N, x = d["X_prev"].shape
    u = d["U_prev"].shape[-1]
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    common = dict(Q=d["Q"], R=d["R"], X_ref=d["X_ref"], U_ref=d["U_ref"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=prob["solver_settings"]["Nc"],
                  x0=d["x0"], lu=d["lu"], uu=d["uu"], symmetric_cost=True)
    Xa, Ua, Xb, Ub = d["X_prev"].clone(), d["U_prev"].clone(), mk(M, N, x), mk(M, N, u)
    bufs = [mk(M, N, x), mk(M, N, x, x), mk(M, N, u, x), mk(M, N, x), mk(M, N, x, x), mk(M, N, u, x)]
    s.lqp_solve(f=bufs[0].zero_(), fx=bufs[1].zero_(), fu=bufs[2].zero_(), X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, cold_start=True,
                **dict(common, lu=None, uu=None))  # (forget the warm-start memory of this shape, as tests/test_device_gpu.py does)
    res, infos, last, done = s.scp_loop(mid, d["params"], steps, f=bufs[0], fx=bufs[1], fu=bufs[2], f2=bufs[3], fx2=bufs[4], fu2=bufs[5],
                                        X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, first_cold=True, **common, **extra)
    s.sync()
    assert done == steps and all(i["status"] == 0 for i in infos), infos
    X, U = (Xb, Ub) if last else (Xa, Ua)
    return res.cpu().numpy(), X.clone(), U.clone(), infos


def test_lane_map_of_the_sweeps_follows_the_model_not_the_dimensions():
    """Unicycle, bicycle, unicycle again on ONE context (same (4, 2) sweep instantiations, two record layouts): every loop equals,
    bit for bit, the same loop on a context of its own; the warm solves ran active-set rounds, i.e. the sweeps read the records."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_BICYCLE, MODEL_UNICYCLE, DeviceSolver

    M, N, steps = 48, 20, 6
    cases = {"unicycle": (MODEL_UNICYCLE, dyn.make_unicycle_problem(M=M, N=N, Nc=1)), "bicycle": (MODEL_BICYCLE, dyn.make_bicycle_problem(M=M, N=N, Nc=1))}
    shared = DeviceSolver(0)
    try:
        for name in ("unicycle", "bicycle", "unicycle"):
            mid, prob = cases[name]
            got = _loop(shared, mid, prob, steps)
            fresh = DeviceSolver(0)
            try:
                ref = _loop(fresh, mid, prob, steps)
            finally:
                fresh.close()
            print(name, [(i["ipm_iters"], i["active_set_rounds"]) for i in got[3]])
            assert sum(i["active_set_rounds"] for i in got[3][1:]) > 0, got[3]
            assert got[3] == ref[3]
            np.testing.assert_array_equal(got[0], ref[0])
            assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
            assert np.isfinite(got[0]).all() and got[0][-1] < got[0][0]  # (and the loop is an SCP loop: its residual falls)
    finally:
        shared.close()


# width of the steering box and size of the lateral jump of the `tight` case (see the test's docstring)
TIGHT_WIDTH, TIGHT_JUMP = 0.05, 6.0

_CHILD = r"""
import json, sys
import numpy as np
import torch
from pmpc_amd import dynamics as dyn
from pmpc_amd.device import MODEL_BICYCLE, DeviceSolver, to_device_problem

case, out, width, jump = sys.argv[1], sys.argv[2], float(sys.argv[3]), float(sys.argv[4])
prob = dyn.make_bicycle_problem(M=48, N=50 if case == "tight" else 20, Nc=1)
if case == "tight":  # a lateral jump of the reference from stage 10 on that the steering box cannot follow
    prob["X_ref"][:, 10:, 1] += jump
    prob["u_u"][..., 1] = width
    prob["u_l"][..., 1] = -width
d = to_device_problem(prob)
M, N, x = d["X_prev"].shape
u = d["U_prev"].shape[-1]
mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
Xa, Ua, Xb, Ub = d["X_prev"].clone(), d["U_prev"].clone(), mk(M, N, x), mk(M, N, u)
s = DeviceSolver(0)
steps = 8
res, infos, last, done = s.scp_loop(MODEL_BICYCLE, d["params"], steps, f=mk(M, N, x), fx=mk(M, N, x, x), fu=mk(M, N, u, x), f2=mk(M, N, x),
                                    fx2=mk(M, N, x, x), fu2=mk(M, N, u, x), X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, first_cold=True, Q=d["Q"],
                                    R=d["R"], X_ref=d["X_ref"], U_ref=d["U_ref"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=1, x0=d["x0"],
                                    lu=d["lu"], uu=d["uu"], symmetric_cost=True)
s.sync()
X, U = (Xb, Ub) if last else (Xa, Ua)
np.savez(out, X=X.cpu().numpy(), U=U.cpu().numpy(), res=res.cpu().numpy(), done=done, infos=json.dumps(infos))
s.close()
"""


def _loop_in_child(case, compact, tmp_path, width=TIGHT_WIDTH, jump=TIGHT_JUMP):
    out = tmp_path / f"{case}_{compact}.npz"
    env = dict(os.environ, PMPC_LIN_COMPACT=str(compact))
    r = subprocess.run([sys.executable, "-c", _CHILD, case, str(out), repr(width), repr(jump)], cwd=str(ROOT), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    return z["X"], z["U"], z["res"], int(z["done"]), json.loads(str(z["infos"]))


@pytest.mark.parametrize("case", ["plain", "tight"])
def test_bicycle_loop_with_and_without_compact_records_walks_the_same_iterates(case, tmp_path):
    """PMPC_LIN_COMPACT=0 / 1 in two fresh processes, 8 iterations: identical iterates, residuals and per-iteration infos.
    `tight` (M 48, N 50): the lateral reference jumps by TIGHT_JUMP from stage 10 on and the steering box is +-TIGHT_WIDTH, so that warm
    solves leave the active-set rounds for the interior-point iteration and the records are expanded on the way (QpSolve::densify,
    k_expand_jac<Bicycle>).  Tuned on an MI355X: at N = 20 no width from 0.3 down to 0.002 and no jump from 3 to 100 made a warm solve hand
    over (2 - 5 rounds each); at N = 50, jump 6.0, width 0.05 the eight solves report (ipm_iters, rounds) = (0, 5), (23, 10), (12, 7), (0, 5),
    (0, 3), (0, 3), (0, 3), (0, 3): the warm solves of iterations 1 and 2 hand over."""
    X0, U0, r0, d0, i0 = _loop_in_child(case, 0, tmp_path)
    X1, U1, r1, d1, i1 = _loop_in_child(case, 1, tmp_path)
    print(case, [(i["ipm_iters"], i["active_set_rounds"]) for i in i1])
    assert d0 == d1 == 8 and all(i["status"] == 0 for i in i1)
    assert i0 == i1
    np.testing.assert_array_equal(r0, r1)
    np.testing.assert_array_equal(X0, X1)
    np.testing.assert_array_equal(U0, U1)
    assert sum(i["active_set_rounds"] for i in i1[1:]) > 0  # the warm solves did run the rounds whose sweeps read the records
    if case == "tight":
        assert any(i["ipm_iters"] > 0 for i in i1[1:]), i1  # ... and at least one of them handed over to the interior-point iteration


@pytest.mark.parametrize("Nc", [0, 1, -1])
def test_library_loop_on_the_bicycle_equals_the_python_driven_loop(Nc):
    """pmpc_scp_loop_device against linearize -> lqp_solve -> residual -> swap driven from Python, 5 iterations: identical residuals
    and iterates (the bound of the unicycle / quadrotor version of this check in tests/test_device_gpu.py)."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_BICYCLE, DeviceSolver, to_device_problem

    M, N, steps = 40, 12, 5
    prob = dyn.make_bicycle_problem(M=M, N=N, Nc=Nc)
    d = to_device_problem(prob)
    common = dict(Q=d["Q"], R=d["R"], X_ref=d["X_ref"], U_ref=d["U_ref"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=Nc, x0=d["x0"], lu=d["lu"],
                  uu=d["uu"], symmetric_cost=True)
    s = DeviceSolver(0)
    try:
        Xa, Ua = d["X_prev"].clone(), d["U_prev"].clone()
        Xb, Ub = torch.empty_like(Xa), torch.empty_like(Ua)
        res_py = []
        for it in range(steps):
            f, fx, fu = s.linearize(MODEL_BICYCLE, d["x0"], Xa, Ua, d["params"])
            _, _, st = s.lqp_solve(f=f, fx=fx, fu=fu, X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, static_cons_bounds=True, prev_is_last_solution=it > 0,
                                   cold_start=it == 0, **common)
            assert st == 0
            res_py.append(float(s.scp_residual(Xb, Xa, Ub, Ua)[0].item()))
            Xa, Xb, Ua, Ub = Xb, Xa, Ub, Ua
    finally:
        s.close()
    # (a context of its own: with Nc = N the cold first solve runs interior-point iterations, and a first_cold loop — unlike
    #  cold_start — may start those from the iterate this shape left on the context)
    s = DeviceSolver(0)
    try:
        res, X_lib, U_lib, infos = _loop(s, MODEL_BICYCLE, prob, steps)
        print("Nc", Nc, "residuals", res, [(i["ipm_iters"], i["active_set_rounds"]) for i in infos])
        np.testing.assert_array_equal(res, np.array(res_py))
        assert torch.equal(X_lib, Xa) and torch.equal(U_lib, Ua)
    finally:
        s.close()


def test_library_loop_on_the_bicycle_drives_the_cone_objective():
    """The same with PMPC_CONE_OBJECTIVE (the reference's default solver path as the sub-problem), M 16, N 10: the library's loop
    against linearize -> lcone_solve -> residual -> swap, a fresh context each.  Bound: that of the existing unicycle version of THIS
    check, tests/test_cone_ties_gpu.py::test_library_scp_loop_drives_the_cone_objective (residuals rtol 1e-6 / atol 1e-9, iterates atol
    1e-6) — the two loops reach the first, cold solve's optimum through different launch sequences (1 round / 6 factorisations in the
    library's loop, 4 / 10 from Python), so bit-for-bit equality, the bound of the QP version above, is not what the cone path gives for
    any model.  Measured on an MI355X: bicycle max |d residual| 4.4e-16, max |dX| 8.9e-16, max |dU| 1.1e-15 (the unicycle at this
    shape: 1.4e-7, 2.2e-7, 1.7e-6)."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_BICYCLE, DeviceSolver, to_device_problem

    M, N, steps = 16, 10, 5
    prob = dyn.make_bicycle_problem(M=M, N=N, Nc=1)
    d = to_device_problem(prob)
    common = dict(Q=d["Q"], R=d["R"], X_ref=d["X_ref"], U_ref=d["U_ref"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=1, x0=d["x0"], lu=d["lu"],
                  uu=d["uu"], symmetric_cost=True)
    s = DeviceSolver(0)
    try:
        Xa, Ua = d["X_prev"].clone(), d["U_prev"].clone()
        Xb, Ub = torch.empty_like(Xa), torch.empty_like(Ua)
        res_py = []
        for it in range(steps):
            f, fx, fu = s.linearize(MODEL_BICYCLE, d["x0"], Xa, Ua, d["params"])
            _, _, st = s.lcone_solve(f=f, fx=fx, fu=fu, X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, static_cons_bounds=True, prev_is_last_solution=it > 0,
                                     cold_start=it == 0, **common)
            assert st == 0, (it, s.last_info)
            res_py.append(float(s.scp_residual(Xb, Xa, Ub, Ua)[0].item()))
            Xa, Xb, Ua, Ub = Xb, Xa, Ub, Ua
    finally:
        s.close()
    s = DeviceSolver(0)
    try:
        res, X_lib, U_lib, _ = _loop(s, MODEL_BICYCLE, prob, steps, cone_objective=True)
    finally:
        s.close()
    print("cone objective: residuals", res, "python-driven", res_py, "max |dX|", float((X_lib - Xa).abs().max()), "max |dU|", float((U_lib - Ua).abs().max()))
    np.testing.assert_allclose(res, np.array(res_py), rtol=1e-6, atol=1e-9)
    assert torch.allclose(X_lib, Xa, rtol=0, atol=1e-6) and torch.allclose(U_lib, Ua, rtol=0, atol=1e-6)


def test_public_solve_with_the_builtin_bicycle_equals_the_host_loop():
    """`pmpc_amd.solve(None, ..., device="cuda", builtin_model="bicycle", params=...)` against the host loop on the numpy callable of the
    same problem: as many iterations (8, res_tol = 0), the same `hist` rows (rel 1e-6) and trajectories (1e-7)."""
    import pmpc_amd
    from pmpc_amd import dynamics as dyn

    M, N = 8, 15
    prob = dyn.make_bicycle_problem(M=M, N=N, Nc=1)
    kw = dict(X_ref=prob["X_ref"], U_ref=prob["U_ref"], X_prev=prob["X_prev"], U_prev=prob["U_prev"], u_l=prob["u_l"], u_u=prob["u_u"],
              reg_x=prob["reg_x"], reg_u=prob["reg_u"], max_it=8, res_tol=0.0, verbose=False, solver_settings=dict(solver="osqp", Nc=1))
    Xh, Uh, dh = pmpc_amd.solve(prob["f_fx_fu_fn"], prob["Q"], prob["R"], prob["x0"], **kw)
    Xd, Ud, dd = pmpc_amd.solve(None, prob["Q"], prob["R"], prob["x0"], device="cuda", builtin_model="bicycle", params=prob["params"], **kw)
    print("iterations", len(dh["hist"]), len(dd["hist"]), "max |dX|", np.abs(Xd - Xh).max(), "max |dU|", np.abs(Ud - Uh).max())
    for a, b in zip(dd["hist"], dh["hist"]):
        print(f"  resid {a['resid']:.12e} {b['resid']:.12e}  obj {a['obj']:.12e} {b['obj']:.12e}")
    assert Xd.shape == (M, N + 1, 4) and Ud.shape == (M, N, 2)
    assert len(dd["hist"]) == len(dh["hist"]) == 8
    for a, b in zip(dd["hist"], dh["hist"]):
        assert abs(a["resid"] - b["resid"]) <= 1e-6 * abs(b["resid"]) and abs(a["obj"] - b["obj"]) <= 1e-6 * abs(b["obj"]), (a, b)
    np.testing.assert_allclose(Xd, Xh, rtol=0, atol=1e-7)
    np.testing.assert_allclose(Ud, Uh, rtol=0, atol=1e-7)
    assert np.all(np.abs(Ud[..., 1]) <= 0.5 + 1e-9) and np.all(np.abs(Ud[..., 0]) <= 2.0 + 1e-9) and np.all(Ud[:, 0] == Ud[0:1, 0])


def test_unknown_model_ids_fail_alike():
    """3 is the first id that names no model: `linearize` fails for it exactly as for 5, and nothing is launched."""
    import torch

    from pmpc_amd.device import DeviceSolver, to_device_problem

    d = to_device_problem(_random_point(3, 2))
    s = DeviceSolver(0)
    try:
        raised = []
        for mid in (3, 5):
            f = torch.full((3, 2, 4), 7.0, dtype=torch.float64, device="cuda")
            with pytest.raises(RuntimeError) as e:
                s.linearize(mid, d["x0"], d["X_prev"], d["U_prev"], d["params"], f=f)
            s.sync()
            raised.append(str(e.value).replace(f"model {mid}", "model #"))
            assert bool((f == 7.0).all())
            with pytest.raises(RuntimeError):
                s.linearize_compact(mid, d["x0"], d["X_prev"], d["U_prev"], d["params"])
        assert raised[0] == raised[1]
    finally:
        s.close()
