"""Custom stage costs on the GPU (pmpc_amd.CustomCost; pmpc_amd/csrc/cost_jit.hip, cost_kernels.h): the runtime-compiled gradient
kernel against closed forms, the public device solve against the host loop, the library's loop against the Python-driven iterates,
models and costs side by side on one solver, `MPCController(builtin_cost=custom)`, the refusals, and a keep-out constraint next to it."""
import ctypes

import numpy as np
import pytest

from tests.support import custom_costs as cc
from tests.support import custom_models as cm

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-12, atol=1e-12)


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def solver():
    from pmpc_amd.device import DeviceSolver

    s = DeviceSolver(0)
    yield s
    s.close()


def _custom(name, P, **kw):
    return dict(kind="custom", cost=cc.make(name, **kw), params=P)


# ---- 1. the gradient kernel ---------------------------------------------------------------------------------------------------------
GRAD_NAMES = ["obstacles_u", "soft_speed"] + [f"generic_{x}_{u}" for x, u in cc.GENERIC_DIMS]
_costs = {}


def _cost(name, uses_u=True):
    """One CustomCost per (name, uses_u) for the module: compiled and loaded once."""
    if (name, uses_u) not in _costs:
        _costs[name, uses_u] = cc.make(name, uses_u=uses_u)
    return _costs[name, uses_u]


@pytest.mark.parametrize("M,N", [(1, 1), (5, 3), (37, 11)])
@pytest.mark.parametrize("name", GRAD_NAMES)
def test_gradient_kernel_equals_the_closed_forms(solver, name, M, N):
    """cx, cu and val of pmpc_jit_cost_grad against numpy at rtol = atol = 1e-12: one unit, a partial single block, several blocks with
    a partial last one (407 units: 6 full blocks of 64 and one of 23); guard words around the three outputs stay intact.  Then the
    same cost compiled with uses_u=False and cu=None: cx and val as before, nothing written past cx."""
    import torch

    from tests.support.keepout_loop import guarded, guards_intact

    e = cc.entry(name)
    x, u, cd = e["dims"]
    X, U, P = cc.rand_inputs(name, M, N, seed=1000 * M + N)
    val, cx, cu = e["np"](X, U, P)
    Xd, Ud, Pd = _dev(X), _dev(U), _dev(P)
    (wx, gx), (wu, gu), (wv, gv) = guarded((M, N, x)), guarded((M, N, u)), guarded((M, N))
    got = solver.custom_cost_grad(_cost(name), Xd, Ud, Pd, value=gv, cx=gx, cu=gu)
    solver.sync()
    assert got[0] is gx and got[1] is gu and got[2] is gv
    err = [float(np.abs(g.cpu().numpy() - w).max()) for g, w in ((gx, cx), (gu, cu), (gv, val))]
    print(f"{name} ({M}, {N}): max |cx - numpy| {err[0]:.3e}, |cu - numpy| {err[1]:.3e}, |val - numpy| {err[2]:.3e}; max |cx| {np.abs(cx).max():.3e} |cu| {np.abs(cu).max():.3e}")
    np.testing.assert_allclose(gx.cpu().numpy(), cx, **TOL)
    np.testing.assert_allclose(gu.cpu().numpy(), cu, **TOL)
    np.testing.assert_allclose(gv.cpu().numpy(), val, **TOL)
    assert guards_intact(wx) and guards_intact(wu) and guards_intact(wv)
    assert torch.equal(Xd, _dev(X)) and torch.equal(Ud, _dev(U)) and torch.equal(Pd, _dev(P))  # (the inputs are not written)
    # without the value: the same gradients
    cx2, cu2 = solver.custom_cost_grad(_cost(name), Xd, Ud, Pd)
    assert torch.equal(cx2, gx) and torch.equal(cu2, gu)
    # uses_u=False: no cu
    (wx, gx), (wv, gv) = guarded((M, N, x)), guarded((M, N))
    got = solver.custom_cost_grad(_cost(name, False), Xd, Ud, Pd, value=gv, cx=gx)
    solver.sync()
    assert got[1] is None
    np.testing.assert_allclose(gx.cpu().numpy(), cx, **TOL)
    np.testing.assert_allclose(gv.cpu().numpy(), val, **TOL)
    assert guards_intact(wx) and guards_intact(wv)


def test_gradient_entry_refusals(solver):
    """Status 2 and nothing launched: an id that is no loaded cost, null cx, null cu for a cost that uses u."""
    import torch

    X, U, P = cc.rand_inputs("soft_speed", 3, 4)
    Xd, Ud, Pd = _dev(X), _dev(U), _dev(P)
    cid = solver.load_cost(_cost("soft_speed"))
    cx, cu = torch.full((3, 4, 4), 7.0, dtype=torch.float64, device="cuda"), torch.full((3, 4, 2), 7.0, dtype=torch.float64, device="cuda")
    call = lambda i, a, b: solver.lib.pmpc_custom_cost_grad_device(solver.h, i, 4, 3, Xd.data_ptr(), Ud.data_ptr(), Pd.data_ptr(), a, b, None)
    assert call(cid + 1000, cx.data_ptr(), cu.data_ptr()) == 2
    assert call(cid, None, cu.data_ptr()) == 2
    assert call(cid, cx.data_ptr(), None) == 2
    solver.sync()
    assert bool((cx == 7.0).all()) and bool((cu == 7.0).all())
    assert call(cid, cx.data_ptr(), cu.data_ptr()) == 0
    solver.sync()
    with pytest.raises(ValueError, match="params must be"):
        solver.custom_cost_grad(_cost("soft_speed"), Xd, Ud, Pd[:, :3].contiguous())


# ---- 2. public solve ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lane_change():
    """The lane-change case of tests/test_lin_cost_gpu.py: bicycle M 8, N 15, 8 iterations, res_tol = 0."""
    from pmpc_amd import dynamics as dyn

    prob = dyn.make_bicycle_problem(M=8, N=15, Nc=1)
    kw = dict(X_ref=prob["X_ref"], U_ref=prob["U_ref"], X_prev=prob["X_prev"], U_prev=prob["U_prev"], u_l=prob["u_l"], u_u=prob["u_u"],
              reg_x=prob["reg_x"], reg_u=prob["reg_u"], max_it=8, res_tol=0.0, verbose=False, solver_settings=dict(solver="osqp", Nc=1))
    return prob, kw


@pytest.mark.parametrize("cw", [0.0, 0.05])
def test_public_solve_with_a_custom_cost_equals_the_host_loop(lane_change, cw):
    """`solve(None, ..., device="cuda", builtin_model="bicycle", builtin_cost=dict(kind="custom", ...))` with obstacles_u against the
    host loop with the numpy closed form as `lin_cost_fn`: 8 iterations, `hist` rows rel 1e-6, trajectories atol 1e-7 (the bounds of
    tests/test_lin_cost_gpu.py).  cw = 0 (compiled with uses_u=False) is the built-in obstacle cost: the same bounds against
    `builtin_cost=OBSTACLES`.  cw = 0.05 is that file's callable case: U_ref is shifted through R."""
    import pmpc_amd
    from tests.test_lin_cost_gpu import CU_WEIGHT, OBSTACLES

    assert cw in (0.0, CU_WEIGHT)
    prob, kw = lane_change
    P = cc.obstacle_params(OBSTACLES, 8, cw)

    def host_fn(X_prev, U_prev, problems):
        _, cx, cu = cc.obstacles_u_np(X_prev, U_prev, P)
        return cx, (cu if cw else None)

    Xh, Uh, dh = pmpc_amd.solve(prob["f_fx_fu_fn"], prob["Q"], prob["R"], prob["x0"], lin_cost_fn=host_fn, **kw)
    device = dict(device="cuda", builtin_model="bicycle", params=prob["params"])
    Xd, Ud, dd = pmpc_amd.solve(None, prob["Q"], prob["R"], prob["x0"], builtin_cost=_custom("obstacles_u", P, uses_u=bool(cw)), **device, **kw)
    legs = [("host loop", Xh, Uh, dh)]
    if not cw:
        legs.append(("built-in obstacle cost", *pmpc_amd.solve(None, prob["Q"], prob["R"], prob["x0"], builtin_cost=OBSTACLES, **device, **kw)))
    for what, Xo, Uo, do in legs:
        print(f"cw {cw} against the {what}: iterations {len(dd['hist'])} {len(do['hist'])}, max |dX| {np.abs(Xd - Xo).max():.3e} max |dU| {np.abs(Ud - Uo).max():.3e}")
        assert len(dd["hist"]) == len(do["hist"]) == 8
        for a, b in zip(dd["hist"], do["hist"]):
            assert abs(a["resid"] - b["resid"]) <= 1e-6 * abs(b["resid"]) and abs(a["obj"] - b["obj"]) <= 1e-6 * abs(b["obj"]), (what, a, b)
        np.testing.assert_allclose(Xd, Xo, rtol=0, atol=1e-7)
        np.testing.assert_allclose(Ud, Uo, rtol=0, atol=1e-7)


# ---- 3. library loop ------------------------------------------------------------------------------------------------------------------
def _loops(mid, prob, cost, steps, first_cold):
    """The `_loops` of tests/test_lin_cost_gpu.py for a custom cost: (residuals, X, U, infos) of the Python-driven loop
    linearize -> custom_cost_grad -> ref_shift Q -> ref_shift R -> lqp_solve -> residual -> swap and of the library's loop with `cost`,
    a fresh context each.  first_cold False: both legs first run ONE cold iteration driven from Python."""
    import torch

    from pmpc_amd.device import DeviceSolver, to_device_problem

    d = to_device_problem(prob)
    M, N, x = d["X_prev"].shape
    u = d["U_prev"].shape[-1]
    Nc = prob["solver_settings"]["Nc"]
    common = dict(Q=d["Q"], R=d["R"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=Nc, x0=d["x0"], lu=d["lu"], uu=d["uu"], symmetric_cost=True)
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    Pd = _dev(cost["params"])

    def python_iterations(s, Xa, Ua, Xb, Ub, n, cold_first):
        res = []
        for it in range(n):
            f, fx, fu = s.linearize(mid, d["x0"], Xa, Ua, d["params"])
            cx, cu = s.custom_cost_grad(cost["cost"], Xa, Ua, Pd)
            Xr = s.ref_shift(d["Q"], cx, d["X_ref"])
            Ur = s.ref_shift(d["R"], cu, d["U_ref"]) if cu is not None else d["U_ref"]
            _, _, st = s.lqp_solve(f=f, fx=fx, fu=fu, X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, X_ref=Xr, U_ref=Ur, static_cons_bounds=True,
                                   prev_is_last_solution=not (cold_first and it == 0), cold_start=cold_first and it == 0, **common)
            assert st == 0, (it, s.last_info)
            res.append(float(s.scp_residual(Xb, Xa, Ub, Ua)[0].item()))
            Xa, Xb, Ua, Ub = Xb, Xa, Ub, Ua
        return res, Xa, Ua, Xb, Ub

    out = []
    for leg in ("python", "library"):
        s = DeviceSolver(0)
        try:
            Xa, Ua, Xb, Ub = d["X_prev"].clone(), d["U_prev"].clone(), mk(M, N, x), mk(M, N, u)
            if not first_cold:
                _, Xa, Ua, Xb, Ub = python_iterations(s, Xa, Ua, Xb, Ub, 1, True)
            if leg == "python":
                res, Xa, Ua, _, _ = python_iterations(s, Xa, Ua, Xb, Ub, steps, first_cold)
                out.append((np.array(res), Xa.clone(), Ua.clone(), None))
            else:
                out.append(_library(s, mid, d, common, cost, steps, first_cold, Xa, Ua, Xb, Ub))
        finally:
            s.close()
    return out


def _library(s, mid, d, common, cost, steps, first_cold, Xa, Ua, Xb, Ub):
    import torch

    M, N, x = Xa.shape
    u = Ua.shape[-1]
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    bufs = [mk(M, N, x), mk(M, N, x, x), mk(M, N, u, x), mk(M, N, x), mk(M, N, x, x), mk(M, N, u, x)]
    if first_cold:  # (forget the warm-start memory of this shape, as tests/test_bicycle_gpu.py does)
        s.lqp_solve(f=bufs[0].zero_(), fx=bufs[1].zero_(), fu=bufs[2].zero_(), X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, cold_start=True,
                    X_ref=d["X_ref"], U_ref=d["U_ref"], **dict(common, lu=None, uu=None))
    res, infos, last, done = s.scp_loop(mid, d["params"], steps, f=bufs[0], fx=bufs[1], fu=bufs[2], f2=bufs[3], fx2=bufs[4], fu2=bufs[5],
                                        X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, X_ref=d["X_ref"], U_ref=d["U_ref"], first_cold=first_cold,
                                        cost=cost, **common)
    s.sync()
    assert done == steps and all(i["status"] == 0 for i in infos), infos
    X, U = (Xb, Ub) if last else (Xa, Ua)
    return res.cpu().numpy(), X.clone(), U.clone(), infos


def _soft_speed_params(M):
    """A limit below the lane-change problem's 5 m/s, so the hinge is on its slope, and an effort weight of the size of R_00 / (1 + v^2)."""
    k = np.arange(M)
    return np.stack([2.0 + 0.01 * k, np.full(M, 4.0), 4.5 + 0.005 * k, np.full(M, 0.002)], -1)


@pytest.mark.parametrize("first_cold", [True, False])
@pytest.mark.parametrize("Nc", [1, -1])
def test_library_loop_with_a_custom_cost_walks_the_python_driven_iterates(Nc, first_cold):
    """6 iterations on the bicycle (M 40, N 12) with soft_speed — both references are shifted, the speculative linearisation runs with
    its three launches —, atol 1e-6 on residuals and iterates (the bound of
    test_library_loop_with_a_cost_walks_the_python_driven_iterates)."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_BICYCLE

    prob = dyn.make_bicycle_problem(M=40, N=12, Nc=Nc)
    cost = _custom("soft_speed", _soft_speed_params(40))
    (rp, Xp, Up, _), (rl, Xl, Ul, infos) = _loops(MODEL_BICYCLE, prob, cost, 6, first_cold)
    print("Nc", Nc, "first_cold", first_cold, "residuals", rl, "python-driven", rp, [(i["ipm_iters"], i["active_set_rounds"]) for i in infos])
    print("  max |dX|", float((Xl - Xp).abs().max()), "max |dU|", float((Ul - Up).abs().max()))
    np.testing.assert_allclose(rl, rp, rtol=0, atol=1e-6)
    assert torch.allclose(Xl, Xp, rtol=0, atol=1e-6) and torch.allclose(Ul, Up, rtol=0, atol=1e-6)
    assert np.isfinite(rl).all() and rl[-1] < rl[0]


def test_library_loop_with_a_custom_cost_on_the_quadrotor():
    """generic<12, 4> (4 passes of 4 directions; the dim 12 and dim 4 bodies of the shift): M 8, N 10, Nc 1, 6 iterations, the same bound."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_QUADROTOR

    prob = dyn.make_quadrotor_problem(M=8, N=10, Nc=1)
    rng = np.random.default_rng(12)
    P = np.concatenate([rng.uniform(0.05, 0.2, (8, 12)), rng.uniform(0.001, 0.003, (8, 4))], -1)
    (rp, Xp, Up, _), (rl, Xl, Ul, infos) = _loops(MODEL_QUADROTOR, prob, _custom("generic_12_4", P), 6, True)
    print("quadrotor residuals", rl, "python-driven", rp, "max |dX|", float((Xl - Xp).abs().max()), "max |dU|", float((Ul - Up).abs().max()))
    np.testing.assert_allclose(rl, rp, rtol=0, atol=1e-6)
    assert torch.allclose(Xl, Xp, rtol=0, atol=1e-6) and torch.allclose(Ul, Up, rtol=0, atol=1e-6)


def test_library_loop_with_obstacles_u_equals_the_builtin_moving_obstacles():
    """obstacles_u with cw = 0, uses_u=False and a drift of 0.05 m per stage IS the built-in cost with the per-stage centres of
    tests/test_lin_cost_gpu.py::_moving: the two library loops (bicycle M 40, N 12, Nc 1, 6 iterations) agree at atol 1e-6, and U_ref
    is bit for bit what it was."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_BICYCLE, DeviceSolver, to_device_problem
    from tests.test_lin_cost_gpu import OBSTACLES, _moving

    prob = dyn.make_bicycle_problem(M=40, N=12, Nc=1)
    static = dict(OBSTACLES, centres=np.array([[1.5, 0.2], [3.5, 2.5]]))
    custom = _custom("obstacles_u", cc.obstacle_params(static, 40), uses_u=False, drift=0.05)
    d = to_device_problem(prob)
    U_ref0 = d["U_ref"].clone()
    common = dict(Q=d["Q"], R=d["R"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=1, x0=d["x0"], lu=d["lu"], uu=d["uu"], symmetric_cost=True)
    out = []
    for cost in (_moving(static, 12), custom):
        s = DeviceSolver(0)
        try:
            Xa, Ua = d["X_prev"].clone(), d["U_prev"].clone()
            out.append(_library(s, MODEL_BICYCLE, d, common, cost, 6, True, Xa, Ua, torch.empty_like(Xa), torch.empty_like(Ua)))
        finally:
            s.close()
    (rb, Xb, Ub, _), (rc, Xc, Uc, _) = out
    print("built-in residuals", rb, "custom", rc, "max |dX|", float((Xc - Xb).abs().max()), "max |dU|", float((Uc - Ub).abs().max()))
    np.testing.assert_allclose(rc, rb, rtol=0, atol=1e-6)
    assert torch.allclose(Xc, Xb, rtol=0, atol=1e-6) and torch.allclose(Uc, Ub, rtol=0, atol=1e-6)
    assert torch.equal(d["U_ref"], U_ref0)


# ---- 4. a custom model and a custom cost on one solver --------------------------------------------------------------------------------
def _pendulum_loop(s, mid, cost, steps=3):
    """A small pendulum problem (M 4, N 8) through the library loop: (done, infos)."""
    import torch

    M, N = 4, 8
    x0, Xp, Up, P = cm.rand_inputs("pendulum", M, N, seed=4)
    eye = lambda d, w: _dev(np.tile(w * np.eye(d), (M, N, 1, 1)))
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    _, infos, _, done = s.scp_loop(mid, _dev(P), steps, f=mk(M, N, 2), fx=mk(M, N, 2, 2), fu=mk(M, N, 1, 2), f2=mk(M, N, 2), fx2=mk(M, N, 2, 2), fu2=mk(M, N, 1, 2),
                                   X_prev=_dev(0.1 * Xp), U_prev=_dev(0.1 * Up), X_out=mk(M, N, 2), U_out=mk(M, N, 1), X_ref=_dev(np.zeros((M, N, 2))),
                                   U_ref=_dev(np.zeros((M, N, 1))), Q=eye(2, 1.0), R=eye(1, 0.5), reg_x=1.0, reg_u=1.0, Nc=1, x0=_dev(0.1 * x0),
                                   lu=_dev(np.full((M, N, 1), -2.0)), uu=_dev(np.full((M, N, 1), 2.0)), symmetric_cost=True, cost=cost)
    s.sync()
    return done, infos


def test_a_custom_model_and_a_custom_cost_on_one_solver():
    """A loop with both; unloading the cost leaves the model usable and the other way round; an unloaded cost id, and one loaded on
    another solver, are refused with status 2 (nothing runs)."""
    from pmpc_amd import _lib
    from pmpc_amd.device import DeviceSolver

    rng = np.random.default_rng(2)
    P = rng.uniform(0.3, 1.2, (4, 3))
    s, other = DeviceSolver(0), DeviceSolver(0)
    try:
        model, cost = cm.make("pendulum"), _custom("generic_2_1", P)
        mid = s.load_model(model)
        done, infos = _pendulum_loop(s, mid, cost)
        assert done == 3 and all(i["status"] == 0 for i in infos), infos
        cid = s.load_cost(cost["cost"])
        assert cid >= _lib.COST_CUSTOM0 and s.load_cost(cost["cost"]) == cid
        stale = s.prepare_cost(cost, 8, 2, "cuda", M=4, u=1)
        s.unload_cost(cid)
        done, infos = _pendulum_loop(s, mid, None)  # the model is still there
        assert done == 3 and all(i["status"] == 0 for i in infos), infos
        done, infos = _pendulum_loop(s, mid, stale)  # ... the cost's id is not
        assert done == 0 and infos[0]["status"] == 2
        with pytest.raises(ValueError, match="not a custom cost loaded"):
            s.unload_cost(cid)
        # the other way round
        cid2 = s.load_cost(cost["cost"])
        s.unload_model(mid)
        X, U, _ = cc.rand_inputs("generic_2_1", 4, 8)
        cx, cu = s.custom_cost_grad(cid2, _dev(X), _dev(U), _dev(P))
        s.sync()
        np.testing.assert_allclose(cx.cpu().numpy(), cc.generic_np(X, U, P)[1], **TOL)
        done, infos = _pendulum_loop(s, mid, cost)  # (the model id is gone: refused)
        assert done == 0 and infos[0]["status"] == 2
        # an id of another solver
        foreign = other.prepare_cost(cost, 8, 2, "cuda", M=4, u=1)
        assert other.lib.pmpc_cost_unload(s.h, foreign[0].id) == 2
        mid = s.load_model(model)
        done, infos = _pendulum_loop(s, mid, foreign)
        assert done == 0 and infos[0]["status"] == 2
        Xd, Ud, Pd = _dev(X), _dev(U), _dev(P)
        assert s.lib.pmpc_custom_cost_grad_device(s.h, foreign[0].id, 8, 4, Xd.data_ptr(), Ud.data_ptr(), Pd.data_ptr(), cx.data_ptr(), cu.data_ptr(), None) == 2
        done, infos = _pendulum_loop(s, mid, cost)  # and the solver's own still runs
        assert done == 3 and all(i["status"] == 0 for i in infos), infos
    finally:
        s.close()
        other.close()


# ---- 5. MPCController -----------------------------------------------------------------------------------------------------------------
def test_controller_step_with_a_custom_cost_equals_the_hand_composed_step():
    """The custom-cost case of tests/test_mpc_gpu.py::test_step_equals_the_hand_composed_step: bicycle M 48, N 20, Nc 1, 3 MPC steps of 3
    SCP iterations with soft_speed; plans atol 1e-7, residuals rtol 1e-6 / atol 1e-9."""
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_BICYCLE, DeviceSolver, to_device_problem
    from tests.test_mpc_gpu import _controller, _hand_step, _plant

    prob = dyn.make_bicycle_problem(M=48, N=20, Nc=1)
    cost = _custom("soft_speed", _soft_speed_params(48))
    d = to_device_problem(prob)
    rng = np.random.default_rng(5)
    s1, s2 = DeviceSolver(0), DeviceSolver(0)
    try:
        ctl = _controller("bicycle", prob, s1, builtin_cost=cost)
        ctl.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
        X_start, U_start, x0 = prob["X_prev"], prob["U_prev"], prob["x0"]
        for k in range(3):
            u0, info = ctl.step(x0, iterations=3, shift=1)
            assert info["status"] == 0 and info["iterations_done"] == 3 and u0.shape == (48, 2)
            X, U = ctl.X.cpu().numpy(), ctl.U.cpu().numpy()
            res_h, X_h, U_h = _hand_step(s2, MODEL_BICYCLE, prob, d, X_start, U_start, x0, 3, cost=cost)
            print(f"custom cost MPC step {k}: residuals {info['resid']} hand-composed {res_h}; max |dX| {np.abs(X - X_h).max():.3e} max |dU| {np.abs(U - U_h).max():.3e}")
            np.testing.assert_allclose(X, X_h, rtol=0, atol=1e-7)
            np.testing.assert_allclose(U, U_h, rtol=0, atol=1e-7)
            np.testing.assert_allclose(info["resid"], res_h, rtol=1e-6, atol=1e-9)
            np.testing.assert_array_equal(u0, U[:, 0])
            X_start, U_start, _ = dyn.shift_plan("bicycle", X, U, prob["params"], s=1)
            x0 = _plant("bicycle", prob, np.broadcast_to(x0, (48, 4))[0], u0, rng)
    finally:
        s1.close()
        s2.close()


def test_set_cost_params_and_warm_shift():
    """`set_cost_params` rewrites the resident parameters: the next step equals the first step of a fresh controller built with the new
    parameters and reset to the same (shifted) plan (atol 1e-7), and differs from one built with the old ones.  `warm_shift=True` next to
    a custom cost runs, and the second step starts warm."""
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver
    from tests.test_mpc_gpu import _controller

    prob = dyn.make_bicycle_problem(M=16, N=12, Nc=1)
    P1 = _soft_speed_params(16)
    P2 = P1.copy()
    P2[:, 2] -= 1.0  # a limit 1 m/s lower
    x1 = prob["x0"] + 0.01
    solvers = [DeviceSolver(0) for _ in range(4)]
    try:
        ctl = _controller("bicycle", prob, solvers[0], builtin_cost=_custom("soft_speed", P1))
        ctl.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
        u0, info = ctl.step(prob["x0"], iterations=3)
        assert info["status"] == 0
        Xs, Us, _ = dyn.shift_plan("bicycle", ctl.X.cpu().numpy(), ctl.U.cpu().numpy(), prob["params"], s=1)
        with pytest.raises(ValueError, match="params must be"):
            ctl.set_cost_params(P2[:, :3])
        ctl.set_cost_params(P2)
        u1, info = ctl.step(x1, iterations=3)
        assert info["status"] == 0
        fresh = []
        for s, P in zip(solvers[1:3], (P2, P1)):
            c = _controller("bicycle", prob, s, builtin_cost=_custom("soft_speed", P))
            c.reset(X_prev=Xs, U_prev=Us)
            u, inf = c.step(x1, iterations=3)
            assert inf["status"] == 0
            fresh.append((u, c.X.cpu().numpy(), c.U.cpu().numpy()))
        X, U = ctl.X.cpu().numpy(), ctl.U.cpu().numpy()
        print(f"set_cost_params: max |dX| to the fresh controller with the new parameters {np.abs(X - fresh[0][1]).max():.3e}, with the old ones {np.abs(X - fresh[1][1]).max():.3e}")
        np.testing.assert_allclose(X, fresh[0][1], rtol=0, atol=1e-7)
        np.testing.assert_allclose(U, fresh[0][2], rtol=0, atol=1e-7)
        np.testing.assert_allclose(u1, fresh[0][0], rtol=0, atol=1e-7)
        assert np.abs(X - fresh[1][1]).max() > 1e-3
        with pytest.raises(ValueError, match="without builtin_cost"):
            _controller("bicycle", prob, solvers[1]).set_cost_params(P2)
        # warm_shift next to the custom cost
        warm = _controller("bicycle", prob, solvers[3], builtin_cost=_custom("soft_speed", P1), warm_shift=True)
        warm.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
        _, i0 = warm.step(prob["x0"], iterations=3)
        _, i1 = warm.step(x1, iterations=3)
        assert i0["status"] == 0 and i1["status"] == 0 and not i0["warm_shift"] and i1["warm_shift"]
    finally:
        for s in solvers:
            s.close()


# ---- 6. refusals and failures ---------------------------------------------------------------------------------------------------------
def test_refusals_come_before_anything_runs():
    """fp32-stored matrices next to a custom cost, and a cost whose dimensions are not the problem's: 0 iterations, infos[0].status = 2,
    nothing written.  A NULL and a kind-0 cost reproduce pmpc_scp_loop_device bit for bit on a fresh context."""
    import torch

    from pmpc_amd import _lib
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver, to_device_problem
    from tests.test_lin_cost_gpu import _raw_loop

    prob = dyn.make_bicycle_problem(M=40, N=12, Nc=1)
    d = to_device_problem(prob)
    s = DeviceSolver(0)
    try:
        sc, keep = s.prepare_cost(_custom("soft_speed", _soft_speed_params(40)), 12, 4, "cuda", M=40, u=2)
        done, res, X, U, status = _raw_loop(s, "pmpc_scp_loop_device_cost", d, prob, 3, (ctypes.byref(sc),), f32=True)
        assert done == 0 and status[0] == 2
        assert torch.equal(X, d["X_prev"]) and torch.equal(U, d["U_prev"])
        other = cc.make("generic_3_5")
        Pd = _dev(np.ones((40, 8)))
        wrong = _lib.PmpcScpCost(kind=2, id=s.load_cost(other), uses_u=1, cparams=Pd.data_ptr())
        done, res, X, U, status = _raw_loop(s, "pmpc_scp_loop_device_cost", d, prob, 3, (ctypes.byref(wrong),))
        assert done == 0 and status[0] == 2
        assert torch.equal(X, d["X_prev"]) and torch.equal(U, d["U_prev"])
        # uses_u that is not what the cost was compiled with, and null parameters
        for bad in (_lib.PmpcScpCost(kind=2, id=sc.id, uses_u=0, cparams=sc.cparams), _lib.PmpcScpCost(kind=2, id=sc.id, uses_u=1, cparams=None)):
            done, _, _, _, status = _raw_loop(s, "pmpc_scp_loop_device_cost", d, prob, 3, (ctypes.byref(bad),))
            assert done == 0 and status[0] == 2
        # the obstacle entry points answer kind 2 with 2
        out = torch.full((40, 12, 4), 7.0, dtype=torch.float64, device="cuda")
        assert s.lib.pmpc_obstacle_cost_grad_device(s.h, ctypes.byref(sc), 4, 12, 40, d["X_prev"].data_ptr(), out.data_ptr()) == 2
        assert s.lib.pmpc_obstacle_ref_shift_device(s.h, ctypes.byref(sc), 4, 12, 40, d["X_prev"].data_ptr(), d["Q"].data_ptr(), d["X_ref"].data_ptr(), out.data_ptr()) == 2
        s.sync()
        assert bool((out == 7.0).all())
        del keep
    finally:
        s.close()
    none = _lib.PmpcScpCost(kind=0)
    runs = []
    for entry, extra in (("pmpc_scp_loop_device", ()), ("pmpc_scp_loop_device_cost", (None,)), ("pmpc_scp_loop_device_cost", (ctypes.byref(none),))):
        s = DeviceSolver(0)
        try:
            runs.append(_raw_loop(s, entry, d, prob, 5, extra))
        finally:
            s.close()
    assert runs[0][0] == 5 and runs[0][4] == [0] * 5
    for r in runs[1:]:
        assert r[0] == 5 and r[4] == runs[0][4]
        assert torch.equal(r[1], runs[0][1]) and torch.equal(r[2], runs[0][2]) and torch.equal(r[3], runs[0][3])


def test_an_indefinite_block_of_R_is_a_value_error_and_the_context_goes_on():
    """One block of R among the M N with a negative eigenvalue: the shift of U_ref refuses it (NaN in its row), the sub-problem fails,
    and `scp_loop` raises the ValueError of `check_bad_pivots`; the context answers the next call."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_BICYCLE, DeviceSolver, to_device_problem

    prob = dyn.make_bicycle_problem(M=40, N=12, Nc=1)
    d = to_device_problem(prob)
    cost = _custom("soft_speed", _soft_speed_params(40))
    common = dict(Q=d["Q"], R=d["R"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=1, x0=d["x0"], lu=d["lu"], uu=d["uu"], symmetric_cost=True)
    bad = d["R"].clone()
    bad[17, 5] = torch.tensor([[0.1, 0.0], [0.0, -0.5]], dtype=torch.float64, device="cuda")
    s = DeviceSolver(0)
    try:
        Xa, Ua = d["X_prev"].clone(), d["U_prev"].clone()
        with pytest.raises(ValueError, match="not symmetric positive definite"):
            _library(s, MODEL_BICYCLE, d, dict(common, R=bad), cost, 3, True, Xa, Ua, torch.empty_like(Xa), torch.empty_like(Ua))
        Xa, Ua = d["X_prev"].clone(), d["U_prev"].clone()
        res, X, U, infos = _library(s, MODEL_BICYCLE, d, common, cost, 3, True, Xa, Ua, torch.empty_like(Xa), torch.empty_like(Ua))
        assert np.isfinite(res).all() and bool(X.isfinite().all())
    finally:
        s.close()


# ---- 7. keep-out and custom cost together -----------------------------------------------------------------------------------------------
def test_keepout_and_a_custom_cost_together():
    """`scp_loop(cstr=, aug=, cost=custom)` against the Python-driven `solve(device=..., builtin_cstr=, builtin_cost=custom)` on
    `bicycle_keepout_problem()`, 3 iterations: 1e-7 relative on X, U and the residuals, the bound
    tests/test_keepout_loop_gpu.py::test_with_the_builtin_cost_as_well applies to this comparison with the built-in cost.  The cost's
    shifted X_ref is the augmentation's, U_ref is shifted beside it, and the cost acts."""
    from pmpc_amd.device import DeviceSolver
    from tests.support.keepout_loop import FEAS, library_loop, outside, python_loop, rel
    from tests.support.keepout_problems import bicycle_keepout_problem

    kw, cstr = bicycle_keepout_problem()
    M = kw["Q"].shape[0]
    P = np.tile(np.array([[2.0, 0.9, 50.0, 50.0, 0.5, 1.0, 2.0, 0.0, 0.05]]), (M, 1))
    cost = _custom("obstacles_u", P)
    s1, s2, s3 = DeviceSolver(0), DeviceSolver(0), DeviceSolver(0)
    try:
        res, X, U, _ = library_loop(s1, "bicycle", kw, cstr, 3, cost=cost)
        Xp, Up, data = python_loop("bicycle", kw, cstr, 3, solver=s2, builtin_cost=cost)
        _, Xn, _, _ = library_loop(s3, "bicycle", kw, cstr, 3)
    finally:
        for s in (s1, s2, s3):
            s.close()
    assert Xp is not None and len(data["hist"]) == 3
    print(f"keep-out library loop with a custom cost: rel X {rel(X, Xp[:, 1:]):.3e} U {rel(U, Up):.3e}; the cost moves the plan by {rel(X, Xn):.3e}")
    assert rel(X, Xn) > 1e-3
    assert rel(X, Xp[:, 1:]) < 1e-7 and rel(U, Up) < 1e-7
    np.testing.assert_allclose(res, [h["resid"] for h in data["hist"]], rtol=1e-7, atol=0)
    assert outside(X, cstr) > -FEAS
