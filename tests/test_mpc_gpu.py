"""`pmpc_amd.MPCController` (pmpc_amd/mpc.py): receding-horizon MPC with the problem resident in HBM — x0 copy, plan shift
(`DeviceSolver.shift_plan`) and the library's SCP loop (`DeviceSolver.scp_loop`, first_cold) per step — against the same step composed
by hand from the numpy shift and the loop on a second context, and against the public `solve(..., device="cuda")`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _controller(name, prob, solver, **kw):
    import pmpc_amd

    args = dict(builtin_model=name, params=prob["params"], Q=prob["Q"], R=prob["R"], X_ref=prob["X_ref"], U_ref=prob["U_ref"], u_l=prob["u_l"],
                u_u=prob["u_u"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], solver_settings=dict(prob["solver_settings"]), solver=solver)
    args.update(kw)
    return pmpc_amd.MPCController(**args)


def _plant(name, prob, x, u0, rng):
    """Particle 0's model stepped with the control the controller returned, plus a seeded disturbance of 0.01."""
    from pmpc_amd import dynamics as dyn

    return getattr(dyn, name)(x, u0[0], prob["params"][0])[0] + 0.01 * rng.standard_normal(x.shape)


def _hand_step(s2, mid, prob, d, X_start, U_start, x0, iterations, **extra):
    """The library's loop, first_cold, from (X_start, U_start) on the context s2 with fresh buffers: (residuals, X, U)."""
    import torch

    M, N, x = X_start.shape
    u = U_start.shape[-1]
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    Xa, Ua, Xb, Ub = dev(X_start), dev(U_start), mk(M, N, x), mk(M, N, u)
    x0d = dev(np.broadcast_to(x0, (M, x)))
    res, infos, last, done = s2.scp_loop(mid, d["params"], iterations, f=mk(M, N, x), fx=mk(M, N, x, x), fu=mk(M, N, u, x), f2=mk(M, N, x),
                                         fx2=mk(M, N, x, x), fu2=mk(M, N, u, x), X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, first_cold=True, Q=d["Q"],
                                         R=d["R"], X_ref=d["X_ref"], U_ref=d["U_ref"], reg_x=prob["reg_x"], reg_u=prob["reg_u"],
                                         Nc=prob["solver_settings"]["Nc"], x0=x0d, lu=d["lu"], uu=d["uu"], symmetric_cost=True, **extra)
    s2.sync()
    assert done == iterations and all(i["status"] == 0 for i in infos), infos
    X, U = (Xb, Ub) if last else (Xa, Ua)
    return res.cpu().numpy(), X.cpu().numpy(), U.cpu().numpy()


def _obstacles():
    from tests.test_lin_cost_gpu import OBSTACLES

    return OBSTACLES


@pytest.mark.parametrize("case", ["osqp", "ecos", "builtin_cost"])
def test_step_equals_the_hand_composed_step(case):
    """Bicycle M 48, N 20, Nc 1, 3 MPC steps of 3 SCP iterations.  Expectation of a step: the numpy `shift_plan` of the controller's
    previous plan, read back (step 0: the problem's X_prev, U_prev), then `scp_loop(first_cold=True, steps=3)` on a second context with
    fresh buffers.  Plans atol 1e-7, residuals rtol 1e-6 / atol 1e-9: the tolerances tests/test_bicycle_gpu.py applies to this solver on
    separately produced inputs."""
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_BICYCLE, DeviceSolver, to_device_problem

    prob = dyn.make_bicycle_problem(M=48, N=20, Nc=1)
    ctl_kw, loop_kw = {}, {}
    if case == "ecos":
        prob["solver_settings"] = dict(solver="ecos", Nc=1)
        loop_kw = dict(cone_objective=True)
    elif case == "builtin_cost":
        ctl_kw, loop_kw = dict(builtin_cost=_obstacles()), dict(cost=_obstacles())
    d = to_device_problem(prob)
    rng = np.random.default_rng(5)
    s1, s2 = DeviceSolver(0), DeviceSolver(0)
    try:
        ctl = _controller("bicycle", prob, s1, **ctl_kw)
        ctl.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
        X_start, U_start, x0 = prob["X_prev"], prob["U_prev"], prob["x0"]
        for k in range(3):
            u0, info = ctl.step(x0, iterations=3, shift=1)
            assert info["status"] == 0 and info["iterations_done"] == 3 and len(info["infos"]) == 3 and u0.shape == (48, 2)
            X, U = ctl.X.cpu().numpy(), ctl.U.cpu().numpy()
            res_h, X_h, U_h = _hand_step(s2, MODEL_BICYCLE, prob, d, X_start, U_start, x0, 3, **loop_kw)
            print(f"{case} MPC step {k}: residuals {info['resid']} hand-composed {res_h}; max |dX| {np.abs(X - X_h).max():.3e} max |dU| {np.abs(U - U_h).max():.3e}; "
                  f"(ipm, rounds) {[(i['ipm_iters'], i['active_set_rounds']) for i in info['infos']]}")
            np.testing.assert_allclose(X, X_h, rtol=0, atol=1e-7)
            np.testing.assert_allclose(U, U_h, rtol=0, atol=1e-7)
            np.testing.assert_allclose(info["resid"], res_h, rtol=1e-6, atol=1e-9)
            np.testing.assert_array_equal(u0, U[:, 0])
            X_start, U_start, _ = dyn.shift_plan("bicycle", X, U, prob["params"], s=1)
            x0 = _plant("bicycle", prob, np.broadcast_to(x0, (48, 4))[0], u0, rng)  # (x,) from the second step on
    finally:
        s1.close()
        s2.close()


def test_one_step_equals_the_public_solve():
    """One step of 3 iterations from a given (x0, X_prev, U_prev) against `pmpc_amd.solve(None, ..., device="cuda", builtin_model="bicycle",
    max_it=3, res_tol=0.0)`: atol 1e-7 on X[:, 1:] and U."""
    import pmpc_amd
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver

    M, N = 8, 15
    prob = dyn.make_bicycle_problem(M=M, N=N, Nc=1)
    Xs, Us, data = pmpc_amd.solve(None, prob["Q"], prob["R"], prob["x0"], device="cuda", builtin_model="bicycle", params=prob["params"], X_ref=prob["X_ref"],
                                  U_ref=prob["U_ref"], X_prev=prob["X_prev"], U_prev=prob["U_prev"], u_l=prob["u_l"], u_u=prob["u_u"], reg_x=prob["reg_x"],
                                  reg_u=prob["reg_u"], max_it=3, res_tol=0.0, verbose=False, solver_settings=dict(solver="osqp", Nc=1))
    assert len(data["hist"]) == 3
    s = DeviceSolver(0)
    try:
        ctl = _controller("bicycle", prob, s)
        ctl.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
        u0, info = ctl.step(prob["x0"], iterations=3)
        X, U = ctl.X.cpu().numpy(), ctl.U.cpu().numpy()
    finally:
        s.close()
    print(f"max |dX| {np.abs(X - Xs[:, 1:]).max():.3e} max |dU| {np.abs(U - Us).max():.3e}; residuals {info['resid']} solve {[h['resid'] for h in data['hist']]}")
    np.testing.assert_allclose(X, Xs[:, 1:], rtol=0, atol=1e-7)
    np.testing.assert_allclose(U, Us, rtol=0, atol=1e-7)
    np.testing.assert_allclose(u0, Us[:, 0], rtol=0, atol=1e-7)


@pytest.mark.parametrize("name,M,N", [("unicycle", 16, 10), ("bicycle", 16, 10), ("quadrotor", 8, 10)])
def test_every_model_runs_in_closed_loop(name, M, N):
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver

    prob = getattr(dyn, f"make_{name}_problem")(M=M, N=N, Nc=1)
    rng = np.random.default_rng(7)
    s = DeviceSolver(0)
    try:
        ctl = _controller(name, prob, s)
        ctl.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
        x0 = prob["x0"]
        for k in range(2):
            u0, info = ctl.step(x0, iterations=3)
            assert info["status"] == 0 and all(i["status"] == 0 for i in info["infos"]), info
            assert np.isfinite(u0).all() and np.isfinite(info["resid"]).all()
            # (the plan moves one stage per step and the boxes do not move with it: stage 0's box is the one that binds u0)
            assert np.all(u0 >= prob["u_l"][:, 0] - 1e-9) and np.all(u0 <= prob["u_u"][:, 0] + 1e-9)
            np.testing.assert_allclose(u0, np.broadcast_to(u0[0], u0.shape), rtol=0, atol=1e-12)  # Nc = 1: one first control
            x0 = _plant(name, prob, np.broadcast_to(x0, (M, x0.shape[-1]))[0], u0, rng)
    finally:
        s.close()


def test_reset_with_rollout_starts_from_a_feasible_iterate():
    """`reset(U_prev=..., rollout=True)`: the next step's start iterate is the rollout of its x0 — its defect under the library's own
    linearisation is <= 1e-12 (rtol = atol, the one-step rule of tests/test_rollout_gpu.py).  After ONE iteration the start iterate is still
    in the loop's other trajectory pair."""
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver, to_device_problem

    from tests.test_rollout import _inputs

    prob, U = _inputs("bicycle", 16, 10)
    s = DeviceSolver(0)
    try:
        ctl = _controller("bicycle", prob, s)
        ctl.reset(U_prev=U, rollout=True)
        u0, info = ctl.step(prob["x0"], iterations=1)
        assert info["status"] == 0
        X_start, U_start = ctl._pairs[ctl._cur ^ 1]
        np.testing.assert_array_equal(U_start.cpu().numpy(), U)
        d = to_device_problem(prob)
        f, _, _ = s.linearize(ctl.model, d["x0"], X_start, U_start, d["params"])
        s.sync()
        print("defect of the rolled-out start iterate under linearize:", float((f - X_start).abs().max()))
        assert np.isfinite(X_start.cpu().numpy()).all()
        np.testing.assert_allclose(f.cpu().numpy(), X_start.cpu().numpy(), rtol=1e-12, atol=1e-12)
        # without the rollout the start iterate is what reset was given
        ctl.reset(X_prev=prob["X_prev"], U_prev=U)
        ctl.step(prob["x0"], iterations=1)
        np.testing.assert_array_equal(ctl._pairs[ctl._cur ^ 1][0].cpu().numpy(), prob["X_prev"])
    finally:
        s.close()


def test_a_single_x0_equals_its_broadcast():
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver

    prob = dyn.make_bicycle_problem(M=16, N=10, Nc=1)
    x0 = prob["x0"][3]
    plans = []
    for given in (x0, np.tile(x0, (16, 1)), torch.as_tensor(x0, device="cuda")):
        s = DeviceSolver(0)
        try:
            ctl = _controller("bicycle", prob, s)
            u0, info = ctl.step(given, iterations=2, return_torch=True)
            assert info["status"] == 0 and torch.is_tensor(u0) and u0.is_cuda
            u1, info = ctl.step(given, iterations=2)
            assert info["status"] == 0 and isinstance(u1, np.ndarray)
            plans.append((ctl.X.clone(), ctl.U.clone()))
        finally:
            s.close()
    for X, U in plans[1:]:
        assert torch.equal(X, plans[0][0]) and torch.equal(U, plans[0][1])


def test_refusals_and_the_failed_state():
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver

    prob = dyn.make_bicycle_problem(M=8, N=6, Nc=1)
    s = DeviceSolver(0)
    try:
        for kw, word in ((dict(builtin_model=None), "builtin_model"), (dict(extra_cstrs_fns=[lambda *a: None]), "extra_cstrs_fns"),
                         (dict(filter_method="momentum"), "filter_method"), (dict(solver_state={}), "solver_state"),
                         (dict(f_fx_fu_fn=prob["f_fx_fu_fn"]), "f_fx_fu_fn"), (dict(solver_settings=dict(solver="osqp", Nc=1, smooth_cstr="squareplus")), "smooth_cstr"),
                         (dict(builtin_model="tricycle"), "tricycle")):
            with pytest.raises(ValueError, match=word):
                _controller("bicycle", prob, s, **kw)
        s.world = 2  # (what init_comm leaves on a sharded context)
        with pytest.raises(ValueError, match="sharded"):
            _controller("bicycle", prob, s)
        s.world = 1
        ctl = _controller("bicycle", prob, s)
        with pytest.raises(ValueError, match="iterations"):
            ctl.step(prob["x0"], iterations=0)
        u0, info = ctl.step(prob["x0"], iterations=2)
        assert info["status"] == 0 and u0 is not None
        ctl.failed = True  # (what a failed sub-problem leaves; not provoked here)
        for _ in range(2):
            with pytest.raises(RuntimeError, match="reset"):
                ctl.step(prob["x0"], iterations=2)
        ctl.reset()
        u0, info = ctl.step(prob["x0"], iterations=2)
        assert info["status"] == 0 and u0 is not None and not ctl.failed
    finally:
        s.close()
