"""Custom dynamics models on the GPU (pmpc_amd.CustomModel, csrc/model_jit.hip): the runtime-compiled linearise / rollout / shift
kernels against numpy closed forms and against built-in model 2, the library SCP loop and `MPCController` on a custom model, and the
refusals of ids that are not (or no longer) loaded.  Each model is compiled once for the module."""
import ctypes

import numpy as np
import pytest

from tests.support import custom_models as cm

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-12, atol=1e-12)  # the tolerance of tests/test_bicycle_gpu.py


@pytest.fixture(scope="module")
def models():
    return {name: cm.make(name) for name in cm.SOURCES}


@pytest.fixture()
def solver():
    from pmpc_amd.device import DeviceSolver

    s = DeviceSolver(0)
    yield s
    s.close()


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


# ---- linearise against the closed forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,N", [("bicycle", 5, 7), ("pendulum", 3, 4), ("ring", 4, 5)])  # bicycle: 35 units, a partial block of 64
def test_linearize_against_closed_forms(models, solver, name, M, N):
    x0, Xp, Up, P = cm.rand_inputs(name, M, N, seed=3)
    mid = solver.load_model(models[name])
    assert mid >= 1000 and solver.load_model(models[name]) == mid  # loaded once per solver
    f, fx, fu = solver.linearize(mid, _dev(x0), _dev(Xp), _dev(Up), _dev(P))
    solver.sync()
    X_ = np.concatenate([x0[:, None], Xp[:, :-1]], 1)
    fo, fxo, fuo = cm.CLOSED_FORMS[name](X_, Up, P)
    f, fx, fu = f.cpu().numpy(), np.swapaxes(fx.cpu().numpy(), -1, -2), np.swapaxes(fu.cpu().numpy(), -1, -2)  # ABI blocks are [column][row]
    print(f"{name}: max |df| {np.abs(f - fo).max():.2e} |dfx| {np.abs(fx - fxo).max():.2e} |dfu| {np.abs(fu - fuo).max():.2e}")
    np.testing.assert_allclose(f, fo, **TOL)
    np.testing.assert_allclose(fx, fxo, **TOL)
    np.testing.assert_allclose(fu, fuo, **TOL)
    # stage 0 is linearised at x0, not at a stage of X_prev
    np.testing.assert_allclose(f[:, 0], cm.CLOSED_FORMS[name](x0[:, None], Up[:, :1], P)[0][:, 0], **TOL)
    assert np.abs(f[:, 0] - cm.CLOSED_FORMS[name](Xp[:, :1], Up[:, :1], P)[0][:, 0]).max() > 1e-3


# ---- the custom bicycle against built-in model 2 ---------------------------------------------------------------------------------
def test_bicycle_linearize_equals_the_builtin(models, solver):
    from pmpc_amd.device import MODEL_BICYCLE

    M, N = 70, 6  # 420 units: several blocks and a partial one
    x0, Xp, Up, P = (_dev(a) for a in cm.rand_inputs("bicycle", M, N, seed=4))
    mid = solver.load_model(models["bicycle"])
    got = solver.linearize(mid, x0, Xp, Up, P)
    want = solver.linearize(MODEL_BICYCLE, x0, Xp, Up, P)
    solver.sync()
    for g, w, what in zip(got, want, ("f", "fx", "fu")):
        np.testing.assert_allclose(g.cpu().numpy(), w.cpu().numpy(), err_msg=what, **TOL)


def test_bicycle_rollout_equals_the_builtin(models, solver):
    from pmpc_amd.device import MODEL_BICYCLE

    M, N = 70, 6  # crosses the 64-lane block
    x0, _, Up, P = (_dev(a) for a in cm.rand_inputs("bicycle", M, N, seed=5))
    mid = solver.load_model(models["bicycle"])
    got, want = solver.rollout(mid, x0, Up, P), solver.rollout(MODEL_BICYCLE, x0, Up, P)
    solver.sync()
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), **TOL)


@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("tail", [False, True])
def test_bicycle_shift_plan_equals_the_builtin(models, solver, s, tail):
    from pmpc_amd.device import MODEL_BICYCLE

    M, N = 70, 6
    _, Xp, Up, P = (_dev(a) for a in cm.rand_inputs("bicycle", M, N, seed=6))
    U_tail = _dev(np.random.default_rng(7).uniform(-0.5, 0.5, (M, s, 2))) if tail else None
    mid = solver.load_model(models["bicycle"])
    got = solver.shift_plan(mid, Xp, Up, P, s=s, U_tail=U_tail)
    want = solver.shift_plan(MODEL_BICYCLE, Xp, Up, P, s=s, U_tail=U_tail)
    solver.sync()
    for g, w, what in zip(got, want, ("X", "U", "um1")):
        np.testing.assert_allclose(g.cpu().numpy(), w.cpu().numpy(), err_msg=what, **TOL)
    np.testing.assert_array_equal(got[2].cpu().numpy(), Up[:, s - 1].cpu().numpy())  # um1: the control that was applied


# ---- the library loop on the custom pendulum ------------------------------------------------------------------------------------
def _pendulum_problem(M=8, N=6, seed=11):
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(8.0, 12.0, M), rng.uniform(0.1, 0.3, M), np.full(M, 0.05)], -1)
    x0 = np.stack([0.6 + 0.1 * rng.standard_normal(M), 0.2 * rng.standard_normal(M)], -1)
    return dict(x0=x0, Q=np.tile(np.diag([4.0, 1.0]), (M, N, 1, 1)), R=np.tile(0.1 * np.eye(1), (M, N, 1, 1)), X_ref=np.zeros((M, N, 2)),
                U_ref=np.zeros((M, N, 1)), X_prev=np.tile(x0[:, None], (1, N, 1)), U_prev=np.zeros((M, N, 1)), u_l=-3.0 * np.ones((M, N, 1)),
                u_u=3.0 * np.ones((M, N, 1)), reg_x=1.0, reg_u=1.0, solver_settings=dict(solver="osqp", Nc=1), params=P)


def test_library_loop_equals_the_python_loop_on_a_torch_callable(models, solver):
    """Custom pendulum, M 8, N 6, three iterations of `scp_loop` against `solve(device="cuda")` driving the same pendulum as a torch
    `f_fx_fu_fn`: residuals rtol 1e-6 / atol 1e-9, iterates atol 1e-6 (loop against loop)."""
    import torch

    import pmpc_amd
    from pmpc_amd.device import to_device_problem

    M, N = 8, 6
    prob = _pendulum_problem(M, N)
    d = to_device_problem(prob)
    P = d["params"][:, None, :]

    def f_fx_fu_fn(X, U):
        gl, damp, dt = P[..., 0], P[..., 1], P[..., 2]
        th, w = X[..., 0], X[..., 1]
        f = torch.stack([th + dt * w, w + dt * (U[..., 0] - gl * torch.sin(th) - damp * w)], -1)
        fx = torch.zeros(f.shape[:-1] + (2, 2), dtype=f.dtype, device=f.device)
        fu = torch.zeros(f.shape[:-1] + (2, 1), dtype=f.dtype, device=f.device)
        fx[..., 0, 0], fx[..., 0, 1] = 1.0, dt.expand(th.shape)
        fx[..., 1, 0], fx[..., 1, 1] = -dt * gl * torch.cos(th), (1.0 - dt * damp).expand(th.shape)
        fu[..., 1, 0] = dt.expand(th.shape)
        return f, fx, fu

    Xs, Us, data = pmpc_amd.solve(f_fx_fu_fn, prob["Q"], prob["R"], prob["x0"], device="cuda", X_ref=prob["X_ref"], U_ref=prob["U_ref"], X_prev=prob["X_prev"],
                                  U_prev=prob["U_prev"], u_l=prob["u_l"], u_u=prob["u_u"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], max_it=3, res_tol=0.0,
                                  verbose=False, solver_settings=dict(prob["solver_settings"]))
    assert len(data["hist"]) == 3
    mid = solver.load_model(models["pendulum"])
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    Xa, Ua, Xb, Ub = d["X_prev"].clone(), d["U_prev"].clone(), mk(M, N, 2), mk(M, N, 1)
    res, infos, last, done = solver.scp_loop(mid, d["params"], 3, f=mk(M, N, 2), fx=mk(M, N, 2, 2), fu=mk(M, N, 1, 2), f2=mk(M, N, 2), fx2=mk(M, N, 2, 2),
                                             fu2=mk(M, N, 1, 2), X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, first_cold=True, Q=d["Q"], R=d["R"],
                                             X_ref=d["X_ref"], U_ref=d["U_ref"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=1, x0=d["x0"], lu=d["lu"],
                                             uu=d["uu"], symmetric_cost=True)
    solver.sync()
    assert done == 3 and all(i["status"] == 0 for i in infos), infos
    X, U = ((Xb, Ub) if last else (Xa, Ua))
    X, U, res = X.cpu().numpy(), U.cpu().numpy(), res.cpu().numpy()
    want = np.array([h["resid"] for h in data["hist"]])
    print(f"pendulum loop: residuals {res} python loop {want}; max |dX| {np.abs(X - Xs[:, 1:]).max():.3e} max |dU| {np.abs(U - Us).max():.3e}")
    np.testing.assert_allclose(res, want, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(X, Xs[:, 1:], rtol=0, atol=1e-6)
    np.testing.assert_allclose(U, Us, rtol=0, atol=1e-6)
    # the same problem through the public front end with the CustomModel object
    Xc, Uc, _ = pmpc_amd.solve(None, prob["Q"], prob["R"], prob["x0"], device="cuda", builtin_model=models["pendulum"], params=prob["params"],
                               X_ref=prob["X_ref"], U_ref=prob["U_ref"], X_prev=prob["X_prev"], U_prev=prob["U_prev"], u_l=prob["u_l"], u_u=prob["u_u"],
                               reg_x=prob["reg_x"], reg_u=prob["reg_u"], max_it=3, res_tol=0.0, verbose=False, solver_settings=dict(prob["solver_settings"]))
    np.testing.assert_allclose(Xc, Xs, rtol=0, atol=1e-6)
    np.testing.assert_allclose(Uc, Us, rtol=0, atol=1e-6)


# ---- MPCController: the custom bicycle against builtin_model="bicycle" ----------------------------------------------------------
def _controller(model, prob, solver, **kw):
    import pmpc_amd

    args = dict(builtin_model=model, params=prob["params"], Q=prob["Q"], R=prob["R"], X_ref=prob["X_ref"], U_ref=prob["U_ref"], u_l=prob["u_l"],
                u_u=prob["u_u"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], solver_settings=dict(prob["solver_settings"]), solver=solver)
    args.update(kw)
    return pmpc_amd.MPCController(**args)


def _two_balls(prob):
    """Two balls of radius 0.3 per particle, 0.6 to the left of the particle's start plan at a third and two thirds of the horizon
    (tools/keepout_time.py make_cstr): the start plan is clear of them, the lane change has to go round them."""
    X = prob["X_prev"]
    M, N = X.shape[:2]
    centres = np.stack([X[:, j, :2] + np.array([0.0, 0.6]) for j in (N // 3, 2 * N // 3)], 1)
    return dict(pos_idx=(0, 1), centres=np.ascontiguousarray(np.broadcast_to(centres[:, None], (M, N, 2, 2))), radius=np.full(2, 0.3))


@pytest.mark.parametrize("case", ["plain", "warm_shift", "keepout"])
def test_controller_on_the_custom_bicycle_equals_the_builtin(models, case):
    """M 16, N 10, three steps of three iterations on two contexts fed the same measured states: plans atol 1e-6, statuses equal.  The
    custom model's loop runs on dense Jacobians, the built-in one's on compact records from the second iteration of a step on."""
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver

    M, N = 16, 10
    prob = dyn.make_bicycle_problem(M=M, N=N, Nc=1)
    kw = dict(warm_shift=True) if case == "warm_shift" else (dict(keepout=_two_balls(prob)) if case == "keepout" else {})
    rng = np.random.default_rng(9)
    s1, s2 = DeviceSolver(0), DeviceSolver(0)
    try:
        a, b = _controller(models["bicycle"], prob, s1, **kw), _controller("bicycle", prob, s2, **kw)
        assert a.model >= 1000 and b.model == 2
        for ctl in (a, b):
            ctl.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
        x0 = prob["x0"]
        for k in range(3):
            (ua, ia), (ub, ib) = a.step(x0, iterations=3), b.step(x0, iterations=3)
            sa, sb = [i["status"] for i in ia["infos"]], [i["status"] for i in ib["infos"]]
            dX, dU = float((a.X - b.X).abs().max()), float((a.U - b.U).abs().max())
            print(f"{case} step {k}: statuses {sa} / {sb}; warm {ia['warm_shift']} / {ib['warm_shift']}; max |dX| {dX:.3e} |dU| {dU:.3e}; "
                  f"residuals {ia['resid']} / {ib['resid']}")
            assert sa == sb and ia["status"] == ib["status"] and ia["warm_shift"] == ib["warm_shift"]
            assert ia["status"] == 0, ia
            np.testing.assert_allclose(a.X.cpu().numpy(), b.X.cpu().numpy(), rtol=0, atol=1e-6)
            np.testing.assert_allclose(a.U.cpu().numpy(), b.U.cpu().numpy(), rtol=0, atol=1e-6)
            np.testing.assert_allclose(ua, ub, rtol=0, atol=1e-6)
            noise = 0.0 if case == "keepout" else 0.01  # (a hard constraint: the plant is the model, tools/mpc_step_time.py)
            x0 = dyn.bicycle(np.broadcast_to(x0, (M, 4))[0], ub[0], prob["params"][0])[0] + noise * rng.standard_normal(4)
        if case == "warm_shift":
            assert ia["warm_shift"]  # the steps after the first one started warm on both
    finally:
        s1.close()
        s2.close()


def test_ring_model_runs_in_closed_loop(models):
    """x = 9, u = 3: a model no built-in id has the dimensions of (tests/test_mpc_gpu.py test_every_model_runs_in_closed_loop)."""
    from pmpc_amd.device import DeviceSolver

    M, N = 8, 10
    rng = np.random.default_rng(7)
    P = np.stack([rng.uniform(0.8, 1.2, M), np.full(M, 0.1)], -1)
    x0 = 0.4 * rng.standard_normal((M, 9))
    prob = dict(params=P, Q=np.tile(np.eye(9), (M, N, 1, 1)), R=np.tile(0.1 * np.eye(3), (M, N, 1, 1)), X_ref=np.zeros((M, N, 9)), U_ref=np.zeros((M, N, 3)),
                u_l=-np.ones((M, N, 3)), u_u=np.ones((M, N, 3)), reg_x=1.0, reg_u=1.0, solver_settings=dict(solver="osqp", Nc=1))
    s = DeviceSolver(0)
    try:
        ctl = _controller(models["ring"], prob, s)
        ctl.reset(X_prev=np.tile(x0[:, None], (1, N, 1)), U_prev=np.zeros((M, N, 3)))
        x = x0
        for k in range(2):
            u0, info = ctl.step(x, iterations=3)
            assert info["status"] == 0 and all(i["status"] == 0 for i in info["infos"]), info
            assert np.isfinite(u0).all() and np.isfinite(info["resid"]).all()
            assert np.all(u0 >= -1 - 1e-9) and np.all(u0 <= 1 + 1e-9)
            np.testing.assert_allclose(u0, np.broadcast_to(u0[0], u0.shape), rtol=0, atol=1e-12)  # Nc = 1: one first control
            # the plan's first state is the model's step from the measured state under the first control (the defect of stage 0 closes
            # with the SCP residual; 3 iterations from a constant start plan leave it small, not zero)
            x = cm.ring_np(np.broadcast_to(x, (M, 9))[:1, None], u0[:1, None], P[:1])[0][0, 0] + 0.01 * rng.standard_normal(9)
    finally:
        s.close()


# ---- id plumbing --------------------------------------------------------------------------------------------------------------------
def _loop_args(prob, d, sentinel):
    import torch

    M, N, x = d["X_prev"].shape
    u = d["U_prev"].shape[-1]
    mk = lambda *shape: torch.full(shape, sentinel, dtype=torch.float64, device="cuda")
    bufs = dict(f=mk(M, N, x), fx=mk(M, N, x, x), fu=mk(M, N, u, x), f2=mk(M, N, x), fx2=mk(M, N, x, x), fu2=mk(M, N, u, x), X_out=mk(M, N, x), U_out=mk(M, N, u))
    kw = dict(bufs, X_prev=d["X_prev"].clone(), U_prev=d["U_prev"].clone(), first_cold=True, Q=d["Q"], R=d["R"], X_ref=d["X_ref"], U_ref=d["U_ref"],
              reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=1, x0=d["x0"], lu=d["lu"], uu=d["uu"], symmetric_cost=True)
    return bufs, kw


def test_a_model_of_other_dimensions_is_refused_by_the_loop(models, solver):
    """The pendulum (2 + 1) on the bicycle problem (4 + 2): status 2, nothing is written."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import to_device_problem

    prob = dyn.make_bicycle_problem(M=8, N=6, Nc=1)
    d = to_device_problem(prob)
    mid = solver.load_model(models["pendulum"])
    bufs, kw = _loop_args(prob, d, -77.0)
    start = kw["X_prev"].clone(), kw["U_prev"].clone()
    res, infos, last, done = solver.scp_loop(mid, _dev(np.ones((8, 3))), 3, **kw)
    solver.sync()
    assert done == 0 and infos[0]["status"] == 2 and not last
    for name, t in bufs.items():
        assert bool(torch.all(t == -77.0)), name
    assert torch.equal(kw["X_prev"], start[0]) and torch.equal(kw["U_prev"], start[1])
    # the shape checks of the methods that hand the library no dimensions
    x0, Xp, Up, P = (_dev(a) for a in cm.rand_inputs("bicycle", 4, 5))
    with pytest.raises(ValueError, match="states of 4 and controls of 2"):
        solver.linearize(mid, x0, Xp, Up, _dev(np.ones((4, 3))))
    with pytest.raises(ValueError, match="params must be"):
        solver.rollout(solver.load_model(models["bicycle"]), x0, Up, _dev(np.ones((4, 3))))


def test_fp32_jacobians_are_refused_for_a_custom_model(models, solver):
    import torch

    x0, Xp, Up, P = (_dev(a) for a in cm.rand_inputs("bicycle", 4, 5))
    mid = solver.load_model(models["bicycle"])
    fx, fu = torch.full((4, 5, 4, 4), -77.0, dtype=torch.float32, device="cuda"), torch.full((4, 5, 2, 4), -77.0, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match=r"failed \(2\)"):
        solver.linearize(mid, x0, Xp, Up, P, fx=fx, fu=fu)
    solver.sync()
    assert bool(torch.all(fx == -77.0)) and bool(torch.all(fu == -77.0))
    assert solver.lib.pmpc_jac_compact_doubles(mid, 5, 4) == -1


def test_unloaded_and_never_loaded_ids_are_unknown(models):
    """An id after `unload_model`, an id of another context, and ids 3 and 999: the unknown-model code of every entry point, nothing runs."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver, to_device_problem

    prob = dyn.make_bicycle_problem(M=8, N=6, Nc=1)
    d = to_device_problem(prob)
    s, other = DeviceSolver(0), DeviceSolver(0)
    try:
        mid = s.load_model(models["bicycle"])
        f, fx, fu = s.linearize(mid, d["x0"], d["X_prev"], d["U_prev"], d["params"])
        s.sync()
        assert bool(torch.isfinite(fx).all())
        s.unload_model(mid)
        with pytest.raises(ValueError, match="not a custom model loaded"):
            s.unload_model(mid)
        lin = lambda sv, m, out: sv.lib.pmpc_linearize_device(sv.h, m, 6, 8, *(ctypes.c_void_p(t.data_ptr()) for t in (d["x0"], d["X_prev"], d["U_prev"], d["params"], *out)))
        mid2 = s.load_model(models["bicycle"])  # (loaded again: a new id; the old one stays unknown)
        assert mid2 != mid
        for sv, m in ((s, mid), (other, mid2), (s, 3), (s, 999), (s, 1000 + 10 ** 6)):
            out = [torch.full_like(t, -77.0) for t in (f, fx, fu)]
            assert lin(sv, m, out) == 2, m
            X = torch.full_like(d["X_prev"], -77.0)
            assert sv.lib.pmpc_rollout_device(sv.h, m, 6, 8, *(ctypes.c_void_p(t.data_ptr()) for t in (d["x0"], d["U_prev"], d["params"], X))) == 2, m
            with pytest.raises(RuntimeError, match=r"failed \(2\)"):
                sv.shift_plan(m, d["X_prev"], d["U_prev"], d["params"], s=1)
            bufs, kw = _loop_args(prob, d, -77.0)
            res, infos, last, done = sv.scp_loop(m, d["params"], 2, **kw)
            sv.sync()
            assert done == 0 and infos[0]["status"] == 2, m
            for name, t in list(bufs.items()) + [("f", out[0]), ("fx", out[1]), ("fu", out[2]), ("X", X)]:
                assert bool(torch.all(t == -77.0)), (m, name)
        assert lin(s, mid2, [f, fx, fu]) == 0  # the id that is loaded on this context still runs
        s.sync()
    finally:
        s.close()
        other.close()
