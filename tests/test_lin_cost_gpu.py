"""Linearised nonlinear costs on the GPU (pmpc_amd/csrc/cost_lin.hip): the reference shift `ref - A^-1 c`, the built-in obstacle
cost, `lin_cost_fn` / `builtin_cost` of the public device solve against the host loop, and the library's loop with a cost against
the Python-driven one."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _spd_blocks(rng, rows, d):
    """diag(0.1 .. 10) + B B', eigenvalues raised to lambda_max / 1e3 (condition number <= 1e3), exactly symmetric."""
    B = rng.standard_normal((rows, d, d))
    A = np.diag(np.linspace(0.1, 10.0, d))[None] + B @ np.swapaxes(B, -1, -2)
    w, V = np.linalg.eigh(A)
    w = np.maximum(w, w.max(-1, keepdims=True) / 1e3)
    A = (V * w[:, None, :]) @ np.swapaxes(V, -1, -2)
    return 0.5 * (A + np.swapaxes(A, -1, -2))


@pytest.fixture(scope="module")
def solver():
    from pmpc_amd.device import DeviceSolver

    s = DeviceSolver(0)
    yield s
    s.close()


# ---- a. ref_shift -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 407, 6500])
@pytest.mark.parametrize("dim", [2, 4, 12, 7])
def test_ref_shift_equals_numpy_solve(solver, dim, rows):
    """out = ref - A^-1 c against np.linalg.solve: max |difference| <= 1e-10 max |result| (cond <= 1e3, so cond dim eps <= 3e-12 rel.);
    dims 2, 4, 12 are the compiled bodies, 7 the generic one; 407 = 37 x 11 rows end inside a workgroup of every body, 6500 take
    several workgroups.  Then the same with `out` aliasing `ref`: bit for bit the same."""
    import torch

    rng = np.random.default_rng(100 * dim + rows)
    A, c, ref = _spd_blocks(rng, rows, dim), rng.standard_normal((rows, dim)), rng.standard_normal((rows, dim))
    want = ref - np.linalg.solve(A, c[..., None])[..., 0]
    Ad, cd, rd = _dev(A), _dev(c), _dev(ref)
    out = solver.ref_shift(Ad, cd, rd)
    solver.sync()
    err = float(np.abs(out.cpu().numpy() - want).max()) / float(np.abs(want).max())
    print(f"ref_shift dim {dim} rows {rows}: max |out - numpy| / max |numpy| = {err:.3e}")
    assert err <= 1e-10
    assert torch.equal(rd, _dev(ref))  # (the inputs are not written)
    alias = rd.clone()
    got = solver.ref_shift(Ad, cd, alias, out=alias)
    solver.sync()
    assert got is alias and torch.equal(alias, out)


def test_ref_shift_refuses_one_indefinite_block_among_407(solver):
    """Block 123 has a negative eigenvalue: its row of `out` is NaN, every other row is as without it, the call raises ValueError —
    and the counter is cleared by that read: the next call on good blocks passes."""
    rng = np.random.default_rng(7)
    rows, dim = 407, 4
    A, c, ref = _spd_blocks(rng, rows, dim), rng.standard_normal((rows, dim)), rng.standard_normal((rows, dim))
    good = solver.ref_shift(_dev(A), _dev(c), _dev(ref)).cpu().numpy()
    w, V = np.linalg.eigh(A[123])
    w[1] = -0.5
    A[123] = (V * w) @ V.T
    A[123] = 0.5 * (A[123] + A[123].T)
    out = _dev(np.zeros((rows, dim)))
    with pytest.raises(ValueError, match="not symmetric positive definite"):
        solver.ref_shift(_dev(A), _dev(c), _dev(ref), out=out)
    got = out.cpu().numpy()
    assert np.isnan(got[123]).all()
    keep = np.arange(rows) != 123
    np.testing.assert_array_equal(got[keep], good[keep])
    assert bool(solver.ref_shift(_dev(_spd_blocks(rng, 5, dim)), _dev(c[:5]), _dev(ref[:5])).isfinite().all())


def test_ref_shift_refuses_dimension_17(solver):
    import torch

    A, c = _dev(np.tile(np.eye(17), (3, 1, 1))), _dev(np.ones((3, 17)))
    out = torch.full((3, 17), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        solver.ref_shift(A, c, c, out=out)
    assert solver.lib.pmpc_ref_shift_device(solver.h, 17, 3, A.data_ptr(), c.data_ptr(), c.data_ptr(), out.data_ptr()) == 2  # (the ABI itself)
    solver.sync()
    assert bool((out == 7.0).all())


# ---- b. obstacle cost ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_stage", [False, True])
@pytest.mark.parametrize("M,N,x,pos_idx", [(37, 11, 4, (0, 1)), (5, 3, 12, (0, 1, 2))])
def test_obstacle_cost_grad_equals_the_numpy_specification(solver, M, N, x, pos_idx, per_stage):
    """k_obstacle_grad against pmpc_amd.dynamics.obstacle_cost: abs 1e-13 max w / min sigma (a gradient entry is a sum of K = 3 terms
    bounded by 0.61 w / sigma, each a product of a handful of correctly rounded factors and one exponential).  The fused form against
    ref_shift(Q, cx, X_ref) of the stand-alone gradient: bit for bit, or 1e-14 relative."""
    import torch

    from pmpc_amd import dynamics as dyn

    rng = np.random.default_rng(1000 * M + 10 * x + per_stage)
    K, pd = 3, len(pos_idx)
    X = 2.0 * rng.standard_normal((M, N, x))
    cost = dict(kind="obstacles", pos_idx=pos_idx, centres=rng.standard_normal((N, K, pd) if per_stage else (K, pd)),
                sigma=rng.uniform(0.5, 2.0, K), w=rng.uniform(0.1, 1.0, K))
    want = dyn.obstacle_cost(X, cost)[1]
    Xd = _dev(X)
    cx = solver.obstacle_cost_grad(Xd, cost)
    solver.sync()
    err, tol = float(np.abs(cx.cpu().numpy() - want).max()), 1e-13 * cost["w"].max() / cost["sigma"].min()
    print(f"obstacle gradient ({M}, {N}, {x}) per_stage {per_stage}: max |cx - numpy| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    assert np.abs(want).max() > 1e-2  # (the point is not in the tails of every bump)
    Q, Xref = _dev(_spd_blocks(rng, M * N, x).reshape(M, N, x, x)), _dev(rng.standard_normal((M, N, x)))
    two = solver.ref_shift(Q, cx, Xref)
    fused = solver.obstacle_cost_grad(Xd, cost, Q=Q, X_ref=Xref)
    solver.sync()
    rel = float((fused - two).abs().max() / two.abs().max())
    print(f"  fused against two launches: bitwise {torch.equal(fused, two)}, max relative difference {rel:.3e}")
    assert torch.equal(fused, two) or rel <= 1e-14


# ---- c. public solve ----------------------------------------------------------------------------------------------------------------
# Two bumps beside the lane-change path of make_bicycle_problem(M=8, N=15) (which passes (3.0, 0.9) and (5.5, 1.9)): sigma = 1 m,
# w = 3 against the lateral weight Q_yy = 10.
OBSTACLES = dict(kind="obstacles", pos_idx=(0, 1), centres=np.array([[3.0, 0.2], [5.5, 2.5]]), sigma=np.array([1.0, 1.0]), w=np.array([3.0, 3.0]))
CU_WEIGHT = 0.05  # the control cost of the callable case: 0.025 |u|^2, gradient 0.05 u


def _min_distance(X):
    return min(float(np.linalg.norm(X[:, 1:, :2] - c, axis=-1).min()) for c in OBSTACLES["centres"])


@pytest.fixture(scope="module")
def lane_change():
    """The problem, its solve arguments, and the device solve WITHOUT a cost (shared by the two cases below)."""
    import pmpc_amd
    from pmpc_amd import dynamics as dyn

    prob = dyn.make_bicycle_problem(M=8, N=15, Nc=1)
    kw = dict(X_ref=prob["X_ref"], U_ref=prob["U_ref"], X_prev=prob["X_prev"], U_prev=prob["U_prev"], u_l=prob["u_l"], u_u=prob["u_u"],
              reg_x=prob["reg_x"], reg_u=prob["reg_u"], max_it=8, res_tol=0.0, verbose=False, solver_settings=dict(solver="osqp", Nc=1))
    X0, _, _ = pmpc_amd.solve(None, prob["Q"], prob["R"], prob["x0"], device="cuda", builtin_model="bicycle", params=prob["params"], **kw)
    return prob, kw, X0


def _compare_with_host_loop(prob, kw, X0, host_fn, device_kw):
    import pmpc_amd

    Xh, Uh, dh = pmpc_amd.solve(prob["f_fx_fu_fn"], prob["Q"], prob["R"], prob["x0"], lin_cost_fn=host_fn, **kw)
    Xd, Ud, dd = pmpc_amd.solve(None, prob["Q"], prob["R"], prob["x0"], device="cuda", builtin_model="bicycle", params=prob["params"], **device_kw, **kw)
    resid = [h["resid"] for h in dh["hist"]]
    print("host residuals", " ".join(f"{r:.4e}" for r in resid))
    print("iterations", len(dh["hist"]), len(dd["hist"]), "max |dX|", np.abs(Xd - Xh).max(), "max |dU|", np.abs(Ud - Uh).max())
    d0, d1 = _min_distance(X0), _min_distance(Xd)
    print(f"closest approach to an obstacle centre: {d0:.4f} m without the cost, {d1:.4f} m with it")
    assert len(dd["hist"]) == len(dh["hist"]) == 8
    assert all(b < a for a, b in zip(resid, resid[1:])), resid  # (the case is a converging SCP loop, as its docstring states)
    for a, b in zip(dd["hist"], dh["hist"]):
        assert abs(a["resid"] - b["resid"]) <= 1e-6 * abs(b["resid"]) and abs(a["obj"] - b["obj"]) <= 1e-6 * abs(b["obj"]), (a, b)
    np.testing.assert_allclose(Xd, Xh, rtol=0, atol=1e-7)
    np.testing.assert_allclose(Ud, Uh, rtol=0, atol=1e-7)
    assert d1 >= d0 + 0.05, (d0, d1)


def test_public_solve_with_the_builtin_obstacle_cost_equals_the_host_loop(lane_change):
    """`solve(None, ..., device="cuda", builtin_model="bicycle", builtin_cost=OBSTACLES)` (fused kernel) against the host loop with
    `make_obstacle_lin_cost_fn(OBSTACLES)`: 8 iterations (res_tol = 0), `hist` rows rel 1e-6, trajectories 1e-7 — the bounds of
    test_public_solve_with_the_builtin_bicycle_equals_the_host_loop; both legs run the same solver on references that differ by
    rounding.  The cost acts: the closest approach over (particle, stage) to an obstacle centre grows by at least 0.05 m.
    On an MI355X the host loop's residual falls in every iteration: 2.1428e+00 9.2273e-01 5.4978e-01 3.9754e-01 2.4470e-01 2.0417e-01
    1.3288e-01 1.2621e-01; closest approach 0.3799 m without the cost, 0.4435 m with it."""
    from pmpc_amd import dynamics as dyn

    prob, kw, X0 = lane_change
    _compare_with_host_loop(prob, kw, X0, dyn.make_obstacle_lin_cost_fn(OBSTACLES), dict(builtin_cost=OBSTACLES))


def test_public_solve_with_a_torch_lin_cost_fn_equals_the_host_loop(lane_change):
    """The same with a callable that returns GPU tensors (cx, cu), cu = CU_WEIGHT u: the shift of U_ref runs the dim = 2 body on R.
    On an MI355X the host loop's residuals: 2.1428e+00 9.2362e-01 5.2884e-01 3.6704e-01 2.0675e-01 1.7104e-01 1.3182e-01 7.8458e-02;
    closest approach 0.3799 m without the cost, 0.4410 m with it."""
    import torch

    from pmpc_amd import dynamics as dyn

    prob, kw, X0 = lane_change
    seen = []

    def device_fn(X_prev, U_prev, problems):
        seen.append((X_prev.is_cuda and U_prev.is_cuda and torch.is_tensor(problems["Q"]), tuple(X_prev.shape), tuple(U_prev.shape)))
        return dyn.obstacle_cost_torch(X_prev, OBSTACLES)[1], CU_WEIGHT * U_prev

    def host_fn(X_prev, U_prev, problems):
        return dyn.obstacle_cost(X_prev, OBSTACLES)[1], CU_WEIGHT * U_prev

    _compare_with_host_loop(prob, kw, X0, host_fn, dict(lin_cost_fn=device_fn))
    assert len(seen) == 8 and all(s == (True, (8, 15, 4), (8, 15, 2)) for s in seen), seen


def test_costs_need_symmetric_blocks_and_the_other_host_only_features_stay_refused(lane_change):
    import pmpc_amd
    from pmpc_amd import dynamics as dyn

    prob, kw, _ = lane_change
    common = dict(device="cuda", builtin_model="bicycle", params=prob["params"], **kw)
    Qn = prob["Q"].copy()
    Qn[..., 0, 1] += 0.1
    for extra in (dict(builtin_cost=OBSTACLES), dict(lin_cost_fn=dyn.make_obstacle_lin_cost_fn(OBSTACLES))):
        with pytest.raises(ValueError, match="symmetric"):
            pmpc_amd.solve(None, Qn, prob["R"], prob["x0"], **extra, **common)
    for extra in (dict(cost_fn=lambda *a: None), dict(extra_cstrs_fns=lambda *a: None), dict(filter_method="AA")):
        with pytest.raises(ValueError, match="does not support"):
            pmpc_amd.solve(None, prob["Q"], prob["R"], prob["x0"], **extra, **common)


# ---- d. library loop ----------------------------------------------------------------------------------------------------------------
QUAD_OBSTACLES = dict(kind="obstacles", pos_idx=(0, 1, 2), centres=np.array([[0.5, 0.5, 0.5], [-1.0, 0.0, 0.5]]), sigma=np.array([1.0, 1.5]),
                      w=np.array([2.0, 1.0]))


def _moving(cost, N):
    """The same obstacles drifting 0.05 m per stage along +x: per-stage centres (N, K, pos_dim)."""
    c = np.tile(cost["centres"][None], (N, 1, 1))
    c[..., 0] += 0.05 * np.arange(N)[:, None]
    return dict(cost, centres=c)


def _loops(mid, prob, cost, steps, first_cold):
    """(residuals, X, U) of the Python-driven loop linearize -> obstacle_cost_grad -> ref_shift -> lqp_solve -> residual -> swap and of
    the library's loop with `cost`, a fresh context each.  first_cold False: both legs first run ONE cold iteration driven from Python,
    and the `steps` compared iterations start from its outputs (the warm-start promise of the library loop's first iteration)."""
    import torch

    from pmpc_amd.device import DeviceSolver, to_device_problem

    d = to_device_problem(prob)
    M, N, x = d["X_prev"].shape
    u = d["U_prev"].shape[-1]
    Nc = prob["solver_settings"]["Nc"]
    common = dict(Q=d["Q"], R=d["R"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=Nc, x0=d["x0"], lu=d["lu"], uu=d["uu"], symmetric_cost=True)
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")

    def python_iterations(s, Xa, Ua, Xb, Ub, n, cold_first):
        res = []
        for it in range(n):
            f, fx, fu = s.linearize(mid, d["x0"], Xa, Ua, d["params"])
            Xr = s.ref_shift(d["Q"], s.obstacle_cost_grad(Xa, cost), d["X_ref"])
            _, _, st = s.lqp_solve(f=f, fx=fx, fu=fu, X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, X_ref=Xr, U_ref=d["U_ref"], static_cons_bounds=True,
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
                out.append((res.cpu().numpy(), X.clone(), U.clone(), infos))
        finally:
            s.close()
    return out


@pytest.mark.parametrize("first_cold", [True, False])
@pytest.mark.parametrize("Nc", [1, -1])
def test_library_loop_with_a_cost_walks_the_python_driven_iterates(Nc, first_cold):
    """6 iterations on the bicycle (M 40, N 12) with moving obstacles, atol 1e-6 on residuals and iterates (the bound of
    test_library_loop_on_the_bicycle_equals_the_python_driven_loop).  Nc = 1: the warm solves are active-set rounds with the next
    linearisation AND its shift enqueued speculatively behind them, on compact Jacobian records; first_cold: the first iteration
    linearises into the dense sets."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_BICYCLE

    prob = dyn.make_bicycle_problem(M=40, N=12, Nc=Nc)
    cost = _moving(dict(OBSTACLES, centres=np.array([[1.5, 0.2], [3.5, 2.5]])), 12)
    (rp, Xp, Up, _), (rl, Xl, Ul, infos) = _loops(MODEL_BICYCLE, prob, cost, 6, first_cold)
    print("Nc", Nc, "first_cold", first_cold, "residuals", rl, "python-driven", rp, [(i["ipm_iters"], i["active_set_rounds"]) for i in infos])
    print("  max |dX|", float((Xl - Xp).abs().max()), "max |dU|", float((Ul - Up).abs().max()))
    np.testing.assert_allclose(rl, rp, rtol=0, atol=1e-6)
    assert torch.allclose(Xl, Xp, rtol=0, atol=1e-6) and torch.allclose(Ul, Up, rtol=0, atol=1e-6)
    assert np.isfinite(rl).all() and rl[-1] < rl[0]


def test_library_loop_with_a_cost_on_the_quadrotor():
    """dim = 12 body of the fused shift with 3-D obstacles: M 8, N 10, Nc 1, 6 iterations, the same bound."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_QUADROTOR

    prob = dyn.make_quadrotor_problem(M=8, N=10, Nc=1)
    (rp, Xp, Up, _), (rl, Xl, Ul, infos) = _loops(MODEL_QUADROTOR, prob, QUAD_OBSTACLES, 6, True)
    print("quadrotor residuals", rl, "python-driven", rp, "max |dX|", float((Xl - Xp).abs().max()), "max |dU|", float((Ul - Up).abs().max()))
    np.testing.assert_allclose(rl, rp, rtol=0, atol=1e-6)
    assert torch.allclose(Xl, Xp, rtol=0, atol=1e-6) and torch.allclose(Ul, Up, rtol=0, atol=1e-6)


def _raw_loop(s, entry, d, prob, steps, cost_ptr, f32=False):
    """One library loop through `entry` (an ABI symbol name) from the problem's start iterate on a primed context."""
    import torch

    from pmpc_amd import _lib
    from pmpc_amd.device import MODEL_BICYCLE, _p

    M, N, x = d["X_prev"].shape
    u = d["U_prev"].shape[-1]
    md = torch.float32 if f32 else torch.float64
    mk = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device="cuda")
    Xa, Ua, Xb, Ub = d["X_prev"].clone(), d["U_prev"].clone(), mk(M, N, x), mk(M, N, u)
    bufs = [mk(M, N, x), mk(M, N, x, x, dtype=md), mk(M, N, u, x, dtype=md), mk(M, N, x), mk(M, N, x, x, dtype=md), mk(M, N, u, x, dtype=md)]
    prob_c, _, _ = s._problem(f=bufs[0], fx=bufs[1], fu=bufs[2], X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, Q=d["Q"].to(md), R=d["R"].to(md),
                              X_ref=d["X_ref"], U_ref=d["U_ref"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=1, x0=d["x0"], lu=d["lu"], uu=d["uu"],
                              symmetric_cost=True)
    res = torch.zeros((steps,), dtype=torch.float64, device="cuda")
    infos, last = (_lib.PmpcInfo * steps)(), ctypes.c_int(0)
    args = [s.h, MODEL_BICYCLE, _p(d["params"]), ctypes.byref(prob_c), _p(bufs[3]), _p(bufs[4], md), _p(bufs[5], md), steps, 1, _p(res), infos, ctypes.byref(last)]
    torch.cuda.synchronize()
    done = getattr(s.lib, entry)(*args, *cost_ptr)
    s.sync()
    X, U = (Xb, Ub) if last.value else (Xa, Ua)
    return done, res.clone(), X.clone(), U.clone(), [infos[k].status for k in range(steps)]


def test_null_cost_is_the_old_entry_point_and_fp32_storage_with_a_cost_is_refused():
    """pmpc_scp_loop_device_cost(..., NULL) and a kind-0 cost against pmpc_scp_loop_device: the same residuals and iterates bit for bit
    (a fresh context each).  pmpc_scp_loop_device IS a call of the new entry point with NULL, so what this pins is that a kind-0 cost
    is no cost and that the old symbol still answers; that a NULL cost enqueues what the parent commit enqueued is shown by the
    parent / branch comparison of bench.py, not here.  A cost next to PMPC_F32_MATRICES: 0 iterations, infos[0].status = 2, nothing
    written."""
    import torch

    from pmpc_amd import _lib
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver, to_device_problem

    prob = dyn.make_bicycle_problem(M=40, N=12, Nc=1)
    d = to_device_problem(prob)
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
    s = DeviceSolver(0)
    try:
        sc, keep = s._scp_cost(OBSTACLES, 12, 4, "cuda")
        done, res, X, U, status = _raw_loop(s, "pmpc_scp_loop_device_cost", d, prob, 3, (ctypes.byref(sc),), f32=True)
        assert done == 0 and status[0] == 2
        assert torch.equal(X, d["X_prev"]) and torch.equal(U, d["U_prev"])
        # ... and through the Python method: the same refusal
        mk = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda")
        M, N, x, u = 40, 12, 4, 2
        _, infos, _, done = s.scp_loop(2, d["params"], 3, f=mk(M, N, x, dtype=torch.float64), fx=mk(M, N, x, x), fu=mk(M, N, u, x), f2=mk(M, N, x, dtype=torch.float64),
                                       fx2=mk(M, N, x, x), fu2=mk(M, N, u, x), X_prev=d["X_prev"].clone(), U_prev=d["U_prev"].clone(), Q=d["Q"].float(),
                                       R=d["R"].float(), X_ref=d["X_ref"], U_ref=d["U_ref"], reg_x=1.0, reg_u=1.0, Nc=1, x0=d["x0"], lu=d["lu"], uu=d["uu"],
                                       symmetric_cost=True, cost=OBSTACLES)
        assert done == 0 and infos[0]["status"] == 2
    finally:
        s.close()
