"""Keep-out constraints in the library SCP loop (`pmpc_scp_loop_device_cstr`, `DeviceSolver.scp_loop(cstr=, aug=)`) and in
`MPCController(keepout=...)` on the GPU: the strip-and-residual kernel against numpy and `scp_residual`, the NULL / kind-0 constraint
against the old entry point, the library loop against the Python-driven loop `solve(..., device="cuda", builtin_cstr=...)` (two drivers of
the same kernels), the library's refusals, and the controller against the step composed by hand.  fp64."""
import ctypes
import math

import numpy as np
import pytest

from tests.support.keepout_loop import (FEAS, SENTINEL, SETTINGS, guarded, guards_intact, library_loop, outside, python_loop, quadrotor_keepout_problem,
                                        rel, unicycle_keepout_problem)
from tests.support.keepout_problems import bicycle_keepout_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from pmpc_amd.device import DeviceSolver

    s = DeviceSolver(0)
    yield s
    s.close()


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


# ---- 1. the strip-and-residual kernel ---------------------------------------------------------------------------------------------------
def _strip(s, x, K, u, N, M, X_aug, Xo, Xp, Uo, Up, out):
    import torch

    from pmpc_amd.device import _p

    torch.cuda.synchronize()  # (the arrays were made on torch's stream; the launch goes to the solver's)
    st = s.lib.pmpc_keepout_strip_residual_device(s.h, x, K, u, N, M, _p(X_aug), _p(Xo), _p(Xp), _p(Uo), _p(Up), _p(out))
    s.sync()
    return st


@pytest.mark.parametrize("shape", [(1, 1, 4, 2, 1), (3, 5, 4, 2, 4), (2, 7, 3, 2, 2), (130, 33, 12, 4, 3), (2, 70, 3, 1, 1), (3, 9, 1, 16, 1)], ids=lambda c: "M%dN%dx%du%dK%d" % c)
def test_strip_and_residual_kernel(solver, shape):
    """Xo is the slice bit for bit, 64 guard doubles on both sides of it untouched; the residual is `scp_residual`'s of the stripped arrays
    (1e-15 relative: the same sums per row in the same order, and a maximum); a NaN row gives inf; a stale larger value in the slot does
    not survive; every refused call writes nothing."""
    import torch

    M, N, x, u, K = shape
    s = solver
    rng = np.random.default_rng(100 + M + N)
    Xa_np = rng.uniform(-1, 1, (M, N, x + K))
    X_aug, Xp, Uo, Up = _dev(Xa_np), _dev(rng.uniform(-1, 1, (M, N, x))), _dev(rng.uniform(-1, 1, (M, N, u))), _dev(rng.uniform(-1, 1, (M, N, u)))
    whole, Xo = guarded((M, N, x))
    out = torch.full((1,), 1e9, dtype=torch.float64, device="cuda")  # a stale larger value: the slot is zeroed first
    torch.cuda.synchronize()
    assert _strip(s, x, K, u, N, M, X_aug, Xo, Xp, Uo, Up, out) == 0
    assert guards_intact(whole)
    assert np.array_equal(Xo.cpu().numpy().view(np.int64), np.ascontiguousarray(Xa_np[..., :x]).view(np.int64))
    ref = float(s.scp_residual(Xo, Xp, Uo, Up)[0])
    s.sync()
    want = max(np.linalg.norm(Xa_np[..., :x] - Xp.cpu().numpy(), axis=-1).max(), np.linalg.norm((Uo - Up).cpu().numpy(), axis=-1).max())
    got = float(out[0])
    print(f"strip+residual {shape}: {got!r} scp_residual {ref!r} numpy {want!r}")
    assert abs(got - ref) <= 1e-15 * ref and abs(got - want) <= 1e-14 * want
    # the maximum in the controls: the U walk counts
    Ubig = Uo.clone()
    Ubig[M - 1, N - 1, u - 1] += 50.0
    assert _strip(s, x, K, u, N, M, X_aug, Xo, Xp, Ubig, Up, out) == 0
    ref = float(s.scp_residual(Xo, Xp, Ubig, Up)[0])
    assert abs(float(out[0]) - ref) <= 1e-15 * ref and ref > 40.0
    # a NaN in a kept entry of one row: inf; in an auxiliary entry: no effect
    bad = X_aug.clone()
    bad[M // 2, N - 1, x - 1] = math.nan
    assert _strip(s, x, K, u, N, M, bad, Xo, Xp, Uo, Up, out) == 0 and math.isinf(float(out[0]))
    bad = X_aug.clone()
    bad[M // 2, N - 1, x] = math.nan
    assert _strip(s, x, K, u, N, M, bad, Xo, Xp, Uo, Up, out) == 0 and float(out[0]) == got
    # refused: nothing is written
    Xo.fill_(SENTINEL)
    out.fill_(7.0)
    for args in ((x, 0, u, N, M), (x, 5, u, N, M), (17 - K, K, u, N, M), (x, K, 0, N, M), (x, K, 17, N, M), (x, K, u, 0, M), (x, K, u, N, 0)):
        assert _strip(s, *args, X_aug, Xo, Xp, Uo, Up, out) == 2, args
    for k in range(6):
        ptrs = [X_aug, Xo, Xp, Uo, Up, out]
        ptrs[k] = None
        assert _strip(s, x, K, u, N, M, *ptrs) == 2, k
    assert bool(torch.all(whole == SENTINEL)) and float(out[0]) == 7.0


# ---- 2. NULL and kind-0 constraint ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cost", [False, True])
def test_null_constraint_is_the_old_entry_point(with_cost):
    """pmpc_scp_loop_device_cstr(..., cstr NULL) and a kind-0 constraint against pmpc_scp_loop_device_cost: residuals, iterates and statuses
    bit for bit, a fresh context each, with and without a cost (`aug` NULL: it is not read)."""
    import torch

    from pmpc_amd import _lib
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver, to_device_problem
    from tests.test_lin_cost_gpu import OBSTACLES, _raw_loop

    prob = dyn.make_bicycle_problem(M=40, N=12, Nc=1)
    d = to_device_problem(prob)
    none = _lib.PmpcScpCstr(kind=0)
    runs = []
    for entry, tail in (("pmpc_scp_loop_device_cost", ()), ("pmpc_scp_loop_device_cstr", (None, None)), ("pmpc_scp_loop_device_cstr", (ctypes.byref(none), None))):
        s = DeviceSolver(0)
        try:
            sc, keep = s._scp_cost(OBSTACLES, 12, 4, "cuda") if with_cost else (None, None)
            runs.append(_raw_loop(s, entry, d, prob, 5, ((ctypes.byref(sc) if with_cost else None),) + tail))
            del keep
        finally:
            s.close()
    assert runs[0][0] == 5 and runs[0][4] == [0] * 5
    for r in runs[1:]:
        assert r[0] == 5 and r[4] == runs[0][4]
        assert torch.equal(r[1], runs[0][1]) and torch.equal(r[2], runs[0][2]) and torch.equal(r[3], runs[0][3])


# ---- 3. the library loop against the Python-driven loop ---------------------------------------------------------------------------------
def _fresh():
    from pmpc_amd.device import DeviceSolver

    return DeviceSolver(0)


def _both(model, kw, cstr, steps, settings=SETTINGS, cost=None):
    """The two drivers on a fresh context each: ((res, X, U, infos) of the library loop, (X, U, data) of the Python-driven one)."""
    s1, s2 = _fresh(), _fresh()
    try:
        lib = library_loop(s1, model, kw, cstr, steps, settings, cost=cost)
        over = dict(builtin_cost=cost) if cost is not None else {}
        py = python_loop(model, kw, cstr, steps, settings, solver=s2, **over)
    finally:
        s1.close()
        s2.close()
    assert py[0] is not None and len(py[2]["hist"]) == steps
    return lib, py


def test_library_loop_walks_the_python_driven_iterates():
    """`bicycle_keepout_problem()` (M 3, N 12, sub-problem at (5, 2)), steps = 1 .. 5: X, U and the residuals agree to 1e-9 relative (the bound
    of test_public_loop_with_a_torch_callable_equals_the_builtin_model for two drivers of the same kernels); every iterate is outside the
    ball by FEAS; a row binds in the final plan — the row is the half-space about the previous iterate (the plan after four iterations, which the
    four-iteration run returns bit for bit), so the clearance that is < 1e-6 is the row's, n'(p - c) - r; the distance to the ball itself grows
    along the tangent (measured: 1.4e-3 after five iterations, -1.0e-13 after one) —; without the constraint the same loop enters the ball by >= 0.2 radii.  Of the five
    iterations of the longest run at least one took the follow-up as enqueued behind the sub-problem's rounds and at least one did not
    (pmpc_scp_loop_follow_ups; the first, cold, iteration normally does not)."""
    from pmpc_amd import _lib

    from pmpc_amd.extra_cstrs import keepout_rows

    kw, cstr = bicycle_keepout_problem()
    r = float(cstr["radius"][0])
    X_before = kw["X_prev"]
    for steps in range(1, 6):
        _lib.scp_loop_follow_ups(reset=True)
        (res, X, U, infos), (Xp, Up, data) = _both("bicycle", kw, cstr, steps)
        behind, after = _lib.scp_loop_follow_ups()
        rp = np.array([h["resid"] for h in data["hist"]])
        clear = outside(X, cstr)
        print(f"keep-out library loop, {steps} iterations: rel X {rel(X, Xp[:, 1:]):.3e} U {rel(U, Up):.3e} resid {np.abs(res - rp).max() / max(rp.max(), 1.0):.3e}; "
              f"clearance {clear:.3e}; follow-ups behind the rounds {behind}, after the solve {after}; "
              f"(ipm, rounds) {[(i['ipm_iters'], i['active_set_rounds']) for i in infos]}")
        assert rel(X, Xp[:, 1:]) < 1e-9 and rel(U, Up) < 1e-9, (steps, rel(X, Xp[:, 1:]), rel(U, Up))
        np.testing.assert_allclose(res, rp, rtol=1e-9, atol=0)
        assert clear > -FEAS, (steps, clear)
        assert behind + after == steps
        a_x, h = keepout_rows(X_before, cstr)  # this iteration's rows: about the iterate before it
        row_clear = float((h - np.einsum("mnkx,mnx->mnk", a_x, X)).min())
        print(f"  clearance of the rows about the previous iterate {row_clear:.3e}")
        assert row_clear > -FEAS, (steps, row_clear)
        X_before = X
    assert row_clear < 1e-6  # a row binds at some stage of the final plan
    assert behind >= 1 and after >= 1, (behind, after)
    s = _fresh()
    try:
        _, Xf, _, _ = library_loop(s, "bicycle", kw, None, 5)
    finally:
        s.close()
    print(f"  without the constraint the plan enters the ball by {-outside(Xf, cstr) / r:.3f} radii")
    assert -outside(Xf, cstr) >= 0.2 * r


# ---- 4. other dispatches ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["unicycle_K2", "quadrotor_K1"])
def test_other_models(case):
    """Unicycle, K = 2, M 4, N 6 (x 4: the sub-problem runs at 6 states) and quadrotor, K = 1, M 2, N 5 (13 states: the generic kernels), per-particle
    centres; 3 iterations against the Python-driven loop, 1e-9 as above."""
    model, (kw, cstr) = ("unicycle", unicycle_keepout_problem()) if case == "unicycle_K2" else ("quadrotor", quadrotor_keepout_problem())
    (res, X, U, infos), (Xp, Up, data) = _both(model, kw, cstr, 3)
    rp = np.array([h["resid"] for h in data["hist"]])
    print(f"keep-out library loop {case}: rel X {rel(X, Xp[:, 1:]):.3e} U {rel(U, Up):.3e}; residuals {res} python-driven {rp}; clearance {outside(X, cstr):.3e}; "
          f"(ipm, rounds) {[(i['ipm_iters'], i['active_set_rounds']) for i in infos]}")
    assert rel(X, Xp[:, 1:]) < 1e-9 and rel(U, Up) < 1e-9
    np.testing.assert_allclose(res, rp, rtol=1e-9, atol=0)
    assert outside(X, cstr) > -FEAS


def test_with_the_builtin_cost_as_well():
    """The cost's shifted reference is the augmentation's X_ref, in the speculative follow-up too: 3 iterations, 1e-7 as
    test_public_loop_with_the_builtin_cost_as_well; the cost acts."""
    kw, cstr = bicycle_keepout_problem()
    cost = dict(kind="obstacles", pos_idx=(0, 1), centres=np.array([[2.0, 0.9]]), sigma=np.array([0.5]), w=np.array([2.0]))
    (res, X, U, _), (Xp, Up, data) = _both("bicycle", kw, cstr, 3, cost=cost)
    s = _fresh()
    try:
        _, Xn, _, _ = library_loop(s, "bicycle", kw, cstr, 3)
    finally:
        s.close()
    print(f"keep-out library loop with the obstacle cost: rel X {rel(X, Xp[:, 1:]):.3e} U {rel(U, Up):.3e}; the cost moves the plan by {rel(X, Xn):.3e}")
    assert rel(X, Xn) > 1e-3
    assert rel(X, Xp[:, 1:]) < 1e-7 and rel(U, Up) < 1e-7
    np.testing.assert_allclose(res, [h["resid"] for h in data["hist"]], rtol=1e-7, atol=0)
    assert outside(X, cstr) > -FEAS


@pytest.mark.parametrize("alpha", [None, 8.0])
def test_cone_objective(alpha):
    """The reference's default path as the sub-problem, hard and smoothed (log barrier 1 / alpha on the boxes, the rows' bounds among them):
    3 iterations, 1e-6, the cone state-row tolerance of tests/test_keepout_gpu.py."""
    kw, cstr = bicycle_keepout_problem()
    settings = dict(solver="ecos", Nc=1) if alpha is None else dict(solver="ecos", Nc=1, smooth_alpha=alpha)
    (res, X, U, _), (Xp, Up, data) = _both("bicycle", kw, cstr, 3, settings=settings)
    print(f"keep-out library loop, cone objective alpha {alpha}: rel X {rel(X, Xp[:, 1:]):.3e} U {rel(U, Up):.3e}; clearance {outside(X, cstr):.3e}")
    assert rel(X, Xp[:, 1:]) < 1e-6 and rel(U, Up) < 1e-6
    np.testing.assert_allclose(res, [h["resid"] for h in data["hist"]], rtol=1e-6, atol=0)
    assert outside(X, cstr) > -FEAS


# ---- 5. the library's refusals ----------------------------------------------------------------------------------------------------------
def _refusal_buffers(M, N, x, u, K, md=None):
    """Every buffer of a call, guarded and filled with SENTINEL: dict name -> (whole, view)."""
    import torch

    md = md or torch.float64
    xd = x + K
    shapes = dict(f=(M, N, x), fx=(M, N, x, x), fu=(M, N, u, x), f2=(M, N, x), fx2=(M, N, x, x), fu2=(M, N, u, x), Xa=(M, N, x), Ua=(M, N, u), Xb=(M, N, x),
                  Ub=(M, N, u), res=(3,), Q=(M, N, x, x), R=(M, N, u, u), aQ=(M, N, xd, xd), ax0=(M, xd), alx=(M, N, xd), aXo=(M, N, xd))
    for k in range(2):
        shapes.update({f"af{k}": (M, N, xd), f"afx{k}": (M, N, xd, xd), f"afu{k}": (M, N, u, xd), f"aXp{k}": (M, N, xd), f"aXr{k}": (M, N, xd), f"axu{k}": (M, N, xd)})
    return {k: guarded(v, dtype=md if k in ("fx", "fu", "fx2", "fu2", "Q", "R") else None) for k, v in shapes.items()}


REFUSALS = ["bad_pos_idx", "K5", "x13_K4", "null_aug", "null_buffer", "stage_cone", "slew", "slew0", "f32", "sharded", "squareplus"]


@pytest.mark.parametrize("case", REFUSALS)
def test_library_refusals(case):
    """Each combination the loop does not carry: 0 iterations, infos[0].status = 2, and not one byte of any buffer (guards included) written."""
    import torch

    from pmpc_amd import _lib
    from pmpc_amd.device import MODEL_BICYCLE, MODEL_QUADROTOR, DeviceSolver, _p

    M, N, u, K = 3, 4, 2, 1
    x, model = (13, MODEL_QUADROTOR) if case == "x13_K4" else (4, MODEL_BICYCLE)
    K = 4 if case == "x13_K4" else K
    md = torch.float32 if case == "f32" else torch.float64
    b = _refusal_buffers(M, N, x, u, K, md)
    v = lambda k: b[k][1]
    dz = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    kw = dict(f=v("f"), fx=v("fx"), fu=v("fu"), X_prev=v("Xa"), U_prev=v("Ua"), X_out=v("Xb"), U_out=v("Ub"), Q=v("Q"), R=v("R"), X_ref=dz(M, N, x), U_ref=dz(M, N, u),
              reg_x=1.0, reg_u=1.0, Nc=1, x0=dz(M, x), lu=dz(M, N, u) - 1.0, uu=dz(M, N, u) + 1.0, symmetric_cost=True)
    if case == "stage_cone":
        kw.update(soc_W=torch.eye(2, dtype=torch.float64, device="cuda"), soc_w0=dz(2), soc_v=dz(2), soc_v0=1.0, soc_u_interior=dz(2))
    elif case == "slew":
        kw.update(slew_reg=dz(M) + 0.1)
    elif case == "slew0":
        kw.update(slew_reg0=dz(M) + 0.1, slew_um1=dz(M, u))
    elif case == "squareplus":
        kw.update(smooth_cstr="squareplus", cone_objective=True, barrier_mu=0.125)
    cen, rad = dz(K, 2) + 5.0, dz(K) + 0.5
    cs = _lib.PmpcScpCstr(kind=1, K=5 if case == "K5" else K, pos_dim=2, pos_idx=(ctypes.c_int * 3)(0, 7 if case == "bad_pos_idx" else 1, 0),
                          centre_stride_particle=0, centre_stride_stage=0, centres=cen.data_ptr(), radius=rad.data_ptr())
    two = lambda name: (ctypes.c_void_p * 2)(_p(v(name + "0")), _p(v(name + "1")))
    ab = _lib.PmpcScpAug(Q=_p(v("aQ")), x0=_p(v("ax0")), lx=_p(v("alx")), f=two("af"), fx=two("afx"), fu=two("afu"), X_prev=two("aXp"), X_ref=two("aXr"),
                         xu=two("axu"), X_out=None if case == "null_buffer" else _p(v("aXo")))
    s = DeviceSolver(0)
    try:
        if case == "sharded":  # (the in-process stand-in communicator of tests/test_multirank_gpu.py: rank 0 of 2; nothing is ever sent)
            assert s.lib.pmpc_comm_init_mock(s.h, 0, 2, 9001) == 0
        prob, _, _ = s._problem(**kw)
        infos, last = (_lib.PmpcInfo * 3)(), ctypes.c_int(5)
        torch.cuda.synchronize()
        done = s.lib.pmpc_scp_loop_device_cstr(s.h, model, _p(dz(M, 4)), ctypes.byref(prob), _p(v("f2")), _p(v("fx2"), md), _p(v("fu2"), md), 3, 1, _p(v("res")), infos,
                                               ctypes.byref(last), None, ctypes.byref(cs), None if case == "null_aug" else ctypes.byref(ab))
        s.sync()
    finally:
        s.close()
    assert done == 0 and infos[0].status == 2 and last.value == 0
    for name, (whole, _) in b.items():
        assert bool(torch.all(whole == SENTINEL)), name


# ---- 6. the controller ------------------------------------------------------------------------------------------------------------------
def _controller(kw, solver, **over):
    import pmpc_amd

    args = dict(builtin_model="bicycle", params=kw["params"], Q=kw["Q"], R=kw["R"], X_ref=kw["X_ref"], U_ref=kw["U_ref"], u_l=kw["u_l"], u_u=kw["u_u"],
                reg_x=kw["reg_x"], reg_u=kw["reg_u"], solver_settings=dict(SETTINGS), solver=solver)
    args.update(over)
    return pmpc_amd.MPCController(**args)


def test_controller_with_keepout():
    """`bicycle_keepout_problem(M=3, N=12)`, 4 MPC steps of 3 iterations, the plant particle 0's model through `DeviceSolver.rollout`.  Each
    step equals the numpy `shift_plan` of the previous plan followed by `solve(device="cuda", builtin_cstr=..., X_prev=, U_prev=, max_it=3,
    res_tol=0)` to 1e-6 (chained solves: the bound of the loop-against-host test); every plan is outside the ball; moving the ball with
    `set_keepout` moves the next plan and the new plan clears the moved ball; without `keepout` the first plan is inside the ball; the
    failed state is kept until `reset`."""
    import torch

    from pmpc_amd import dynamics as dyn

    M, N = 3, 12
    kw, cstr = bicycle_keepout_problem(M=M, N=N)
    keepout = {k: cstr[k] for k in ("pos_idx", "centres", "radius")}
    s1, s2 = _fresh(), _fresh()
    try:
        ctl = _controller(kw, s1, keepout=keepout)
        ctl.reset(X_prev=kw["X_prev"], U_prev=kw["U_prev"])
        X_start, U_start, x0 = kw["X_prev"], kw["U_prev"], kw["x0"]
        p0 = _dev(kw["params"][:1])
        for k in range(4):
            u0, info = ctl.step(x0, iterations=3)
            assert info["status"] == 0 and info["iterations_done"] == 3 and u0.shape == (M, 2), info
            X, U = ctl.X.cpu().numpy(), ctl.U.cpu().numpy()
            Xh, Uh, dh = python_loop("bicycle", dict(kw, x0=np.array(np.broadcast_to(x0, (M, 4))), X_prev=X_start, U_prev=U_start), cstr, 3, solver=s2)
            assert Xh is not None
            print(f"keep-out MPC step {k}: rel X {rel(X, Xh[:, 1:]):.3e} U {rel(U, Uh):.3e}; residuals {info['resid']} hand-composed {[h['resid'] for h in dh['hist']]}; "
                  f"clearance {outside(X, cstr):.3e}")
            assert rel(X, Xh[:, 1:]) < 1e-6 and rel(U, Uh) < 1e-6
            np.testing.assert_array_equal(u0, U[:, 0])
            assert outside(X, cstr) > -FEAS
            X_start, U_start, _ = dyn.shift_plan("bicycle", X, U, kw["params"], s=1)
            x0 = s1.rollout(ctl.model, _dev(np.array(np.broadcast_to(x0, (M, 4))[:1])), _dev(u0[:1, None, :]), p0)[0, 0].cpu().numpy()
        # the ball moves away from the side the plan passes on: the next plan follows, and clears the moved ball
        moved = dict(cstr, centres=np.array([[2.4, -0.3]]))
        X_before = ctl.X.cpu().numpy()
        ctl.set_keepout(centres=moved["centres"])
        u0, info = ctl.step(x0, iterations=3)
        assert info["status"] == 0
        X_moved = ctl.X.cpu().numpy()
        Xh, Uh, _ = python_loop("bicycle", dict(kw, x0=np.array(np.broadcast_to(x0, (M, 4))), X_prev=X_start, U_prev=U_start), moved, 3, solver=s2)
        Xs, _, _ = python_loop("bicycle", dict(kw, x0=np.array(np.broadcast_to(x0, (M, 4))), X_prev=X_start, U_prev=U_start), cstr, 3, solver=s2)
        print(f"keep-out MPC, moved ball: rel to the hand-composed step {rel(X_moved, Xh[:, 1:]):.3e}; the move changes the plan by {rel(X_moved, Xs[:, 1:]):.3e}; "
              f"clearance of the moved ball {outside(X_moved, moved):.3e}")
        assert rel(X_moved, Xh[:, 1:]) < 1e-6
        assert rel(X_moved, Xs[:, 1:]) > 1e-3 and not np.array_equal(X_moved, X_before)
        assert outside(X_moved, moved) > -FEAS
        with pytest.raises(ValueError, match="radius"):
            ctl.set_keepout(radius=np.array([-1.0]))
        # the failed state (not provoked: what a failed sub-problem leaves), as tests/test_mpc_gpu.py
        ctl.failed = True
        with pytest.raises(RuntimeError, match="reset"):
            ctl.step(x0, iterations=3)
        ctl.reset(X_prev=kw["X_prev"], U_prev=kw["U_prev"])
        u0, info = ctl.step(kw["x0"], iterations=3)
        assert info["status"] == 0 and not ctl.failed and outside(ctl.X.cpu().numpy(), moved) > -FEAS
        # without the constraint: through the ball
        free = _controller(kw, s2)
        free.reset(X_prev=kw["X_prev"], U_prev=kw["U_prev"])
        with pytest.raises(ValueError, match="without keepout"):
            free.set_keepout(centres=moved["centres"])
        u0, info = free.step(kw["x0"], iterations=3)
        assert info["status"] == 0
        print(f"  without keepout the first plan enters the ball by {-outside(free.X.cpu().numpy(), cstr):.3f}")
        assert outside(free.X.cpu().numpy(), cstr) < 0.0
        assert torch.isfinite(ctl.X).all()
    finally:
        s1.close()
        s2.close()
