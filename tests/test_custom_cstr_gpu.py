"""Custom state constraints on the GPU (pmpc_amd/csrc/cstr_jit.hip, cstr_kernels.h, cstr_rows.hip): the rows kernel against the closed
forms and against the keep-out rows, the dense-row augmentation kernel against its numpy specification, the entry points' refusals, the
count of rows that had to be dropped, one sub-problem against the oracle, a linear constraint against the state box it is, the library
loop against the Python-driven loop, the built-in keep-out and the host loop, the three kinds of custom code on one solver, and the
controller.  fp64.  Each test constraint is compiled once per process (tests/support/custom_cstrs.py `make`)."""
import ctypes
import math

import numpy as np
import pytest

from tests.support import custom_cstrs as cg
from tests.support.keepout_loop import FEAS, SENTINEL, SETTINGS, guarded, guards_intact, library_loop, outside, python_loop, rel, unicycle_keepout_problem
from tests.support.keepout_problems import bicycle_keepout_problem, keepout_subproblem, rows_of

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-12, atol=1e-12)  # AD against closed forms (tests/test_custom_model.py)
SUB_TOL = 1e-7  # TOL of tests/test_keepout_gpu.py: one sub-problem against the oracle


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _devT(a):
    return _dev(np.swapaxes(a, -1, -2))


def _fresh():
    from pmpc_amd.device import DeviceSolver

    return DeviceSolver(0)


@pytest.fixture(scope="module")
def solver():
    s = _fresh()
    yield s
    s.close()


def _custom(name, P):
    return dict(kind="custom", cstr=cg.make(name), params=P)


# ---- 1. the rows kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(1, 1), (5, 3), (37, 11)])
@pytest.mark.parametrize("name", cg.NAMES)
def test_rows_kernel_equals_the_closed_forms(solver, name, M, N):
    """a, h and g against numpy at 1e-12; guard doubles around the three outputs intact; the inputs unwritten; g=None gives the same a and
    h.  (1, 1): one unit; (5, 3): a partial block; (37, 11): 407 units in six blocks of 64 and one of 23."""
    import torch

    x, K, pd = cg.entry(name)["dims"]
    X, P = cg.rand_inputs(name, M, N, seed=M + N)
    a_ref, h_ref, g_ref = cg.rows_np(name, X, P)
    Xd, Pd = _dev(X), _dev(P)
    keep = [Xd.clone(), Pd.clone()]
    (wa, a), (wh, h), (wg, g) = guarded((M, N, K, x)), guarded((M, N, K)), guarded((M, N, K))
    torch.cuda.synchronize()
    got = solver.custom_cstr_rows(cg.make(name), Xd, Pd, value=g, a=a, h=h, check=True)
    solver.sync()
    assert got[0] is a and got[1] is h and got[2] is g
    assert guards_intact(wa) and guards_intact(wh) and guards_intact(wg)
    assert torch.equal(Xd, keep[0]) and torch.equal(Pd, keep[1])
    np.testing.assert_allclose(a.cpu().numpy(), a_ref, **TOL)
    np.testing.assert_allclose(h.cpu().numpy(), h_ref, **TOL)
    np.testing.assert_allclose(g.cpu().numpy(), g_ref, **TOL)
    a2, h2 = solver.custom_cstr_rows(cg.make(name), Xd, Pd)
    solver.sync()
    assert torch.equal(a2, a) and torch.equal(h2, h)


def test_rows_of_balls_are_the_keepout_rows(solver):
    from pmpc_amd.extra_cstrs import keepout_rows

    M, N = 5, 3
    rng = np.random.default_rng(8)
    X = rng.uniform(-1, 1, (M, N, 4))
    cstr = dict(kind="keepout", pos_idx=(0, 1), centres=rng.uniform(2, 3, (2, 2)), radius=np.array([0.3, 0.6]))  # (every |pbar - c| >= 1)
    a, h = solver.custom_cstr_rows(cg.make("balls"), _dev(X), _dev(cg.ball_params(cstr, M)), check=True)
    solver.sync()
    a_ref, h_ref = keepout_rows(X, cstr)
    np.testing.assert_allclose(a.cpu().numpy(), a_ref, **TOL)
    np.testing.assert_allclose(h.cpu().numpy(), h_ref, **TOL)


# ---- 2. the augmentation kernel ----------------------------------------------------------------------------------------------------------
AUG_SHAPES = [(1, 1, 4, 2, 1), (3, 11, 4, 2, 2), (2, 5, 12, 4, 4), (2, 3, 15, 1, 1), (2, 3, 1, 16, 4)]


@pytest.mark.parametrize("with_ref", [True, False], ids=["xref", "noxref"])
@pytest.mark.parametrize("shape", AUG_SHAPES, ids=lambda s: "M%dN%dx%du%dK%d" % s)
def test_augmentation_kernel_equals_the_numpy_specification(solver, shape, with_ref):
    """Copied and zero entries bit for bit; combined entries within 1e-13 max(1, |entry|), the bound of tests/test_keepout_gpu.py for the
    keep-out kernel; guard doubles untouched; of x_u~ only the auxiliary entries written; X_ref~ left alone without an X_ref.
    (3, 11): 33 units, one workgroup of 32 and one unit."""
    import torch

    from pmpc_amd.extra_cstrs import rows_augment

    M, N, x, u, K = shape
    xd = x + K
    rng = np.random.default_rng(500 + AUG_SHAPES.index(shape) + int(with_ref))
    U = lambda *s: rng.uniform(-1, 1, s)
    a, h, f, fx, fu, Xp, Xr = U(M, N, K, x), U(M, N, K), U(M, N, x), U(M, N, x, x), U(M, N, x, u), U(M, N, x), U(M, N, x)
    spec = rows_augment(a, h, np.zeros((M, x)), f, fx, fu, Xp, Xr, np.zeros((M, N, x, x)), 1.0)
    want = dict(f=spec["f"], fx=np.swapaxes(spec["fx"], -1, -2), fu=np.swapaxes(spec["fu"], -1, -2), X_prev=spec["X_prev"], X_ref=spec["X_ref"])
    shapes = dict(f=(M, N, xd), fx=(M, N, xd, xd), fu=(M, N, u, xd), X_prev=(M, N, xd), X_ref=(M, N, xd), xu=(M, N, xd))
    whole, out = {}, {}
    for k, sh in shapes.items():
        whole[k], out[k] = guarded(sh)
    ins = [_dev(a), _dev(h), _dev(Xp), _dev(f), _devT(fx), _devT(fu)]
    keep = [t.clone() for t in ins]
    torch.cuda.synchronize()
    got = solver.rows_augment(*ins, X_ref=_dev(Xr) if with_ref else None, out=out)
    solver.sync()
    assert got is out
    assert all(torch.equal(p, q) for p, q in zip(ins, keep))  # the inputs are not written
    for k in shapes:
        assert guards_intact(whole[k]), f"{k}: guard doubles written"
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if not with_ref:
        assert np.all(res["X_ref"] == SENTINEL)
    worst = 0.0
    for k in ("f", "fx", "fu", "X_prev") + (("X_ref",) if with_ref else ()):
        g, w = res[k], want[k]
        comb = np.zeros(g.shape, bool)
        if k in ("f", "fx", "fu"):
            comb[..., x:] = True
        if k == "fx":
            comb[..., x:, :] = False  # columns >= x: zero
        assert np.array_equal(g[~comb].view(np.int64), w[~comb].view(np.int64)), f"{k}: a copied or zero entry differs"
        if comb.any():
            err = np.max(np.abs(g[comb] - w[comb]) / np.maximum(1.0, np.abs(w[comb])))
            worst = max(worst, err)
            assert err <= 1e-13, (k, err)
    assert np.all(res["xu"][..., :x] == SENTINEL)  # the caller's bounds
    assert np.array_equal(res["xu"][..., x:], h)
    print(f"rows_augment {shape}: max relative difference of a combined entry {worst:.3e}")


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------
def test_invalid_calls_return_2_and_launch_nothing(solver):
    import torch

    from pmpc_amd import _lib

    M, N, x, u, K = 2, 3, 4, 2, 2
    rng = np.random.default_rng(43)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    gid = solver.load_cstr(cg.make("speed_band"))
    other = _fresh()
    try:
        foreign = other.load_cstr(cg.make("speed_band"))
        # the rows entry
        X, P = _dev(rng.uniform(-1, 1, (M, N, x))), _dev(rng.uniform(0, 1, (M, 3)))
        outs = [torch.full(s, SENTINEL, dtype=torch.float64, device="cuda") for s in ((M, N, K, x), (M, N, K), (M, N, K))]
        torch.cuda.synchronize()
        rows = lambda id_=gid, N_=N, M_=M, X_=X, P_=P, o=outs, ctx=solver.h: solver.lib.pmpc_custom_cstr_rows_device(ctx, id_, N_, M_, vp(X_), vp(P_), *[vp(t) for t in o])
        assert foreign != gid  # (one table for the process: an id is owned by the context that loaded it)
        bad = [dict(id_=gid + 1000), dict(id_=5), dict(id_=foreign), dict(ctx=other.h), dict(ctx=None), dict(N_=0), dict(M_=0), dict(X_=None), dict(P_=None),
               dict(o=[None, outs[1], outs[2]]), dict(o=[outs[0], None, outs[2]])]
        for kw in bad:
            assert rows(**kw) == 2, kw
        solver.sync()
        other.sync()
        # the augmentation entry
        ins = [_dev(rng.uniform(-1, 1, s)) for s in ((M, N, K, x), (M, N, K), (M, N, x), (M, N, x), (M, N, x, x), (M, N, u, x), (M, N, x))]
        big = [torch.full(s, SENTINEL, dtype=torch.float64, device="cuda") for s in ((M, N, 16), (M, N, 16, 16), (M, N, 16, 16), (M, N, 16), (M, N, 16), (M, N, 16))]
        torch.cuda.synchronize()

        def aug(K_=K, x_=x, u_=u, N_=N, M_=M, ins_=None, outs_=None, ctx=solver.h):
            return solver.lib.pmpc_rows_augment_device(ctx, K_, x_, u_, N_, M_, *[vp(t) for t in (ins_ or ins)], *[vp(t) for t in (outs_ or big)])

        bad = [dict(K_=0), dict(K_=5), dict(K_=-1), dict(x_=13, K_=4), dict(x_=15), dict(x_=0), dict(u_=0), dict(u_=17), dict(N_=0), dict(M_=0), dict(ctx=None)]
        for i in range(6):  # a null input (X_ref, the seventh, may be null)
            bad.append(dict(ins_=[None if j == i else t for j, t in enumerate(ins)]))
        for i in range(6):  # a null output; X_ref_aug may be null only when X_ref is
            bad.append(dict(outs_=[None if j == i else t for j, t in enumerate(big)]))
        for kw in bad:
            assert aug(**kw) == 2, kw
        # pmpc_keepout_augment_device answers a kind-2 descriptor with 2
        sc = _lib.PmpcScpCstr(kind=2, K=K, id=gid, gparams=P.data_ptr())
        assert solver.lib.pmpc_keepout_augment_device(solver.h, ctypes.byref(sc), x, u, N, M, *[vp(t) for t in ins[2:]], *[vp(t) for t in big]) == 2
        solver.sync()
        assert all(bool((t == SENTINEL).all()) for t in outs + big)  # nothing was launched
        assert solver.lib.pmpc_cstr_bad_rows(solver.h, 0) == 0
        # the controls: the valid calls run, g and X_ref / X_ref_aug may be null
        assert rows() == 0 and rows(o=[outs[0], outs[1], None]) == 0
        xd = x + K
        ok = [torch.full(s, SENTINEL, dtype=torch.float64, device="cuda") for s in ((M, N, xd), (M, N, xd, xd), (M, N, u, xd), (M, N, xd), (M, N, xd), (M, N, xd))]
        torch.cuda.synchronize()
        assert aug(outs_=ok) == 0 and aug(ins_=ins[:6] + [None], outs_=ok[:4] + [None, ok[5]]) == 0
        solver.sync()
        assert not bool((outs[0] == SENTINEL).any()) and not bool((ok[0] == SENTINEL).any())
        # unloading: an unknown id, a foreign id and a null context are refused
        assert solver.lib.pmpc_cstr_unload(solver.h, gid + 1000) == 2 and solver.lib.pmpc_cstr_unload(solver.h, foreign) == 2
        assert solver.lib.pmpc_cstr_unload(None, gid) == 2
    finally:
        other.close()


# ---- 4. rows that cannot be linearised -----------------------------------------------------------------------------------------------------
def test_a_row_with_a_non_finite_value_is_dropped_and_counted():
    import pmpc_amd

    M, N = 2, 3
    rng = np.random.default_rng(4)
    X = rng.uniform(0.5, 1.5, (M, N, 4))
    X[1, 2, 0] = -0.7
    P = np.full((M, 1), 0.2)
    s = _fresh()
    try:
        a, h, g = s.custom_cstr_rows(cg.make("log"), _dev(X), _dev(P), value=True)
        s.sync()
        a, h, g = a.cpu().numpy(), h.cpu().numpy(), g.cpu().numpy()
        assert s.lib.pmpc_cstr_bad_rows(s.h, 0) == 1
        assert h[1, 2, 0] == math.inf and not a[1, 2].any() and not np.isnan(h).any() and np.isnan(g[1, 2, 0])
        good = np.ones((M, N), bool)
        good[1, 2] = False
        a_ref, h_ref, _ = cg.rows_np("log", X, P)
        np.testing.assert_allclose(a[good], a_ref[good], **TOL)
        np.testing.assert_allclose(h[good], h_ref[good], **TOL)
        with pytest.raises(ValueError, match="1 constraint row"):
            s.check_bad_rows("test")
        assert s.lib.pmpc_cstr_bad_rows(s.h, 0) == 0  # read and cleared
        # solve(device=...): one stage of the start plan has a negative x0, where log(x0) is undefined (the bound itself, x0 >= e^-5, is loose)
        kw, _ = unicycle_keepout_problem()
        Xneg = kw["X_prev"].copy()
        Xneg[1, 2, 0] = -0.5
        with pytest.raises(ValueError, match="non-finite value or gradient"):
            python_loop("unicycle", dict(kw, X_prev=Xneg), _custom("log", np.full((4, 1), -5.0)), 2, solver=s)
        # the solver answers the next call
        X, U, data = python_loop("unicycle", kw, None, 2, solver=s)
        assert X is not None and len(data["hist"]) == 2
        assert isinstance(pmpc_amd.CustomConstraint, type)
    finally:
        s.close()


# ---- 5. one sub-problem against the oracle -------------------------------------------------------------------------------------------------
EXACT_CASES = [(9710, 1, 4, 4, 2, 1, 2, 1), (9711, 2, 4, 4, 2, 1, 2, 1)]  # tests/test_keepout_gpu.py: seed, M, N, x, u, K, pd, Nc


def _z_of(X, U, Nc):
    return np.concatenate([U[0, :Nc].reshape(-1), U[:, Nc:].reshape(-1), X.reshape(-1)])


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "M%dN%dK%d" % (c[1], c[2], c[5]))
def test_sub_problem_with_balls_equals_the_joint_qp_with_the_rows_as_rows(solver, case, oracle):
    """The inputs of tests/test_keepout_gpu.py's EXACT_CASES with the constraint imposed as `balls`: rows kernel -> augmentation kernel ->
    the solve at x + K states, against the oracle's joint QP with the keep-out rows as rows.  Checked with the oracle on the CPU before the
    cases were committed: 1 of 4 and 2 of 8 rows bind."""
    import torch

    seed, M, N, x, u, K, pd, Nc = case
    args, kw, cstr = keepout_subproblem(seed, M, N, x, u, K, pd)
    tup, rows = rows_of(cstr, args, Nc)
    Xo, Uo = oracle.lqp_solve_py(*args, Nc=Nc, rows=rows, **kw)
    slack_o = rows[0] @ _z_of(Xo, Uo, Nc) - rows[1]
    assert np.sum(slack_o > -FEAS) > 0  # the oracle says a row binds
    x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref = args
    name = f"balls_{x}_{K}_{pd}"
    p = dict(f=_dev(f), fx=_devT(fx), fu=_devT(fu), X_prev=_dev(X_prev), U_prev=_dev(U_prev), Q=_devT(Q), R=_devT(R), X_ref=_dev(X_ref), U_ref=_dev(U_ref),
             reg_x=kw["reg_x"], reg_u=kw["reg_u"], Nc=Nc, x0=_dev(x0), lu=_dev(kw["u_l"]), uu=_dev(kw["u_u"]),
             symmetric_cost=bool(np.array_equal(Q, np.swapaxes(Q, -1, -2)) and np.array_equal(R, np.swapaxes(R, -1, -2))))
    a, h = solver.custom_cstr_rows(cg.make(name), p["X_prev"], _dev(cg.ball_params(cstr, M)), check=True)
    aug = solver.rows_augment(a, h, p["X_prev"], p["f"], p["fx"], p["fu"], X_ref=p["X_ref"])
    xd = x + K
    aug["xu"][..., :x] = float("inf")
    Qa = torch.zeros((M, N, xd, xd), dtype=torch.float64, device="cuda")
    Qa[..., :x, :x] = p["Q"]
    Qa[..., torch.arange(x, xd), torch.arange(x, xd)] = -float(kw["reg_x"])
    x0a = torch.zeros((M, xd), dtype=torch.float64, device="cuda")
    x0a[:, :x] = p["x0"]
    p.update(f=aug["f"], fx=aug["fx"], fu=aug["fu"], X_prev=aug["X_prev"], X_ref=aug["X_ref"], Q=Qa, x0=x0a, ux=aug["xu"],
             lx=torch.full((M, N, xd), -float("inf"), dtype=torch.float64, device="cuda"))
    X, U, status = solver.lqp_solve(**p)
    solver.sync()
    assert status == 0
    X, U = X.cpu().numpy()[..., :x], U.cpu().numpy()
    slack = rows[0] @ _z_of(X, U, Nc) - rows[1]
    print(f"custom balls {case}: device against the joint QP: rel X {rel(X, Xo):.3e} U {rel(U, Uo):.3e}; max(G z - h) {slack.max():.3e}, binding {int(np.sum(slack > -FEAS))}")
    assert rel(X, Xo) < SUB_TOL and rel(U, Uo) < SUB_TOL, (rel(X, Xo), rel(U, Uo))
    assert slack.max() < FEAS and np.sum(slack > -FEAS) > 0


# ---- 6. the library loop -------------------------------------------------------------------------------------------------------------------
def _loop(s, kw, model, steps, cstr=None, cost=None, x_l=None, x_u=None, settings=SETTINGS):
    """`steps` iterations of the library loop on `s` from the problem's start iterate, every buffer fresh, state boxes and a custom model
    allowed: (residuals, X, U, infos, done) as numpy."""
    import torch

    from pmpc_amd.custom_model import CustomModel
    from pmpc_amd.device_problem import build_problem, keepout_buffers

    p = build_problem(kw["Q"], kw["R"], kw["x0"], kw["X_ref"], kw["U_ref"], kw["X_prev"], kw["U_prev"], x_l, x_u, kw["u_l"], kw["u_u"], kw["reg_x"],
                      kw["reg_u"], None, None, dict(settings), None, model, kw["params"], "cuda")
    M, N, x, u = p.M, p.N, p.xdim, p.udim
    mid = s.load_model(p.model) if isinstance(p.model, CustomModel) else p.model
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    handle = aug = None
    if cstr is not None:
        handle = s.prepare_cstr(cstr, M, N, x)
        aug = keepout_buffers(p, handle[0].K)
    Xb, Ub = mk(M, N, x), mk(M, N, u)
    torch.cuda.synchronize()
    res, infos, last, done = s.scp_loop(mid, p.params, steps, f=mk(M, N, x), fx=mk(M, N, x, x), fu=mk(M, N, u, x), f2=mk(M, N, x), fx2=mk(M, N, x, x),
                                        fu2=mk(M, N, u, x), X_prev=p.X_prev, U_prev=p.U_prev, X_out=Xb, U_out=Ub, X_ref=p.X_ref, U_ref=p.U_ref,
                                        cost=cost, cstr=handle, aug=aug, **p.solve_kw())
    s.sync()
    X, U = (Xb, Ub) if last else (p.X_prev, p.U_prev)
    return res.cpu().numpy(), X.cpu().numpy(), U.cpu().numpy(), infos, done


def test_a_linear_constraint_is_a_state_box():
    """`speed_band` with constant bounds 0 <= v <= 1.8 on the bicycle (M 3, N 6; the plan is asked to hold 2 m/s), four iterations of the
    library loop, against the same loop with x_l / x_u on v and no constraint: 1e-6, the project's parity bound.  The upper bound is active
    in the final plan."""
    M, N, vmin, vmax = 3, 6, 0.0, 1.8
    kw, _ = bicycle_keepout_problem(M=M, N=N)
    x_l, x_u = np.full((M, N, 4), -np.inf), np.full((M, N, 4), np.inf)
    x_l[..., 3], x_u[..., 3] = vmin, vmax
    s1, s2 = _fresh(), _fresh()
    try:
        rc, Xc, Uc, ic, dc = _loop(s1, kw, "bicycle", 4, cstr=_custom("speed_band", np.tile([vmax, 0.0, vmin], (M, 1))))
        rb, Xb, Ub, ib, db = _loop(s2, kw, "bicycle", 4, x_l=x_l, x_u=x_u)
    finally:
        s1.close()
        s2.close()
    assert dc == db == 4 and all(i["status"] == 0 for i in ic + ib), (ic, ib)
    print(f"speed band against the state box after 4 iterations: rel X {rel(Xc, Xb):.3e} U {rel(Uc, Ub):.3e}; max v {Xc[..., 3].max()!r}")
    assert rel(Xc, Xb) < 1e-6 and rel(Uc, Ub) < 1e-6, (rel(Xc, Xb), rel(Uc, Ub))
    assert Xc[..., 3].max() <= vmax + FEAS and Xc[..., 3].max() > vmax - 1e-6  # a bound is active


def test_library_loop_with_balls_walks_the_python_driven_iterates_and_the_builtin_keepout():
    """`unicycle_keepout_problem()` with the constraint as `balls`, steps = 1 .. 4: the library loop against the Python-driven loop, two
    drivers of the same kernels, at 1e-9 (tests/test_keepout_loop_gpu.py); against the built-in keep-out constraint, another lowering of the
    same rows, at the 1e-6 parity bound; every plan clears the balls by FEAS."""
    kw, cstr = unicycle_keepout_problem()
    custom = _custom("balls", cg.ball_params(cstr, 4))
    for steps in range(1, 5):
        s1, s2, s3 = _fresh(), _fresh(), _fresh()
        try:
            res, X, U, infos = library_loop(s1, "unicycle", kw, custom, steps)
            Xp, Up, data = python_loop("unicycle", kw, custom, steps, solver=s2)
            rk, Xk, Uk, _ = library_loop(s3, "unicycle", kw, cstr, steps)
        finally:
            for s in (s1, s2, s3):
                s.close()
        assert Xp is not None and len(data["hist"]) == steps
        rp = np.array([h["resid"] for h in data["hist"]])
        print(f"custom balls, {steps} iterations: library against Python-driven rel X {rel(X, Xp[:, 1:]):.3e} U {rel(U, Up):.3e}; against the built-in keep-out "
              f"rel X {rel(X, Xk):.3e} U {rel(U, Uk):.3e}; clearance {outside(X, cstr):.3e}")
        assert rel(X, Xp[:, 1:]) < 1e-9 and rel(U, Up) < 1e-9, (steps, rel(X, Xp[:, 1:]), rel(U, Up))
        np.testing.assert_allclose(res, rp, rtol=1e-9, atol=0)
        assert rel(X, Xk) < 1e-6 and rel(U, Uk) < 1e-6, (steps, rel(X, Xk), rel(U, Uk))
        assert outside(X, cstr) > -FEAS, (steps, outside(X, cstr))


def test_public_loop_with_a_custom_constraint_equals_the_host_loop():
    """5 iterations (res_tol = 0) of `solve(device="cuda", builtin_model="bicycle", builtin_cstr=dict(kind="custom", ...))` against the host
    loop with `extra_cstrs_fns=make_rows_extra_cstrs_fn(...)`: 1e-6, the bound of test_public_loop_equals_the_host_loop_with_extra_cstrs_fns."""
    import pmpc_amd
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.extra_cstrs import make_rows_extra_cstrs_fn

    kw, cstr = bicycle_keepout_problem()
    M = kw["x0"].shape[0]
    P = cg.ball_params(cstr, M)
    fn = cg.entry("balls_4_1_2")["np"]
    Xd, Ud, dd = python_loop("bicycle", kw, _custom("balls_4_1_2", P), 5)
    pp = kw["params"][:, None, :]
    keys = ("X_ref", "U_ref", "X_prev", "U_prev", "u_l", "u_u", "reg_x", "reg_u")
    Xh, Uh, dh = pmpc_amd.solve(lambda X, U: dyn.bicycle(X, U, pp), kw["Q"], kw["R"], kw["x0"],
                                extra_cstrs_fns=make_rows_extra_cstrs_fn(lambda Z: fn(Z, P)[0], lambda Z: fn(Z, P)[1], SETTINGS["Nc"]),
                                **{k: kw[k] for k in keys}, max_it=5, res_tol=0.0, verbose=False, solver_settings=dict(SETTINGS))
    assert Xd is not None and Xh is not None and len(dd["hist"]) == len(dh["hist"]) == 5
    print(f"custom constraint: device against host after 5 iterations: rel X {rel(Xd, Xh):.3e} U {rel(Ud, Uh):.3e}; clearance {outside(Xd[:, 1:], cstr):.3e}")
    assert rel(Xd, Xh) < 1e-6 and rel(Ud, Uh) < 1e-6, (rel(Xd, Xh), rel(Ud, Uh))
    assert outside(Xd[:, 1:], cstr) > -FEAS


def test_a_keepout_loop_is_the_same_before_and_after_a_constraint_was_loaded():
    """A kind-1 loop on `unicycle_keepout_problem()`: the same bits before and after a custom constraint has been loaded and run on the context."""
    kw, cstr = unicycle_keepout_problem()
    s = _fresh()
    try:
        before = library_loop(s, "unicycle", kw, cstr, 3)
        a, h = s.custom_cstr_rows(cg.make("balls"), _dev(kw["X_prev"]), _dev(cg.ball_params(cstr, 4)), check=True)
        library_loop(s, "unicycle", kw, _custom("balls", cg.ball_params(cstr, 4)), 2)
        fresh = _fresh()
        try:
            again_fresh = library_loop(fresh, "unicycle", kw, cstr, 3)
        finally:
            fresh.close()
        s2 = _fresh()
        try:
            s2.load_cstr(cg.make("balls"))
            after = library_loop(s2, "unicycle", kw, cstr, 3)
        finally:
            s2.close()
    finally:
        s.close()
    for k in range(3):
        assert np.array_equal(before[k], after[k]) and np.array_equal(before[k], again_fresh[k]), k


# ---- 7. the three kinds of custom code on one solver ---------------------------------------------------------------------------------------
def test_a_custom_model_cost_and_constraint_on_one_solver():
    """The bicycle as a custom model, `soft_speed` as a custom cost and `speed_band` as a custom constraint in one library loop; unloading
    one leaves the others working; an unloaded constraint id is refused with status 2 (nothing runs)."""
    from pmpc_amd import _lib
    from tests.support import custom_costs as cc
    from tests.support import custom_models as cm

    M, N = 3, 6
    kw, _ = bicycle_keepout_problem(M=M, N=N)
    model = cm.make("bicycle")
    cost = dict(kind="custom", cost=cc.make("soft_speed"), params=np.tile([1.0, 4.0, 1.9, 0.1], (M, 1)))
    band = _custom("speed_band", np.tile([1.8, 0.3, 0.0], (M, 1)))
    s = _fresh()
    try:
        res, X, U, infos, done = _loop(s, kw, model, 3, cstr=band, cost=cost)
        assert done == 3 and all(i["status"] == 0 for i in infos), infos
        j = np.arange(N)[None, :]
        assert (X[..., 3] <= 1.8 - 0.3 * j / N + FEAS).all() and (X[..., 3] >= -FEAS).all()  # the band, tightening along the horizon
        gid = s.load_cstr(band["cstr"])
        assert gid >= _lib.CSTR_CUSTOM0 and s.load_cstr(band["cstr"]) == gid
        s.unload_cost(s.load_cost(cost["cost"]))
        r2, X2, U2, i2, d2 = _loop(s, kw, model, 3, cstr=band)  # the model and the constraint are still there
        assert d2 == 3 and all(i["status"] == 0 for i in i2), i2
        stale = s.prepare_cstr(band, M, N, 4)
        s.unload_cstr(gid)
        r3, X3, U3, i3, d3 = _loop(s, kw, model, 3, cost=cost)  # the model and the (reloaded) cost work without it
        assert d3 == 3 and all(i["status"] == 0 for i in i3), i3
        r4, X4, U4, i4, d4 = _loop(s, kw, model, 3, cstr=stale)  # ... the constraint's id is gone
        assert d4 == 0 and i4[0]["status"] == 2
        with pytest.raises(ValueError, match="not a custom constraint loaded"):
            s.unload_cstr(gid)
        r5, X5, U5, i5, d5 = _loop(s, kw, "bicycle", 3, cstr=band)  # loaded again on first use; the built-in model
        assert d5 == 3 and rel(X5, X2) < 1e-6
    finally:
        s.close()


# ---- 8. the library's refusals ---------------------------------------------------------------------------------------------------------------
def test_library_loop_refuses_what_it_cannot_run():
    """An id that is not the context's, null parameters, a K that is not the constraint's, a constraint of another state dimension:
    status 2 before anything runs, the outputs untouched."""
    import torch

    from pmpc_amd import _lib
    from pmpc_amd.device_problem import build_problem, keepout_buffers

    M, N = 3, 6
    kw, _ = bicycle_keepout_problem(M=M, N=N)
    s = _fresh()
    try:
        band = s.prepare_cstr(_custom("speed_band", np.tile([1.8, 0.0, 0.0], (M, 1))), M, N, 4)
        sc, keep = band
        mk = lambda **over: (_lib.PmpcScpCstr(**{**dict(kind=2, K=sc.K, id=sc.id, gparams=sc.gparams), **over}), keep)
        three = s.prepare_cstr(_custom("generic_3_3", np.ones((M, 6))), M, N, 3)  # a constraint of other dimensions
        for what, handle in (("unknown id", mk(id=sc.id + 500)), ("null gparams", mk(gparams=None)), ("K not the constraint's", mk(K=1)),
                             ("xdim not the problem's", mk(id=three[0].id, K=3))):
            # (the buffers fit the descriptor's K, so that nothing but the descriptor is wrong)
            p = build_problem(kw["Q"], kw["R"], kw["x0"], kw["X_ref"], kw["U_ref"], kw["X_prev"], kw["U_prev"], None, None, kw["u_l"], kw["u_u"], kw["reg_x"],
                              kw["reg_u"], None, None, dict(SETTINGS), None, "bicycle", kw["params"], "cuda")
            e = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
            aug = keepout_buffers(p, handle[0].K)
            Xb = torch.full((M, N, 4), SENTINEL, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            _, infos, _, done = s.scp_loop(p.model, p.params, 2, f=e(M, N, 4), fx=e(M, N, 4, 4), fu=e(M, N, 2, 4), f2=e(M, N, 4), fx2=e(M, N, 4, 4), fu2=e(M, N, 2, 4),
                                           X_prev=p.X_prev, U_prev=p.U_prev, X_out=Xb, U_out=e(M, N, 2), X_ref=p.X_ref, U_ref=p.U_ref, cstr=handle, aug=aug,
                                           **p.solve_kw())
            s.sync()
            assert done == 0 and infos[0]["status"] == 2, what
            assert bool((Xb == SENTINEL).all()), what
    finally:
        s.close()


# ---- 9. MPCController --------------------------------------------------------------------------------------------------------------------------
def _controller(kw, solver, **over):
    import pmpc_amd

    args = dict(builtin_model="bicycle", params=kw["params"], Q=kw["Q"], R=kw["R"], X_ref=kw["X_ref"], U_ref=kw["U_ref"], u_l=kw["u_l"], u_u=kw["u_u"],
                reg_x=kw["reg_x"], reg_u=kw["reg_u"], solver_settings=dict(SETTINGS), solver=solver)
    args.update(over)
    return pmpc_amd.MPCController(**args)


def test_controller_with_a_custom_constraint():
    """`bicycle_keepout_problem(M=3, N=12)` with the ball as `balls_4_1_2`, 3 MPC steps of 3 iterations: each step equals the numpy `shift_plan`
    of the previous plan followed by the Python-driven loop from it, to 1e-6 (test_controller_with_keepout); `set_constraint_params` moves
    the ball and with it the next plan by more than 1e-3; the refusals fire."""
    from pmpc_amd import dynamics as dyn

    M, N = 3, 12
    kw, cstr = bicycle_keepout_problem(M=M, N=N)
    P = cg.ball_params(cstr, M)
    con = dict(cstr=cg.make("balls_4_1_2"), params=P)
    s1, s2 = _fresh(), _fresh()
    try:
        ctl = _controller(kw, s1, constraint=con)
        ctl.reset(X_prev=kw["X_prev"], U_prev=kw["U_prev"])
        X_start, U_start, x0 = kw["X_prev"], kw["U_prev"], kw["x0"]
        p0 = _dev(kw["params"][:1])
        for k in range(3):
            u0, info = ctl.step(x0, iterations=3)
            assert info["status"] == 0 and info["iterations_done"] == 3 and u0.shape == (M, 2), info
            X, U = ctl.X.cpu().numpy(), ctl.U.cpu().numpy()
            Xh, Uh, _ = python_loop("bicycle", dict(kw, x0=np.array(np.broadcast_to(x0, (M, 4))), X_prev=X_start, U_prev=U_start), dict(con, kind="custom"), 3, solver=s2)
            print(f"custom-constraint MPC step {k}: rel X {rel(X, Xh[:, 1:]):.3e} U {rel(U, Uh):.3e}; clearance {outside(X, cstr):.3e}")
            assert rel(X, Xh[:, 1:]) < 1e-6 and rel(U, Uh) < 1e-6
            assert outside(X, cstr) > -FEAS
            X_start, U_start, _ = dyn.shift_plan("bicycle", X, U, kw["params"], s=1)
            x0 = s1.rollout(ctl.model, _dev(np.array(np.broadcast_to(x0, (M, 4))[:1])), _dev(u0[:1, None, :]), p0)[0, 0].cpu().numpy()
        moved = dict(cstr, centres=np.array([[2.4, -0.3]]))
        P2 = cg.ball_params(moved, M)
        ctl.set_constraint_params(P2)
        u0, info = ctl.step(x0, iterations=3)
        assert info["status"] == 0
        X_moved = ctl.X.cpu().numpy()
        kw_now = dict(kw, x0=np.array(np.broadcast_to(x0, (M, 4))), X_prev=X_start, U_prev=U_start)
        Xh, _, _ = python_loop("bicycle", kw_now, dict(con, kind="custom", params=P2), 3, solver=s2)
        Xs, _, _ = python_loop("bicycle", kw_now, dict(con, kind="custom"), 3, solver=s2)
        print(f"custom-constraint MPC, new parameters: rel to the hand-composed step {rel(X_moved, Xh[:, 1:]):.3e}; they change the plan by {rel(X_moved, Xs[:, 1:]):.3e}")
        assert rel(X_moved, Xh[:, 1:]) < 1e-6 and rel(X_moved, Xs[:, 1:]) > 1e-3
        assert outside(X_moved, moved) > -FEAS
        with pytest.raises(ValueError, match=r"params must be \(M, pdim\)"):
            ctl.set_constraint_params(np.ones((M, 2)))
        with pytest.raises(ValueError, match="without keepout"):
            ctl.set_keepout(centres=moved["centres"])
        free = _controller(kw, s2)
        with pytest.raises(ValueError, match="without constraint"):
            free.set_constraint_params(P2)
        with pytest.raises(ValueError, match="not supported next to keepout"):
            _controller(kw, s2, constraint=con, keepout={k: cstr[k] for k in ("pos_idx", "centres", "radius")})
        with pytest.raises(ValueError, match="warm_shift=True is not supported next to constraint"):
            _controller(kw, s2, constraint=con, warm_shift=True)
    finally:
        s1.close()
        s2.close()
