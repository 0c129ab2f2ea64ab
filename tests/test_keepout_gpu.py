"""Keep-out constraints on the GPU (pmpc_amd/csrc/keepout.hip): the augmentation kernel against its numpy specification, one
sub-problem lowered on the device against the host lowering (`extra_cstrs`) and against the oracle's joint programs with the rows as
rows, and `solve(..., device="cuda", builtin_cstr=...)` against the host loop with `extra_cstrs_fns`.  fp64.  The inputs come from
tests/support/keepout_problems.py: feasible by construction, rows that bind (checked with the oracle before they were committed)."""
import ctypes

import numpy as np
import pytest

from tests.support.keepout_problems import bicycle_keepout_problem, keepout_subproblem, rows_of

pytestmark = pytest.mark.gpu
TOL = 1e-7
FEAS = 1e-8  # the feasibility bound of tests/test_state_rows_gpu.py
GUARD, SENTINEL = 64, 1234.5


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _devT(a):
    return _dev(np.swapaxes(a, -1, -2))


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def solver():
    from pmpc_amd.device import DeviceSolver

    s = DeviceSolver(0)
    yield s
    s.close()


# ---- 1. the kernel against the numpy specification -----------------------------------------------------------------------------------
def _guarded(shape):
    """A tensor of `shape` inside a flat allocation with GUARD sentinel doubles on both sides: (whole, view)."""
    import torch

    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(*shape)


def _kernel_case(rng, M, N, x, u, K, pd, kind):
    pos_idx = [int(k) for k in rng.permutation(x)[:pd]]
    cshape = {"static": (K, pd), "stage": (N, K, pd), "particle": (M, N, K, pd)}[kind]
    cstr = dict(kind="keepout", pos_idx=pos_idx, centres=rng.uniform(-1, 1, cshape), radius=rng.uniform(0.2, 0.6, K))
    U = lambda *s: rng.uniform(-1, 1, s)
    f, fx, fu, Xp, Xr = U(M, N, x), U(M, N, x, x), U(M, N, x, u), U(M, N, x), U(M, N, x)
    c = cstr["centres"]
    Xp[M - 1, N - 1, pos_idx] = c[K - 1] if kind == "static" else c[N - 1, K - 1] if kind == "stage" else c[M - 1, N - 1, K - 1]  # pbar = c exactly
    return cstr, f, fx, fu, Xp, Xr


SHAPES = [(1, 1, 4, 2, 1, 2), (3, 5, 4, 2, 4, 2), (2, 7, 3, 2, 2, 2), (130, 33, 12, 4, 3, 3)]


@pytest.mark.parametrize("with_ref", [True, False], ids=["xref", "noxref"])
@pytest.mark.parametrize("kind", ["static", "stage", "particle"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M%dN%dx%du%dK%dp%d" % s)
def test_kernel_equals_the_numpy_specification(solver, shape, kind, with_ref):
    """Copied and zero entries bit for bit; combined entries (at most 3 products of numbers in [-1, 1] times a unit direction) within
    1e-13 max(1, |entry|); guard doubles on both sides of every output untouched; of x_u~ only the auxiliary entries written; X_ref~ left
    alone without an X_ref.  (130, 33): 4290 units = 134 workgroups and 2 units; (1, 1): a workgroup of one unit."""
    from pmpc_amd.extra_cstrs import keepout_augment, keepout_rows

    M, N, x, u, K, pd = shape
    xd = x + K
    rng = np.random.default_rng(300 + 7 * SHAPES.index(shape) + len(kind) + int(with_ref))
    cstr, f, fx, fu, Xp, Xr = _kernel_case(rng, M, N, x, u, K, pd, kind)
    spec = keepout_augment(cstr, np.zeros((M, x)), f, fx, fu, Xp, Xr, np.zeros((M, N, x, x)), 1.0)
    a_x, h = keepout_rows(Xp, cstr)
    assert np.array_equal(a_x[M - 1, N - 1, K - 1, cstr["pos_idx"]], -np.eye(pd)[0])  # the degenerate unit is in the case
    want = dict(f=spec["f"], fx=np.swapaxes(spec["fx"], -1, -2), fu=np.swapaxes(spec["fu"], -1, -2), X_prev=spec["X_prev"], X_ref=spec["X_ref"])
    shapes = dict(f=(M, N, xd), fx=(M, N, xd, xd), fu=(M, N, u, xd), X_prev=(M, N, xd), X_ref=(M, N, xd), xu=(M, N, xd))
    whole, out = {}, {}
    for k, sh in shapes.items():
        whole[k], out[k] = _guarded(sh)
    ins = [_dev(Xp), _dev(f), _devT(fx), _devT(fu)]
    keep = [t.clone() for t in ins]
    got = solver.keepout_augment(cstr, *ins, X_ref=_dev(Xr) if with_ref else None, out=out)
    solver.sync()
    assert got is out
    import torch

    assert all(torch.equal(a, b) for a, b in zip(ins, keep))  # the inputs are not written
    for k in shapes:
        w = whole[k].cpu().numpy()
        assert np.all(w[:GUARD] == SENTINEL) and np.all(w[-GUARD:] == SENTINEL), f"{k}: guard doubles written"
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if not with_ref:
        assert np.all(res["X_ref"] == SENTINEL)
    # row index of every entry (the last axis in the ABI layout), column index for fx: which entries are copies, zeros, combinations
    worst = 0.0
    for k in ("f", "fx", "fu", "X_prev") + (("X_ref",) if with_ref else ()):
        g, w = res[k], want[k]
        comb = np.zeros(g.shape, bool)
        if k in ("f", "fx", "fu"):
            comb[..., x:] = True
        if k == "fx":
            comb[..., x:, :] = False  # columns >= x: zero
        assert np.array_equal(_bits(g)[~comb], _bits(w)[~comb]), f"{k}: a copied or zero entry differs"
        if comb.any():
            err = np.max(np.abs(g[comb] - w[comb]) / np.maximum(1.0, np.abs(w[comb])))
            worst = max(worst, err)
            assert err <= 1e-13, (k, err)
    assert np.all(res["xu"][..., :x] == SENTINEL)  # the caller's bounds
    err = np.max(np.abs(res["xu"][..., x:] - h) / np.maximum(1.0, np.abs(h)))
    worst = max(worst, err)
    print(f"keepout_augment {shape} {kind}: max relative difference of a combined entry {worst:.3e}")
    assert err <= 1e-13, err


def test_invalid_calls_return_2_and_launch_nothing(solver):
    import torch

    from pmpc_amd import _lib

    M, N, x, u, K, pd = 2, 3, 4, 2, 2, 2
    xd = x + K
    rng = np.random.default_rng(41)
    ins = [_dev(rng.uniform(-1, 1, s)) for s in ((M, N, x), (M, N, x), (M, N, x, x), (M, N, u, x), (M, N, x))]  # X_prev, f, fx, fu, X_ref
    outs = [torch.full(s, SENTINEL, dtype=torch.float64, device="cuda") for s in ((M, N, 16), (M, N, 16, 16), (M, N, u, 16), (M, N, 16), (M, N, 16), (M, N, 16))]
    cen, rad = _dev(rng.uniform(-1, 1, (4, 3))), _dev(np.full(4, 0.3))
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(xdim=x, N_=N, M_=M, ins_=None, outs_=None, ctx=None, **fields):
        d = dict(kind=1, K=K, pos_dim=pd, pos_idx=(0, 1, 0), centre_stride_particle=0, centre_stride_stage=0, centres=cen.data_ptr(), radius=rad.data_ptr())
        d.update(fields)
        d["pos_idx"] = (ctypes.c_int * 3)(*d["pos_idx"])
        sc = _lib.PmpcScpCstr(**d)
        return solver.lib.pmpc_keepout_augment_device(solver.h if ctx is None else ctx, ctypes.byref(sc), xdim, u, N_, M_, *[vp(t) for t in (ins_ or ins)],
                                                      *[vp(t) for t in (outs_ or outs)])

    bad = [dict(K=0), dict(K=5), dict(pos_dim=1), dict(pos_dim=4), dict(pos_idx=(0, 4, 0)), dict(pos_idx=(-1, 1, 0)), dict(pos_idx=(1, 1, 0)),
           dict(pos_dim=3, pos_idx=(0, 1, 1)), dict(kind=0), dict(xdim=13, K=4), dict(centres=None), dict(radius=None), dict(centre_stride_stage=-1),
           dict(N_=0), dict(M_=0)]
    for i in range(4):  # a null input (X_ref, the fifth, may be null)
        bad.append(dict(ins_=[None if j == i else t for j, t in enumerate(ins)]))
    for i in (0, 1, 2, 3, 5):  # a null output; X_ref_aug (4) may be null only when X_ref is
        bad.append(dict(outs_=[None if j == i else t for j, t in enumerate(outs)]))
    bad.append(dict(outs_=[None if j == 4 else t for j, t in enumerate(outs)]))
    for kw in bad:
        assert call(**kw) == 2, kw
    solver.sync()
    assert all(bool((t == SENTINEL).all()) for t in outs)  # nothing was launched
    # the control: the valid call runs, and X_ref / X_ref_aug may both be null
    outs_ok = [torch.full(s, SENTINEL, dtype=torch.float64, device="cuda") for s in ((M, N, xd), (M, N, xd, xd), (M, N, u, xd), (M, N, xd), (M, N, xd), (M, N, xd))]
    assert call(outs_=outs_ok) == 0
    assert call(ins_=ins[:4] + [None], outs_=outs_ok[:4] + [None, outs_ok[5]]) == 0
    solver.sync()
    assert not bool((outs_ok[0] == SENTINEL).any())


# ---- 2. - 4. one sub-problem -------------------------------------------------------------------------------------------------------------
def z_of(X, U, Nc):
    Ncc = U.shape[1] if Nc < 0 else Nc
    return np.concatenate([U[0, :Ncc].reshape(-1), U[:, Ncc:].reshape(-1), X.reshape(-1)])


def solve_device(s, args, kw, Nc, cstr, cone=False, smooth_alpha=float("nan")):
    """Leg A: the device lowering — `keepout_augment`, the static parts in torch (as `solve(device=...)` makes them), the solve at
    x + K states, the auxiliary states stripped.  cstr None: the solve without the constraint."""
    import torch

    x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref = args
    M, N, x = f.shape
    sym = bool(np.array_equal(Q, np.swapaxes(Q, -1, -2)) and np.array_equal(R, np.swapaxes(R, -1, -2)))
    p = dict(f=_dev(f), fx=_devT(fx), fu=_devT(fu), X_prev=_dev(X_prev), U_prev=_dev(U_prev), Q=_devT(Q), R=_devT(R), X_ref=_dev(X_ref), U_ref=_dev(U_ref),
             reg_x=kw["reg_x"], reg_u=kw["reg_u"], Nc=Nc, x0=_dev(x0), lu=_dev(kw["u_l"]), uu=_dev(kw["u_u"]), symmetric_cost=sym)
    if cstr is not None:
        aug = s.keepout_augment(cstr, p["X_prev"], p["f"], p["fx"], p["fu"], X_ref=p["X_ref"])
        xd = aug["f"].shape[-1]
        aug["xu"][..., :x] = float("inf")
        Qa = torch.zeros((M, N, xd, xd), dtype=torch.float64, device="cuda")
        Qa[..., :x, :x] = p["Q"]
        Qa[..., torch.arange(x, xd), torch.arange(x, xd)] = -float(kw["reg_x"])
        x0a = torch.zeros((M, xd), dtype=torch.float64, device="cuda")
        x0a[:, :x] = p["x0"]
        p.update(f=aug["f"], fx=aug["fx"], fu=aug["fu"], X_prev=aug["X_prev"], X_ref=aug["X_ref"], Q=Qa, x0=x0a, ux=aug["xu"],
                 lx=torch.full((M, N, xd), -float("inf"), dtype=torch.float64, device="cuda"))
    X, U, status = s.lcone_solve(smooth_alpha=smooth_alpha, **p) if cone else s.lqp_solve(**p)
    s.sync()
    assert status == 0, status
    return X.cpu().numpy()[..., :x], U.cpu().numpy()


def solve_host(args, kw, Nc, tuples, **settings):
    """Leg B: the host lowering — `backend.aff_solve` with the rows as an `extra_cstrs` tuple."""
    from pmpc_amd import backend

    x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref = args
    X, U, _ = backend.aff_solve(f, fx, fu, x0, X_prev, U_prev, Q, R, X_ref, U_ref, kw["reg_x"], kw["reg_u"], None, None, None, None,
                                kw["u_l"], kw["u_u"], solver_settings=dict(Nc=Nc, extra_cstrs=tuples, **settings))
    assert not np.isnan(U).any(), "solver failed"
    return X[:, 1:], U


def _outside(X, cstr):
    """min over (particle, stage, ball) of |p - c| - r."""
    c, r, idx = np.asarray(cstr["centres"]), np.asarray(cstr["radius"]), list(cstr["pos_idx"])
    return float((np.linalg.norm(X[:, :, None, idx] - c, axis=-1) - r).min())


def _check_rows(X, U, Nc, rows, cstr, X_free):
    slack = rows[0] @ z_of(X, U, Nc) - rows[1]
    print(f"  max(G z - h) {slack.max():.3e}, rows binding {int(np.sum(slack > -FEAS))} of {slack.size}, clearance {_outside(X, cstr):.3e}, "
          f"moved by the rows {_rel(X, X_free):.3e}")
    assert slack.max() < FEAS
    assert _outside(X, cstr) > -FEAS  # every stage outside every ball
    assert np.sum(slack > -FEAS) > 0  # some row binds
    assert _rel(X, X_free) > 1e-3  # the rows move the answer


#             seed, M, N, x,  u, K, pd, Nc
SUB_CASES = [(9702, 3, 6, 4, 2, 2, 2, 1),    # bicycle size
             (9709, 3, 6, 12, 4, 1, 3, 1),   # quadrotor size: 13 states
             (9702, 3, 6, 4, 2, 2, 2, 0),    # no consensus
             (9709, 3, 6, 4, 2, 2, 2, -1)]   # every control shared


@pytest.mark.parametrize("case", SUB_CASES, ids=lambda c: "M%dN%dx%dK%dNc%d" % (c[1], c[2], c[3], c[5], c[7]))
def test_device_lowering_equals_host_lowering(solver, case):
    seed, M, N, x, u, K, pd, Nc = case
    args, kw, cstr = keepout_subproblem(seed, M, N, x, u, K, pd)
    tup, rows = rows_of(cstr, args, Nc)
    Xa, Ua = solve_device(solver, args, kw, Nc, cstr)
    Xb, Ub = solve_host(args, kw, Nc, [tup], solver="osqp")
    X0, _ = solve_device(solver, args, kw, Nc, None)
    print(f"keep-out {case}: device against host lowering: rel X {_rel(Xa, Xb):.3e} U {_rel(Ua, Ub):.3e}")
    _check_rows(Xa, Ua, Nc, rows, cstr, X0)
    assert _rel(Xa, Xb) < TOL and _rel(Ua, Ub) < TOL, (_rel(Xa, Xb), _rel(Ua, Ub))


#               seed, M, N, x, u, K, pd, Nc      (M N K <= 8 rows: the range in which the state-row tests use the exact solver)
EXACT_CASES = [(9710, 1, 4, 4, 2, 1, 2, 1), (9711, 2, 4, 4, 2, 1, 2, 1)]


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "M%dN%dK%d" % (c[1], c[2], c[5]))
def test_device_lowering_equals_the_joint_qp_with_the_rows_as_rows(solver, case, oracle):
    seed, M, N, x, u, K, pd, Nc = case
    args, kw, cstr = keepout_subproblem(seed, M, N, x, u, K, pd)
    tup, rows = rows_of(cstr, args, Nc)
    Xo, Uo = oracle.lqp_solve_py(*args, Nc=Nc, rows=rows, **kw)
    X0, _ = oracle.lqp_solve_py(*args, Nc=Nc, **kw)
    X, U = solve_device(solver, args, kw, Nc, cstr)
    print(f"keep-out {case}: device against the joint QP: rel X {_rel(X, Xo):.3e} U {_rel(U, Uo):.3e}")
    _check_rows(X, U, Nc, rows, cstr, X0)
    assert _rel(X, Xo) < TOL and _rel(U, Uo) < TOL, (_rel(X, Xo), _rel(U, Uo))


@pytest.mark.parametrize("alpha", [None, 8.0])
def test_cone_path_equals_the_reference_program_with_the_rows(solver, alpha, oracle):
    """The reference's default path (eps-anchored epigraph objective) with the rows through augment_cone_problem!: hard, and smoothed
    with the boxes (log barrier 1 / alpha per row).  1e-6: the cone state-row tolerance of tests/test_state_rows_gpu.py."""
    from oracle import cone_oracle as co

    seed, M, N, x, u, K, pd, Nc = EXACT_CASES[1]
    args, kw, cstr = keepout_subproblem(seed, M, N, x, u, K, pd)
    tup, rows = rows_of(cstr, args, Nc)
    skw = {} if alpha is None else dict(smooth_alpha=alpha)
    Xo, Uo = co.lcone_direct_py(*args, Nc=Nc, extra_cstrs=[tup], **skw, **kw)
    X, U = solve_device(solver, args, kw, Nc, cstr, cone=True, smooth_alpha=float("nan") if alpha is None else alpha)
    slack = rows[0] @ z_of(X, U, Nc) - rows[1]
    print(f"keep-out cone path alpha {alpha}: rel X {_rel(X, Xo):.3e} U {_rel(U, Uo):.3e}, max(G z - h) {slack.max():.3e}")
    assert _rel(X, Xo) < 1e-6 and _rel(U, Uo) < 1e-6, (_rel(X, Xo), _rel(U, Uo))
    assert slack.max() < FEAS and _outside(X, cstr) > -FEAS


# ---- 5. / 6. the public loop ---------------------------------------------------------------------------------------------------------------
SETTINGS = dict(solver="osqp", Nc=1)


def _loop_args(kw, **over):
    keys = ("X_ref", "U_ref", "X_prev", "U_prev", "u_l", "u_u", "reg_x", "reg_u")
    return {**{k: kw[k] for k in keys}, **dict(max_it=5, res_tol=0.0, verbose=False, solver_settings=dict(SETTINGS)), **over}


@pytest.fixture(scope="module")
def loop_legs():
    """The device leg with the built-in model and the constraint (shared by the cases below)."""
    import pmpc_amd

    kw, cstr = bicycle_keepout_problem()
    Xd, Ud, dd = pmpc_amd.solve(None, kw["Q"], kw["R"], kw["x0"], device="cuda", builtin_model="bicycle", params=kw["params"], builtin_cstr=cstr,
                                **_loop_args(kw))
    return kw, cstr, Xd, Ud, dd


def test_public_loop_equals_the_host_loop_with_extra_cstrs_fns(loop_legs):
    """5 iterations (res_tol = 0) of `solve(device="cuda", builtin_model="bicycle", builtin_cstr=...)` against the host loop with
    `extra_cstrs_fns=make_keepout_extra_cstrs_fn(...)`: 1e-6 relative (five chained solves amplify last-bit differences of the two
    lowerings).  Every iterate of the device leg is outside the ball; the same call without the constraint drives through it."""
    import pmpc_amd
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.extra_cstrs import make_keepout_extra_cstrs_fn

    kw, cstr, Xd, Ud, dd = loop_legs
    pp = kw["params"][:, None, :]
    Xh, Uh, dh = pmpc_amd.solve(lambda X, U: dyn.bicycle(X, U, pp), kw["Q"], kw["R"], kw["x0"], extra_cstrs_fns=make_keepout_extra_cstrs_fn(cstr, SETTINGS["Nc"]),
                                **_loop_args(kw))
    assert Xd is not None and Xh is not None and len(dd["hist"]) == len(dh["hist"]) == 5
    print(f"keep-out loop: device against host after 5 iterations: rel X {_rel(Xd, Xh):.3e} U {_rel(Ud, Uh):.3e}; clearance {_outside(Xd[:, 1:], cstr):.3e}")
    assert _rel(Xd, Xh) < 1e-6 and _rel(Ud, Uh) < 1e-6, (_rel(Xd, Xh), _rel(Ud, Uh))
    for its in range(1, 6):  # every iterate: the loop stopped after `its` iterations
        Xi, _, _ = (Xd, None, None) if its == 5 else pmpc_amd.solve(None, kw["Q"], kw["R"], kw["x0"], device="cuda", builtin_model="bicycle",
                                                                     params=kw["params"], builtin_cstr=cstr, **_loop_args(kw, max_it=its))
        assert _outside(Xi[:, 1:], cstr) > -FEAS, (its, _outside(Xi[:, 1:], cstr))
    Xf, _, _ = pmpc_amd.solve(None, kw["Q"], kw["R"], kw["x0"], device="cuda", builtin_model="bicycle", params=kw["params"], **_loop_args(kw))
    r = float(cstr["radius"][0])
    print(f"  without the constraint the plan enters the ball by {-_outside(Xf[:, 1:], cstr) / r:.3f} radii")
    assert -_outside(Xf[:, 1:], cstr) >= 0.2 * r


def test_public_loop_with_a_torch_callable_equals_the_builtin_model(loop_legs):
    import pmpc_amd
    import torch
    from pmpc_amd import dynamics as dyn

    kw, cstr, Xd, Ud, _ = loop_legs
    pp = torch.as_tensor(kw["params"], dtype=torch.float64, device="cuda")[:, None, :]
    Xt, Ut, _ = pmpc_amd.solve(lambda X, U: dyn.bicycle_torch(X, U, pp), kw["Q"], kw["R"], kw["x0"], device="cuda", builtin_cstr=cstr, **_loop_args(kw))
    print(f"keep-out loop: torch callable against the built-in model: rel X {_rel(Xt, Xd):.3e} U {_rel(Ut, Ud):.3e}")
    assert _rel(Xt, Xd) < 1e-9 and _rel(Ut, Ud) < 1e-9, (_rel(Xt, Xd), _rel(Ut, Ud))


def test_public_loop_with_the_builtin_cost_as_well():
    """`builtin_cost` shifts X_ref every iteration, so the kernel's X_ref input is this iteration's: one iteration against the host loop
    with both callables, 1e-7."""
    import pmpc_amd
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.extra_cstrs import make_keepout_extra_cstrs_fn

    kw, cstr = bicycle_keepout_problem()
    cost = dict(kind="obstacles", pos_idx=(0, 1), centres=np.array([[2.0, 0.9]]), sigma=np.array([0.5]), w=np.array([2.0]))
    pp = kw["params"][:, None, :]
    la = _loop_args(kw, max_it=1)
    Xh, Uh, _ = pmpc_amd.solve(lambda X, U: dyn.bicycle(X, U, pp), kw["Q"], kw["R"], kw["x0"], extra_cstrs_fns=make_keepout_extra_cstrs_fn(cstr, SETTINGS["Nc"]),
                               lin_cost_fn=dyn.make_obstacle_lin_cost_fn(cost), **la)
    Xn, _, _ = pmpc_amd.solve(None, kw["Q"], kw["R"], kw["x0"], device="cuda", builtin_model="bicycle", params=kw["params"], builtin_cstr=cstr, **la)
    Xd, Ud, _ = pmpc_amd.solve(None, kw["Q"], kw["R"], kw["x0"], device="cuda", builtin_model="bicycle", params=kw["params"], builtin_cstr=cstr,
                               builtin_cost=cost, **la)
    print(f"keep-out loop with the obstacle cost: rel X {_rel(Xd, Xh):.3e} U {_rel(Ud, Uh):.3e}; the cost moves the plan by {_rel(Xd, Xn):.3e}")
    assert _rel(Xd, Xn) > 1e-3  # the cost acts: the kernel saw a shifted X_ref
    assert _rel(Xd, Xh) < TOL and _rel(Ud, Uh) < TOL, (_rel(Xd, Xh), _rel(Ud, Uh))
    assert _outside(Xd[:, 1:], cstr) > -FEAS
