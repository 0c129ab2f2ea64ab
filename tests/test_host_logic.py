"""CPU tests (no GPU) of the host layer: ABI export, layout helpers, sentinel marshalling, the SCP loop
against the reference's own loop (golden hist rows), filters and the table printer."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"


def test_library_exports_every_declared_symbol():
    from pmpc_amd import _lib

    lib = _lib.load()  # must load without a GPU
    header = (ROOT / "include" / "pmpc_abi.h").read_text()
    declared = set(re.findall(r"\b(c_l\w+_solve|pmpc_\w+)\s*\(", header)) - {"pmpc_ctx", "pmpc_problem", "pmpc_info"}
    assert {"c_lqp_solve", "c_lcone_solve", "pmpc_lqp_solve_device", "pmpc_comm_init"} <= declared
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert set(_lib.ABI_SYMBOLS) == declared
    assert b"gfx950" in lib.pmpc_version()


def test_py2jl_roundtrip_and_abi_layout():
    from pmpc_amd.backend import jl2py, py2jl

    rng = np.random.default_rng(0)
    fx = rng.standard_normal((3, 5, 4, 4))  # (M,N,row,col)
    j = py2jl(fx, 2)
    assert j.shape == (4, 4, 5, 3) and j[1, 2, 3, 0] == fx[0, 3, 1, 2]
    np.testing.assert_array_equal(jl2py(j, 2), fx)
    # Fortran-order memory of the Julia-shaped array == C-order (M,N,col,row)
    np.testing.assert_array_equal(np.asfortranarray(j).ravel(order="K"), np.swapaxes(fx, -1, -2).ravel())
    v = rng.standard_normal((3, 5, 4))
    np.testing.assert_array_equal(np.asfortranarray(py2jl(v, 1)).ravel(order="K"), v.ravel())


def test_aff_solve_marshalling(monkeypatch):
    """Sentinels and argument order handed to the ABI (pmpc/static_backend.py:242-276, :311)."""
    from pmpc_amd import backend

    seen = {}

    def fake_lqp(*args, verbose=False):
        seen["lqp"] = args
        Nc, x0, f = args[0], args[1], args[2]
        xdim, N, M = f.shape
        return np.zeros((M, N, xdim)), np.zeros((M, N, args[6].shape[0]))

    def fake_cone(*args, verbose=False, solver="ecos", k=None):
        seen["cone"] = (args, solver)
        seen["k"] = k
        f = args[2]
        xdim, N, M = f.shape
        return np.zeros((M, N, xdim)), np.zeros((M, N, args[6].shape[0]))

    monkeypatch.setattr(backend, "lqp_solve", fake_lqp)
    monkeypatch.setattr(backend, "lcone_solve", fake_cone)
    M, N, x, u = 2, 4, 3, 2
    rng = np.random.default_rng(0)
    f, fx, fu = rng.standard_normal((M, N, x)), rng.standard_normal((M, N, x, x)), rng.standard_normal((M, N, x, u))
    x0 = rng.standard_normal((M, x))
    Q, R = np.tile(np.eye(x), (M, N, 1, 1)), np.tile(np.eye(u), (M, N, 1, 1))
    z3 = lambda d: np.zeros((M, N, d))
    empty = np.zeros((0, 0, 0))
    X, U, data = backend.aff_solve(f, fx, fu, x0, z3(x), z3(u), Q, R, z3(x), z3(u), 1.0, 0.1, 0.0, None, empty, empty,
                                   -np.ones((M, N, u)), np.ones((M, N, u)), solver_settings=dict(solver="osqp", Nc=2))
    a = seen["lqp"]
    assert a[0] == 2 and a[1].shape == (x, M) and a[3].shape == (x, x, N, M) and a[4].shape == (x, u, N, M)
    assert np.all(np.isnan(a[11])) and np.all(np.isnan(a[12]))  # no state bounds -> NaN sentinel
    assert np.all(a[13] == -1) and np.all(a[14] == 1)
    assert np.all(a[17] == 0.0) and np.all(np.isnan(a[18])) and np.all(np.isnan(a[19]))  # slew_rate 0, no slew0/um1
    assert X.shape == (M, N + 1, x) and np.all(X[:, 0] == x0) and data == {}
    # default solver is the cone path, Nc defaults to -1 (static_backend.py:242-257)
    backend.aff_solve(f, fx, fu, x0, z3(x), z3(u), Q, R, z3(x), z3(u), 1.0, 0.1, None, None, empty, empty, empty, empty,
                      solver_settings=dict())
    args, solver = seen["cone"]
    assert solver == "ecos" and args[0] == -1 and np.isnan(args[20]) and np.all(np.isnan(args[17]))


def _run_scp(oracle, N, regs, max_it):
    import pmpc_amd.scp_mpc as scp
    from pmpc_amd import dynamics as dyn

    p = np.array([1.0, 1.0, 0.3])
    f_fx_fu_fn = lambda X, U: dyn.unicycle(X, U, p)
    Q, R = np.tile(np.eye(4), (N, 1, 1)), np.tile(1e-2 * np.eye(2), (N, 1, 1))
    kw = dict(u_l=-np.ones((N, 2)), u_u=np.ones((N, 2)), max_it=max_it, solver_settings=dict(solver="osqp"), **regs)
    return scp.scp_solve(f_fx_fu_fn, Q, R, np.ones(4), np.zeros((N, 4)), np.zeros((N, 2)), np.zeros((N, 4)), np.zeros((N, 2)), **kw)


@pytest.mark.parametrize("name,regs", [("scp_unicycle_simple.npz", {}), ("scp_unicycle_remote.npz", dict(reg_x=1.0, reg_u=1.0))])
def test_scp_loop_matches_reference_loop(name, regs, oracle, monkeypatch):
    """pmpc_amd.scp_solve (aff_solve := oracle) reproduces the hist rows the REFERENCE's scp_solve produced
    over the same oracle (tests/golden/make_golden.py): same residual / objective definitions, same defaults."""
    import pmpc_amd.scp_mpc as scp

    monkeypatch.setattr(scp, "aff_solve", oracle.aff_solve)
    g = np.load(GOLD / name)
    X, U, data = _run_scp(oracle, int(g["N"]), regs, int(g["max_it"]))
    hist = np.array([[h["it"], h["obj"], h["resid"], h["reg_x"], h["reg_u"]] for h in data["hist"]])
    assert hist.shape == g["hist"].shape
    np.testing.assert_allclose(hist[:, [0, 3, 4]], g["hist"][:, [0, 3, 4]])
    # the first linearisation is at U_prev = 0 where the reference's closed form divides O(u2^2)
    # differences by u2^2 with u2 = 1e-6 (tests/dubins_car.py:62-85): torch.autograd (golden) and the
    # analytic Jacobian agree only to ~1e-4 there; later iterates agree to solver precision
    np.testing.assert_allclose(hist[:, 1], g["hist"][:, 1], rtol=2e-4)
    np.testing.assert_allclose(hist[5:, 1], g["hist"][5:, 1], rtol=1e-5)
    np.testing.assert_allclose(hist[:, 2], g["hist"][:, 2], rtol=5e-3, atol=1e-7)
    np.testing.assert_allclose(X, g["X"], atol=2e-5)
    np.testing.assert_allclose(U, g["U"], atol=2e-5)
    assert X.shape == (int(g["N"]) + 1, 4) and set(data) >= {"hist", "solver_data", "t_aff_solve"}


def test_solver_failure_returns_none(monkeypatch):
    import pmpc_amd.scp_mpc as scp

    def nan_solve(f, *a, **k):
        M, N, x = f.shape
        return np.full((M, N + 1, x), np.nan), np.zeros((M, N, 2)), {}

    monkeypatch.setattr(scp, "aff_solve", nan_solve)
    from pmpc_amd import dynamics as dyn

    out = scp.scp_solve(lambda X, U: dyn.unicycle(X, U, np.array([1.0, 1.0, 0.3])), np.tile(np.eye(4), (5, 1, 1)),
                        np.tile(np.eye(2), (5, 1, 1)), np.ones(4))
    assert out == (None, None, None)


def test_filters_and_table_printer():
    from pmpc_amd.scp_mpc import AA_method, select_method, smooth_method
    from pmpc_amd.utils import TablePrinter, atleast_nd

    rng = np.random.default_rng(0)
    Fs = [rng.standard_normal(7) for _ in range(4)]
    for fn in (AA_method, select_method, smooth_method):
        assert abs(np.sum(fn(Fs)) - 1.0) < 1e-9
    tp = TablePrinter(["it", "elaps"], fmts=["%04d", "%8.3e"])
    assert tp.make_values((3, 1.5)).count("|") == 3 and "0003" in tp.make_values((3, 1.5))
    assert tp.make_header().splitlines()[0] == tp.make_footer()
    assert atleast_nd(np.zeros((2, 3)), 4).shape == (1, 1, 2, 3) and atleast_nd(None, 3) is None


def test_problem_builder_defaults_and_tiling():
    """pmpc/problem_struct.py:10-155 behaviour: dims inference, defaults, M-tiling, Nc injection, Mapping."""
    from pmpc_amd.problem_struct import Problem

    p = Problem(N=20, xdim=4, udim=2)
    assert p.Q.shape == (20, 4, 4) and np.all(p.R[0] == 0.1 * np.eye(2)) and p.reg_x == 1.0 and p.max_it == 30
    p.x0 = np.ones(4)
    p.u_l = -np.ones(2)  # tiled over N
    assert p.u_l.shape == (20, 2) and p.x_l is None
    p.f_fx_fu_fn = lambda X, U: None
    d = dict(**p)
    assert set(d) >= {"Q", "R", "x0", "X_ref", "U_ref", "X_prev", "U_prev", "u_l", "u_u", "x_l", "x_u", "solver_settings",
                      "reg_x", "reg_u", "max_it", "res_tol", "verbose", "slew_rate", "f_fx_fu_fn"}
    assert "Nc" not in d["solver_settings"]
    q = Problem(xdim=4, udim=2, N=20, M=3, Nc=3, max_it=100, verbose=False)
    q.X_ref = np.ones((20, 4))
    assert q.X_ref.shape == (3, 20, 4) and q.Q.shape == (3, 20, 4, 4) and q.x0.shape == (3, 4)
    q.f_fx_fu_fn = lambda X, U: None
    assert q.to_dict()["solver_settings"]["Nc"] == 3 and q.to_dict()["max_it"] == 100
    r = Problem(Q=np.tile(np.eye(3), (7, 1, 1)), R=np.tile(np.eye(1), (7, 1, 1)))  # dims from arrays
    assert r.dims == dict(N=7, xdim=3, udim=1)
    with pytest.raises(ValueError):
        Problem(N=3, xdim=2)


def test_problem_builder_matches_reference():
    """`Problem.to_dict()` against the reference builder's output for the same arguments (stored by
    tests/golden/make_golden.py: arrays under their keys, every other entry in the JSON string `meta`)."""
    import json

    from pmpc_amd.problem_struct import Problem

    g = np.load(GOLD / "ref_problem_struct_dict.npz")
    meta = json.loads(str(g["meta"]))
    kw = dict(xdim=4, udim=2, N=9, M=2, Nc=2, reg_x=3.0, X_ref=np.arange(36.0).reshape(9, 4))
    a = Problem(**kw)
    a.f_fx_fu_fn = lambda X, U: None
    a.u_l, a.u_u = -np.ones(2), np.ones(2)
    da = a.to_dict()
    assert set(da) == set(meta["keys"])
    for k in meta["keys"]:
        if k in g.files:
            np.testing.assert_array_equal(da[k], g[k], err_msg=k)
        elif k != "f_fx_fu_fn":
            assert da[k] == meta["entries"][k], k


@pytest.mark.parametrize("case_idx", [0, 3, 5, 7, 8, 9, 10, 13, 14, 28])
def test_problem_matrices_match_oracle_assembly(case_idx, oracle):
    """`lqp_generate_problem_matrices` (vectorised numpy, product side) against the line-by-line C restatement of
    lqp_repr_Pq / lqp_repr_Ab / lqp_repr_Gla: identical P, q, A, b, G, l, u — every slew / consensus / bound branch."""
    from pmpc_amd import lqp_generate_problem_matrices
    from tests.support.problems import CASES, rand_problem

    case = CASES[case_idx]
    M, N, x, u, Nc = case[:5]
    args, kw = rand_problem(np.random.default_rng(77 + case_idx), M, N, x, u, *case[5:])
    x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref = args
    nan = np.full(1, np.nan)
    qp = oracle.assemble_abi(
        x, u, N, M, Nc, f, oracle.to_abi_mat(fx), oracle.to_abi_mat(fu), X_prev, U_prev, oracle.to_abi_mat(Q), oracle.to_abi_mat(R),
        X_ref, U_ref, kw.get("x_l", nan), kw.get("x_u", nan), kw.get("u_l", nan), kw.get("u_u", nan), kw["reg_x"], kw["reg_u"],
        kw.get("slew_reg", nan), kw.get("slew_reg0", nan), kw.get("slew_um1", nan))
    P, q, A, b, G, lo, hi = lqp_generate_problem_matrices(
        x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref, Nc=Nc, reg_x=kw["reg_x"], reg_u=kw["reg_u"],
        slew_reg=kw.get("slew_reg"), slew_reg0=kw.get("slew_reg0"), slew_um1=kw.get("slew_um1"), lx=kw.get("x_l"), ux=kw.get("x_u"),
        lu=kw.get("u_l"), uu=kw.get("u_u"))
    assert P.shape == qp.P.shape and A.shape == qp.A.shape and G.shape == qp.G.shape
    assert abs(P - qp.P).max() <= 1e-12 * max(1.0, abs(qp.P).max())
    assert abs(A - qp.A).max() == 0.0 and (G.shape[0] == 0 or abs(G - qp.G).max() == 0.0)
    np.testing.assert_allclose(q, qp.q, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b, qp.b, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(lo, qp.l)
    np.testing.assert_array_equal(hi, qp.u)


def test_tune_scp_picks_smallest_residual():
    import pmpc_amd

    calls = []

    def fake_solve(*a, reg_x=None, reg_u=None, **kw):
        calls.append((reg_x, reg_u))
        return None, None, dict(hist=[dict(resid=abs(np.log10(reg_x) - 1.0))])

    reg_x, reg_u = pmpc_amd.tune_scp(solve_fn=fake_solve, sample_nb=7, reg_rng=(-3, 3), reg_ratio=0.5)
    assert np.isclose(reg_x, 10.0) and np.isclose(reg_u, 5.0) and len(calls) == 7
    assert all(np.isclose(ru, 0.5 * rx) for rx, ru in calls)


def test_oracle_and_host_loop_reproduce_reference_notebook_table(oracle, monkeypatch):
    """PIN against the reference's own solver stack: the 50-row table printed by `pmpc.solve` (Julia + ECOS) in
    examples/gpu_solver.ipynb is reproduced to its 4 printed digits by this repository's SCP loop + numpy unicycle +
    the oracle's exact cone-path solve (M = 1: the minimiser of the QP)."""
    import pmpc_amd.scp_mpc as scp
    from tests.support import notebook_problem as nbp

    args, kw, table = nbp.load()

    def oracle_aff_solve(f, fx, fu, x0, X_prev, U_prev, Q, R, X_ref, U_ref, reg_x, reg_u, slew_rate, u_slew, x_l, x_u, u_l, u_u,
                         solver_settings=None, **_):
        X, U = oracle.lcone_solve_py(x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref, reg_x=reg_x, reg_u=reg_u, Nc=-1, u_l=u_l, u_u=u_u)
        return np.concatenate([x0[:, None, :], X], 1), U, dict()

    monkeypatch.setattr(scp, "aff_solve", oracle_aff_solve)
    X, U, data = scp.scp_solve(*args, solver_settings=dict(solver="ecos"), **kw)
    nbp.check_rows(data["hist"], table)


def _oracle_cone_aff_solve(oracle):
    def aff(f, fx, fu, x0, X_prev, U_prev, Q, R, X_ref, U_ref, reg_x, reg_u, slew_rate, u_slew, x_l, x_u, u_l, u_u, solver_settings=None, **_):
        s = solver_settings or {}
        X, U = oracle.lcone_solve_py(x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref, reg_x=reg_x, reg_u=reg_u, Nc=s.get("Nc", -1),
                                     u_l=u_l, u_u=u_u, slew_reg=slew_rate if slew_rate else None,
                                     smooth_alpha=s.get("smooth_alpha", float("nan")))
        return np.concatenate([x0[:, None, :], X], 1), U, dict()

    return aff


@pytest.mark.parametrize("name", ["ref_root_testing_single", "ref_root_testing_consensus", "ref_logbarrier_tests"])
def test_oracle_reproduces_reference_tables_on_consensus_slew_and_smoothing(oracle, monkeypatch, name):
    """PINS beyond M = 1 / hard boxes: tables printed by the reference's own Julia stack in tests/root_testing.ipynb
    (M = 1 with slew_rate 1e2 and smooth_alpha 1e-1; M = 20 consensus with Nc = 5, slew 1e2, smooth_alpha 1 — every row to the
    4 printed digits) and tests/logbarrier_tests.ipynb.  The consensus table separates the readings: the plain-sum QP with
    the same barrier is off by up to 2e-3 in `resid` (systematically), hard boxes by 6e-3 / 6e-2, no slew by 50 %; the
    eps-anchored cone objective with the LOG BARRIER (not the slack*log(alpha*slack) reading) fits all 23 rows."""
    import pmpc_amd.scp_mpc as scp
    from tests.support import notebook_problem as nbp

    args, kw, settings, table = nbp.load_table(name)
    monkeypatch.setattr(scp, "aff_solve", _oracle_cone_aff_solve(oracle))
    X, U, data = scp.scp_solve(*args, solver_settings=settings, **kw)
    nbp.check_table(name, data["hist"], table)


@pytest.mark.parametrize("name", ["ref_experimental_cpu", "ref_demo_cost_convex", "ref_demo_cost_external"])
def test_oracle_reaches_the_fixed_points_of_the_remaining_reference_tables(oracle, monkeypatch, name):
    """Tables whose early rows nobody can reproduce (unstored warm start / Jacobian round-off at U = 0 amplified by a
    bang-bang solution, see notebook_problem.check_fixed_point): first row, converged objective, contraction factor.
    tests/experimental.ipynb's fixed point separates smooth_alpha = 1e3 (1.617, printed) from hard boxes (1.616)."""
    import pmpc_amd.scp_mpc as scp
    from tests.support import notebook_problem as nbp

    args, kw, settings, table = nbp.load_table(name)
    if name == "ref_experimental_cpu":
        kw["max_it"] = 150  # cold start here (the notebook's warm start is not stored): converged to 4 digits by then
    monkeypatch.setattr(scp, "aff_solve", _oracle_cone_aff_solve(oracle))
    X, U, data = scp.scp_solve(*args, solver_settings=settings, **kw)
    nbp.check_fixed_point(name, data["hist"], table)


def test_extra_cstrs_linear_rows_become_boxes_and_the_rest_is_refused(monkeypatch):
    """`extra_cstrs` tuples (README.md:219-239) on the host path: single-variable linear rows G z <= h are folded into the boxes
    handed to the ABI (intersected with the caller's), consensus columns bound the shared control; a tuple outside the
    supported cases raises — it is never dropped silently."""
    import scipy.sparse as sp

    from pmpc_amd import backend
    from pmpc_amd.extra_cstrs import linear_rows_to_boxes

    M, N, x, u, Nc = 3, 5, 4, 2, 2
    ncu = Nc * u + M * (N - Nc) * u
    n = ncu + M * N * x
    G = sp.lil_matrix((4, n))
    G[0, 1] = 2.0                                   # shared control, stage 0, component 1:  2 u <= 1
    G[1, Nc * u + 1 * (N - Nc) * u + 2 * u] = -1.0  # particle 1, stage Nc + 2, component 0:  -u <= 0.3
    G[2, ncu + 2 * N * x + 3 * x + 1] = 1.0         # particle 2, stage 3, state 1 <= 7
    G[3, ncu] = -4.0                                # particle 0, stage 0, state 0:  -4 x <= 8
    cstr = (4, [], 0, G.tocsr(), sp.csr_matrix((4, 0)), np.array([1.0, 0.3, 7.0, 8.0]), np.zeros(n), np.zeros(0))
    xl, xu, ul, uu = linear_rows_to_boxes(cstr, M, N, x, u, Nc)
    assert np.all(uu[:, 0, 1] == 0.5) and ul[1, Nc + 2, 0] == -0.3 and xu[2, 3, 1] == 7.0 and xl[0, 0, 0] == -2.0
    assert np.isinf(uu).sum() == uu.size - 3 and np.isinf(ul).sum() == ul.size - 1 and np.isinf(xl).sum() == xl.size - 1

    seen = {}

    def fake_lqp(*args, verbose=False):
        seen["args"] = args
        f = args[2]
        xdim, Nn, Mm = f.shape
        return np.zeros((Mm, Nn, xdim)), np.zeros((Mm, Nn, args[6].shape[0]))

    monkeypatch.setattr(backend, "lqp_solve", fake_lqp)
    rng = np.random.default_rng(0)
    f, fx, fu = rng.standard_normal((M, N, x)), rng.standard_normal((M, N, x, x)), rng.standard_normal((M, N, x, u))
    z3 = lambda d: np.zeros((M, N, d))
    Q, R = np.tile(np.eye(x), (M, N, 1, 1)), np.tile(np.eye(u), (M, N, 1, 1))
    empty = np.zeros((0, 0, 0))
    backend.aff_solve(f, fx, fu, np.zeros((M, x)), z3(x), z3(u), Q, R, z3(x), z3(u), 1.0, 0.1, 0.0, None, empty, empty, -0.4 * np.ones((M, N, u)),
                      0.4 * np.ones((M, N, u)), solver_settings=dict(solver="osqp", Nc=Nc, extra_cstrs=[cstr]))
    a = seen["args"]
    lx, ux, lu, uub = (backend.jl2py(a[k], 1) for k in (11, 12, 13, 14))
    assert lu[1, Nc + 2, 0] == -0.3 and np.all(uub[:, 0, 1] == 0.4) and np.all(lu[0] == -0.4)  # intersected with the caller's +-0.4
    assert ux[2, 3, 1] == 7.0 and lx[0, 0, 0] == -2.0 and np.isinf(ux).sum() == ux.size - 1
    G2 = G.copy()
    G2[0, 3] = 1.0  # a row coupling two variables
    bad = (4, [], 0, G2.tocsr(), sp.csr_matrix((4, 0)), np.ones(4), np.zeros(n), np.zeros(0))
    with pytest.raises(ValueError, match="this is not"):  # (rows on states that couple variables: not a box, not a stage-local cone)
        backend.aff_solve(f, fx, fu, np.zeros((M, x)), z3(x), z3(u), Q, R, z3(x), z3(u), 1.0, 0.1, 0.0, None, empty, empty, empty, empty,
                          solver_settings=dict(solver="osqp", Nc=Nc, extra_cstrs=[bad]))


def test_extra_cstrs_tuple_to_stage_cones():
    """The reference's `extra_cstrs` tuple format (README.md:219-239) for the stage-wise thrust cone is recognised and
    mapped to the device solver's `(W, w0, v, v0)`; anything outside that structure is refused with a reason."""
    import scipy.sparse as sp

    from pmpc_amd.extra_cstrs import stage_soc_from_extra_cstrs, stage_soc_to_extra_cstrs

    M, N, x, u, Nc = 3, 5, 12, 4, 2
    W = np.zeros((2, 4)); W[0, 1] = W[1, 2] = 1.0
    cstr = stage_soc_to_extra_cstrs(W, [0.1, -0.2], [0.3, 0, 0, 0], 0.05, M, N, x, u, Nc)
    assert cstr[0] == 0 and cstr[2] == 0 and len(cstr[1]) == Nc + M * (N - Nc) and cstr[3].shape[1] == Nc * u + M * (N - Nc) * u + M * N * x
    soc = stage_soc_from_extra_cstrs(cstr, M, N, x, u, Nc)
    np.testing.assert_array_equal(soc["W"], W)
    np.testing.assert_array_equal(soc["w0"], [0.1, -0.2])
    np.testing.assert_array_equal(soc["v"], [0.3, 0, 0, 0])
    assert soc["v0"] == 0.05
    bad = list(cstr); bad[0] = 2
    with pytest.raises(ValueError, match="second-order"):
        stage_soc_from_extra_cstrs(bad, M, N, x, u, Nc)
    G = cstr[3].tolil(); G[0, G.shape[1] - 1] = 1.0
    with pytest.raises(ValueError, match="states"):
        stage_soc_from_extra_cstrs((0, cstr[1], 0, G.tocsr(), cstr[4], cstr[5], cstr[6], cstr[7]), M, N, x, u, Nc)
    G = cstr[3].tolil(); G[3, 5] = 1.0  # second cone (block 1) reaches into block 1 and ... column 5 is block 1: make it span block 0
    G[3, 1] = 1.0
    with pytest.raises(ValueError, match="several stages"):
        stage_soc_from_extra_cstrs((0, cstr[1], 0, G.tocsr(), cstr[4], cstr[5], cstr[6], cstr[7]), M, N, x, u, Nc)
    h = cstr[5].copy(); h[3] += 1.0
    with pytest.raises(ValueError, match="stage-dependent"):
        stage_soc_from_extra_cstrs((0, cstr[1], 0, cstr[3], cstr[4], h, cstr[6], cstr[7]), M, N, x, u, Nc)
    with pytest.raises(ValueError, match="one cone per control block"):
        stage_soc_from_extra_cstrs((0, cstr[1][:-1], 0, cstr[3][:-3], cstr[4], cstr[5][:-3], cstr[6], cstr[7]), M, N, x, u, Nc)


def test_unsupported_extra_cstrs_tuples_are_refused_with_the_reason():
    """pmpc_amd/extra_cstrs.py recognises stage-local linear rows and second-order cones on the controls; everything else of the
    reference's tuple format (PMPC.jl/src/main.jl:293-316) is refused with the reason, never dropped."""
    import scipy.sparse as sp

    from pmpc_amd.extra_cstrs import stage_cones_from_extra_cstrs

    M, N, x, u, Nc = 2, 4, 3, 2, 0
    ncu, n = M * N * u, M * N * u + M * N * x
    base = lambda G, l=1, q=(), e=0, Gr=None, cl=None, cr=None: (l, list(q), e, G, sp.csr_matrix((G.shape[0], 0)) if Gr is None else Gr, np.ones(G.shape[0]),
                                                                 np.zeros(n) if cl is None else cl, np.zeros(0) if cr is None else cr)
    row = lambda cols: sp.csr_matrix((np.ones(len(cols)), (np.zeros(len(cols), int), cols)), shape=(1, n))
    with pytest.raises(ValueError, match="several stages"):
        stage_cones_from_extra_cstrs([base(row([0, u]))], M, N, x, u, Nc)
    with pytest.raises(ValueError, match="states"):
        stage_cones_from_extra_cstrs([base(row([0, ncu + 1]))], M, N, x, u, Nc)
    with pytest.raises(ValueError, match="exponential"):
        stage_cones_from_extra_cstrs([base(sp.vstack([row([0])] * 3), l=0, e=1)], M, N, x, u, Nc)
    with pytest.raises(ValueError, match="new variables"):
        stage_cones_from_extra_cstrs([base(row([0]), Gr=sp.csr_matrix(np.ones((1, 1))))], M, N, x, u, Nc)
    with pytest.raises(ValueError, match="same list"):
        stage_cones_from_extra_cstrs([base(row([0]))], M, N, x, u, Nc)  # only block 0 carries a row


def test_general_conic_oracle_agrees_with_the_stage_cone_oracle(oracle):
    """Two independent restatements of the same problem: `lsoc_solve_py` (per-block cone data) and `lconic_solve_py` (arbitrary
    sparse conic rows over the joint variable vector, here built from the reference-format tuple)."""
    import scipy.sparse as sp

    from pmpc_amd.extra_cstrs import stage_soc_to_extra_cstrs
    from tests.support.problems import rand_problem

    M, N, x, u, Nc = 3, 5, 4, 3, 1
    args, kw = rand_problem(np.random.default_rng(3), M, N, x, u, 0.6)
    W = np.zeros((2, 3)); W[0, 1] = W[1, 2] = 1.0
    v, v0, w0, u_int = np.array([0.5, 0, 0]), 0.05, np.zeros(2), np.array([0.2, 0, 0])
    Xo, Uo = oracle.lsoc_solve_py(*args, Nc=Nc, reg_x=kw["reg_x"], reg_u=kw["reg_u"], u_l=kw["u_l"], u_u=kw["u_u"], soc_W=W, soc_w0=w0, soc_v=v,
                                  soc_v0=v0, u_interior=u_int)
    l, q, e, G, Gr, h, cl, cr = stage_soc_to_extra_cstrs(W, w0, v, v0, M, N, x, u, Nc)
    G = sp.csr_matrix(G)
    socs = [(G[k * 3:(k + 1) * 3], h[k * 3:(k + 1) * 3]) for k in range(len(q))]
    ncu = Nc * u + M * (N - Nc) * u
    X, U = oracle.lconic_solve_py(*args, Nc=Nc, reg_x=kw["reg_x"], reg_u=kw["reg_u"], u_l=kw["u_l"], u_u=kw["u_u"], socs=socs,
                                  z0=np.tile(u_int, ncu // u))
    assert np.abs(X - Xo).max() < 1e-9 and np.abs(U - Uo).max() < 1e-9



def test_cone_rounds_model_matches_the_cone_oracle_over_an_scp_sequence(oracle):
    """The METHOD of pmpc_amd/csrc/kernels_cone.hip restated in numpy (tools/proto/cone_ssn.py: semismooth Newton on the natural map
    of each stage cone — interior / apex / boundary branch of the projection's generalised Jacobian —, boxes by the primal-dual
    active-set rule, one structured Newton solve per round) on the quadrotor with config E's thrust cones: three SCP iterations,
    cold start then warm starts from the previous branches and multipliers, each against the sparse cone oracle.  (CPU check of the
    algorithm; the HIP path itself is tests/test_cone_gpu.py and tests/test_configs_gpu.py.)"""
    import importlib.util
    from pathlib import Path

    from pmpc_amd import dynamics as dyn
    from tests.support.structured_np import Problem

    spec = importlib.util.spec_from_file_location("cone_ssn", Path(__file__).resolve().parents[1] / "tools" / "proto" / "cone_ssn.py")
    ssn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ssn)
    M, N, Nc = 4, 20, 1
    prob = dyn.make_quadrotor_problem(M=M, N=N, Nc=Nc)
    W = np.zeros((2, 4))
    W[0, 1] = W[1, 2] = 1.0
    v, v0, w0 = np.array([0.3, 0, 0, 0.0]), 0.0, np.zeros(2)
    Xp, Up, state, rounds = prob["X_prev"].copy(), prob["U_prev"].copy(), None, []
    for it in range(3):
        X_ = np.concatenate([prob["x0"][:, None, :], Xp[:, :-1]], 1)
        f, fx, fu = prob["f_fx_fu_fn"](X_, Up)
        p = Problem(f, fx, fu, Xp, Up, prob["Q"], prob["R"], prob["X_ref"], prob["U_ref"], prob["reg_x"], prob["reg_u"], Nc=Nc, u_l=prob["u_l"],
                    u_u=prob["u_u"])
        cas = ssn.ConeAS(p, W, w0, v, v0)
        if state is None:
            U0 = np.tile(np.array([9.81, 0, 0, 0.0]), (M, N, 1))
            act0, apex0, z0 = ssn.initial_from_solution(cas, U0)
        else:
            U0, z0, act0, apex0 = state
        U, z, act, apex, r, ok = cas.solve(U0, z0, act0, apex0)
        assert ok
        X = p.rollout(U)
        Xo, Uo = oracle.lsoc_solve_py(prob["x0"], f, fx, fu, Xp, Up, prob["Q"], prob["R"], prob["X_ref"], prob["U_ref"], reg_x=prob["reg_x"],
                                      reg_u=prob["reg_u"], Nc=Nc, u_l=prob["u_l"], u_u=prob["u_u"], soc_W=W, soc_w0=w0, soc_v=v, soc_v0=v0,
                                      u_interior=np.array([9.81, 0, 0, 0.0]))
        assert np.linalg.norm(X - Xo) / np.linalg.norm(Xo) < 1e-8 and np.linalg.norm(U - Uo) / np.linalg.norm(Uo) < 1e-8, it
        assert np.max(np.linalg.norm(U[..., 1:3], axis=-1) - 0.3 * U[..., 0]) < 1e-9  # inside every thrust cone
        rounds.append(r)
        state, Xp, Up = (U, z, act, apex), X, U
    assert max(rounds) <= 12, rounds


def test_state_rows_restated_as_auxiliary_states_are_the_same_problem(oracle):
    """`extra_cstrs` rows on the state and control of one stage (main.jl:293-316) -> upper bounds on auxiliary states the dynamics
    produce (`pmpc_amd.extra_cstrs.aux_state_problem`): the oracle solves the joint QP with the rows as rows, and the restated problem
    with state boxes only — the same minimiser to round-off (the auxiliary block's cost -reg_x cancels the proximal term exactly)."""
    import scipy.sparse as sp

    from pmpc_amd.extra_cstrs import aux_state_problem, stage_rows_from_extra_cstrs
    from tests.support.problems import rand_problem

    rng = np.random.default_rng(0)
    M, N, x, u, Nc = 3, 6, 4, 2, 1
    args, kw = rand_problem(rng, M, N, x, u, 1.0)
    x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref = args
    X0, U0 = oracle.lqp_solve_py(*args, Nc=Nc, **kw)
    ncu = Nc * u + M * (N - Nc) * u
    n = ncu + M * N * x
    xcol = lambda i, j, r: ncu + (i * N + j) * x + r
    ucol = lambda i, j, r: j * u + r if j < Nc else Nc * u + (i * (N - Nc) + (j - Nc)) * u + r
    spec = [(0, 2, 0), (1, 3, 1), (2, 0, 0), (0, 2, 0), (1, 5, 0)]
    G, h = np.zeros((len(spec), n)), np.zeros(len(spec))
    for k, (i, t, form) in enumerate(spec):
        a, b = rng.standard_normal(x), rng.standard_normal(u)
        jx = t - 1 if form == 1 else t
        for r in range(x):
            G[k, xcol(i, jx, r)] = a[r]
        for r in range(u):
            G[k, ucol(i, t, r)] = b[r]
        h[k] = a @ X0[i, jx] + b @ U0[i, t] - 0.3
    cstr = (len(h), [], 0, sp.csr_matrix(G), sp.csr_matrix((len(h), 0)), h, np.zeros(n), np.zeros(0))
    rows = stage_rows_from_extra_cstrs([cstr], M, N, x, u, Nc)
    assert [(r[0], r[1], r[2]) for r in rows] == spec
    aug = aux_state_problem(rows, x0, f, fx, fu, X_prev, U_prev, Q, X_ref, kw["reg_x"], None, None)
    assert aug["m"] == 2 and aug["f"].shape == (M, N, x + 2)
    Xa, Ua = oracle.lqp_solve_py(aug["x0"], aug["f"], aug["fx"], aug["fu"], aug["X_prev"], U_prev, aug["Q"], R, aug["X_ref"], U_ref, reg_x=kw["reg_x"],
                                 reg_u=kw["reg_u"], Nc=Nc, u_l=kw["u_l"], u_u=kw["u_u"], x_l=aug["x_l"], x_u=aug["x_u"])
    Xd, Ud = oracle.lqp_solve_py(*args, Nc=Nc, rows=(sp.csr_matrix(G), h), **kw)
    assert np.abs(Xd - X0).max() > 1e-2
    assert np.abs(Xa[..., :x] - Xd).max() < 1e-9 and np.abs(Ua - Ud).max() < 1e-9
    # refusals name the reason
    bad = np.zeros((1, n)); bad[0, xcol(0, 1, 0)] = 1.0; bad[0, xcol(1, 1, 0)] = 1.0
    with pytest.raises(ValueError, match="several particles"):
        stage_rows_from_extra_cstrs([(1, [], 0, bad, np.zeros((1, 0)), np.ones(1), np.zeros(n), np.zeros(0))], M, N, x, u, Nc)
    bad = np.zeros((1, n)); bad[0, xcol(0, 0, 0)] = 1.0; bad[0, ucol(0, 3, 0)] = 1.0
    with pytest.raises(ValueError, match="couples state stage"):
        stage_rows_from_extra_cstrs([(1, [], 0, bad, np.zeros((1, 0)), np.ones(1), np.zeros(n), np.zeros(0))], M, N, x, u, Nc)


def test_every_context_option_is_documented_where_a_maintainer_looks():
    """The option table of the library (pmpc_set_option / the environment variables that set the defaults) against include/pmpc_abi.h and
    INTEGRATION.md: an option added to the table and not to the documents fails here, not in a reader's hands."""
    import re
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    table = (root / "pmpc_amd" / "csrc" / "solver.hip").read_text()
    opts = re.findall(r'\{"([a-z_0-9]+)", "(PMPC_[A-Z_0-9]+)", [^}]+\}', table)
    assert len(opts) >= 20, opts
    header, integ = (root / "include" / "pmpc_abi.h").read_text(), (root / "INTEGRATION.md").read_text()
    missing = [(n, e) for n, e in opts if n not in header or e not in header or (e not in integ and n not in integ)]
    assert not missing, missing
