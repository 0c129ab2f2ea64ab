"""Shared pieces of the tests of the stage-cone PATH-FOLLOWING iteration (kernels_soc.hip, QpSolve::soc_interior_point): seeded cone
data, the oracle's optimum (computed once per case), the conditions a case must meet so that it cannot pass vacuously, the device
call, and the checks against the oracle.  Everything in py layout (oracle/lqp_oracle.py) until `device_solve` transposes."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from tests.support.problems import rand_problem

TOL = 1e-6  # BASELINE.json north_star, as tests/test_cone_gpu.py
COMPILED_UQ = {(4, 2), (4, 3), (4, 1), (3, 2), (3, 1), (2, 1)}  # PMPC_SOC_DIMS of kernels_soc.hip; every other pair: the run-time-size instance


class Case(NamedTuple):
    M: int
    N: int
    x: int
    u: int
    Nc: int
    box: Optional[float]  # +-box on every control; None: no boxes
    q: int
    v0: float
    seed: int = 0
    one_sided: bool = False  # every control keeps ONE side of its box (which one alternates), the other is +-inf

    def instance(self):
        return f"soc{self.u}x{self.q}" if (self.u, self.q) in COMPILED_UQ else f"socRT(u{self.u}q{self.q})"

    def nc_class(self):
        return {0: "Nc0", -1: "NcAll"}.get(self.Nc, f"Nc{self.Nc}")

    def id(self, family):
        box = "nobox" if self.box is None else ("onesided" if self.one_sided else "box")
        return f"{self.instance()}-{family}-{self.nc_class()}-M{self.M}N{self.N}x{self.x}u{self.u}-{box}"


def cone_data(u, q, v0, seed=0):
    """|| W u + w0 || <= v'u + v0 with W[p, (1 + p) % u] in 1 .. 1.3 (0.3 x that on column 0, which v weighs), w0 ~ 0.02 N(0, 1), v = 0.5 e0 and
    u_interior = 0.2 e0; udim 1: |u + w0| <= 0.2 u + v0 from u_interior = 0."""
    rng = np.random.default_rng(31000 + 97 * seed + 8 * u + q)
    W = np.zeros((q, u))
    if u == 1:
        assert q == 1
        W[0, 0], v, u_int = 1.0, np.array([0.2]), np.zeros(1)
    else:
        for p in range(q):
            col = (1 + p) % u
            W[p, col] = (1.0 + 0.3 * rng.random()) * (0.3 if col == 0 else 1.0)
        v, u_int = 0.5 * np.eye(u)[0], 0.2 * np.eye(u)[0]
    w0 = 0.02 * rng.standard_normal(q)
    soc = dict(W=W, w0=w0, v=v, v0=float(v0), u_interior=u_int)
    assert cone_slack(u_int, soc) > 1e-3, "u_interior is not strictly inside the cone"
    return soc


def cone_slack(U, soc):
    """v'u + v0 - || W u + w0 || on the last axis of U."""
    return U @ soc["v"] + soc["v0"] - np.linalg.norm(U @ soc["W"].T + soc["w0"], axis=-1)


def make(case: Case):
    """(args, kw, soc) of a case: `rand_problem` with its boxes, the cone data above."""
    args, kw = rand_problem(np.random.default_rng(52000 + case.seed), case.M, case.N, case.x, case.u, case.box)
    if case.one_sided:
        keep_lo = (np.arange(case.N)[:, None] + np.arange(case.u)[None, :]) % 2 == 0  # (N, u): the same on every particle
        kw["u_l"] = np.where(keep_lo, kw["u_l"], -np.inf)
        kw["u_u"] = np.where(~keep_lo, kw["u_u"], np.inf)
    return args, kw, cone_data(case.u, case.q, case.v0, case.seed)


def oracle_solve(oracle, args, kw, Nc, soc):
    return oracle.lsoc_solve_py(*args, Nc=Nc, reg_x=kw["reg_x"], reg_u=kw["reg_u"], u_l=kw.get("u_l"), u_u=kw.get("u_u"), soc_W=soc["W"],
                                soc_w0=soc["w0"], soc_v=soc["v"], soc_v0=soc["v0"], u_interior=soc["u_interior"])


_reference = {}


def reference(oracle, case: Case):
    """(args, kw, soc, Xo, Uo) of a case, the oracle run once per session; the arrays are shared: read them, never write."""
    if case not in _reference:
        args, kw, soc = make(case)
        Xo, Uo = oracle_solve(oracle, args, kw, case.Nc, soc)
        for a in (*args, Xo, Uo, *(v for v in kw.values() if isinstance(v, np.ndarray)), *(v for v in soc.values() if isinstance(v, np.ndarray))):
            a.setflags(write=False)
        _reference[case] = (args, kw, soc, Xo, Uo)
    return _reference[case]


def counted_slacks(Uo, Nc, soc):
    """Cone slacks of the cones the problem HAS: a consensus stage's shared control carries one (particle 0's copy), a free stage one per particle."""
    N = Uo.shape[1]
    k = N if Nc < 0 else Nc
    sl = cone_slack(Uo, soc)
    return np.concatenate([sl[0, :k].ravel(), sl[:, k:].ravel()])


def assert_input_conditions(Uo, kw, Nc, soc):
    """From the oracle's optimum alone: of the counted cones one at least is active (slack < 1e-6) and one inactive (> 1e-3); with boxes, one
    control at least lies on a box side.  (Consensus stages use particle 0's boxes.)"""
    sl = counted_slacks(Uo, Nc, soc)
    assert (sl < 1e-6).sum() >= 1, ("no active cone", sl.min())
    assert (sl > 1e-3).sum() >= 1, ("no inactive cone", sl.max())
    if "u_l" in kw:
        lo, hi = effective_boxes(kw, Nc)
        assert ((np.abs(Uo - lo) < 1e-7) | (np.abs(hi - Uo) < 1e-7)).sum() >= 1, "no control on a box side"


def effective_boxes(kw, Nc):
    lo, hi = np.array(kw["u_l"], copy=True), np.array(kw["u_u"], copy=True)
    k = lo.shape[1] if Nc < 0 else Nc
    lo[:, :k], hi[:, :k] = lo[0:1, :k], hi[0:1, :k]
    return lo, hi


def device_solve(s, args, kw, Nc, soc, *, symmetric_cost=True, dtype=None, u_interior=None, **flags):
    """One `DeviceSolver.lsoc_solve` on the context `s`: (X, U, status, info) with numpy outputs.  `dtype`: storage type of fx, fu, Q, R."""
    import torch

    md = torch.float64 if dtype is None else dtype
    x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref = args
    dev = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    T = lambda a: dev(np.swapaxes(a, -1, -2), md)
    bounds = dict(lu=dev(kw["u_l"]), uu=dev(kw["u_u"])) if "u_l" in kw else {}
    X, U, status = s.lsoc_solve(f=dev(f), fx=T(fx), fu=T(fu), X_prev=dev(X_prev), U_prev=dev(U_prev), Q=T(Q), R=T(R), X_ref=dev(X_ref),
                                U_ref=dev(U_ref), reg_x=kw["reg_x"], reg_u=kw["reg_u"], Nc=Nc, symmetric_cost=symmetric_cost, soc_W=dev(soc["W"]),
                                soc_w0=dev(soc["w0"]), soc_v=dev(soc["v"]), soc_v0=soc["v0"],
                                soc_u_interior=dev(soc["u_interior"] if u_interior is None else u_interior), **bounds, **flags)
    s.sync()
    return X.cpu().numpy(), U.cpu().numpy(), status, dict(s.last_info)


def errors(X, U, Xo, Uo):
    """|X - X*| / |X*| and |U - U*| / max(|U*|, 1)."""
    return np.linalg.norm(X - Xo) / np.linalg.norm(Xo), np.linalg.norm(U - Uo) / max(np.linalg.norm(Uo), 1.0)


def assert_matches(X, U, Xo, Uo, kw, Nc, soc, tol=TOL, label=""):
    """Feasible to round-off (cone slack > -1e-9, boxes within 1e-9) and within `tol` of the oracle; prints the two errors first.  Returns them."""
    ex, eu = errors(X, U, Xo, Uo)
    print(f"soc_path {label}: rel err X {ex:.3e} U {eu:.3e}")
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(U))
    assert cone_slack(U, soc).min() > -1e-9, cone_slack(U, soc).min()
    if "u_l" in kw:
        lo, hi = effective_boxes(kw, Nc)
        assert (U - lo).min() > -1e-9 and (hi - U).min() > -1e-9, ((U - lo).min(), (hi - U).min())
    assert ex < tol and eu < tol, (label, ex, eu)
    return ex, eu
