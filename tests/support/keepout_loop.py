"""Helpers of tests/test_keepout_loop.py and tests/test_keepout_loop_gpu.py: the two drivers of the SCP loop with a keep-out constraint (the
library loop `DeviceSolver.scp_loop(cstr=, aug=)` and the Python-driven `pmpc_amd.solve(..., device="cuda", builtin_cstr=...)`) on one
problem, guarded allocations, and the keep-out problems of the models tests/support/keepout_problems.py has none for."""
from __future__ import annotations

import math

import numpy as np

GUARD, SENTINEL = 64, 1234.5
FEAS = 1e-8  # the feasibility bound of tests/test_keepout_gpu.py
SETTINGS = dict(solver="osqp", Nc=1)
LOOP_KEYS = ("X_ref", "U_ref", "X_prev", "U_prev", "u_l", "u_u", "reg_x", "reg_u")


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1.0)


def outside(X, cstr):
    """min over (particle, stage, ball) of |p - c| - r for stages X (M, N, x): >= 0 means no stage is inside a ball."""
    from pmpc_amd.extra_cstrs import _keepout_arrays

    M, N, x = X.shape
    pos_idx, cen, rad = _keepout_arrays(cstr, M, N, x)
    d = np.linalg.norm(X[:, :, None, pos_idx] - np.broadcast_to(cen, (M, N, rad.shape[0], len(pos_idx))), axis=-1)
    return float((d - rad).min())


def guarded(shape, dtype=None, fill=SENTINEL):
    """A CUDA tensor of `shape` inside a flat allocation with GUARD sentinel entries on both sides: (whole, view)."""
    import torch

    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype or torch.float64, device="cuda")
    view = whole[GUARD:GUARD + n].view(*shape)
    if fill != SENTINEL:
        view.fill_(fill)
    return whole, view


def guards_intact(whole):
    import torch

    return bool(torch.all(whole[:GUARD] == SENTINEL)) and bool(torch.all(whole[-GUARD:] == SENTINEL))


def python_loop(model, kw, cstr, steps, settings=SETTINGS, solver=None, **over):
    """`steps` iterations (res_tol = 0) of the Python-driven device loop: (X (M, N + 1, x), U, data)."""
    import pmpc_amd

    args = {**{k: kw[k] for k in LOOP_KEYS}, **dict(max_it=steps, res_tol=0.0, verbose=False, solver_settings=dict(settings)), **over}
    return pmpc_amd.solve(None, kw["Q"], kw["R"], kw["x0"], device="cuda", builtin_model=model, params=kw["params"], builtin_cstr=cstr, solver=solver, **args)


def library_loop(s, model, kw, cstr, steps, settings=SETTINGS, cost=None, first_cold=True):
    """`steps` iterations of the library loop on the context `s` from the problem's start iterate, every buffer fresh:
    (residuals, X (M, N, x), U, infos) as numpy.  The problem goes through `build_problem`, as the controller's does."""
    import torch

    from pmpc_amd.device_problem import build_problem, keepout_buffers

    p = build_problem(kw["Q"], kw["R"], kw["x0"], kw["X_ref"], kw["U_ref"], kw["X_prev"], kw["U_prev"], None, None, kw["u_l"], kw["u_u"], kw["reg_x"],
                      kw["reg_u"], None, None, dict(settings), None, model, kw["params"], "cuda")
    M, N, x, u = p.M, p.N, p.xdim, p.udim
    extra = dict(cone_objective=True, barrier_mu=0.0 if math.isnan(p.smooth_alpha) else 1.0 / p.smooth_alpha) if p.cone else {}
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    handle = aug = None
    if cstr is not None:
        handle = s.prepare_cstr(cstr, M, N, x)
        aug = keepout_buffers(p, handle[0].K)
    Xb, Ub = mk(M, N, x), mk(M, N, u)
    torch.cuda.synchronize()
    res, infos, last, done = s.scp_loop(p.model, p.params, steps, f=mk(M, N, x), fx=mk(M, N, x, x), fu=mk(M, N, u, x), f2=mk(M, N, x), fx2=mk(M, N, x, x),
                                        fu2=mk(M, N, u, x), X_prev=p.X_prev, U_prev=p.U_prev, X_out=Xb, U_out=Ub, X_ref=p.X_ref, U_ref=p.U_ref,
                                        first_cold=first_cold, cost=cost, cstr=handle, aug=aug, **p.solve_kw(), **extra)
    s.sync()
    assert done == steps and all(i["status"] == 0 for i in infos), infos
    X, U = (Xb, Ub) if last else (p.X_prev, p.U_prev)
    return res.cpu().numpy(), X.cpu().numpy(), U.cpu().numpy(), infos


def _beside(P, stage, side, gap):
    """A point `gap` beside stage `stage` of the planar paths P (M, N, 2), on the left (side +1) or the right (-1) of the direction of travel."""
    t = P[:, stage + 1] - P[:, stage - 1]
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    return P[:, stage] + side * gap * np.stack([-t[:, 1], t[:, 0]], -1)


def unicycle_keepout_problem(M=4, N=6):
    """`make_unicycle_problem` (x 4: the sub-problem with K = 2 runs at 6 states) started from the rollout of zero controls — a dynamically
    feasible plan inside the control boxes — with two balls of radius 0.2 per particle, 0.3 beside stages 1 and 3 of the particle's own
    start plan (centres (M, N, K, 2), the same at every stage): clear of every stage of the start plan by 0.1 and more, so the first
    sub-problem is strictly feasible.  Returns (kw, cstr) like `bicycle_keepout_problem`."""
    from pmpc_amd import dynamics as dyn

    prob = dyn.make_unicycle_problem(M=M, N=N, Nc=1)
    kw = {k: prob[k] for k in ("Q", "R", "x0", "params") + LOOP_KEYS}
    kw["X_prev"] = dyn.rollout("unicycle", prob["x0"], prob["U_prev"], prob["params"])
    P = kw["X_prev"][..., :2]
    cen = np.stack([_beside(P, 1, +1, 0.3), _beside(P, 3, -1, 0.3)], 1)  # (M, K, 2)
    cstr = dict(kind="keepout", pos_idx=(0, 1), centres=np.ascontiguousarray(np.broadcast_to(cen[:, None], (M, N, 2, 2))), radius=np.array([0.2, 0.2]))
    return kw, cstr


def quadrotor_keepout_problem(M=2, N=5):
    """`make_quadrotor_problem` (x 12, K = 1: 13 states, the generic kernels) started from the rollout of the hover controls, with one
    ball of radius 0.2 per particle, 0.3 from the particle's start position towards the origin the references pull to (centres
    (M, N, 1, 3)): the hovering start plan clears it by 0.1."""
    from pmpc_amd import dynamics as dyn

    prob = dyn.make_quadrotor_problem(M=M, N=N, Nc=1)
    kw = {k: prob[k] for k in ("Q", "R", "x0", "params") + LOOP_KEYS}
    kw["X_prev"] = dyn.rollout("quadrotor", prob["x0"], prob["U_prev"], prob["params"])
    p0 = prob["x0"][:, :3]
    cen = p0 - 0.3 * p0 / np.linalg.norm(p0, axis=-1, keepdims=True)
    cstr = dict(kind="keepout", pos_idx=(0, 1, 2), centres=np.ascontiguousarray(np.broadcast_to(cen[:, None, None], (M, N, 1, 3))), radius=np.array([0.2]))
    return kw, cstr
