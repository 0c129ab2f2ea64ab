"""Seeded inputs of the keep-out tests (py layout), shared by tests/test_keepout_gpu.py and the checks that were run on them before they
were committed: every sub-problem here is feasible by construction, its rows bind and they move the optimum."""
from __future__ import annotations

import numpy as np

from tests.support.problems import rand_problem


def keepout_subproblem(seed, M, N, x, u, K, pd, bu=1.0):
    """One linearised sub-problem with K balls.  `rand_problem`'s dynamics with f := X_prev, so that u = U_prev reproduces the plan X_prev
    exactly: the plan clears every ball by half a radius (r_k = nearest plan position / 1.5) and lies strictly inside the control boxes,
    hence the sub-problem with the rows about X_prev is strictly feasible.  The position references sit on the balls' centres (stage j on
    centre j mod K): the optimum without the rows is pulled into the balls.  Returns (args, kw, cstr)."""
    rng = np.random.default_rng(seed)
    args, kw = rand_problem(rng, M, N, x, u, bu)
    x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref = args
    f = X_prev.copy()
    centres = 0.3 * rng.standard_normal((K, pd))
    dist = np.linalg.norm(X_prev[:, :, None, :pd] - centres, axis=-1)  # (M, N, K)
    radius = dist.min((0, 1)) / 1.5
    X_ref = X_ref.copy()
    X_ref[..., :pd] = centres[np.arange(N) % K][None]
    cstr = dict(kind="keepout", pos_idx=tuple(range(pd)), centres=centres, radius=radius)
    return (x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref), kw, cstr


def rows_of(cstr, args, Nc):
    """(tuple, (G, h)) of the keep-out rows about the sub-problem's X_prev, over z = [U_cons; U_free; X]."""
    from pmpc_amd.extra_cstrs import make_keepout_extra_cstrs_fn

    tup = make_keepout_extra_cstrs_fn(cstr, Nc)(args[4], args[5], None)[0]
    return tup, (tup[3], tup[5])


def bicycle_keepout_problem(M=3, N=12):
    """A slow car (2 m/s, 0.2 s steps, 1 m wheelbase +- 5 %) asked to drive along y = 0 through a ball of radius 0.4 at (2.4, 0) — where
    stage 5 of the straight plan is —, starting 0.6 - 0.8 m to the left of the line; the start plan is the rollout of zero controls:
    straight on, clear of the ball by 0.2 m and more.  Returns the keyword arguments of `solve` (numpy, with `params`) and the constraint."""
    dt, v0 = 0.2, 2.0
    L = 1.0 * (1 + 0.05 * np.array([0.0, 1.0, -1.0, 0.5, -0.5])[np.arange(M) % 5])
    params = np.stack([L, np.full(M, dt)], -1)
    x0 = np.zeros((M, 4))
    x0[:, 1] = 0.7 + 0.1 * np.array([0.0, 1.0, -1.0, 0.5, -0.5])[np.arange(M) % 5]
    x0[:, 3] = v0
    t = dt * np.arange(1, N + 1)
    X_ref = np.zeros((M, N, 4))
    X_ref[..., 0] = v0 * t[None, :]
    X_ref[..., 3] = v0
    X_prev = np.tile(x0[:, None, :], (1, N, 1))
    X_prev[..., 0] = v0 * t[None, :]
    bound = np.array([2.0, 0.5])
    kw = dict(Q=np.tile(np.diag([1.0, 10.0, 1.0, 1.0]), (M, N, 1, 1)), R=np.tile(np.diag([0.1, 1.0]), (M, N, 1, 1)), x0=x0, X_ref=X_ref,
              U_ref=np.zeros((M, N, 2)), X_prev=X_prev, U_prev=np.zeros((M, N, 2)), u_l=np.tile(-bound, (M, N, 1)), u_u=np.tile(bound, (M, N, 1)),
              reg_x=1.0, reg_u=1.0, params=params)
    cstr = dict(kind="keepout", pos_idx=(0, 1), centres=np.array([[2.4, 0.0]]), radius=np.array([0.4]))
    return kw, cstr
