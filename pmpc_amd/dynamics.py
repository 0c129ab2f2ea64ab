"""Host (numpy) definitions of the dynamics used by the benchmark configs, with analytic
Jacobians, in the reference's `f_fx_fu_fn(X, U) -> f, fx, fu` contract
(README.md:136-145; call site pmpc/scp_mpc.py:338-342):

    f[..., r]      = F_r(x, u)
    fx[..., r, t]  = dF_r/dx_t
    fu[..., r, t]  = dF_r/du_t

* `unicycle`  — the 4-state / 2-control car of the reference's tests/dubins_car.py:48-90
  (the reference differentiates it with torch.autograd, :11-30; the closed form here is the
  same function, checked against that autograd in tests/test_dynamics.py).
* `quadrotor` — the synthetic 12-state / 4-control rigid body of SURVEY.md §8(d) (NOT in the
  reference): x = [p(3), v(3), rpy(3), w(3)], u = [T, tx, ty, tz], explicit Euler, dt = 0.05.

* `bicycle`   — the kinematic bicycle (NOT in the reference): x = [px, py, theta, v], u = [a, delta], p = [L, dt],
  forward Euler; checked against complex-step differentiation of its own `f` in tests/test_bicycle_model.py.

These are the specifications the on-device linearisation kernels (csrc/dynamics.hip) follow.

`obstacle_cost` is the specification of the built-in obstacle cost (csrc/cost_lin.hip), `make_obstacle_lin_cost_fn` wraps it as a
`lin_cost_fn` of the SCP loops (pmpc/scp_mpc.py:171-185).
"""
from __future__ import annotations

import numpy as np

G_ACC = 9.81


# -------------------------------------------------------------------------------------------------
# unicycle (reference tests/dubins_car.py:48-90)
# -------------------------------------------------------------------------------------------------
def unicycle(x, u, p, eps=1e-6):
    """x (...,4) = [px, py, v, th]; u (...,2) = [acc, turn]; p (...,3) = [v_scale, w_scale, T]."""
    x, u, p = np.asarray(x, float), np.asarray(u, float), np.asarray(p, float)
    vs, ws, T = p[..., 0], p[..., 1], p[..., 2]
    u1 = vs * u[..., 0]
    u2 = -ws * u[..., 1]
    u1 = u1 + np.where(u1 >= 0.0, eps, -eps)
    u2 = u2 + np.where(u2 >= 0.0, eps, -eps)
    px, py, v0, th0 = x[..., 0], x[..., 1], x[..., 2], x[..., 3]
    a = T * u2 + th0
    sa, ca, s0, c0 = np.sin(a), np.cos(a), np.sin(th0), np.cos(th0)
    iu2 = 1.0 / u2
    iu22 = iu2 * iu2
    # xp1 = px + (u2 sa v0 + T u1 u2 sa + u1 ca)/u2^2 - (s0 u2 v0 + c0 u1)/u2^2
    n1 = u2 * sa * v0 + T * u1 * u2 * sa + u1 * ca - s0 * u2 * v0 - c0 * u1
    # xp2 = py - (u2 ca v0 - u1 sa + T u1 u2 ca)/u2^2 + (c0 u2 v0 - s0 u1)/u2^2
    n2 = -(u2 * ca * v0 - u1 * sa + T * u1 * u2 * ca) + c0 * u2 * v0 - s0 * u1
    f = np.stack([px + n1 * iu22, py + n2 * iu22, v0 + T * u1, a], -1)

    shp = x.shape[:-1]
    fx = np.zeros(shp + (4, 4))
    fu = np.zeros(shp + (4, 2))
    # d/dv0, d/dth0 (da/dth0 = 1)
    dn1_dv = u2 * sa - s0 * u2
    dn1_dth = u2 * ca * v0 + T * u1 * u2 * ca - u1 * sa - c0 * u2 * v0 + s0 * u1
    dn2_dv = -u2 * ca + c0 * u2
    dn2_dth = -(-u2 * sa * v0 - u1 * ca - T * u1 * u2 * sa) - s0 * u2 * v0 - c0 * u1
    fx[..., 0, 0] = 1.0
    fx[..., 0, 2] = dn1_dv * iu22
    fx[..., 0, 3] = dn1_dth * iu22
    fx[..., 1, 1] = 1.0
    fx[..., 1, 2] = dn2_dv * iu22
    fx[..., 1, 3] = dn2_dth * iu22
    fx[..., 2, 2] = 1.0
    fx[..., 3, 3] = 1.0
    # d/du1, d/du2 (da/du2 = T), then chain to the raw controls: du1/dU0 = vs, du2/dU1 = -ws
    dn1_du1 = T * u2 * sa + ca - c0
    dn2_du1 = sa - T * u2 * ca - s0
    dn1_du2 = sa * v0 + u2 * ca * T * v0 + T * u1 * sa + T * u1 * u2 * ca * T - u1 * sa * T - s0 * v0
    dn2_du2 = -(ca * v0 - u2 * sa * T * v0 - u1 * ca * T + T * u1 * ca - T * T * u1 * u2 * sa) + c0 * v0
    d1_du2 = dn1_du2 * iu22 - 2.0 * n1 * iu22 * iu2
    d2_du2 = dn2_du2 * iu22 - 2.0 * n2 * iu22 * iu2
    fu[..., 0, 0] = dn1_du1 * iu22 * vs
    fu[..., 1, 0] = dn2_du1 * iu22 * vs
    fu[..., 2, 0] = T * vs
    fu[..., 0, 1] = d1_du2 * (-ws)
    fu[..., 1, 1] = d2_du2 * (-ws)
    fu[..., 3, 1] = T * (-ws)
    return f, fx, fu


def unicycle_torch(x, u, p, eps=1e-6):
    """`unicycle` on torch tensors of any device (same closed form, same outputs) — an example of an `f_fx_fu_fn` for
    the device-resident loop `solve(..., device="cuda")`."""
    import torch

    vs, ws, T = p[..., 0], p[..., 1], p[..., 2]
    u1, u2 = vs * u[..., 0], -ws * u[..., 1]
    u1 = u1 + torch.where(u1 >= 0.0, eps, -eps)
    u2 = u2 + torch.where(u2 >= 0.0, eps, -eps)
    px, py, v0, th0 = x[..., 0], x[..., 1], x[..., 2], x[..., 3]
    a = T * u2 + th0
    sa, ca, s0, c0 = torch.sin(a), torch.cos(a), torch.sin(th0), torch.cos(th0)
    iu2 = 1.0 / u2
    iu22 = iu2 * iu2
    n1 = u2 * sa * v0 + T * u1 * u2 * sa + u1 * ca - s0 * u2 * v0 - c0 * u1
    n2 = -(u2 * ca * v0 - u1 * sa + T * u1 * u2 * ca) + c0 * u2 * v0 - s0 * u1
    f = torch.stack([px + n1 * iu22, py + n2 * iu22, v0 + T * u1, a], -1)
    fx = torch.zeros(x.shape[:-1] + (4, 4), dtype=x.dtype, device=x.device)
    fu = torch.zeros(x.shape[:-1] + (4, 2), dtype=x.dtype, device=x.device)
    fx[..., 0, 0] = fx[..., 1, 1] = fx[..., 2, 2] = fx[..., 3, 3] = 1.0
    fx[..., 0, 2] = (u2 * sa - s0 * u2) * iu22
    fx[..., 0, 3] = (u2 * ca * v0 + T * u1 * u2 * ca - u1 * sa - c0 * u2 * v0 + s0 * u1) * iu22
    fx[..., 1, 2] = (-u2 * ca + c0 * u2) * iu22
    fx[..., 1, 3] = (-(-u2 * sa * v0 - u1 * ca - T * u1 * u2 * sa) - s0 * u2 * v0 - c0 * u1) * iu22
    dn1_du1, dn2_du1 = T * u2 * sa + ca - c0, sa - T * u2 * ca - s0
    dn1_du2 = sa * v0 + u2 * ca * T * v0 + T * u1 * sa + T * u1 * u2 * ca * T - u1 * sa * T - s0 * v0
    dn2_du2 = -(ca * v0 - u2 * sa * T * v0 - u1 * ca * T + T * u1 * ca - T * T * u1 * u2 * sa) + c0 * v0
    fu[..., 0, 0], fu[..., 1, 0], fu[..., 2, 0] = dn1_du1 * iu22 * vs, dn2_du1 * iu22 * vs, T * vs
    fu[..., 0, 1] = (dn1_du2 * iu22 - 2.0 * n1 * iu22 * iu2) * (-ws)
    fu[..., 1, 1] = (dn2_du2 * iu22 - 2.0 * n2 * iu22 * iu2) * (-ws)
    fu[..., 3, 1] = T * (-ws)
    return f, fx, fu


# -------------------------------------------------------------------------------------------------
# kinematic bicycle, forward Euler (built-in model 2)
# -------------------------------------------------------------------------------------------------
def bicycle(x, u, p):
    """x (...,4) = [px, py, theta, v]; u (...,2) = [a, delta] (acceleration, steering angle); p (...,2) = [L, dt]
    (wheelbase, step).  Complex inputs are kept complex (complex-step differentiation of `f`)."""
    num = lambda a: np.asarray(a, complex if np.iscomplexobj(a) else float)
    x, u, p = num(x), num(u), num(p)
    L, dt = p[..., 0], p[..., 1]
    px, py, th, v = x[..., 0], x[..., 1], x[..., 2], x[..., 3]
    acc, td = u[..., 0], np.tan(u[..., 1])
    s, c = np.sin(th), np.cos(th)
    dtv = dt * v
    f = np.stack([px + dtv * c, py + dtv * s, th + dtv * td / L, v + dt * acc], -1)
    shp = f.shape[:-1]
    fx = np.zeros(shp + (4, 4), dtype=f.dtype)
    fu = np.zeros(shp + (4, 2), dtype=f.dtype)
    for k in range(4):
        fx[..., k, k] = 1.0
    fx[..., 0, 2] = -dtv * s
    fx[..., 0, 3] = dt * c
    fx[..., 1, 2] = dtv * c
    fx[..., 1, 3] = dt * s
    fx[..., 2, 3] = dt * td / L
    fu[..., 3, 0] = dt
    fu[..., 2, 1] = dtv * (1.0 + td * td) / L  # sec^2 = 1 + tan^2
    return f, fx, fu


def bicycle_torch(x, u, p):
    """`bicycle` on torch tensors of any device — an `f_fx_fu_fn` body for the device-resident loop `solve(..., device="cuda")`."""
    import torch

    L, dt = p[..., 0], p[..., 1]
    px, py, th, v = x[..., 0], x[..., 1], x[..., 2], x[..., 3]
    acc, td = u[..., 0], torch.tan(u[..., 1])
    s, c = torch.sin(th), torch.cos(th)
    dtv = dt * v
    f = torch.stack([px + dtv * c, py + dtv * s, th + dtv * td / L, v + dt * acc], -1)
    fx = torch.zeros(f.shape[:-1] + (4, 4), dtype=f.dtype, device=f.device)
    fu = torch.zeros(f.shape[:-1] + (4, 2), dtype=f.dtype, device=f.device)
    fx[..., 0, 0] = fx[..., 1, 1] = fx[..., 2, 2] = fx[..., 3, 3] = 1.0
    fx[..., 0, 2], fx[..., 0, 3] = -dtv * s, dt * c
    fx[..., 1, 2], fx[..., 1, 3] = dtv * c, dt * s
    fx[..., 2, 3] = dt * td / L
    fu[..., 3, 0] = dt
    fu[..., 2, 1] = dtv * (1.0 + td * td) / L
    return f, fx, fu


# -------------------------------------------------------------------------------------------------
# synthetic quadrotor
# -------------------------------------------------------------------------------------------------
QUAD_DT = 0.05


def quadrotor(x, u, p, dt=QUAD_DT):
    """x (...,12), u (...,4), p (...,4) = [mass, Jx, Jy, Jz]. Explicit Euler step of a rigid body with
    ZYX Euler angles rpy = (phi, theta, psi)."""
    x, u, p = np.asarray(x, float), np.asarray(u, float), np.asarray(p, float)
    m, Jx, Jy, Jz = (p[..., i] for i in range(4))
    v = x[..., 3:6]
    ph, th, ps = x[..., 6], x[..., 7], x[..., 8]
    wx, wy, wz = x[..., 9], x[..., 10], x[..., 11]
    T, tx, ty, tz = (u[..., i] for i in range(4))
    sph, cph, sth, cth, sps, cps = np.sin(ph), np.cos(ph), np.sin(th), np.cos(th), np.sin(ps), np.cos(ps)
    tth, icth = sth / cth, 1.0 / cth
    # thrust direction b = R e3
    bx = cps * sth * cph + sps * sph
    by = sps * sth * cph - cps * sph
    bz = cth * cph
    a = T / m
    shp = x.shape[:-1]
    xd = np.zeros(shp + (12,))
    xd[..., 0:3] = v
    xd[..., 3], xd[..., 4], xd[..., 5] = a * bx, a * by, a * bz - G_ACC
    xd[..., 6] = wx + sph * tth * wy + cph * tth * wz
    xd[..., 7] = cph * wy - sph * wz
    xd[..., 8] = sph * icth * wy + cph * icth * wz
    xd[..., 9] = (tx - (Jz - Jy) * wy * wz) / Jx
    xd[..., 10] = (ty - (Jx - Jz) * wz * wx) / Jy
    xd[..., 11] = (tz - (Jy - Jx) * wx * wy) / Jz
    f = x + dt * xd

    A = np.zeros(shp + (12, 12))
    B = np.zeros(shp + (12, 4))
    for i in range(3):
        A[..., i, 3 + i] = 1.0
    # d b / d(ph, th, ps)
    dbx = (-cps * sth * sph + sps * cph, cps * cth * cph, -sps * sth * cph + cps * sph)
    dby = (-sps * sth * sph - cps * cph, sps * cth * cph, cps * sth * cph + sps * sph)
    dbz = (-cth * sph, -sth * cph, np.zeros_like(ph))
    for k in range(3):
        A[..., 3, 6 + k] = a * dbx[k]
        A[..., 4, 6 + k] = a * dby[k]
        A[..., 5, 6 + k] = a * dbz[k]
    sec2 = icth * icth
    # rpy rates
    A[..., 6, 6] = cph * tth * wy - sph * tth * wz
    A[..., 6, 7] = sph * sec2 * wy + cph * sec2 * wz
    A[..., 6, 9], A[..., 6, 10], A[..., 6, 11] = 1.0, sph * tth, cph * tth
    A[..., 7, 6] = -sph * wy - cph * wz
    A[..., 7, 10], A[..., 7, 11] = cph, -sph
    A[..., 8, 6] = cph * icth * wy - sph * icth * wz
    A[..., 8, 7] = (sph * wy + cph * wz) * sth * sec2
    A[..., 8, 10], A[..., 8, 11] = sph * icth, cph * icth
    # body rates
    A[..., 9, 10], A[..., 9, 11] = -(Jz - Jy) * wz / Jx, -(Jz - Jy) * wy / Jx
    A[..., 10, 9], A[..., 10, 11] = -(Jx - Jz) * wz / Jy, -(Jx - Jz) * wx / Jy
    A[..., 11, 9], A[..., 11, 10] = -(Jy - Jx) * wy / Jz, -(Jy - Jx) * wx / Jz
    B[..., 3, 0], B[..., 4, 0], B[..., 5, 0] = bx / m, by / m, bz / m
    B[..., 9, 1], B[..., 10, 2], B[..., 11, 3] = 1.0 / Jx, 1.0 / Jy, 1.0 / Jz
    fx = np.eye(12) + dt * A
    fu = dt * B
    return f, fx, fu


# -------------------------------------------------------------------------------------------------
# nonlinear rollout and receding-horizon shift of the built-in models (specifications of csrc/dynamics.hip k_rollout, k_shift_plan)
# -------------------------------------------------------------------------------------------------
MODEL_NAMES = ("unicycle", "quadrotor", "bicycle")  # position = the model id of include/pmpc_abi.h


def model_id(model):
    """The id of a built-in model given by name or by id."""
    if isinstance(model, str):
        if model not in MODEL_NAMES:
            raise ValueError(f"unknown built-in model {model!r}: one of {MODEL_NAMES}")
        return MODEL_NAMES.index(model)
    if int(model) not in range(len(MODEL_NAMES)):
        raise ValueError(f"unknown built-in model id {model}: 0 .. {len(MODEL_NAMES) - 1}")
    return int(model)


def _model_fn(model):
    return (unicycle, quadrotor, bicycle)[model_id(model)]


def rollout(model, x0, U, params):
    """X (M, N, x) with X[:, j] = F(X[:, j - 1], U[:, j]; params), X[:, -1] = x0: x0 (M, x), U (M, N, u), params (M, p)."""
    F = _model_fn(model)
    x, U, params = np.asarray(x0, float), np.asarray(U, float), np.asarray(params, float)
    X = np.empty(U.shape[:2] + x.shape[-1:])
    for j in range(U.shape[1]):
        x = F(x, U[:, j], params)[0]
        X[:, j] = x
    return X


def shift_plan(model, X, U, params, s=1, U_tail=None):
    """The plan (X, U) moved `s` stages on, 1 <= s < N: (X', U', um1') with X'[:, j] = X[:, j + s], U'[:, j] = U[:, j + s] for j < N - s, the
    last s controls from `U_tail` (M, s, u) (None: U[:, N - 1] held), the last s states rolled out from X[:, N - 1] under them, and
    um1' = U[:, s - 1], the control that was applied last."""
    X, U = np.asarray(X, float), np.asarray(U, float)
    N = U.shape[1]
    if not 1 <= int(s) < N:
        raise ValueError(f"shift_plan: s = {s} is outside 1 .. N - 1 = {N - 1}")
    s = int(s)
    tail = np.repeat(U[:, N - 1:], s, 1) if U_tail is None else np.asarray(U_tail, float).reshape(U.shape[0], s, U.shape[2])
    Un = np.concatenate([U[:, s:], tail], 1)
    Xn = np.concatenate([X[:, s:], rollout(model, X[:, N - 1], tail, params)], 1)
    return Xn, Un, U[:, s - 1].copy()


def shift_active_set(act, U, lo, hi, Nc, s, U_tail=None):
    """The control-box statuses `act` (M, N, u) int32 (0 free, 1 on the lower, 2 on the upper bound) of the plan's controls U moved `s`
    stages on together with them, 1 <= s < N, into the boxes lo / hi (M, N, u; None: -inf / +inf) of the stages they arrive at — the
    boxes do not move with the horizon: (act', U') (specification of csrc/dynamics.hip k_shift_active_set).  Entry (i, j, r) takes the
    control z and the status a of stage j + s (j >= N - s: of `U_tail` (M, s, u) with a = 0; None: of stage N - 1, hold); on a consensus
    stage j < Nc (Nc < 0: N) every particle takes particle 0's source and particle 0's box, as the solver does.  z is clamped into
    [l, h]; the status stays where the control is still on that bound, a control the clamp moved is held on the bound it was moved to,
    everything else is free.  An empty box (l > h) or a NaN control passes through with status 0: the solve's own check refuses it.
    U' is then bitwise the base point of act' — l where 1, h where 2, inside the box where 0 — and uniform over the particles on the
    consensus stages: what the first round of the solver's no-rollout warm start verifies of its start iterate."""
    act, U = np.asarray(act, np.int32), np.asarray(U, float)
    M, N, u = U.shape
    if not 1 <= int(s) < N:
        raise ValueError(f"shift_active_set: s = {s} is outside 1 .. N - 1 = {N - 1}")
    s = int(s)
    if act.shape != U.shape:
        raise ValueError(f"shift_active_set: act {act.shape} and U {U.shape} differ in shape")
    lo = np.full(U.shape, -np.inf) if lo is None else np.broadcast_to(np.asarray(lo, float), U.shape)
    hi = np.full(U.shape, np.inf) if hi is None else np.broadcast_to(np.asarray(hi, float), U.shape)
    Nc = N if Nc < 0 else min(int(Nc), N)
    if U_tail is None:
        z, a = np.concatenate([U[:, s:], np.repeat(U[:, N - 1:], s, 1)], 1), np.concatenate([act[:, s:], np.repeat(act[:, N - 1:], s, 1)], 1)
    else:
        z = np.concatenate([U[:, s:], np.asarray(U_tail, float).reshape(M, s, u)], 1)
        a = np.concatenate([act[:, s:], np.zeros((M, s, u), np.int32)], 1)
    l, h = lo.copy(), hi.copy()
    z[:, :Nc], a[:, :Nc], l[:, :Nc], h[:, :Nc] = z[:1, :Nc], a[:1, :Nc], lo[:1, :Nc], hi[:1, :Nc]
    with np.errstate(invalid="ignore"):
        zc = np.where(z < l, l, np.where(z > h, h, z))  # (not min / max: a signed zero comes out as the kernel's comparisons leave it)
        an = np.where((zc == l) & ((a == 1) | (z < l)), 1, np.where((zc == h) & ((a == 2) | (z > h)), 2, 0)).astype(np.int32)
        through = (l > h) | np.isnan(z)
    return np.where(through, 0, an).astype(np.int32), np.where(through, z, zc)


# -------------------------------------------------------------------------------------------------
# built-in obstacle cost (include/pmpc_abi.h pmpc_scp_cost; NOT in the reference, whose lin_cost_fn is a user callback)
# -------------------------------------------------------------------------------------------------
def _obstacle_arrays(cost, N, xp=np):
    """(pos_idx list, centres (1 | N, K, pos_dim), sigma (K,), w (K,)) of a cost dict(pos_idx=, centres=, sigma=, w=)."""
    if cost.get("kind", "obstacles") != "obstacles":
        raise ValueError(f"unknown built-in cost kind {cost.get('kind')!r}: 'obstacles' is the only one")
    pos_idx = [int(k) for k in cost["pos_idx"]]
    centres = xp.asarray(cost["centres"])
    sigma, w = xp.asarray(cost["sigma"]).reshape(-1), xp.asarray(cost["w"]).reshape(-1)
    K, pd = sigma.shape[0], len(pos_idx)
    if pd not in (2, 3) or len(set(pos_idx)) != pd or not 1 <= K <= 16:
        raise ValueError("obstacle cost: pos_idx holds 2 or 3 distinct state indices, and there are 1 to 16 obstacles")
    if tuple(centres.shape) not in ((K, pd), (N, K, pd)) or w.shape[0] != K:
        raise ValueError(f"obstacle cost: centres must be ({K}, {pd}) or ({N}, {K}, {pd}) and w ({K},), got {tuple(centres.shape)}, {tuple(w.shape)}")
    return pos_idx, centres.reshape((-1, K, pd)), sigma, w


def obstacle_cost(X, cost):
    """J = sum_{i,j,k} w_k exp(-|X[i, j, pos_idx] - c_jk|^2 / (2 sigma_k^2)) and its gradient cx (the shape of X, zero outside pos_idx).
    X (..., N, x): stage j is row j (the state after j + 1 steps, as X_prev of the SCP loop); cost = dict(pos_idx=(2 or 3 state
    indices), centres=(K, pos_dim) | (N, K, pos_dim) for moving obstacles, sigma=(K,), w=(K,)), K <= 16 obstacles shared by all particles."""
    X = np.asarray(X, float)
    pos_idx, cen, sigma, w = _obstacle_arrays(cost, X.shape[-2])
    d = X[..., None, pos_idx] - cen  # (..., N, K, pos_dim)
    is2 = 1.0 / (sigma * sigma)
    e = w * np.exp(-0.5 * np.sum(d * d, -1) * is2)  # (..., N, K)
    cx = np.zeros_like(X)
    cx[..., pos_idx] = np.sum((-e * is2)[..., None] * d, -2)
    return float(np.sum(e)), cx


def obstacle_cost_torch(X, cost):
    """`obstacle_cost` on torch tensors of any device (`cost` entries: tensors on X's device, or anything `torch.as_tensor` takes)."""
    import torch

    class _xp:  # the two array functions _obstacle_arrays needs
        asarray = staticmethod(lambda a: torch.as_tensor(a, dtype=X.dtype, device=X.device))

    pos_idx, cen, sigma, w = _obstacle_arrays(cost, X.shape[-2], _xp)
    d = X[..., None, pos_idx] - cen
    is2 = 1.0 / (sigma * sigma)
    e = w * torch.exp(-0.5 * torch.sum(d * d, -1) * is2)
    cx = torch.zeros_like(X)
    cx[..., pos_idx] = torch.sum((-e * is2)[..., None] * d, -2)
    return torch.sum(e), cx


def make_obstacle_lin_cost_fn(cost):
    """A `lin_cost_fn(X_prev, U_prev, problems) -> (cx, None)` of the obstacle cost for the SCP loops: numpy in, numpy out (the host
    loop), torch in, torch out (`device=...`)."""

    def lin_cost_fn(X_prev, U_prev, problems=None):
        if type(X_prev).__module__.split(".")[0] == "torch":
            return obstacle_cost_torch(X_prev, cost)[1], None
        return obstacle_cost(X_prev, cost)[1], None

    return lin_cost_fn


# -------------------------------------------------------------------------------------------------
# benchmark problem generators (BASELINE.md §2 / SURVEY.md §8d), seeded
# -------------------------------------------------------------------------------------------------
def make_unicycle_problem(M=256, N=30, seed=2020, Nc=1):
    """Config A (M=1: p=[1,1,0.3], x0=1) / config B (per-particle p and x0 jitter)."""
    rng = np.random.default_rng(seed)
    xdim, udim = 4, 2
    if M == 1:
        p = np.array([[1.0, 1.0, 0.3]])
        x0 = np.ones((1, xdim))
    else:
        p = np.stack([1 + 0.1 * rng.standard_normal(M), 1 + 0.1 * rng.standard_normal(M), np.full(M, 0.3)], -1)
        x0 = 1.0 + 0.05 * rng.standard_normal((M, xdim))
    Q = np.tile(np.eye(xdim), (M, N, 1, 1))
    R = np.tile(1e-2 * np.eye(udim), (M, N, 1, 1))
    prob = dict(
        x0=x0, Q=Q, R=R, X_ref=np.zeros((M, N, xdim)), U_ref=np.zeros((M, N, udim)),
        X_prev=np.zeros((M, N, xdim)), U_prev=np.zeros((M, N, udim)),
        u_l=-np.ones((M, N, udim)), u_u=np.ones((M, N, udim)), reg_x=1.0, reg_u=1.0,
        solver_settings=dict(solver="osqp", Nc=Nc),
    )
    pp = p[:, None, :]

    def f_fx_fu_fn(X, U):
        return unicycle(X, U, pp)

    prob["f_fx_fu_fn"] = f_fx_fu_fn
    prob["params"] = p
    return prob


def make_quadrotor_problem(M=1024, N=50, seed=2020, Nc=1):
    """Configs C/D: synthetic quadrotor, box constraints on the controls."""
    rng = np.random.default_rng(seed)
    xdim, udim = 12, 4
    mass = 1.0 * (1 + 0.1 * rng.standard_normal(M))
    J = np.array([0.01, 0.01, 0.02])[None, :] * (1 + 0.1 * rng.standard_normal((M, 1)))
    p = np.concatenate([mass[:, None], J], -1)
    x0 = np.zeros((M, xdim))
    x0[:, :3] = rng.uniform(-2, 2, (M, 3))
    Qd = np.concatenate([10 * np.ones(3), np.ones(3), np.ones(3), 0.1 * np.ones(3)])
    Q = np.tile(np.diag(Qd), (M, N, 1, 1))
    R = np.tile(0.1 * np.eye(udim), (M, N, 1, 1))
    U_ref = np.zeros((M, N, udim))
    U_ref[..., 0] = (mass * G_ACC)[:, None]
    u_l = np.zeros((M, N, udim))
    u_u = np.zeros((M, N, udim))
    u_l[..., 0], u_u[..., 0] = 0.0, (2 * mass * G_ACC)[:, None]
    u_l[..., 1:], u_u[..., 1:] = -0.5, 0.5
    X_prev = np.tile(x0[:, None, :], (1, N, 1))
    prob = dict(
        x0=x0, Q=Q, R=R, X_ref=np.zeros((M, N, xdim)), U_ref=U_ref, X_prev=X_prev, U_prev=U_ref.copy(),
        u_l=u_l, u_u=u_u, reg_x=1.0, reg_u=1e-1, solver_settings=dict(solver="osqp", Nc=Nc),
    )
    pp = p[:, None, :]

    def f_fx_fu_fn(X, U):
        return quadrotor(X, U, pp)

    prob["f_fx_fu_fn"] = f_fx_fu_fn
    prob["params"] = p
    return prob


BICYCLE_DT = 0.1


def make_bicycle_problem(M=256, N=30, seed=2020, Nc=1):
    """Lane change: every particle drives along +x at about 5 m/s and is asked to move over to a lane `w` to the left (its own
    w around 2 m) a third of the way into the horizon; |a| <= 2, |delta| <= 0.5, wheelbase L = 2.7 m +- 10 % per particle."""
    rng = np.random.default_rng(seed)
    xdim, udim, dt = 4, 2, BICYCLE_DT
    L = 2.7 * (1 + rng.uniform(-0.1, 0.1, M))
    p = np.stack([L, np.full(M, dt)], -1)
    v0 = 5.0 + 0.25 * rng.standard_normal(M)
    x0 = np.zeros((M, xdim))
    x0[:, 1] = 0.05 * rng.standard_normal(M)
    x0[:, 2] = 0.02 * rng.standard_normal(M)
    x0[:, 3] = v0
    w = 2.0 + 0.2 * rng.standard_normal(M)
    t = dt * np.arange(1, N + 1)
    X_ref = np.zeros((M, N, xdim))
    X_ref[..., 0] = x0[:, None, 0] + v0[:, None] * t[None, :]
    X_ref[..., 1] = np.where(np.arange(N)[None, :] >= N // 3, w[:, None], 0.0)
    X_ref[..., 3] = v0[:, None]
    Q = np.tile(np.diag([1.0, 10.0, 1.0, 1.0]), (M, N, 1, 1))
    R = np.tile(np.diag([0.1, 1.0]), (M, N, 1, 1))
    X_prev = np.tile(x0[:, None, :], (1, N, 1))
    X_prev[..., 0] = X_ref[..., 0]  # start iterate: straight on at the initial speed
    bound = np.array([2.0, 0.5])
    prob = dict(
        x0=x0, Q=Q, R=R, X_ref=X_ref, U_ref=np.zeros((M, N, udim)), X_prev=X_prev, U_prev=np.zeros((M, N, udim)),
        u_l=np.tile(-bound, (M, N, 1)), u_u=np.tile(bound, (M, N, 1)), reg_x=1.0, reg_u=1.0,
        solver_settings=dict(solver="osqp", Nc=Nc),
    )
    pp = p[:, None, :]

    def f_fx_fu_fn(X, U):
        return bicycle(X, U, pp)

    prob["f_fx_fu_fn"] = f_fx_fu_fn
    prob["params"] = p
    return prob
