"""The test costs of the runtime-compiled stage costs (pmpc_amd.CustomCost): device source, dimensions (x, u, cd), and numpy closed forms
(val (M, N), cx (M, N, x), cu (M, N, u)) for arrays X (M, N, x), U (M, N, u), P (M, cd); stage j of the closed forms is axis 1."""
import numpy as np

# Two Gaussian bumps in (x0, x1) plus 0.5 cw |u|^2.  p = [c0x, c0y, c1x, c1y, sigma0, sigma1, w0, w1, cw].  With cw = 0 (and uses_u=False)
# it is the built-in obstacle cost with K = 2, pos_idx (0, 1); OBS_DRIFT (a macro in front of the source, default 0) moves both
# centres by OBS_DRIFT * j along +x: the per-stage centres of tests/test_lin_cost_gpu.py::_moving.
OBSTACLES_U_SRC = """
#ifndef OBS_DRIFT
#define OBS_DRIFT 0.0
#endif
template <class T>
__device__ T stage_cost(const T *x, const T *u, const double *p, int j, int N) {
  T c = 0.5 * p[8] * (u[0] * u[0] + u[1] * u[1]);
  for (int k = 0; k < 2; k++) {
    const T dx = x[0] - (p[2 * k] + OBS_DRIFT * j), dy = x[1] - p[2 * k + 1];
    c += p[6 + k] * exp(-0.5 * (dx * dx + dy * dy) / (p[4 + k] * p[4 + k]));
  }
  return c;
}
"""
OBSTACLES_U_DIMS = (4, 2, 9)

# soft speed limit on x3 (a kink-free hinge) plus a control-effort term coupled to the state that grows with the stage.
# p = [w, k, vmax, wu]
SOFT_SPEED_SRC = """
template <class T>
__device__ T stage_cost(const T *x, const T *u, const double *p, int j, int N) {
  const double w = p[0], k = p[1], vmax = p[2], wu = p[3];
  return w * log(1.0 + exp(k * (x[3] - vmax))) / k + 0.5 * wu * u[0] * u[0] * (1.0 + x[3] * x[3]) * (double)(j + 1) / (double)N;
}
"""
SOFT_SPEED_DIMS = (4, 2, 4)

# sum_k sin(a_k x_k) (1 + sum_m b_m u_m^2) for any dimensions; p = [a (XD) | b (UD)], CD = XD + UD
GENERIC_SRC = """
template <class T>
__device__ T stage_cost(const T *x, const T *u, const double *p, int j, int N) {
  T s = 0.0, q = 1.0;
#pragma unroll
  for (int k = 0; k < XD; k++) s += sin(p[k] * x[k]);
#pragma unroll
  for (int m = 0; m < UD; m++) q += p[XD + m] * u[m] * u[m];
  return s * q;
}
"""


def obstacles_u_np(X, U, P, drift=0.0):
    j = np.arange(X.shape[1])[None, :]
    val = 0.5 * P[:, None, 8] * (U ** 2).sum(-1)
    cx = np.zeros_like(X)
    for k in range(2):
        dx, dy = X[..., 0] - (P[:, None, 2 * k] + drift * j), X[..., 1] - P[:, None, 2 * k + 1]
        s2 = P[:, None, 4 + k] ** 2
        e = P[:, None, 6 + k] * np.exp(-0.5 * (dx * dx + dy * dy) / s2)
        val = val + e
        cx[..., 0] -= e * dx / s2
        cx[..., 1] -= e * dy / s2
    return val, cx, P[:, None, 8:9] * U


def soft_speed_np(X, U, P):
    w, k, vmax, wu = (P[:, None, i] for i in range(4))
    N = X.shape[1]
    g = (np.arange(N)[None, :] + 1.0) / N
    v, u0 = X[..., 3], U[..., 0]
    z = k * (v - vmax)
    val = w * np.logaddexp(0.0, z) / k + 0.5 * wu * u0 * u0 * (1.0 + v * v) * g
    cx, cu = np.zeros_like(X), np.zeros_like(U)
    cx[..., 3] = w / (1.0 + np.exp(-z)) + wu * u0 * u0 * v * g
    cu[..., 0] = wu * u0 * (1.0 + v * v) * g
    return val, cx, cu


def generic_np(X, U, P):
    x = X.shape[-1]
    a, b = P[:, None, :x], P[:, None, x:]
    s, q = np.sin(a * X).sum(-1), 1.0 + (b * U * U).sum(-1)
    return s * q, a * np.cos(a * X) * q[..., None], s[..., None] * 2.0 * b * U


COSTS = {
    "obstacles_u": dict(src=OBSTACLES_U_SRC, dims=OBSTACLES_U_DIMS, np=obstacles_u_np),
    "soft_speed": dict(src=SOFT_SPEED_SRC, dims=SOFT_SPEED_DIMS, np=soft_speed_np),
}
GENERIC_DIMS = [(1, 1), (3, 5), (12, 4), (16, 16)]  # a part-filled single pass, odd sizes, 4 passes, 8 passes on 32 directions


def generic(x, u):
    return dict(src=GENERIC_SRC, dims=(x, u, x + u), np=generic_np)


def entry(name):
    """"obstacles_u", "soft_speed" or "generic_<x>_<u>" -> dict(src, dims, np)."""
    if name.startswith("generic_"):
        _, x, u = name.split("_")
        return generic(int(x), int(u))
    return COSTS[name]


def make(name, uses_u=True, drift=None):
    import pmpc_amd

    e = entry(name)
    src = e["src"] if drift is None else f"#define OBS_DRIFT {float(drift)!r}\n" + e["src"]
    return pmpc_amd.CustomCost(src, *e["dims"], uses_u=uses_u, name=name)


def obstacle_params(cost, M, cw=0.0):
    """P (M, 9) of obstacles_u for a built-in obstacle dict with K = 2 static centres (K, 2) in two position entries."""
    c, s, w = np.asarray(cost["centres"], float), np.asarray(cost["sigma"], float), np.asarray(cost["w"], float)
    assert c.shape == (2, 2) and s.shape == (2,) and w.shape == (2,)
    return np.tile(np.concatenate([c.reshape(-1), s, w, [cw]])[None], (M, 1))


def rand_inputs(name, M, N, seed=0):
    """X (M, N, x), U (M, N, u), P (M, cd): moderate sizes, parameters per particle."""
    x, u, cd = entry(name)["dims"]
    rng = np.random.default_rng(seed)
    X, U = rng.uniform(-1.5, 1.5, (M, N, x)), rng.uniform(-0.8, 0.8, (M, N, u))
    if name == "obstacles_u":
        P = np.concatenate([rng.uniform(-1, 1, (M, 4)), rng.uniform(0.5, 2.0, (M, 2)), rng.uniform(0.5, 3.0, (M, 2)), rng.uniform(0.01, 0.1, (M, 1))], -1)
    elif name == "soft_speed":
        P = np.stack([rng.uniform(0.5, 2.0, M), rng.uniform(2.0, 6.0, M), rng.uniform(-0.5, 0.5, M), rng.uniform(0.1, 1.0, M)], -1)
    else:
        P = rng.uniform(0.3, 1.7, (M, cd))
    return X, U, P
