"""The test models of the runtime-compiled dynamics (pmpc_amd.CustomModel): device source, and numpy closed forms of F and its
Jacobians in the py layout (fx (.., row, col) = dF_row / dx_col), for arrays X_ (M, N, x), U (M, N, u), P (M, p)."""
import numpy as np

# the expressions of Bicycle::step (pmpc_amd/csrc/dynamics.hip), in the same order
BICYCLE_SRC = """
template <class T>
__device__ void step(const T *x, const T *u, const double *p, T *xn) {
  const double Lw = p[0], dt = p[1];
  const T s = sin(x[2]), c = cos(x[2]);
  const T td = tan(u[1]), dtv = dt * x[3];
  xn[0] = x[0] + dtv * c;
  xn[1] = x[1] + dtv * s;
  xn[2] = x[2] + dtv * td / Lw;
  xn[3] = x[3] + dt * u[0];
}
"""
BICYCLE_DIMS = (4, 2, 2)

# damped pendulum, forward Euler: x = [angle, rate], u = [torque], p = [g / l, damping, dt]
PENDULUM_SRC = """
template <class T>
__device__ void step(const T *x, const T *u, const double *p, T *xn) {
  const double gl = p[0], damp = p[1], dt = p[2];
  xn[0] = x[0] + dt * x[1];
  xn[1] = x[1] + dt * (u[0] - gl * sin(x[0]) - damp * x[1]);
}
"""
PENDULUM_DIMS = (2, 1, 3)

# ring: xn[k] = x[k] + dt (x[k] sin(x[(k + 1) % 9]) + p0 u[k % 3] cos(x[k])), p = [p0, dt]; 9 + 3 directions: more than one AD chunk
RING_SRC = """
template <class T>
__device__ void step(const T *x, const T *u, const double *p, T *xn) {
  const double p0 = p[0], dt = p[1];
#pragma unroll
  for (int k = 0; k < XD; k++) xn[k] = x[k] + dt * (x[k] * sin(x[(k + 1) % XD]) + p0 * u[k % UD] * cos(x[k]));
}
"""
RING_DIMS = (9, 3, 2)

SOURCES = {"bicycle": (BICYCLE_SRC, BICYCLE_DIMS), "pendulum": (PENDULUM_SRC, PENDULUM_DIMS), "ring": (RING_SRC, RING_DIMS)}


def make(name):
    import pmpc_amd

    src, (x, u, p) = SOURCES[name]
    return pmpc_amd.CustomModel(src, x, u, p, name=name)


def bicycle_np(X, U, P):
    Lw, dt = P[:, None, 0], P[:, None, 1]
    th, v, acc, de = X[..., 2], X[..., 3], U[..., 0], U[..., 1]
    s, c, td = np.sin(th), np.cos(th), np.tan(U[..., 1])
    f = np.stack([X[..., 0] + dt * v * c, X[..., 1] + dt * v * s, th + dt * v * td / Lw, v + dt * acc], -1)
    fx = np.zeros(X.shape + (4,))
    fx[..., np.arange(4), np.arange(4)] = 1.0
    fx[..., 0, 2], fx[..., 0, 3] = -dt * v * s, dt * c
    fx[..., 1, 2], fx[..., 1, 3] = dt * v * c, dt * s
    fx[..., 2, 3] = dt * td / Lw
    fu = np.zeros(X.shape + (2,))
    fu[..., 3, 0] = dt
    fu[..., 2, 1] = dt * v * (1.0 + td * td) / Lw
    return f, fx, fu


def pendulum_np(X, U, P):
    gl, damp, dt = P[:, None, 0], P[:, None, 1], P[:, None, 2]
    th, w = X[..., 0], X[..., 1]
    f = np.stack([th + dt * w, w + dt * (U[..., 0] - gl * np.sin(th) - damp * w)], -1)
    fx = np.zeros(X.shape + (2,))
    fx[..., 0, 0], fx[..., 0, 1] = 1.0, dt
    fx[..., 1, 0], fx[..., 1, 1] = -dt * gl * np.cos(th), 1.0 - dt * damp
    fu = np.zeros(X.shape + (1,))
    fu[..., 1, 0] = dt
    return f, fx, fu


def ring_np(X, U, P):
    p0, dt = P[:, None, None, 0], P[:, None, None, 1]
    k = np.arange(9)
    xk, xn, uk = X, X[..., (k + 1) % 9], U[..., k % 3]
    f = xk + dt * (xk * np.sin(xn) + p0 * uk * np.cos(xk))
    fx = np.zeros(X.shape + (9,))
    fx[..., k, k] = 1.0 + dt * (np.sin(xn) - p0 * uk * np.sin(xk))
    fx[..., k, (k + 1) % 9] = dt * xk * np.cos(xn)
    fu = np.zeros(X.shape + (3,))
    fu[..., k, k % 3] = dt * p0 * np.cos(xk)
    return f, fx, fu


CLOSED_FORMS = {"bicycle": bicycle_np, "pendulum": pendulum_np, "ring": ring_np}


def rand_inputs(name, M, N, seed=0):
    """x0 (M, x), X_prev (M, N, x), U_prev (M, N, u), params (M, p) of moderate size (tan and the ring's sines stay well-conditioned)."""
    x, u, p = SOURCES[name][1]
    rng = np.random.default_rng(seed)
    x0, Xp, Up = rng.uniform(-1, 1, (M, x)), rng.uniform(-1, 1, (M, N, x)), rng.uniform(-0.5, 0.5, (M, N, u))
    if name == "bicycle":
        P = np.stack([rng.uniform(2.0, 3.0, M), rng.uniform(0.05, 0.15, M)], -1)
    elif name == "pendulum":
        P = np.stack([rng.uniform(5.0, 15.0, M), rng.uniform(0.0, 0.5, M), rng.uniform(0.02, 0.1, M)], -1)
    else:
        P = np.stack([rng.uniform(0.5, 1.5, M), rng.uniform(0.05, 0.15, M)], -1)
    return x0, Xp, Up, P
