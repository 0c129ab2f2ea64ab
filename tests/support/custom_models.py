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


# ---- the model family of the dimension tests: one body for any XD, UD, PD >= 1 that uses everything model_dual.h offers ----------------
# dt = p[0]; row k of xn is chosen by k % 8; row 7 is a constant (every derivative is zero and must still be written)
FAMILY_SRC = """
template <class T>
__device__ void step(const T *x, const T *u, const double *p, T *xn) {
  const double dt = p[0];
#pragma unroll
  for (int k = 0; k < XD; k++) {
    const T a = x[k], b = x[(k + 1) % XD], c = u[k % UD], d = u[(k + 3) % UD];
    switch (k % 8) {
      case 0: xn[k] = a + dt * (sin(b) * cos(c) + tan(0.3 * d)); break;
      case 1: xn[k] = a + dt * (exp(-b * b) + log(2.0 + c * c)); break;
      case 2: xn[k] = a + dt * (sqrt(1.5 + b * c) + tanh(d)); break;
      case 3: xn[k] = a + dt * (atan(b) + atan2(c, 2.0 + d * d) + atan2(b, 1.5) + atan2(0.7, 2.0 + c)); break;
      case 4: xn[k] = a + dt * (pow(2.0 + b, 1.5) / (3.0 + c * c) + 1.0 / (2.0 + d * d)); break;
      case 5: xn[k] = a + dt * (fabs(b) + fmin(c, d) + fmax(b, 0.1) + fmin(0.2, c)); break;
      case 6: {
        T r = a;
        r += dt * b;
        r *= (1.0 + 0.1 * c);
        r -= d;
        r /= (2.0 + c * c);
        xn[k] = r;
      } break;
      default: xn[k] = p[PD - 1];
    }
  }
}
"""

# (x, u, p) by what the case reaches in pmpc_jit_linearize: U units per block, 256 / U threads per unit, NPASS = ceil((x + u) / 4)
FAMILY_CASES = {
    "smallest_half_empty_chunk": (1, 1, 1),      # U 64, NPASS 1; REC odd
    "one_full_chunk": (3, 1, 1),                 # U 64, NPASS 1
    "second_trip_of_the_pass_loop": (5, 12, 1),  # U 64, NPASS 5: a thread does passes 0 and 4; the last chunk holds one direction
    "second_trip_one_state": (1, 16, 2),         # U 64, NPASS 5, XD 1
    "units_32_four_full_chunks": (9, 7, 4),      # U 32, NPASS 4
    "units_32_even_record": (12, 8, 2),          # U 32, NPASS 5; REC 252 even, LD 253; 64,768 B of LDS
    "units_16": (16, 1, 3),                      # U 16, NPASS 5
    "every_limit": (16, 16, 16),                 # U 8, NPASS 8, 32 threads per unit
    # in the two second-trip cases above the body does not use the last control, so the one direction of pass 4 has a zero derivative;
    # here row 6 subtracts u[9], the direction of pass 4, and the records just fit 64 units (LD 127: 65,024 B of 65,536)
    "second_trip_last_direction_live": (7, 10, 2),  # U 64, NPASS 5
}
FAMILY_UNITS = {"smallest_half_empty_chunk": 64, "one_full_chunk": 64, "second_trip_of_the_pass_loop": 64, "second_trip_one_state": 64,
                "units_32_four_full_chunks": 32, "units_32_even_record": 32, "units_16": 16, "every_limit": 8, "second_trip_last_direction_live": 64}
KINK_MARGIN = 1e-3


def make_family(case):
    import pmpc_amd

    x, u, p = FAMILY_CASES[case]
    return pmpc_amd.CustomModel(FAMILY_SRC, x, u, p, name=f"family_{x}_{u}_{p}")


def lin_units(x, u):
    """Units (particle, stage) per block of pmpc_jit_linearize: the largest power of two <= 64 whose records [f | fx | fu] of doubles,
    at the odd stride LD, fit 64 KB of LDS (lin_units of pmpc_amd/csrc/model_jit.hip, restated)."""
    ld = (x + x * x + x * u) | 1
    n = 64
    while n > 1 and n * ld * 8 > 65536:
        n //= 2
    return n


def _family_rows(X, U, P):
    """The rows of FAMILY_SRC in float64 torch: X (B, x), U (B, u), P (B, p) -> (B, x).  Shares no code with model_dual.h."""
    import torch

    xd, ud = X.shape[-1], U.shape[-1]
    dt = P[:, 0]
    rows = []
    for k in range(xd):
        a, b, c, d = X[:, k], X[:, (k + 1) % xd], U[:, k % ud], U[:, (k + 3) % ud]
        t = k % 8
        if t == 0:
            r = a + dt * (torch.sin(b) * torch.cos(c) + torch.tan(0.3 * d))
        elif t == 1:
            r = a + dt * (torch.exp(-b * b) + torch.log(2.0 + c * c))
        elif t == 2:
            r = a + dt * (torch.sqrt(1.5 + b * c) + torch.tanh(d))
        elif t == 3:
            r = a + dt * (torch.atan(b) + torch.atan2(c, 2.0 + d * d) + torch.atan2(b, torch.full_like(b, 1.5))
                          + torch.atan2(torch.full_like(c, 0.7), 2.0 + c))
        elif t == 4:
            r = a + dt * (torch.pow(2.0 + b, 1.5) / (3.0 + c * c) + 1.0 / (2.0 + d * d))
        elif t == 5:
            r = a + dt * (torch.abs(b) + torch.minimum(c, d) + torch.clamp(b, min=0.1) + torch.clamp(c, max=0.2))
        elif t == 6:
            r = ((a + dt * b) * (1.0 + 0.1 * c) - d) / (2.0 + c * c)
        else:
            r = P[:, -1] + 0.0 * a  # (a constant row that still hangs on the graph: its derivatives come out as zeros)
        rows.append(r)
    return torch.stack(rows, -1)


def family_f(X_, U, P):
    """F alone in float64: X_ (M, N, x), U (M, N, u), P (M, p) numpy -> (M, N, x) numpy."""
    import torch

    M, N, x = X_.shape
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))  # (a copy: the caller's array may be read-only)
    with torch.no_grad():
        f = _family_rows(t(X_).reshape(M * N, x), t(U).reshape(M * N, -1), t(np.repeat(P, N, 0)))
    return f.reshape(M, N, x).numpy()


def family_ref(X_, U, P):
    """f (M, N, x), fx (M, N, x, x), fu (M, N, x, u) of the family in the py layout (fx (.., row, col) = dF_row / dx_col): float64 torch on
    the CPU, the Jacobians by torch.autograd (one backward pass per row; the units are independent, so the gradient of a row summed
    over the units is that row's gradient of every unit)."""
    import torch

    M, N, x = X_.shape
    u = U.shape[-1]
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))  # (a copy: the caller's array may be read-only)
    Xt, Ut = t(X_).reshape(M * N, x).requires_grad_(True), t(U).reshape(M * N, u).requires_grad_(True)
    f = _family_rows(Xt, Ut, t(np.repeat(P, N, 0)))
    fx, fu = torch.zeros(M * N, x, x, dtype=torch.float64), torch.zeros(M * N, x, u, dtype=torch.float64)
    for r in range(x):
        gx, gu = torch.autograd.grad(f[:, r].sum(), (Xt, Ut), retain_graph=True, allow_unused=True)
        if gx is not None:
            fx[:, r] = gx
        if gu is not None:
            fu[:, r] = gu
    return f.detach().reshape(M, N, x).numpy(), fx.reshape(M, N, x, x).numpy(), fu.reshape(M, N, x, u).numpy()


def family_rollout(x0, U, P):
    """X (M, N, x): X[:, j] = F(X[:, j - 1], U[:, j]), X[:, -1] = x0, by family_f."""
    X, xs = [], x0
    for j in range(U.shape[1]):
        xs = family_f(xs[:, None], U[:, j:j + 1], P)[:, 0]
        X.append(xs)
    return np.stack(X, 1)


def family_kink_margin(X_, U):
    """The smallest distance of the inputs X_ (.., x), U (.., u) from a kink of row type 5, taken over every k (not only k % 8 == 5):
    |b|, |b - 0.1|, |c - 0.2|, and |c - d| where c and d are different entries of u (the same entry: the tie is harmless)."""
    xd, ud = X_.shape[-1], U.shape[-1]
    m = min(np.abs(X_).min(), np.abs(X_ - 0.1).min())
    for k in range(xd):
        c, d = k % ud, (k + 3) % ud
        m = min(m, np.abs(U[..., c] - 0.2).min())
        if c != d:
            m = min(m, np.abs(U[..., c] - U[..., d]).min())
    return float(m)


def family_inputs(dims, M, N, seed=0):
    """x0 (M, x), X_prev (M, N, x), U_prev (M, N, u), params (M, p): |x| <= 1, |u| <= 0.5, p[0] = dt in [0.05, 0.15], the other
    parameters in [0.5, 1.5]; entries closer than KINK_MARGIN to a kink (family_kink_margin) are drawn again."""
    x, u, p = dims
    rng = np.random.default_rng(seed)
    Xa, Up = rng.uniform(-1, 1, (M, N + 1, x)), rng.uniform(-0.5, 0.5, (M, N, u))
    P = np.concatenate([rng.uniform(0.05, 0.15, (M, 1)), rng.uniform(0.5, 1.5, (M, p - 1))], -1)
    for _ in range(100):
        bad_x = (np.abs(Xa) < KINK_MARGIN) | (np.abs(Xa - 0.1) < KINK_MARGIN)
        bad_u = np.abs(Up - 0.2) < KINK_MARGIN
        for k in range(x):
            c, d = k % u, (k + 3) % u
            if c != d:
                bad_u[..., c] |= np.abs(Up[..., c] - Up[..., d]) < KINK_MARGIN
        if not bad_x.any() and not bad_u.any():
            break
        Xa[bad_x] = rng.uniform(-1, 1, int(bad_x.sum()))
        Up[bad_u] = rng.uniform(-0.5, 0.5, int(bad_u.sum()))
    return np.ascontiguousarray(Xa[:, 0]), np.ascontiguousarray(Xa[:, 1:]), Up, P


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
