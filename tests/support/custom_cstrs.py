"""The test constraints of the runtime-compiled state constraints (pmpc_amd.CustomConstraint): device source, dimensions (x, K, pd), and
numpy closed forms (g (M, N, K), a = dg/dx (M, N, K, x)) for arrays X (M, N, x), P (M, pd); stage j of the closed forms is axis 1."""
import numpy as np

# K balls in the first BALL_PD states (a macro in front of the source, default 2): g_k = r_k - |x[:pd] - c_k|.
# p = [c_0 (pd) | .. | c_{K-1} (pd) | r_0 .. r_{K-1}].  Its rows about an iterate away from the centres are the keep-out constraint's.
BALLS_SRC = """
#ifndef BALL_PD
#define BALL_PD 2
#endif
template <class T>
__device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g) {
  for (int k = 0; k < KD; k++) {
    T s = 0.0;
    for (int q = 0; q < BALL_PD; q++) {
      const T d = x[q] - p[k * BALL_PD + q];
      s += d * d;
    }
    g[k] = p[KD * BALL_PD + k] - sqrt(s);
  }
}
"""

# the example of the documentation: a speed band on x3 whose upper end tightens along the horizon.  p = [vmax, tighten, vmin]
SPEED_BAND_SRC = """
template <class T> __device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g) {   // x[XD], p[PD] -> g[KD]
  g[0] = x[3] - (p[0] - p[1] * j / N);          // v <= vmax, tightening along the horizon
  g[1] = p[2] - x[3];                           // v >= vmin
}
"""
SPEED_BAND_DIMS = (4, 2, 3)

# g_k = sum_c sin(p_c x_c + 0.3 k) / (1 + c) + p_{XD + k} exp(0.2 x_{k % XD}) x_{(k + 1) % XD} - (1 + j / N), any dimensions; PD = XD + KD
GENERIC_SRC = """
template <class T>
__device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g) {
#pragma unroll
  for (int k = 0; k < KD; k++) {
    T s = p[XD + k] * exp(0.2 * x[k % XD]) * x[(k + 1) % XD] - (1.0 + (double)j / (double)N);
#pragma unroll
    for (int c = 0; c < XD; c++) s += sin(p[c] * x[c] + 0.3 * k) / (1.0 + c);
    g[k] = s;
  }
}
"""

# undefined for x0 <= 0: the rows kernel must drop such a row and count it.  p = [bound]
LOG_SRC = """
template <class T> __device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g) { g[0] = p[0] - log(x[0]); }
"""
LOG_DIMS = (4, 1, 1)


def balls_np(X, P, K=2, pd=2):
    M, N, x = X.shape
    cen, rad = P[:, :K * pd].reshape(M, 1, K, pd), P[:, None, K * pd:]
    d = X[:, :, None, :pd] - cen
    nrm = np.sqrt((d * d).sum(-1))
    a = np.zeros((M, N, K, x))
    a[..., :pd] = -d / nrm[..., None]
    return rad - nrm, a


def speed_band_np(X, P):
    M, N, x = X.shape
    j = np.arange(N)[None, :]
    v = X[..., 3]
    g = np.stack([v - (P[:, None, 0] - P[:, None, 1] * j / N), P[:, None, 2] - v], -1)
    a = np.zeros((M, N, 2, x))
    a[..., 0, 3], a[..., 1, 3] = 1.0, -1.0
    return g, a


def generic_np(X, P, K):
    M, N, x = X.shape
    j = np.arange(N)[None, :]
    g, a = np.zeros((M, N, K)), np.zeros((M, N, K, x))
    c = np.arange(x)
    for k in range(K):
        i1, i2 = k % x, (k + 1) % x
        ph = P[:, None, :x] * X + 0.3 * k
        w = P[:, None, x + k]
        e = np.exp(0.2 * X[..., i1])
        g[..., k] = (np.sin(ph) / (1.0 + c)).sum(-1) + w * e * X[..., i2] - (1.0 + j / N)
        a[..., k, :] = P[:, None, :x] * np.cos(ph) / (1.0 + c)
        a[..., k, i1] += w * 0.2 * e * X[..., i2]
        a[..., k, i2] += w * e
    return g, a


def log_np(X, P):
    M, N, x = X.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (P[:, None, 0] - np.log(X[..., 0]))[..., None]
    a = np.zeros((M, N, 1, x))
    a[..., 0, 0] = -1.0 / X[..., 0]
    return g, a


GENERIC_DIMS = [(15, 1), (12, 4), (1, 4), (3, 3)]  # a partial last pass, the largest record, one pass with three dead directions, odd sizes
NAMES = ["balls", "speed_band"] + [f"generic_{x}_{K}" for x, K in GENERIC_DIMS]


def entry(name):
    """"balls" (x 4, K 2, in the plane), "balls_<x>_<K>_<pd>", "speed_band", "log" or "generic_<x>_<K>" -> dict(src, dims (x, K, pd), np)."""
    if name.startswith("generic_"):
        x, K = (int(v) for v in name.split("_")[1:])
        return dict(src=GENERIC_SRC, dims=(x, K, x + K), np=lambda X, P: generic_np(X, P, K))
    if name.startswith("balls"):
        x, K, pd = (int(v) for v in name.split("_")[1:]) if "_" in name else (4, 2, 2)
        return dict(src=f"#define BALL_PD {pd}\n" + BALLS_SRC, dims=(x, K, K * pd + K), np=lambda X, P: balls_np(X, P, K, pd))
    return {"speed_band": dict(src=SPEED_BAND_SRC, dims=SPEED_BAND_DIMS, np=speed_band_np), "log": dict(src=LOG_SRC, dims=LOG_DIMS, np=log_np)}[name]


_made = {}


def make(name):
    """The CustomConstraint of a test constraint, one object (and so one compile per architecture) per name and process."""
    import pmpc_amd

    if name not in _made:
        e = entry(name)
        _made[name] = pmpc_amd.CustomConstraint(e["src"], *e["dims"], name=name)
    return _made[name]


def rows_np(name, X, P):
    """(a (M, N, K, x), h (M, N, K), g (M, N, K)) of the closed forms: the rows about X."""
    g, a = entry(name)["np"](X, P)
    return a, np.einsum("mnkx,mnx->mnk", a, X) - g, g


def ball_params(cstr, M):
    """P (M, K pd + K) of `balls` for a keep-out dict with static centres (K, pd) or per-particle centres (M, N, K, pd) that are the same at
    every stage; the position sub-space must be the first pd states."""
    cen, rad = np.asarray(cstr["centres"], float), np.asarray(cstr["radius"], float).reshape(-1)
    K, pd = rad.shape[0], len(cstr["pos_idx"])
    assert tuple(cstr["pos_idx"]) == tuple(range(pd))
    if cen.ndim == 2:
        cen = np.broadcast_to(cen[None], (M, K, pd))
    else:
        assert cen.shape[0] == M and np.all(cen == cen[:, :1])
        cen = cen[:, 0]
    return np.concatenate([cen.reshape(M, K * pd), np.broadcast_to(rad[None], (M, K))], -1)


def rand_inputs(name, M, N, seed=0):
    """X (M, N, x), P (M, pd): moderate sizes, parameters per particle; the balls' centres stay clear of the states."""
    x, K, pd = entry(name)["dims"]
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.5, 1.5, (M, N, x))
    if name.startswith("balls"):
        bpd = (pd - K) // K
        P = np.concatenate([rng.uniform(2.0, 3.0, (M, K * bpd)), rng.uniform(0.2, 0.8, (M, K))], -1)
    elif name == "speed_band":
        P = np.stack([rng.uniform(1.0, 2.0, M), rng.uniform(0.1, 0.5, M), rng.uniform(-1.0, 0.0, M)], -1)
    else:
        P = rng.uniform(0.3, 1.7, (M, pd))
    return X, P
