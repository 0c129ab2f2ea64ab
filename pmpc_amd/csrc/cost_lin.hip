// cost_lin.hip — linearised nonlinear costs of the SCP loop (the reference's lin_cost_fn, pmpc/scp_mpc.py:171-185, 352): the loop
// tracks X_ref - Q^-1 cx (U_ref - R^-1 cu) for one iteration, cx the cost gradient at the previous iterate.
//
//   k_ref_shift       out[r] = ref[r] - A[r]^-1 c[r] for `rows` independent SPD blocks (Cholesky, two triangular solves, fp64)
//   k_obstacle_grad   dense gradient of the built-in obstacle cost (include/pmpc_abi.h, pmpc_scp_cost); numpy specification:
//                     pmpc_amd/dynamics.py obstacle_cost
//   k_ref_shift<.., OBS = true>   the two in one launch: the gradient goes from registers into the solve, cx never exists
//
// A workgroup takes UNITS consecutive blocks.  They are consecutive in A, c, ref and out, so every load and store instruction of the
// workgroup touches consecutive doubles: all threads stream [lower triangle of A | c] into an LDS record per block (odd record stride:
// the per-block accesses below are conflict-free), the first UNITS threads factor and solve their record (in registers for the compiled
// dimensions), all threads stream ref - solution out.  Q at 4096 particles x 50 stages x 12 states is 236 MB per pass: the dim 12 body
// streams it at 2.4 - 2.6 TB/s on an MI355X (CHANGELOG.md); the other bodies were not timed.
#include "cost_lin.h"
#include <cstring>

namespace {

struct ObsArgs {  // OBS: c is the obstacle-cost gradient at X (rows, x) instead of an array
  pmpc_scp_cost cost;
  const double *X;
  int N;
};

// gradient of  sum_k w_k exp(-|x[pos_idx] - c_jk|^2 / (2 sigma_k^2))  in the pos_idx entries of one state x = xrow, stage j.
// Every sum is an explicit fma chain: the stand-alone and the fused kernel give the same bits.
__device__ __forceinline__ void obstacle_grad(const pmpc_scp_cost &o, const double *xrow, int j, double g[3]) {
  const int pd = o.pos_dim;
  const double *cen = o.centres + (o.per_stage ? (size_t)j * o.K * pd : 0);
  double p[3] = {0.0, 0.0, 0.0};
  for (int d = 0; d < pd; d++) p[d] = xrow[o.pos_idx[d]];
  g[0] = g[1] = g[2] = 0.0;
  for (int k = 0; k < o.K; k++) {
    double dd[3] = {0.0, 0.0, 0.0}, r2 = 0.0;
    for (int d = 0; d < pd; d++) {
      dd[d] = p[d] - cen[k * pd + d];
      r2 = fma(dd[d], dd[d], r2);
    }
    const double is2 = 1.0 / (o.sigma[k] * o.sigma[k]);
    const double coef = -(o.w[k] * exp(-0.5 * r2 * is2)) * is2;
    for (int d = 0; d < pd; d++) g[d] = fma(coef, dd[d], g[d]);
  }
}

// lower triangle (row r >= column c) of a d x d block, column after column
__device__ __forceinline__ int tri(int r, int c, int d) { return c * d - (c * (c - 1)) / 2 + (r - c); }

// one record [lower triangle of A, d (d + 1) / 2 | v (d)] in LDS: v <- A^-1 v.  False (and v = NaN) if a pivot is not positive.
// Compiled dimension: the record is read into registers once and every index is a compile-time constant (no chain of LDS latencies).
template <int DIM>
__device__ __forceinline__ bool chol_solve_record(double *a) {
  constexpr int d = DIM, T = DIM * (DIM + 1) / 2;
  double L[T], v[DIM];
#pragma unroll
  for (int k = 0; k < T; k++) L[k] = a[k];
#pragma unroll
  for (int k = 0; k < d; k++) v[k] = a[T + k];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < d; j++) {
    double s = L[tri(j, j, d)];
#pragma unroll
    for (int k = 0; k < j; k++) s = fma(-L[tri(j, k, d)], L[tri(j, k, d)], s);
    ok = ok && (s > 0.0);  // (false for a NaN as well)
    const double inv = 1.0 / sqrt(s);
    L[tri(j, j, d)] = inv;  // the diagonal keeps 1 / l_jj
#pragma unroll
    for (int i = j + 1; i < d; i++) {
      double t = L[tri(i, j, d)];
#pragma unroll
      for (int k = 0; k < j; k++) t = fma(-L[tri(i, k, d)], L[tri(j, k, d)], t);
      L[tri(i, j, d)] = t * inv;
    }
  }
#pragma unroll
  for (int i = 0; i < d; i++) {  // L y = c
    double t = v[i];
#pragma unroll
    for (int k = 0; k < i; k++) t = fma(-L[tri(i, k, d)], v[k], t);
    v[i] = t * L[tri(i, i, d)];
  }
#pragma unroll
  for (int i = d - 1; i >= 0; i--) {  // L' x = y
    double t = v[i];
#pragma unroll
    for (int k = i + 1; k < d; k++) t = fma(-L[tri(k, i, d)], v[k], t);
    v[i] = t * L[tri(i, i, d)];
  }
#pragma unroll
  for (int i = 0; i < d; i++) a[T + i] = ok ? v[i] : __longlong_as_double(0x7ff8000000000000LL);
  return ok;
}
// the same for a runtime dimension, in place in LDS
__device__ __forceinline__ bool chol_solve_record_any(double *a, int d) {
  const int T = d * (d + 1) / 2;
  double *L = a, *v = a + T;
  bool ok = true;
  for (int j = 0; j < d; j++) {
    double s = L[tri(j, j, d)];
    for (int k = 0; k < j; k++) s = fma(-L[tri(j, k, d)], L[tri(j, k, d)], s);
    ok = ok && (s > 0.0);  // (false for a NaN as well)
    const double inv = 1.0 / sqrt(s);
    L[tri(j, j, d)] = inv;  // the diagonal keeps 1 / l_jj
    for (int i = j + 1; i < d; i++) {
      double t = L[tri(i, j, d)];
      for (int k = 0; k < j; k++) t = fma(-L[tri(i, k, d)], L[tri(j, k, d)], t);
      L[tri(i, j, d)] = t * inv;
    }
  }
  for (int i = 0; i < d; i++) {  // L y = c
    double t = v[i];
    for (int k = 0; k < i; k++) t = fma(-L[tri(i, k, d)], v[k], t);
    v[i] = t * L[tri(i, i, d)];
  }
  for (int i = d - 1; i >= 0; i--) {  // L' x = y
    double t = v[i];
    for (int k = i + 1; k < d; k++) t = fma(-L[tri(k, i, d)], v[k], t);
    v[i] = t * L[tri(i, i, d)];
  }
  if (!ok)
    for (int i = 0; i < d; i++) v[i] = __longlong_as_double(0x7ff8000000000000LL);
  return ok;
}

// DIM > 0: compiled dimension; 0: d_rt (<= REF_SHIFT_MAX_DIM).  Dynamic LDS: UNITS records of LD = (d (d + 1) / 2 + d) | 1 doubles.
template <int DIM, int UNITS, int THREADS, bool OBS>
__global__ void __launch_bounds__(THREADS) k_ref_shift(int d_rt, long long rows, const double *A, const double *c, const double *ref, double *out,
                                                       unsigned *bad, ObsArgs o) {
  const int d = DIM > 0 ? DIM : d_rt, dd = d * d, T = d * (d + 1) / 2, LD = (T + d) | 1;
  extern __shared__ double rec[];
  const int t = threadIdx.x;
  const long long first = (long long)blockIdx.x * UNITS;
  const int n = (int)((rows - first) < UNITS ? (rows - first) : UNITS);
  // consecutive lanes, consecutive doubles, BATCH loads in flight per thread before the first LDS store waits for one (a plain
  // load-store loop runs one memory latency per trip: 72 trips a workgroup at dim 12); the upper triangles are not kept
  constexpr int BATCH = 8;
  for (int e0 = t; e0 < n * dd; e0 += THREADS * BATCH) {
    double tmp[BATCH];
#pragma unroll
    for (int q = 0; q < BATCH; q++) {
      const int e = e0 + q * THREADS;
      tmp[q] = e < n * dd ? A[first * dd + e] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < BATCH; q++) {
      const int e = e0 + q * THREADS, k = e % dd, col = k / d, row = k % d;
      if (e < n * dd && row >= col) rec[(e / dd) * LD + tri(row, col, d)] = tmp[q];
    }
  }
  if (OBS) {
    if (t < n) {
      double g[3];
      obstacle_grad(o.cost, o.X + (first + t) * d, (int)((first + t) % o.N), g);
      double *v = rec + t * LD + T;
      for (int k = 0; k < d; k++) v[k] = 0.0;
      for (int k = 0; k < o.cost.pos_dim; k++) v[o.cost.pos_idx[k]] = g[k];
    }
  } else {
    for (int e = t; e < n * d; e += THREADS) rec[(e / d) * LD + T + e % d] = c[first * d + e];
  }
  __syncthreads();
  if (t < n) {
    bool ok;
    if constexpr (DIM > 0) ok = chol_solve_record<DIM>(rec + t * LD);
    else ok = chol_solve_record_any(rec + t * LD, d);
    if (!ok) atomicAdd(bad, 1u);
  }
  __syncthreads();
  // (out may be ref: every element is read and written by the same thread)
  for (int e0 = t; e0 < n * d; e0 += THREADS * BATCH) {
    double tmp[BATCH];
#pragma unroll
    for (int q = 0; q < BATCH; q++) {
      const int e = e0 + q * THREADS;
      tmp[q] = e < n * d ? ref[first * d + e] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < BATCH; q++) {
      const int e = e0 + q * THREADS;
      if (e < n * d) out[first * d + e] = tmp[q] - rec[(e / d) * LD + T + e % d];
    }
  }
}

__global__ void __launch_bounds__(256) k_obstacle_grad(pmpc_scp_cost o, int x, int N, long long rows, const double *X, double *cx) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * x) return;
  const long long row = e / x;
  const int k = (int)(e % x);
  double val = 0.0;
  bool mine = false;
  for (int d = 0; d < o.pos_dim; d++) mine = mine || o.pos_idx[d] == k;
  if (mine) {  // (the lanes of a row's position entries each evaluate the row: 2 - 3 times the exponentials, consecutive stores)
    double g[3];
    obstacle_grad(o, X + row * x, (int)(row % N), g);
    for (int d = 0; d < o.pos_dim; d++)
      if (o.pos_idx[d] == k) val = g[d];
  }
  cx[e] = val;
}

template <int DIM, int UNITS, int THREADS, bool OBS>
void launch_shift_as(int d, long long rows, const double *A, const double *c, const double *ref, double *out, unsigned *bad, const ObsArgs &o,
                     hipStream_t s) {
  static_assert(UNITS <= THREADS, "one thread factors one record");
  const size_t lds = (size_t)UNITS * (size_t)((d * (d + 1) / 2 + d) | 1) * sizeof(double);
  const unsigned grid = (unsigned)((rows + UNITS - 1) / UNITS);
  hipLaunchKernelGGL((k_ref_shift<DIM, UNITS, THREADS, OBS>), dim3(grid), dim3(THREADS), lds, s, d, rows, A, c, ref, out, bad, o);
}
// the compiled (x, u) sizes, and a generic body for the rest.  dim 12 (the 236 MB stream): 128 threads per 64 records, 47 KB of LDS — three
// workgroups per CU, every second wave factors — ; the others: 11 - 20 KB
template <bool OBS>
void launch_shift(int d, long long rows, const double *A, const double *c, const double *ref, double *out, unsigned *bad, const ObsArgs &o, hipStream_t s) {
  if (rows <= 0) return;
  if (d == 2) launch_shift_as<2, 256, 256, OBS>(d, rows, A, c, ref, out, bad, o, s);
  else if (d == 4) launch_shift_as<4, 128, 256, OBS>(d, rows, A, c, ref, out, bad, o, s);
  else if (d == 12) launch_shift_as<12, 64, 128, OBS>(d, rows, A, c, ref, out, bad, o, s);
  else launch_shift_as<0, 16, 256, OBS>(d, rows, A, c, ref, out, bad, o, s);
}

}  // namespace

void launch_ref_shift(int dim, long long rows, const double *A, const double *c, const double *ref, double *out, unsigned *bad, hipStream_t s) {
  ObsArgs none;
  memset(&none, 0, sizeof(none));
  launch_shift<false>(dim, rows, A, c, ref, out, bad, none, s);
}

bool obstacle_cost_valid(const pmpc_scp_cost *o, int xdim) {
  if (!o || o->kind != 1 || o->K < 1 || o->K > 16 || o->pos_dim < 2 || o->pos_dim > 3 || xdim < 1 || xdim > REF_SHIFT_MAX_DIM) return false;
  if (!o->centres || !o->sigma || !o->w) return false;
  for (int d = 0; d < o->pos_dim; d++) {
    if (o->pos_idx[d] < 0 || o->pos_idx[d] >= xdim) return false;
    for (int e = 0; e < d; e++)
      if (o->pos_idx[e] == o->pos_idx[d]) return false;
  }
  return true;
}

void launch_obstacle_grad(const pmpc_scp_cost &cost, int x, int N, int M, const double *X, double *cx, hipStream_t s) {
  const long long rows = (long long)M * N, n = rows * x;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_obstacle_grad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cost, x, N, rows, X, cx);
}

void launch_obstacle_ref_shift(const pmpc_scp_cost &cost, int x, int N, int M, const double *X, const double *Q, const double *X_ref, double *out,
                               unsigned *bad, hipStream_t s) {
  ObsArgs o;
  o.cost = cost; o.X = X; o.N = N;
  launch_shift<true>(x, (long long)M * N, Q, nullptr, X_ref, out, bad, o, s);
}
