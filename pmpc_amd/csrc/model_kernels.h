// model_kernels.h — the three kernels of a runtime-compiled dynamics model (model_jit.hip compiles this text with hiprtc, behind
// model_dual.h and the user's `template <class T> __device__ void step(const T *x, const T *u, const double *p, T *xn)`).
// XD, UD, PD (state, control, parameter counts) and PMPC_JIT_UNITS are macros the host defines in front of the program.
// Specifications: k_linearize, k_rollout and k_shift_plan of dynamics.hip — the same arguments, layouts and launch geometry.
//
// Linearisation by forward-mode AD: X_ = [x0, X_prev[:-1]]; f[j] = F(X_[j], U_prev[j]), fx[j] = dF/dx, fu[j] = dF/du in the ABI layout
// (column-major blocks: direction c of the XD + UD is a contiguous run of XD outputs).  The directions are taken PMPC_JIT_W at a time:
// ceil((XD + UD) / W) passes of step<Dual<W>> per (particle, stage) unit, which bounds the registers for XD + UD up to 32; the passes of
// a unit are spread over the block's threads (thread t: unit t % UNITS, passes t / UNITS, + THREADS / UNITS, ..), pass 0 also stores f.
// AD writes every entry of the record, so nothing is cleared.  Records [f | fx | fu] are staged in LDS at an odd stride (conflict-free
// stores) and streamed out by the whole block: consecutive lanes store consecutive doubles.
#ifndef PMPC_JIT_W
#define PMPC_JIT_W 4  // (CHANGELOG.md: registers and scratch at 4 + 2 and 12 + 4 for W = 2, 4, 8)
#endif
#define PMPC_JIT_THREADS 256
#define PMPC_JIT_LANES 64

namespace pmpc_jit {
constexpr int W = PMPC_JIT_W, UNITS = PMPC_JIT_UNITS, THREADS = PMPC_JIT_THREADS;
constexpr int REC = XD + XD * XD + XD * UD, LD = REC | 1;
constexpr int NDIR = XD + UD, NPASS = (NDIR + W - 1) / W;
static_assert(XD >= 1 && XD <= 16 && UD >= 1 && UD <= 16 && PD >= 1 && PD <= 16, "dimensions outside the solver's limits");
static_assert(UNITS >= 1 && UNITS <= 64 && (UNITS & (UNITS - 1)) == 0 && UNITS * LD * 8 <= 65536, "units per block: a power of two whose records fit 64 KB");
}  // namespace pmpc_jit

// what this code object was compiled for: pmpc_model_load checks it against the dimensions its caller states
extern "C" __device__ int pmpc_jit_dims[4] = {XD, UD, PD, PMPC_JIT_UNITS};

extern "C" __global__ void __launch_bounds__(PMPC_JIT_THREADS) pmpc_jit_linearize(int N, long long tot, const double *x0, const double *X_prev,
                                                                                   const double *U_prev, const double *params, double *f,
                                                                                   double *fx, double *fu) {
  using namespace pmpc_jit;
  typedef pmpc_dual::Dual<W> D;
  __shared__ double rec[UNITS * LD];
  const int t = threadIdx.x, unit = t % UNITS;
  const long long first = (long long)blockIdx.x * UNITS, idx = first + unit;
  if (idx < tot) {  // (the partial last block: units past the end are neither evaluated nor stored)
    const long long i = idx / N;
    const int j = (int)(idx % N);
    const double *xs = j == 0 ? x0 + i * XD : X_prev + (idx - 1) * XD;
    const double *us = U_prev + idx * UD, *ps = params + i * PD;
    double xv[XD], uv[UD], p[PD];
#pragma unroll
    for (int k = 0; k < XD; k++) xv[k] = xs[k];
#pragma unroll
    for (int k = 0; k < UD; k++) uv[k] = us[k];
#pragma unroll
    for (int k = 0; k < PD; k++) p[k] = ps[k];
    double *mine = rec + unit * LD;
    for (int pass = t / UNITS; pass < NPASS; pass += THREADS / UNITS) {
      const int c0 = pass * W;  // this pass differentiates along directions c0 .. c0 + W - 1 of [x | u]
      D x[XD], u[UD], xn[XD];
#pragma unroll
      for (int k = 0; k < XD; k++) {
        x[k].v = xv[k];
#pragma unroll
        for (int w = 0; w < W; w++) x[k].d[w] = (k == c0 + w) ? 1.0 : 0.0;
      }
#pragma unroll
      for (int k = 0; k < UD; k++) {
        u[k].v = uv[k];
#pragma unroll
        for (int w = 0; w < W; w++) u[k].d[w] = (XD + k == c0 + w) ? 1.0 : 0.0;
      }
      step<D>(x, u, p, xn);
      if (pass == 0) {
#pragma unroll
        for (int r = 0; r < XD; r++) mine[r] = xn[r].v;
      }
#pragma unroll
      for (int w = 0; w < W; w++)
        if (c0 + w < NDIR) {
#pragma unroll
          for (int r = 0; r < XD; r++) mine[XD + (c0 + w) * XD + r] = xn[r].d[w];
        }
    }
  }
  __syncthreads();
  const int n = (int)((tot - first) < UNITS ? (tot - first) : UNITS);
  for (int e = t; e < n * XD; e += THREADS) f[first * XD + e] = rec[(e / XD) * LD + e % XD];
  for (int e = t; e < n * XD * XD; e += THREADS) fx[first * (XD * XD) + e] = rec[(e / (XD * XD)) * LD + XD + e % (XD * XD)];
  for (int e = t; e < n * XD * UD; e += THREADS) fu[first * (XD * UD) + e] = rec[(e / (XD * UD)) * LD + XD + XD * XD + e % (XD * UD)];
}

// X[i, j] = F(X[i, j-1], U[i, j]; params[i]), X[i, -1] = x0[i]: one lane per particle, the state in registers, one wave per block
extern "C" __global__ void __launch_bounds__(PMPC_JIT_LANES) pmpc_jit_rollout(int N, int M, const double *x0, const double *U, const double *params,
                                                                               double *X) {
  const int i = (int)blockIdx.x * PMPC_JIT_LANES + (int)threadIdx.x;
  if (i >= M) return;
  double x[XD], xn[XD], u[UD], p[PD];
#pragma unroll
  for (int k = 0; k < PD; k++) p[k] = params[(size_t)i * PD + k];
#pragma unroll
  for (int k = 0; k < XD; k++) x[k] = x0[(size_t)i * XD + k];
  const double *Ui = U + (size_t)i * N * UD;
  double *Xi = X + (size_t)i * N * XD;
  for (int j = 0; j < N; j++) {
#pragma unroll
    for (int k = 0; k < UD; k++) u[k] = Ui[(size_t)j * UD + k];
    step<double>(x, u, p, xn);
#pragma unroll
    for (int k = 0; k < XD; k++) Xi[(size_t)j * XD + k] = x[k] = xn[k];
  }
}

// The receding-horizon shift by s stages (1 <= s < N) from (X, U) into (Xn, Un), which must not overlap them: the first tail_blocks
// blocks run the s tail steps from the SOURCE's last state, one lane per particle (U_tail null: the last control is held); the others
// copy element by element, consecutive lanes consecutive doubles.  um1n[i] = U[i, s - 1] (null: not written).
extern "C" __global__ void __launch_bounds__(PMPC_JIT_LANES) pmpc_jit_shift_plan(int N, int M, int s, int tail_blocks, const double *X, const double *U,
                                                                                  const double *params, const double *U_tail, double *Xn, double *Un,
                                                                                  double *um1n) {
  const int keep = N - s;
  if ((int)blockIdx.x < tail_blocks) {
    const int i = (int)blockIdx.x * PMPC_JIT_LANES + (int)threadIdx.x;
    if (i >= M) return;
    double x[XD], xn[XD], u[UD], p[PD];
#pragma unroll
    for (int k = 0; k < PD; k++) p[k] = params[(size_t)i * PD + k];
#pragma unroll
    for (int k = 0; k < XD; k++) x[k] = X[((size_t)i * N + (N - 1)) * XD + k];
    for (int t = 0; t < s; t++) {
      const double *us = U_tail ? U_tail + ((size_t)i * s + t) * UD : U + ((size_t)i * N + (N - 1)) * UD;
#pragma unroll
      for (int k = 0; k < UD; k++) u[k] = us[k];
      step<double>(x, u, p, xn);
#pragma unroll
      for (int k = 0; k < XD; k++) x[k] = xn[k];
      const size_t row = (size_t)i * N + keep + t;
#pragma unroll
      for (int k = 0; k < UD; k++) Un[row * UD + k] = u[k];
#pragma unroll
      for (int k = 0; k < XD; k++) Xn[row * XD + k] = x[k];
    }
    return;
  }
  const long long nx = (long long)M * keep * XD, nu = (long long)M * keep * UD, nm = um1n ? (long long)M * UD : 0;
  const long long stride = (long long)((int)gridDim.x - tail_blocks) * PMPC_JIT_LANES;
  for (long long e = (long long)((int)blockIdx.x - tail_blocks) * PMPC_JIT_LANES + threadIdx.x; e < nx + nu + nm; e += stride) {
    if (e < nx) {
      const long long i = e / (keep * XD), r = e % (keep * XD);
      Xn[i * N * XD + r] = X[i * N * XD + (long long)s * XD + r];
    } else if (e < nx + nu) {
      const long long q = e - nx, i = q / (keep * UD), r = q % (keep * UD);
      Un[i * N * UD + r] = U[i * N * UD + (long long)s * UD + r];
    } else {
      const long long q = e - nx - nu, i = q / UD, k = q % UD;
      um1n[q] = U[(i * N + (s - 1)) * UD + k];
    }
  }
}
