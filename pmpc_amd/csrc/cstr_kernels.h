// cstr_kernels.h — the kernel of a runtime-compiled state constraint (cstr_jit.hip compiles this text with hiprtc, behind model_dual.h and
// the user's `template <class T> __device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g)`).
// XD, KD, PD (state, constraint-row and parameter counts) are macros the host defines in front of the program.
//
// The constraint is g_k(x; p, j, N) <= 0, k < KD, on every (particle, stage) unit.  About xbar = the unit's row of X_prev the kernel gives
// the rows  a_k'x <= h_k  with a_k = grad g_k(xbar), h_k = a_k'xbar - g_k(xbar), by forward-mode AD on the plan of pmpc_jit_cost_grad
// (cost_kernels.h): the XD directions of a unit are taken W at a time — ceil(XD / W) passes of stage_cstr<Dual<W>>, each of which yields
// the partials of ALL KD outputs along its W directions —, the passes of a unit are spread over the block's threads, pass 0 also stores
// the values.  AD writes every entry of the unit's KD records [g_k | a_k], so nothing is cleared.
//
// Block shape: 64 units x 4 pass slots = 256 threads, whatever the dimensions; XD <= 15, so one trip of the pass loop covers every
// direction.  A wave is one pass slot of 64 consecutive units: its lanes run the same pass and read consecutive rows of X_prev.  A unit's
// records are KD (1 + XD) <= 52 doubles (KD = 4, XD = 12), staged in LDS at the odd stride LD = 53 at most: 64 units take at most
// 27.1 KB, and lane l of a wave stores at double l LD + const, which with LD odd spreads the lanes over all banks.
// After the barrier one thread per (unit, k) forms h_k as an fma chain over c = 0 .. XD - 1, minus g_k, and stores h and g — consecutive
// lanes, consecutive doubles.  A row with a non-finite g_k or gradient entry gets h = +inf and a = 0 (no constraint: never a NaN, which
// in an upper bound means "no state bounds" to the solver) and counts in *bad.  After a second barrier the whole block streams a out.
#ifndef PMPC_JIT_W
#define PMPC_JIT_W 4  // (as model_kernels.h)
#endif
#define PMPC_JIT_CSTR_THREADS 256
#define PMPC_JIT_CSTR_UNITS 64

namespace pmpc_jit_cstr {
constexpr int W = PMPC_JIT_W, UNITS = PMPC_JIT_CSTR_UNITS, THREADS = PMPC_JIT_CSTR_THREADS;
constexpr int ROW = 1 + XD;           // one record [g_k | a_k]
constexpr int REC = KD * ROW, LD = REC | 1;
constexpr int NPASS = (XD + W - 1) / W;
static_assert(XD >= 1 && KD >= 1 && KD <= 4 && XD + KD <= 16 && PD >= 1 && PD <= 64, "dimensions outside the limits");
static_assert(UNITS * LD * 8 <= 65536 && THREADS % UNITS == 0, "64 units' records fit LDS; whole pass slots");
}  // namespace pmpc_jit_cstr

// what this code object was compiled for: pmpc_cstr_load checks it against what its caller states
extern "C" __device__ int pmpc_jit_cstr_dims[3] = {XD, KD, PD};

// a (tot, KD, XD), h (tot, KD), g (tot, KD; null: not stored) at X_prev (tot, XD), gparams (tot / N, PD); tot = M N units, unit idx =
// particle idx / N, stage idx % N; *bad: rows refused (atomic count)
extern "C" __global__ void __launch_bounds__(PMPC_JIT_CSTR_THREADS) pmpc_jit_cstr_rows(int N, long long tot, const double *X_prev, const double *gparams,
                                                                                        double *a, double *h, double *g, unsigned *bad) {
  using namespace pmpc_jit_cstr;
  typedef pmpc_dual::Dual<W> D;
  __shared__ double rec[UNITS * LD];
  const int t = threadIdx.x, unit = t % UNITS;
  const long long first = (long long)blockIdx.x * UNITS, idx = first + unit;
  if (idx < tot) {  // (the partial last block: units past the end are neither evaluated nor stored)
    const long long i = idx / N;
    const int j = (int)(idx % N);
    const double *xs = X_prev + idx * XD, *p = gparams + i * PD;
    double *mine = rec + unit * LD;
    for (int pass = t / UNITS; pass < NPASS; pass += THREADS / UNITS) {
      const int c0 = pass * W;  // this pass differentiates along directions c0 .. c0 + W - 1 of x
      D x[XD], gv[KD];
#pragma unroll
      for (int k = 0; k < XD; k++) {
        x[k].v = xs[k];
#pragma unroll
        for (int w = 0; w < W; w++) x[k].d[w] = (k == c0 + w) ? 1.0 : 0.0;
      }
      stage_cstr<D>(x, p, j, N, gv);
#pragma unroll
      for (int k = 0; k < KD; k++) {
        if (pass == 0) mine[k * ROW] = gv[k].v;
#pragma unroll
        for (int w = 0; w < W; w++)
          if (c0 + w < XD) mine[k * ROW + 1 + c0 + w] = gv[k].d[w];
      }
    }
  }
  __syncthreads();
  const int n = (int)((tot - first) < UNITS ? (tot - first) : UNITS);
  for (int e = t; e < n * KD; e += THREADS) {  // one (unit, k) row each; e is the row's index in h and g past the block's first
    double *row = rec + (e / KD) * LD + (e % KD) * ROW;
    const double *xs = X_prev + (first + e / KD) * XD;
    const double gk = row[0];
    bool ok = gk - gk == 0.0;  // finite
    double acc = row[1] * xs[0];
#pragma unroll
    for (int c = 1; c < XD; c++) acc = fma(row[1 + c], xs[c], acc);
#pragma unroll
    for (int c = 0; c < XD; c++) ok = ok && (row[1 + c] - row[1 + c] == 0.0);
    if (!ok) {
#pragma unroll
      for (int c = 0; c < XD; c++) row[1 + c] = 0.0;
      atomicAdd(bad, 1u);
    }
    h[first * KD + e] = ok ? acc - gk : __longlong_as_double(0x7ff0000000000000LL);
    if (g) g[first * KD + e] = gk;
  }
  __syncthreads();
  for (int e = t; e < n * KD * XD; e += THREADS) {
    const int un = e / (KD * XD), r = e % (KD * XD);
    a[first * (KD * XD) + e] = rec[un * LD + (r / XD) * ROW + 1 + r % XD];
  }
}
