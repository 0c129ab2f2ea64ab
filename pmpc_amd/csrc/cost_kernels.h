// cost_kernels.h — the kernel of a runtime-compiled stage cost (cost_jit.hip compiles this text with hiprtc, behind model_dual.h and the
// user's `template <class T> __device__ T stage_cost(const T *x, const T *u, const double *p, int j, int N)`).
// XD, UD, CD (state, control, cost-parameter counts) and PMPC_COST_USES_U (0 / 1) are macros the host defines in front of the program.
//
// Gradient by forward-mode AD, on the plan of pmpc_jit_linearize (model_kernels.h): the directions [x | u] of a (particle, stage) unit
// are taken W at a time — ceil((XD + UD) / W) passes of stage_cost<Dual<W>>, with PMPC_COST_USES_U = 0 ceil(XD / W) passes in which u
// carries no direction —, the passes of a unit are spread over the block's threads, pass 0 also stores the value.  AD writes every entry
// of the record [val | cx | cu], so nothing is cleared.  The records are staged in LDS at an odd stride and streamed out by the whole
// block: consecutive lanes store consecutive doubles of val, of cx and of cu.  p is the particle's row of cparams in global memory as
// it is (never copied into registers: CD goes up to 64); x and u are read once per thread.
//
// Block shape: 64 units x 4 pass slots = 256 threads, whatever the dimensions.  A record is at most 1 + 16 + 16 = 33 doubles, so 64 of
// them take at most 16.9 KB of LDS and the unit count never has to shrink (pmpc_jit_linearize's does).  With 64 units a wave is one
// pass slot of 64 consecutive units: its lanes run the same pass (no divergence on the pass index) and read consecutive rows of X_prev
// and U_prev; four slots cover 16 directions in one trip (12 + 4), the 32 of the limits in two.  Lane l of a wave stores its record
// entry at double l LD + const: with LD odd the lanes spread over all LDS banks (at the even stride 32 they would share two).
#ifndef PMPC_JIT_W
#define PMPC_JIT_W 4  // (as model_kernels.h)
#endif
#define PMPC_JIT_COST_THREADS 256
#define PMPC_JIT_COST_UNITS 64

namespace pmpc_jit_cost {
constexpr int W = PMPC_JIT_W, UNITS = PMPC_JIT_COST_UNITS, THREADS = PMPC_JIT_COST_THREADS;
constexpr int NU = PMPC_COST_USES_U ? UD : 0;  // directions (and record entries) of u
constexpr int NUD = NU > 0 ? NU : 1;           // (a divisor for code that is dead at NU = 0)
constexpr int REC = 1 + XD + NU, LD = REC | 1;
constexpr int NDIR = XD + NU, NPASS = (NDIR + W - 1) / W;
static_assert(XD >= 1 && XD <= 16 && UD >= 1 && UD <= 16 && CD >= 1 && CD <= 64, "dimensions outside the limits");
static_assert(UNITS * LD * 8 <= 65536 && THREADS % UNITS == 0, "64 records fit LDS; whole pass slots");
}  // namespace pmpc_jit_cost

// what this code object was compiled for: pmpc_cost_load checks it against what its caller states
extern "C" __device__ int pmpc_jit_cost_dims[4] = {XD, UD, CD, PMPC_COST_USES_U};

// cx (tot, XD), cu (tot, UD; never touched with PMPC_COST_USES_U = 0), val (tot; null: not stored) at X_prev (tot, XD), U_prev (tot, UD),
// cparams (tot / N, CD); tot = M N units, unit idx = particle idx / N, stage idx % N
extern "C" __global__ void __launch_bounds__(PMPC_JIT_COST_THREADS) pmpc_jit_cost_grad(int N, long long tot, const double *X_prev, const double *U_prev,
                                                                                        const double *cparams, double *cx, double *cu, double *val) {
  using namespace pmpc_jit_cost;
  typedef pmpc_dual::Dual<W> D;
  __shared__ double rec[UNITS * LD];
  const int t = threadIdx.x, unit = t % UNITS;
  const long long first = (long long)blockIdx.x * UNITS, idx = first + unit;
  if (idx < tot) {  // (the partial last block: units past the end are neither evaluated nor stored)
    const long long i = idx / N;
    const int j = (int)(idx % N);
    const double *xs = X_prev + idx * XD, *us = U_prev + idx * UD, *p = cparams + i * CD;
    double xv[XD], uv[UD];
#pragma unroll
    for (int k = 0; k < XD; k++) xv[k] = xs[k];
#pragma unroll
    for (int k = 0; k < UD; k++) uv[k] = us[k];
    double *mine = rec + unit * LD;
    for (int pass = t / UNITS; pass < NPASS; pass += THREADS / UNITS) {
      const int c0 = pass * W;  // this pass differentiates along directions c0 .. c0 + W - 1 of [x | u]
      D x[XD], u[UD];
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
        for (int w = 0; w < W; w++) u[k].d[w] = (NU > 0 && XD + k == c0 + w) ? 1.0 : 0.0;
      }
      const D c = stage_cost<D>(x, u, p, j, N);
      if (pass == 0) mine[0] = c.v;
#pragma unroll
      for (int w = 0; w < W; w++)
        if (c0 + w < NDIR) mine[1 + c0 + w] = c.d[w];
    }
  }
  __syncthreads();
  const int n = (int)((tot - first) < UNITS ? (tot - first) : UNITS);
  if (val)
    for (int e = t; e < n; e += THREADS) val[first + e] = rec[e * LD];
  for (int e = t; e < n * XD; e += THREADS) cx[first * XD + e] = rec[(e / XD) * LD + 1 + e % XD];
  if (NU > 0)
    for (int e = t; e < n * NU; e += THREADS) cu[first * NU + e] = rec[(e / NUD) * LD + 1 + XD + e % NUD];
}
