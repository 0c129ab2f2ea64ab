// cost_jit.hip — custom stage costs: J = sum_ij stage_cost(X[i,j], U[i,j]; p_i, j, N) handed over as device code, compiled at run time
// with forward-mode automatic differentiation for the gradients (cx, cu) — include/pmpc_abi.h: pmpc_cost_*.
//
// The program hiprtc compiles (jit_module.hip: jit_compile) is
//     #define XD / UD / CD / PMPC_COST_USES_U
//     #include "model_dual.h"        (the dual arithmetic of the custom models)
//     <the user's `template <class T> __device__ T stage_cost(const T *x, const T *u, const double *p, int j, int N)`>
//     #include "cost_kernels.h"      (pmpc_jit_cost_grad over stage_cost<>)
// The loaded costs sit in g_jit_costs (jit_module.h), a table apart from the models', dims = {x, u, cd, uses_u}.
#include "solver_internal.h"
#include "cost_jit.h"
#include "jit_module.h"

namespace {

constexpr int kUnits = 64, kThreads = 256;  // PMPC_JIT_COST_UNITS / _THREADS of cost_kernels.h

bool cost_dims_ok(int x, int u, int cd) { return x >= 1 && x <= 16 && u >= 1 && u <= 16 && cd >= 1 && cd <= 64; }

}  // namespace

bool custom_cost_known(const pmpc_ctx *c, int id) { return g_jit_costs.known(c, id); }
bool custom_cost_dims(int id, int *xdim, int *udim, int *cdim, int *uses_u) {
  JitEntry m;
  if (!g_jit_costs.find(id, &m)) return false;
  int *out[4] = {xdim, udim, cdim, uses_u};
  for (int k = 0; k < 4; k++)
    if (out[k]) *out[k] = m.dims[k];
  return true;
}

void custom_launch_cost_grad(int id, int N, int M, const double *X_prev, const double *U_prev, const double *cparams, double *cx, double *cu,
                             double *val, hipStream_t s) {
  const JitEntry m = g_jit_costs.need(id, "custom cost id not loaded");
  long long tot = (long long)M * N;
  if (tot <= 0) return;
  const unsigned grid = (unsigned)((tot + kUnits - 1) / kUnits);
  void *args[] = {&N, &tot, &X_prev, &U_prev, &cparams, &cx, &cu, &val};
  HIP_CHECK(hipModuleLaunchKernel(m.fn[0], grid, 1, 1, kThreads, 1, 1, 0, s, args, nullptr));  // (the records are static LDS)
}

extern "C" {

int pmpc_cost_compile(const char *source, int xdim, int udim, int cdim, int uses_u, const char *arch, void **code, size_t *bytes, char *log,
                      size_t log_cap) {
  return jit_compile(kJitCostKind, cost_dims_ok(xdim, udim, cdim) ? nullptr : "xdim and udim must be in 1 .. 16, cdim in 1 .. 64",
                     {{"XD", xdim}, {"UD", udim}, {"CD", cdim}, {"PMPC_COST_USES_U", uses_u ? 1 : 0}}, source, arch, code, bytes, log, log_cap);
}

// (what the null cu of a cost compiled with uses_u = 0 rests on is among the dimensions the load compares)
int pmpc_cost_load(pmpc_ctx *c, const void *code, size_t bytes, int xdim, int udim, int cdim, int uses_u) {
  if (!cost_dims_ok(xdim, udim, cdim)) return -2;
  const int dims[4] = {xdim, udim, cdim, uses_u ? 1 : 0};
  return g_jit_costs.load(c, code, bytes, dims);
}

int pmpc_cost_unload(pmpc_ctx *c, int id) { return g_jit_costs.unload(c, id); }

}  // extern "C"
