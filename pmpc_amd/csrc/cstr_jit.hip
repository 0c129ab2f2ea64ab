// cstr_jit.hip — custom state constraints: g_k(X[i,j]; p_i, j, N) <= 0 handed over as device code, compiled at run time with forward-mode
// automatic differentiation for the rows a_k'x <= h_k the SCP loops impose about the previous iterate — include/pmpc_abi.h: pmpc_cstr_*.
//
// The program hiprtc compiles (jit_module.hip: jit_compile) is
//     #define XD / KD / PD
//     #include "model_dual.h"        (the dual arithmetic of the custom models)
//     <the user's `template <class T> __device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g)`>
//     #include "cstr_kernels.h"      (pmpc_jit_cstr_rows over stage_cstr<>)
// The loaded constraints sit in g_jit_cstrs (jit_module.h), a table apart from the models' and the costs', dims = {x, k, pd}.
#include "solver_internal.h"
#include "cstr_jit.h"
#include "jit_module.h"

namespace {

constexpr int kUnits = 64, kThreads = 256;  // PMPC_JIT_CSTR_UNITS / _THREADS of cstr_kernels.h

bool cstr_dims_ok(int x, int k, int pd) { return x >= 1 && k >= 1 && k <= 4 && x + k <= 16 && pd >= 1 && pd <= 64; }

}  // namespace

bool custom_cstr_known(const pmpc_ctx *c, int id) { return g_jit_cstrs.known(c, id); }
bool custom_cstr_dims(int id, int *xdim, int *kdim, int *pdim) {
  JitEntry m;
  if (!g_jit_cstrs.find(id, &m)) return false;
  int *out[3] = {xdim, kdim, pdim};
  for (int k = 0; k < 3; k++)
    if (out[k]) *out[k] = m.dims[k];
  return true;
}

void custom_launch_cstr_rows(int id, int N, int M, const double *X_prev, const double *gparams, double *a, double *h, double *g, unsigned *bad,
                             hipStream_t s) {
  const JitEntry m = g_jit_cstrs.need(id, "custom constraint id not loaded");
  long long tot = (long long)M * N;
  if (tot <= 0) return;
  const unsigned grid = (unsigned)((tot + kUnits - 1) / kUnits);
  void *args[] = {&N, &tot, &X_prev, &gparams, &a, &h, &g, &bad};
  HIP_CHECK(hipModuleLaunchKernel(m.fn[0], grid, 1, 1, kThreads, 1, 1, 0, s, args, nullptr));  // (the records are static LDS)
}

extern "C" {

int pmpc_cstr_compile(const char *source, int xdim, int kdim, int pdim, const char *arch, void **code, size_t *bytes, char *log, size_t log_cap) {
  return jit_compile(kJitCstrKind,
                     cstr_dims_ok(xdim, kdim, pdim) ? nullptr : "xdim must be at least 1, kdim in 1 .. 4, xdim + kdim at most 16, pdim in 1 .. 64",
                     {{"XD", xdim}, {"KD", kdim}, {"PD", pdim}}, source, arch, code, bytes, log, log_cap);
}

int pmpc_cstr_load(pmpc_ctx *c, const void *code, size_t bytes, int xdim, int kdim, int pdim) {
  if (!cstr_dims_ok(xdim, kdim, pdim)) return -2;
  const int dims[3] = {xdim, kdim, pdim};
  return g_jit_cstrs.load(c, code, bytes, dims);
}

int pmpc_cstr_unload(pmpc_ctx *c, int id) { return g_jit_cstrs.unload(c, id); }

}  // extern "C"
