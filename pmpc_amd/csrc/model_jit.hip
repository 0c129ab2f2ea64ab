// model_jit.hip — custom dynamics models: x+ = F(x, u; p) handed over as device code, compiled at run time for the device's
// architecture, with forward-mode automatic differentiation for the Jacobians (model_dual.h) — include/pmpc_abi.h: pmpc_model_*.
//
// The program hiprtc compiles (jit_module.hip: jit_compile) is
//     #define XD / UD / PD / PMPC_JIT_UNITS
//     #include "model_dual.h"        (the dual arithmetic)
//     <the user's `template <class T> __device__ void step(const T *x, const T *u, const double *p, T *xn)`>
//     #include "model_kernels.h"     (pmpc_jit_linearize / _rollout / _shift_plan over step<>)
// The loaded models sit in g_jit_models (jit_module.h), dims = {x, u, p, units per block of the linearisation}.
#include "solver_internal.h"
#include "model_jit.h"
#include "jit_module.h"

namespace {

constexpr int kLanes = 64;  // PMPC_JIT_LANES of model_kernels.h: rollout and shift run one wave per block
enum { kLin, kRoll, kShift };  // JitEntry::fn, the order of g_jit_models' kernel names

bool dims_ok(int x, int u, int p) { return x >= 1 && x <= 16 && u >= 1 && u <= 16 && p >= 1 && p <= 16; }  // the solver's own limits
// units per block of the linearisation: the largest power of two <= 64 whose LDS records (odd stride) fit 64 KB
int lin_units(int x, int u) {
  const int ld = (x + x * x + x * u) | 1;
  int n = 64;
  while (n > 1 && n * ld * 8 > 65536) n >>= 1;
  return n;
}
JitEntry need_model(int model) { return g_jit_models.need(model, "custom model id not loaded"); }

}  // namespace

bool model_known(const pmpc_ctx *c, int model) { return model_custom(model) ? g_jit_models.known(c, model) : model_known(model); }
bool custom_model_dims(int model, int *xdim, int *udim) {
  JitEntry m;
  if (!g_jit_models.find(model, &m)) return false;
  *xdim = m.dims[0];
  *udim = m.dims[1];
  return true;
}

void custom_launch_linearize(int model, int N, int M, const double *x0, const double *X_prev, const double *U_prev, const double *params,
                             double *f, double *fx, double *fu, hipStream_t s) {
  const JitEntry m = need_model(model);
  const int units = m.dims[3];
  long long tot = (long long)M * N;
  const unsigned grid = (unsigned)((tot + units - 1) / units);
  void *args[] = {&N, &tot, &x0, &X_prev, &U_prev, &params, &f, &fx, &fu};
  HIP_CHECK(hipModuleLaunchKernel(m.fn[kLin], grid, 1, 1, 256, 1, 1, 0, s, args, nullptr));  // (256: PMPC_JIT_THREADS; the records are static LDS)
}
void custom_launch_rollout(int model, int N, int M, const double *x0, const double *U, const double *params, double *X, hipStream_t s) {
  const JitEntry m = need_model(model);
  const unsigned grid = (unsigned)((M + kLanes - 1) / kLanes);
  void *args[] = {&N, &M, &x0, &U, &params, &X};
  HIP_CHECK(hipModuleLaunchKernel(m.fn[kRoll], grid, 1, 1, kLanes, 1, 1, 0, s, args, nullptr));
}
void custom_launch_shift_plan(int model, int N, int M, int sh, const double *X, const double *U, const double *params, const double *U_tail,
                              double *Xn, double *Un, double *um1n, hipStream_t s) {
  const JitEntry m = need_model(model);
  int tail_blocks = (M + kLanes - 1) / kLanes;
  const long long n = (long long)M * (N - sh) * (m.dims[0] + m.dims[1]) + (long long)M * m.dims[1];
  long long cb = (n + 4 * kLanes - 1) / (4 * kLanes);  // about four elements per lane, as launch_shift_plan
  if (cb > 8192) cb = 8192;
  void *args[] = {&N, &M, &sh, &tail_blocks, &X, &U, &params, &U_tail, &Xn, &Un, &um1n};
  HIP_CHECK(hipModuleLaunchKernel(m.fn[kShift], (unsigned)(tail_blocks + cb), 1, 1, kLanes, 1, 1, 0, s, args, nullptr));
}

extern "C" {

int pmpc_model_compile(const char *source, int xdim, int udim, int pdim, const char *arch, void **code, size_t *bytes, char *log, size_t log_cap) {
  const bool ok = dims_ok(xdim, udim, pdim);
  return jit_compile(kJitModelKind, ok ? nullptr : "xdim, udim and pdim must be in 1 .. 16",
                     {{"XD", xdim}, {"UD", udim}, {"PD", pdim}, {"PMPC_JIT_UNITS", ok ? lin_units(xdim, udim) : 0}}, source, arch, code, bytes, log, log_cap);
}

void pmpc_model_free_code(void *code) { free(code); }

int pmpc_model_load(pmpc_ctx *c, const void *code, size_t bytes, int xdim, int udim, int pdim) {
  if (!dims_ok(xdim, udim, pdim)) return -2;
  const int dims[4] = {xdim, udim, pdim, lin_units(xdim, udim)};
  return g_jit_models.load(c, code, bytes, dims);
}

int pmpc_model_unload(pmpc_ctx *c, int id) { return g_jit_models.unload(c, id); }

}  // extern "C"
