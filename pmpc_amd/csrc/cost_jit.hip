// cost_jit.hip — custom stage costs: J = sum_ij stage_cost(X[i,j], U[i,j]; p_i, j, N) handed over as device code, compiled at run time
// with forward-mode automatic differentiation for the gradients (cx, cu) — include/pmpc_abi.h: pmpc_cost_*.
//
// The program hiprtc compiles is
//     #define XD / UD / CD / PMPC_COST_USES_U
//     #include "model_dual.h"        (the dual arithmetic of the custom models)
//     <the user's `template <class T> __device__ T stage_cost(const T *x, const T *u, const double *p, int j, int N)`>
//     #include "cost_kernels.h"      (pmpc_jit_cost_grad over stage_cost<>; wrapped into cost_kernels.inc by the Makefile)
// through jit_compile of model_jit.hip.  Loaded costs sit in one table keyed by id, apart from the models': each entry is owned by the
// context it was loaded on, and pmpc_destroy unloads what the context still owns.
#include <string>

#include "solver_internal.h"
#include "model_jit.h"
#include "cost_jit.h"

namespace {

const char kCostKernelsHeader[] =
#include "cost_kernels.inc"
    ;

constexpr int kUnits = 64, kThreads = 256;  // PMPC_JIT_COST_UNITS / _THREADS of cost_kernels.h

bool cost_dims_ok(int x, int u, int cd) { return x >= 1 && x <= 16 && u >= 1 && u <= 16 && cd >= 1 && cd <= 64; }

struct JitCost {
  pmpc_ctx *owner = nullptr;
  int x = 0, u = 0, cd = 0, uses_u = 0;
  std::vector<char> image;  // the code object, kept for as long as the module is loaded
  hipModule_t mod = nullptr;
  hipFunction_t grad = nullptr;
};
std::map<int, JitCost> g_costs;
std::mutex g_costs_mutex;
int g_next_cost_id = PMPC_COST_CUSTOM0;

bool find_cost(int id, JitCost *out) {  // (a copy of the handles: the table may change behind the caller)
  std::lock_guard<std::mutex> lk(g_costs_mutex);
  auto it = g_costs.find(id);
  if (it == g_costs.end()) return false;
  out->owner = it->second.owner;
  out->x = it->second.x; out->u = it->second.u; out->cd = it->second.cd; out->uses_u = it->second.uses_u;
  out->grad = it->second.grad;
  return true;
}

}  // namespace

bool custom_cost_known(const pmpc_ctx *c, int id) {
  JitCost m;
  return c && find_cost(id, &m) && m.owner == c;
}
bool custom_cost_dims(int id, int *xdim, int *udim, int *cdim, int *uses_u) {
  JitCost m;
  if (!find_cost(id, &m)) return false;
  if (xdim) *xdim = m.x;
  if (udim) *udim = m.u;
  if (cdim) *cdim = m.cd;
  if (uses_u) *uses_u = m.uses_u;
  return true;
}
void custom_costs_unload_all(pmpc_ctx *c) {
  std::lock_guard<std::mutex> lk(g_costs_mutex);
  for (auto it = g_costs.begin(); it != g_costs.end();) {
    if (it->second.owner == c) {
      HIP_WARN(hipModuleUnload(it->second.mod));
      it = g_costs.erase(it);
    } else {
      ++it;
    }
  }
}

void custom_launch_cost_grad(int id, int N, int M, const double *X_prev, const double *U_prev, const double *cparams, double *cx, double *cu,
                             double *val, hipStream_t s) {
  JitCost m;
  if (!find_cost(id, &m)) throw PmpcHipError{(int)hipErrorInvalidValue, "custom cost id not loaded", __FILE__, __LINE__};
  long long tot = (long long)M * N;
  if (tot <= 0) return;
  const unsigned grid = (unsigned)((tot + kUnits - 1) / kUnits);
  void *args[] = {&N, &tot, &X_prev, &U_prev, &cparams, &cx, &cu, &val};
  HIP_CHECK(hipModuleLaunchKernel(m.grad, grid, 1, 1, kThreads, 1, 1, 0, s, args, nullptr));  // (the records are static LDS)
}

extern "C" {

int pmpc_cost_compile(const char *source, int xdim, int udim, int cdim, int uses_u, const char *arch, void **code, size_t *bytes, char *log,
                      size_t log_cap) {
  jit_write_log(log, log_cap, "");
  if (!source || !arch || !code || !bytes) return 1;
  *code = nullptr;
  *bytes = 0;
  if (!cost_dims_ok(xdim, udim, cdim)) {
    jit_write_log(log, log_cap, "pmpc_cost_compile: xdim and udim must be in 1 .. 16, cdim in 1 .. 64");
    return 1;
  }
  const std::string program = "#define XD " + std::to_string(xdim) + "\n#define UD " + std::to_string(udim) + "\n#define CD " + std::to_string(cdim) +
                              "\n#define PMPC_COST_USES_U " + std::to_string(uses_u ? 1 : 0) + "\n#include \"model_dual.h\"\n#line 1 \"stage_cost\"\n" +
                              source + "\n#include \"cost_kernels.h\"\n";
  const char *headers[] = {jit_dual_header(), kCostKernelsHeader}, *names[] = {"model_dual.h", "cost_kernels.h"};
  return jit_compile("pmpc_cost_compile", "custom costs", program, "pmpc_custom_cost.hip", 2, headers, names, arch, code, bytes, log, log_cap);
}

int pmpc_cost_load(pmpc_ctx *c, const void *code, size_t bytes, int xdim, int udim, int cdim, int uses_u) {
  if (!c || !code || bytes == 0 || !cost_dims_ok(xdim, udim, cdim)) return -2;
  JitCost m;
  m.owner = c;
  m.x = xdim; m.u = udim; m.cd = cdim; m.uses_u = uses_u ? 1 : 0;
  m.image.assign((const char *)code, (const char *)code + bytes);
  try {
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipModuleLoadData(&m.mod, m.image.data()));
  } catch (const PmpcHipError &) {
    return -1;
  }
  // what the code object was compiled for must be what the caller states: grids, array extents and the null cu rest on it
  int dims[4] = {0, 0, 0, 0};
  hipDeviceptr_t dptr = nullptr;
  size_t dbytes = 0;
  bool ok = hipModuleGetGlobal(&dptr, &dbytes, m.mod, "pmpc_jit_cost_dims") == hipSuccess && dbytes == sizeof(dims) &&
            hipMemcpy(dims, dptr, sizeof(dims), hipMemcpyDeviceToHost) == hipSuccess;
  ok = ok && dims[0] == m.x && dims[1] == m.u && dims[2] == m.cd && dims[3] == m.uses_u;
  ok = ok && hipModuleGetFunction(&m.grad, m.mod, "pmpc_jit_cost_grad") == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    HIP_WARN(hipModuleUnload(m.mod));
    return -3;
  }
  std::lock_guard<std::mutex> lk(g_costs_mutex);
  const int id = g_next_cost_id++;
  JitCost &slot = g_costs[id];
  slot = std::move(m);
  return id;
}

int pmpc_cost_unload(pmpc_ctx *c, int id) {
  if (!c) return 2;
  std::lock_guard<std::mutex> lk(g_costs_mutex);
  auto it = g_costs.find(id);
  if (it == g_costs.end() || it->second.owner != c) return 2;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);  // (a launch of the module may still be in flight)
  HIP_WARN(hipModuleUnload(it->second.mod));
  g_costs.erase(it);
  return 0;
}

}  // extern "C"
