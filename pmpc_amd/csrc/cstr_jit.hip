// cstr_jit.hip — custom state constraints: g_k(X[i,j]; p_i, j, N) <= 0 handed over as device code, compiled at run time with forward-mode
// automatic differentiation for the rows a_k'x <= h_k the SCP loops impose about the previous iterate — include/pmpc_abi.h: pmpc_cstr_*.
//
// The program hiprtc compiles is
//     #define XD / KD / PD
//     #include "model_dual.h"        (the dual arithmetic of the custom models)
//     <the user's `template <class T> __device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g)`>
//     #include "cstr_kernels.h"      (pmpc_jit_cstr_rows over stage_cstr<>; wrapped into cstr_kernels.inc by the Makefile)
// through jit_compile of model_jit.hip.  Loaded constraints sit in one table keyed by id, apart from the models' and the costs': each
// entry is owned by the context it was loaded on, and pmpc_destroy unloads what the context still owns.
#include <string>

#include "solver_internal.h"
#include "model_jit.h"
#include "cstr_jit.h"

namespace {

const char kCstrKernelsHeader[] =
#include "cstr_kernels.inc"
    ;

constexpr int kUnits = 64, kThreads = 256;  // PMPC_JIT_CSTR_UNITS / _THREADS of cstr_kernels.h

bool cstr_dims_ok(int x, int k, int pd) { return x >= 1 && k >= 1 && k <= 4 && x + k <= 16 && pd >= 1 && pd <= 64; }

struct JitCstr {
  pmpc_ctx *owner = nullptr;
  int x = 0, k = 0, pd = 0;
  std::vector<char> image;  // the code object, kept for as long as the module is loaded
  hipModule_t mod = nullptr;
  hipFunction_t rows = nullptr;
};
std::map<int, JitCstr> g_cstrs;
std::mutex g_cstrs_mutex;
int g_next_cstr_id = PMPC_CSTR_CUSTOM0;

bool find_cstr(int id, JitCstr *out) {  // (a copy of the handles: the table may change behind the caller)
  std::lock_guard<std::mutex> lk(g_cstrs_mutex);
  auto it = g_cstrs.find(id);
  if (it == g_cstrs.end()) return false;
  out->owner = it->second.owner;
  out->x = it->second.x; out->k = it->second.k; out->pd = it->second.pd;
  out->rows = it->second.rows;
  return true;
}

}  // namespace

bool custom_cstr_known(const pmpc_ctx *c, int id) {
  JitCstr m;
  return c && find_cstr(id, &m) && m.owner == c;
}
bool custom_cstr_dims(int id, int *xdim, int *kdim, int *pdim) {
  JitCstr m;
  if (!find_cstr(id, &m)) return false;
  if (xdim) *xdim = m.x;
  if (kdim) *kdim = m.k;
  if (pdim) *pdim = m.pd;
  return true;
}
void custom_cstrs_unload_all(pmpc_ctx *c) {
  std::lock_guard<std::mutex> lk(g_cstrs_mutex);
  for (auto it = g_cstrs.begin(); it != g_cstrs.end();) {
    if (it->second.owner == c) {
      HIP_WARN(hipModuleUnload(it->second.mod));
      it = g_cstrs.erase(it);
    } else {
      ++it;
    }
  }
}

void custom_launch_cstr_rows(int id, int N, int M, const double *X_prev, const double *gparams, double *a, double *h, double *g, unsigned *bad,
                             hipStream_t s) {
  JitCstr m;
  if (!find_cstr(id, &m)) throw PmpcHipError{(int)hipErrorInvalidValue, "custom constraint id not loaded", __FILE__, __LINE__};
  long long tot = (long long)M * N;
  if (tot <= 0) return;
  const unsigned grid = (unsigned)((tot + kUnits - 1) / kUnits);
  void *args[] = {&N, &tot, &X_prev, &gparams, &a, &h, &g, &bad};
  HIP_CHECK(hipModuleLaunchKernel(m.rows, grid, 1, 1, kThreads, 1, 1, 0, s, args, nullptr));  // (the records are static LDS)
}

extern "C" {

int pmpc_cstr_compile(const char *source, int xdim, int kdim, int pdim, const char *arch, void **code, size_t *bytes, char *log, size_t log_cap) {
  jit_write_log(log, log_cap, "");
  if (!source || !arch || !code || !bytes) return 1;
  *code = nullptr;
  *bytes = 0;
  if (!cstr_dims_ok(xdim, kdim, pdim)) {
    jit_write_log(log, log_cap, "pmpc_cstr_compile: xdim must be at least 1, kdim in 1 .. 4, xdim + kdim at most 16, pdim in 1 .. 64");
    return 1;
  }
  const std::string program = "#define XD " + std::to_string(xdim) + "\n#define KD " + std::to_string(kdim) + "\n#define PD " + std::to_string(pdim) +
                              "\n#include \"model_dual.h\"\n#line 1 \"stage_cstr\"\n" + source + "\n#include \"cstr_kernels.h\"\n";
  const char *headers[] = {jit_dual_header(), kCstrKernelsHeader}, *names[] = {"model_dual.h", "cstr_kernels.h"};
  return jit_compile("pmpc_cstr_compile", "custom constraints", program, "pmpc_custom_cstr.hip", 2, headers, names, arch, code, bytes, log, log_cap);
}

int pmpc_cstr_load(pmpc_ctx *c, const void *code, size_t bytes, int xdim, int kdim, int pdim) {
  if (!c || !code || bytes == 0 || !cstr_dims_ok(xdim, kdim, pdim)) return -2;
  JitCstr m;
  m.owner = c;
  m.x = xdim; m.k = kdim; m.pd = pdim;
  m.image.assign((const char *)code, (const char *)code + bytes);
  try {
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipModuleLoadData(&m.mod, m.image.data()));
  } catch (const PmpcHipError &) {
    return -1;
  }
  // what the code object was compiled for must be what the caller states: grids and array extents rest on it
  int dims[3] = {0, 0, 0};
  hipDeviceptr_t dptr = nullptr;
  size_t dbytes = 0;
  bool ok = hipModuleGetGlobal(&dptr, &dbytes, m.mod, "pmpc_jit_cstr_dims") == hipSuccess && dbytes == sizeof(dims) &&
            hipMemcpy(dims, dptr, sizeof(dims), hipMemcpyDeviceToHost) == hipSuccess;
  ok = ok && dims[0] == m.x && dims[1] == m.k && dims[2] == m.pd;
  ok = ok && hipModuleGetFunction(&m.rows, m.mod, "pmpc_jit_cstr_rows") == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    HIP_WARN(hipModuleUnload(m.mod));
    return -3;
  }
  std::lock_guard<std::mutex> lk(g_cstrs_mutex);
  const int id = g_next_cstr_id++;
  JitCstr &slot = g_cstrs[id];
  slot = std::move(m);
  return id;
}

int pmpc_cstr_unload(pmpc_ctx *c, int id) {
  if (!c) return 2;
  std::lock_guard<std::mutex> lk(g_cstrs_mutex);
  auto it = g_cstrs.find(id);
  if (it == g_cstrs.end() || it->second.owner != c) return 2;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);  // (a launch of the module may still be in flight)
  HIP_WARN(hipModuleUnload(it->second.mod));
  g_cstrs.erase(it);
  return 0;
}

}  // extern "C"
