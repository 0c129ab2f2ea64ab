// model_jit.hip — custom dynamics models: x+ = F(x, u; p) handed over as device code, compiled at run time for the device's
// architecture, with forward-mode automatic differentiation for the Jacobians (model_dual.h) — include/pmpc_abi.h: pmpc_model_*.
//
// The program hiprtc compiles is
//     #define XD / UD / PD / PMPC_JIT_UNITS
//     #include "model_dual.h"        (the dual arithmetic: the file of that name, wrapped into model_dual.inc by the Makefile)
//     <the user's `template <class T> __device__ void step(const T *x, const T *u, const double *p, T *xn)`>
//     #include "model_kernels.h"     (pmpc_jit_linearize / _rollout / _shift_plan over step<>; likewise model_kernels.inc)
// jit_compile is the runtime compile itself, shared with the custom stage costs (cost_jit.hip).
// Compiling needs neither a context nor a GPU.  Loading puts the code object on a context's device; the loaded models of the process
// sit in one table keyed by id, each entry owned by the context it was loaded on: an id is known to that context only, and
// pmpc_destroy unloads what the context still owns.  The kernels are launched with hipModuleLaunchKernel on the caller's stream.
#include <dlfcn.h>
#include <hip/hiprtc.h>

#include <string>

#include "solver_internal.h"
#include "model_jit.h"

namespace {

const char kDualHeader[] =
#include "model_dual.inc"
    ;
const char kKernelsHeader[] =
#include "model_kernels.inc"
    ;

// ---- lazily bound hiprtc (the library must load, and everything else must run, where it is absent) ----
struct Hiprtc {
  void *h = nullptr;
  hiprtcResult (*CreateProgram)(hiprtcProgram *, const char *, const char *, int, const char *const *, const char *const *) = nullptr;
  hiprtcResult (*CompileProgram)(hiprtcProgram, int, const char *const *) = nullptr;
  hiprtcResult (*DestroyProgram)(hiprtcProgram *) = nullptr;
  hiprtcResult (*GetProgramLogSize)(hiprtcProgram, size_t *) = nullptr;
  hiprtcResult (*GetProgramLog)(hiprtcProgram, char *) = nullptr;
  hiprtcResult (*GetCodeSize)(hiprtcProgram, size_t *) = nullptr;
  hiprtcResult (*GetCode)(hiprtcProgram, char *) = nullptr;
  bool load() {
    if (h) return true;
    const char *names[] = {"libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"};  // torch bundles soname libhiprtc.so: reuse the loaded copy
    for (const char *n : names)
      if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return false;
    CreateProgram = (decltype(CreateProgram))dlsym(h, "hiprtcCreateProgram");
    CompileProgram = (decltype(CompileProgram))dlsym(h, "hiprtcCompileProgram");
    DestroyProgram = (decltype(DestroyProgram))dlsym(h, "hiprtcDestroyProgram");
    GetProgramLogSize = (decltype(GetProgramLogSize))dlsym(h, "hiprtcGetProgramLogSize");
    GetProgramLog = (decltype(GetProgramLog))dlsym(h, "hiprtcGetProgramLog");
    GetCodeSize = (decltype(GetCodeSize))dlsym(h, "hiprtcGetCodeSize");
    GetCode = (decltype(GetCode))dlsym(h, "hiprtcGetCode");
    const bool ok = CreateProgram && CompileProgram && DestroyProgram && GetProgramLogSize && GetProgramLog && GetCodeSize && GetCode;
    if (!ok) h = nullptr;
    return ok;
  }
};
Hiprtc g_rtc;
std::mutex g_rtc_mutex;

constexpr int kLanes = 64;  // PMPC_JIT_LANES of model_kernels.h: rollout and shift run one wave per block

bool dims_ok(int x, int u, int p) { return x >= 1 && x <= 16 && u >= 1 && u <= 16 && p >= 1 && p <= 16; }  // the solver's own limits
// units per block of the linearisation: the largest power of two <= 64 whose LDS records (odd stride) fit 64 KB
int lin_units(int x, int u) {
  const int ld = (x + x * x + x * u) | 1;
  int n = 64;
  while (n > 1 && n * ld * 8 > 65536) n >>= 1;
  return n;
}

struct JitModel {
  pmpc_ctx *owner = nullptr;
  int x = 0, u = 0, p = 0, units = 0;
  std::vector<char> image;  // the code object, kept for as long as the module is loaded
  hipModule_t mod = nullptr;
  hipFunction_t lin = nullptr, roll = nullptr, shift = nullptr;
};
std::map<int, JitModel> g_models;
std::mutex g_models_mutex;
int g_next_id = PMPC_MODEL_CUSTOM0;

bool find_model(int model, JitModel *out) {  // (a copy of the handles: the table may change behind the caller)
  std::lock_guard<std::mutex> lk(g_models_mutex);
  auto it = g_models.find(model);
  if (it == g_models.end()) return false;
  out->owner = it->second.owner;
  out->x = it->second.x; out->u = it->second.u; out->p = it->second.p; out->units = it->second.units;
  out->lin = it->second.lin; out->roll = it->second.roll; out->shift = it->second.shift;
  return true;
}
JitModel need_model(int model) {
  JitModel m;
  if (!find_model(model, &m)) throw PmpcHipError{(int)hipErrorInvalidValue, "custom model id not loaded", __FILE__, __LINE__};
  return m;
}

void write_log(char *log, size_t cap, const std::string &text) {
  if (!log || cap == 0) return;
  const size_t n = std::min(text.size(), cap - 1);
  memcpy(log, text.data(), n);
  log[n] = 0;
}

}  // namespace

const char *jit_dual_header() { return kDualHeader; }

void jit_write_log(char *log, size_t cap, const std::string &text) { write_log(log, cap, text); }

// The runtime compile, written once for models and costs: the target-id check, the lazily bound compiler, create / compile / log /
// code object / destroy.  `who` names the entry in the messages, `what` what needs the compiler.  *code is malloc'd.
int jit_compile(const char *who, const char *what, const std::string &program, const char *program_name, int nheaders, const char *const *headers,
                const char *const *names, const char *arch, void **code, size_t *bytes, char *log, size_t log_cap) {
  const std::string me(who);
  std::string target(arch);
  target = target.substr(0, target.find(':'));  // the target id alone: no feature suffix (never an xnack+ code object)
  if (target.empty() || target.find_first_not_of("abcdefghijklmnopqrstuvwxyz0123456789") != std::string::npos) {
    write_log(log, log_cap, me + ": arch must be a target id such as gfx950");
    return 1;
  }
  std::lock_guard<std::mutex> lk(g_rtc_mutex);
  if (!g_rtc.load()) {
    write_log(log, log_cap, me + ": libhiprtc.so could not be loaded: " + what + " need the HIP runtime compiler");
    return 2;
  }
  hiprtcProgram prog = nullptr;
  if (g_rtc.CreateProgram(&prog, program.c_str(), program_name, nheaders, headers, names) != HIPRTC_SUCCESS) {
    write_log(log, log_cap, me + ": hiprtcCreateProgram failed");
    return 2;
  }
  const std::string opt_arch = "--offload-arch=" + target;
  const char *opts[] = {opt_arch.c_str(), "-O3", "-std=c++17"};
  const hiprtcResult rc = g_rtc.CompileProgram(prog, 3, opts);
  size_t ln = 0;
  std::string text;
  if (g_rtc.GetProgramLogSize(prog, &ln) == HIPRTC_SUCCESS && ln > 1) {
    text.resize(ln);
    if (g_rtc.GetProgramLog(prog, &text[0]) != HIPRTC_SUCCESS) text.clear();
  }
  int ret = 0;
  if (rc != HIPRTC_SUCCESS) {
    write_log(log, log_cap, text.empty() ? me + ": hiprtcCompileProgram failed without a log" : text);
    ret = 3;
  } else {
    write_log(log, log_cap, text);  // (warnings, if any)
    size_t n = 0;
    char *buf = nullptr;
    if (g_rtc.GetCodeSize(prog, &n) != HIPRTC_SUCCESS || n == 0 || !(buf = (char *)malloc(n)) || g_rtc.GetCode(prog, buf) != HIPRTC_SUCCESS) {
      free(buf);
      write_log(log, log_cap, me + ": the compiler returned no code object");
      ret = 2;
    } else {
      *code = buf;
      *bytes = n;
    }
  }
  g_rtc.DestroyProgram(&prog);
  return ret;
}

bool model_known(const pmpc_ctx *c, int model) {
  if (!model_custom(model)) return model_known(model);
  JitModel m;
  return c && find_model(model, &m) && m.owner == c;
}
bool custom_model_dims(int model, int *xdim, int *udim) {
  JitModel m;
  if (!find_model(model, &m)) return false;
  *xdim = m.x;
  *udim = m.u;
  return true;
}
void custom_models_unload_all(pmpc_ctx *c) {
  std::lock_guard<std::mutex> lk(g_models_mutex);
  for (auto it = g_models.begin(); it != g_models.end();) {
    if (it->second.owner == c) {
      HIP_WARN(hipModuleUnload(it->second.mod));
      it = g_models.erase(it);
    } else {
      ++it;
    }
  }
}

void custom_launch_linearize(int model, int N, int M, const double *x0, const double *X_prev, const double *U_prev, const double *params,
                             double *f, double *fx, double *fu, hipStream_t s) {
  const JitModel m = need_model(model);
  long long tot = (long long)M * N;
  const unsigned grid = (unsigned)((tot + m.units - 1) / m.units);
  void *args[] = {&N, &tot, &x0, &X_prev, &U_prev, &params, &f, &fx, &fu};
  HIP_CHECK(hipModuleLaunchKernel(m.lin, grid, 1, 1, 256, 1, 1, 0, s, args, nullptr));  // (256: PMPC_JIT_THREADS; the records are static LDS)
}
void custom_launch_rollout(int model, int N, int M, const double *x0, const double *U, const double *params, double *X, hipStream_t s) {
  const JitModel m = need_model(model);
  const unsigned grid = (unsigned)((M + kLanes - 1) / kLanes);
  void *args[] = {&N, &M, &x0, &U, &params, &X};
  HIP_CHECK(hipModuleLaunchKernel(m.roll, grid, 1, 1, kLanes, 1, 1, 0, s, args, nullptr));
}
void custom_launch_shift_plan(int model, int N, int M, int sh, const double *X, const double *U, const double *params, const double *U_tail,
                              double *Xn, double *Un, double *um1n, hipStream_t s) {
  const JitModel m = need_model(model);
  int tail_blocks = (M + kLanes - 1) / kLanes;
  const long long n = (long long)M * (N - sh) * (m.x + m.u) + (long long)M * m.u;
  long long cb = (n + 4 * kLanes - 1) / (4 * kLanes);  // about four elements per lane, as launch_shift_plan
  if (cb > 8192) cb = 8192;
  void *args[] = {&N, &M, &sh, &tail_blocks, &X, &U, &params, &U_tail, &Xn, &Un, &um1n};
  HIP_CHECK(hipModuleLaunchKernel(m.shift, (unsigned)(tail_blocks + cb), 1, 1, kLanes, 1, 1, 0, s, args, nullptr));
}

extern "C" {

int pmpc_model_compile(const char *source, int xdim, int udim, int pdim, const char *arch, void **code, size_t *bytes, char *log, size_t log_cap) {
  write_log(log, log_cap, "");
  if (!source || !arch || !code || !bytes) return 1;
  *code = nullptr;
  *bytes = 0;
  if (!dims_ok(xdim, udim, pdim)) {
    write_log(log, log_cap, "pmpc_model_compile: xdim, udim and pdim must be in 1 .. 16");
    return 1;
  }
  const std::string program = "#define XD " + std::to_string(xdim) + "\n#define UD " + std::to_string(udim) + "\n#define PD " + std::to_string(pdim) +
                              "\n#define PMPC_JIT_UNITS " + std::to_string(lin_units(xdim, udim)) + "\n#include \"model_dual.h\"\n#line 1 \"step\"\n" +
                              source + "\n#include \"model_kernels.h\"\n";
  const char *headers[] = {kDualHeader, kKernelsHeader}, *names[] = {"model_dual.h", "model_kernels.h"};
  return jit_compile("pmpc_model_compile", "custom models", program, "pmpc_custom_model.hip", 2, headers, names, arch, code, bytes, log, log_cap);
}

void pmpc_model_free_code(void *code) { free(code); }

int pmpc_model_load(pmpc_ctx *c, const void *code, size_t bytes, int xdim, int udim, int pdim) {
  if (!c || !code || bytes == 0 || !dims_ok(xdim, udim, pdim)) return -2;
  JitModel m;
  m.owner = c;
  m.x = xdim; m.u = udim; m.p = pdim; m.units = lin_units(xdim, udim);
  m.image.assign((const char *)code, (const char *)code + bytes);
  try {
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipModuleLoadData(&m.mod, m.image.data()));
  } catch (const PmpcHipError &) {
    return -1;
  }
  // the dimensions the code object was compiled for must be the caller's: grids and array extents are computed from them here
  int dims[4] = {0, 0, 0, 0};
  hipDeviceptr_t dptr = nullptr;
  size_t dbytes = 0;
  bool ok = hipModuleGetGlobal(&dptr, &dbytes, m.mod, "pmpc_jit_dims") == hipSuccess && dbytes == sizeof(dims) &&
            hipMemcpy(dims, dptr, sizeof(dims), hipMemcpyDeviceToHost) == hipSuccess;
  ok = ok && dims[0] == m.x && dims[1] == m.u && dims[2] == m.p && dims[3] == m.units;
  ok = ok && hipModuleGetFunction(&m.lin, m.mod, "pmpc_jit_linearize") == hipSuccess &&
       hipModuleGetFunction(&m.roll, m.mod, "pmpc_jit_rollout") == hipSuccess &&
       hipModuleGetFunction(&m.shift, m.mod, "pmpc_jit_shift_plan") == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    HIP_WARN(hipModuleUnload(m.mod));
    return -3;
  }
  std::lock_guard<std::mutex> lk(g_models_mutex);
  const int id = g_next_id++;
  JitModel &slot = g_models[id];
  slot = std::move(m);
  return id;
}

int pmpc_model_unload(pmpc_ctx *c, int id) {
  if (!c) return 2;
  std::lock_guard<std::mutex> lk(g_models_mutex);
  auto it = g_models.find(id);
  if (it == g_models.end() || it->second.owner != c) return 2;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);  // (a launch of the module may still be in flight)
  HIP_WARN(hipModuleUnload(it->second.mod));
  g_models.erase(it);
  return 0;
}

}  // extern "C"
