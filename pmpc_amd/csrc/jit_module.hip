// jit_module.hip — the plumbing of the runtime-compiled models, costs and constraints, written once (jit_module.h).
// Compiling needs neither a context nor a GPU.  Loading puts the code object on a context's device; the loaded code objects of a kind
// sit in one table keyed by id, each entry owned by the context it was loaded on: an id is known to that context only, and
// pmpc_destroy unloads what the context still owns.  The kernels are launched with hipModuleLaunchKernel on the caller's stream.
#include <dlfcn.h>
#include <hip/hiprtc.h>

#include "solver_internal.h"
#include "jit_module.h"

namespace {

// the headers the runtime compiler reads: the files of these names, each wrapped into one raw string literal by the Makefile
const char kDualHeader[] =
#include "model_dual.inc"
    ;
const char kModelKernels[] =
#include "model_kernels.inc"
    ;
const char kCostKernels[] =
#include "cost_kernels.inc"
    ;
const char kCstrKernels[] =
#include "cstr_kernels.inc"
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

void write_log(char *log, size_t cap, const std::string &text) {
  if (!log || cap == 0) return;
  const size_t n = std::min(text.size(), cap - 1);
  memcpy(log, text.data(), n);
  log[n] = 0;
}

}  // namespace

const JitKind kJitModelKind = {"pmpc_model_compile", "custom models", "step", "model_kernels.h", kModelKernels, "pmpc_custom_model.hip"};
const JitKind kJitCostKind = {"pmpc_cost_compile", "custom costs", "stage_cost", "cost_kernels.h", kCostKernels, "pmpc_custom_cost.hip"};
const JitKind kJitCstrKind = {"pmpc_cstr_compile", "custom constraints", "stage_cstr", "cstr_kernels.h", kCstrKernels, "pmpc_custom_cstr.hip"};

JitTable g_jit_models("pmpc_jit_dims", 4, {"pmpc_jit_linearize", "pmpc_jit_rollout", "pmpc_jit_shift_plan"}, PMPC_MODEL_CUSTOM0);
JitTable g_jit_costs("pmpc_jit_cost_dims", 4, {"pmpc_jit_cost_grad"}, PMPC_COST_CUSTOM0);
JitTable g_jit_cstrs("pmpc_jit_cstr_dims", 3, {"pmpc_jit_cstr_rows"}, PMPC_CSTR_CUSTOM0);

void jit_unload_all(pmpc_ctx *c) {
  for (JitTable *t : {&g_jit_models, &g_jit_costs, &g_jit_cstrs}) t->unload_all(c);
}

// The argument checks, the program text, the target-id check, the lazily bound compiler, create / compile / log / code object / destroy.
int jit_compile(const JitKind &kind, const char *limits, std::initializer_list<JitDefine> defines, const char *source, const char *arch, void **code,
                size_t *bytes, char *log, size_t log_cap) {
  const std::string me(kind.entry);
  write_log(log, log_cap, "");
  if (!source || !arch || !code || !bytes) return 1;
  *code = nullptr;
  *bytes = 0;
  if (limits) {
    write_log(log, log_cap, me + ": " + limits);
    return 1;
  }
  std::string program;
  for (const JitDefine &d : defines) program += std::string("#define ") + d.name + " " + std::to_string(d.value) + "\n";
  program += std::string("#include \"model_dual.h\"\n#line 1 \"") + kind.line_label + "\"\n" + source + "\n#include \"" + kind.kernels_name + "\"\n";
  const char *headers[] = {kDualHeader, kind.kernels_text}, *names[] = {"model_dual.h", kind.kernels_name};

  std::string target(arch);
  target = target.substr(0, target.find(':'));  // the target id alone: no feature suffix (never an xnack+ code object)
  if (target.empty() || target.find_first_not_of("abcdefghijklmnopqrstuvwxyz0123456789") != std::string::npos) {
    write_log(log, log_cap, me + ": arch must be a target id such as gfx950");
    return 1;
  }
  std::lock_guard<std::mutex> lk(g_rtc_mutex);
  if (!g_rtc.load()) {
    write_log(log, log_cap, me + ": libhiprtc.so could not be loaded: " + kind.subject + " need the HIP runtime compiler");
    return 2;
  }
  hiprtcProgram prog = nullptr;
  if (g_rtc.CreateProgram(&prog, program.c_str(), kind.program_name, 2, headers, names) != HIPRTC_SUCCESS) {
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

// ---- the table ----
void JitTable::drop(JitEntry &e) { HIP_WARN(hipModuleUnload(e.mod)); }

int JitTable::load(pmpc_ctx *c, const void *code, size_t bytes, const int *dims) {
  if (!c || !code || bytes == 0) return -2;
  JitEntry m;
  m.owner = c;
  std::copy(dims, dims + ndims_, m.dims);
  m.image.assign((const char *)code, (const char *)code + bytes);
  try {
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipModuleLoadData(&m.mod, m.image.data()));
  } catch (const PmpcHipError &) {
    return -1;
  }
  // what the code object was compiled for must be what the caller states: grids and array extents are computed from it on the host
  int got[4] = {0, 0, 0, 0};
  hipDeviceptr_t dptr = nullptr;
  size_t dbytes = 0;
  bool ok = hipModuleGetGlobal(&dptr, &dbytes, m.mod, dims_symbol_) == hipSuccess && dbytes == ndims_ * sizeof(int) &&
            hipMemcpy(got, dptr, dbytes, hipMemcpyDeviceToHost) == hipSuccess && std::equal(got, got + ndims_, m.dims);
  for (size_t k = 0; ok && k < kernels_.size(); k++) ok = hipModuleGetFunction(&m.fn[k], m.mod, kernels_[k]) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    drop(m);
    return -3;
  }
  std::lock_guard<std::mutex> lk(mutex_);
  entries_[next_id_] = std::move(m);
  return next_id_++;
}

int JitTable::unload(pmpc_ctx *c, int id) {
  if (!c) return 2;
  std::lock_guard<std::mutex> lk(mutex_);
  auto it = entries_.find(id);
  if (it == entries_.end() || it->second.owner != c) return 2;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);  // (a launch of the module may still be in flight)
  drop(it->second);
  entries_.erase(it);
  return 0;
}

void JitTable::unload_all(pmpc_ctx *c) {
  std::lock_guard<std::mutex> lk(mutex_);
  for (auto it = entries_.begin(); it != entries_.end();) {
    if (it->second.owner == c) {
      drop(it->second);
      it = entries_.erase(it);
    } else {
      ++it;
    }
  }
}

bool JitTable::find(int id, JitEntry *out) {
  std::lock_guard<std::mutex> lk(mutex_);
  auto it = entries_.find(id);
  if (it == entries_.end()) return false;
  out->owner = it->second.owner;
  std::copy(it->second.dims, it->second.dims + 4, out->dims);
  std::copy(it->second.fn, it->second.fn + 3, out->fn);
  return true;
}

bool JitTable::known(const pmpc_ctx *c, int id) {
  JitEntry m;
  return c && find(id, &m) && m.owner == c;
}

JitEntry JitTable::need(int id, const char *what) {
  JitEntry m;
  if (!find(id, &m)) throw PmpcHipError{(int)hipErrorInvalidValue, what, __FILE__, __LINE__};
  return m;
}
