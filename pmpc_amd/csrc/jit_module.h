// jit_module.h — what the runtime-compiled dynamics models (model_jit.hip), stage costs (cost_jit.hip) and state constraints
// (cstr_jit.hip) share: the compile of the user's device code with hiprtc, and the table of code objects loaded on contexts.
// A kind is one JitKind (how its program is put together) and one JitTable (what a loaded code object must export); both are defined
// in jit_module.hip, next to the texts of the headers the runtime compiler reads.  What is a kind's own, its limits, its define list,
// its launchers and its extern "C" entry points, lives in its own unit.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pmpc_abi.h"

// ---- the compile half: needs neither a context nor a GPU ----
struct JitKind {
  const char *entry;         // the entry point, for the messages: "pmpc_model_compile"
  const char *subject;       // what needs the compiler: "custom models"
  const char *line_label;    // the file name the compiler's messages give the user's source: "step"
  const char *kernels_name;  // the header included behind the user's source, and its text
  const char *kernels_text;
  const char *program_name;
};
extern const JitKind kJitModelKind, kJitCostKind, kJitCstrKind;

struct JitDefine {
  const char *name;
  int value;
};
// The body of a pmpc_*_compile: the program is
//     #define <name> <value>          (one line per entry of `defines`)
//     #include "model_dual.h"         (the dual arithmetic)
//     #line 1 "<line_label>"
//     <source>
//     #include "<kernels_name>"
// compiled for the target id `arch` (a feature suffix is dropped).  `limits`: null, or why the dimensions are refused.
// 0: *code (malloc'd) holds *bytes; 1 a null argument, refused dimensions or a bad arch; 2 no runtime compiler; 3 compile error (the
// compiler's text goes to log).
int jit_compile(const JitKind &kind, const char *limits, std::initializer_list<JitDefine> defines, const char *source, const char *arch, void **code,
                size_t *bytes, char *log, size_t log_cap);

// ---- the load half: the code objects of one kind loaded in the process, keyed by id, each owned by the context it was loaded on ----
struct JitEntry {
  pmpc_ctx *owner = nullptr;
  int dims[4] = {0, 0, 0, 0};
  std::vector<char> image;  // the code object, kept for as long as the module is loaded
  hipModule_t mod = nullptr;
  hipFunction_t fn[3] = {nullptr, nullptr, nullptr};  // in the order of the table's kernel names
};

class JitTable {
 public:
  // `dims_symbol`: the device global of `ndims` ints that states what the code object was compiled for
  JitTable(const char *dims_symbol, int ndims, std::initializer_list<const char *> kernels, int first_id)
      : dims_symbol_(dims_symbol), ndims_(ndims), kernels_(kernels), next_id_(first_id) {}
  // The body of a pmpc_*_load once the kind's limits hold: the id (taken only on success); -1 the module does not load on the context's
  // device; -2 a null argument; -3 the code object is not of this kind or was compiled for other than `dims`.
  int load(pmpc_ctx *c, const void *code, size_t bytes, const int *dims);
  int unload(pmpc_ctx *c, int id);  // 0; 2: not an id loaded on this context
  void unload_all(pmpc_ctx *c);
  bool find(int id, JitEntry *out);  // a copy of the handles (not of the image): the table may change behind the caller
  bool known(const pmpc_ctx *c, int id);
  JitEntry need(int id, const char *what);  // find, or throw PmpcHipError with the message `what`

 private:
  static void drop(JitEntry &e);
  const char *dims_symbol_;
  const int ndims_;
  const std::vector<const char *> kernels_;
  std::mutex mutex_;
  std::map<int, JitEntry> entries_;
  int next_id_;
};
extern JitTable g_jit_models, g_jit_costs, g_jit_cstrs;  // three id spaces

void jit_unload_all(pmpc_ctx *c);  // pmpc_destroy: every kind's code objects the context still owns
