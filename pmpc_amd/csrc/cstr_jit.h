// cstr_jit.h — custom state constraints: device code the user hands over as text, compiled at run time (cstr_jit.hip).
// A loaded constraint has an id >= PMPC_CSTR_CUSTOM0 in a table of its own (an id means a constraint only where a constraint is asked
// for: kind 2 of pmpc_scp_cstr, pmpc_custom_cstr_rows_device).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pmpc_abi.h"

bool custom_cstr_known(const pmpc_ctx *c, int id);               // a constraint id loaded on this context
bool custom_cstr_dims(int id, int *xdim, int *kdim, int *pdim);  // false: no such loaded constraint (null outputs are skipped)
// a (M, N, K, x), h (M, N, K), g (M, N, K) or null: one launch of pmpc_jit_cstr_rows; *bad counts the rows it refused
void custom_launch_cstr_rows(int id, int N, int M, const double *X_prev, const double *gparams, double *a, double *h, double *g, unsigned *bad,
                             hipStream_t s);
