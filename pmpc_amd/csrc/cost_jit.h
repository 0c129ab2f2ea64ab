// cost_jit.h — custom stage costs: device code the user hands over as text, compiled at run time (cost_jit.hip).
// A loaded cost has an id >= PMPC_COST_CUSTOM0 in a table of its own (an id means a cost only where a cost is asked for: kind 2 of
// pmpc_scp_cost, pmpc_custom_cost_grad_device).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pmpc_abi.h"

bool custom_cost_known(const pmpc_ctx *c, int id);                              // a cost id loaded on this context
bool custom_cost_dims(int id, int *xdim, int *udim, int *cdim, int *uses_u);    // false: no such loaded cost (null outputs are skipped)
// cx (M, N, x), cu (M, N, u; not touched by a cost compiled with uses_u = 0), val (M, N) or null: one launch of pmpc_jit_cost_grad
void custom_launch_cost_grad(int id, int N, int M, const double *X_prev, const double *U_prev, const double *cparams, double *cx, double *cu,
                             double *val, hipStream_t s);
