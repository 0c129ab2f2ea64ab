// model_jit.h — custom dynamics models: device code the user hands over as text, compiled at run time (model_jit.hip).
// A loaded model has an id >= PMPC_MODEL_CUSTOM0 and enters every entry point that takes a built-in id; the launchers of
// dynamics.hip branch to the custom_launch_* below at their top.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pmpc_abi.h"

inline bool model_custom(int model) { return model >= PMPC_MODEL_CUSTOM0; }
bool model_known(const pmpc_ctx *c, int model);           // a built-in id, or a custom id loaded on this context
bool custom_model_dims(int model, int *xdim, int *udim);  // false: no such loaded model
// the arguments of launch_linearize / launch_rollout / launch_shift_plan (pmpc_dev.h); fx / fu are always doubles
void custom_launch_linearize(int model, int N, int M, const double *x0, const double *X_prev, const double *U_prev, const double *params,
                             double *f, double *fx, double *fu, hipStream_t s);
void custom_launch_rollout(int model, int N, int M, const double *x0, const double *U, const double *params, double *X, hipStream_t s);
void custom_launch_shift_plan(int model, int N, int M, int sh, const double *X, const double *U, const double *params, const double *U_tail,
                              double *Xn, double *Un, double *um1n, hipStream_t s);
