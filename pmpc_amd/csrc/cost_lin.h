// cost_lin.h — launchers of cost_lin.hip (linearised nonlinear costs: the reference shift X_ref - Q^-1 cx and the built-in obstacle cost)
#pragma once
#include "../../include/pmpc_abi.h"
#include "pmpc_dev.h"

constexpr int REF_SHIFT_MAX_DIM = 16;

// out[r] = ref[r] - A[r]^-1 c[r], r < rows (out may be ref); *bad += blocks with a pivot that is not positive.  dim in 1 .. REF_SHIFT_MAX_DIM.
void launch_ref_shift(int dim, long long rows, const double *A, const double *c, const double *ref, double *out, unsigned *bad, hipStream_t s);
// a kind-1 description the kernels below can run for this state dimension
bool obstacle_cost_valid(const pmpc_scp_cost *cost, int xdim);
// cx (rows = M N, x) = gradient of the obstacle cost at X (dense, zero outside pos_idx)
void launch_obstacle_grad(const pmpc_scp_cost &cost, int x, int N, int M, const double *X, double *cx, hipStream_t s);
// out = X_ref - Q^-1 cx(X) in one launch (cx never stored; the same arithmetic as the two launches above)
void launch_obstacle_ref_shift(const pmpc_scp_cost &cost, int x, int N, int M, const double *X, const double *Q, const double *X_ref, double *out,
                               unsigned *bad, hipStream_t s);
