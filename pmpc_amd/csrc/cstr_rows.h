// cstr_rows.h — launcher of cstr_rows.hip (dense rows a_k'x <= h_k on the states of the SCP loop, restated as bounds on auxiliary states:
// what a custom constraint, cstr_jit.hip, linearises into)
#pragma once
#include "../../include/pmpc_abi.h"
#include "pmpc_dev.h"

// the augmented linearisation of M N (particle, stage) units from their K dense rows a (M, N, K, x), h (M, N, K), one launch; outputs as
// launch_keepout_augment's (keepout.h); X_ref null: X_ref_aug is not written
void launch_rows_augment(int K, int x, int u, int N, int M, const double *a, const double *h, const double *X_prev, const double *f, const double *fx,
                         const double *fu, const double *X_ref, double *f_aug, double *fx_aug, double *fu_aug, double *X_prev_aug, double *X_ref_aug,
                         double *xu_aug, hipStream_t s);
unsigned *cstr_bad_counter(pmpc_ctx *c);  // the workspace's counter of rows pmpc_jit_cstr_rows refused, zeroed when it is created
