// keepout.h — launcher of keepout.hip (keep-out constraints of the SCP loop: obstacle half-spaces restated as bounds on auxiliary states)
#pragma once
#include "../../include/pmpc_abi.h"
#include "pmpc_dev.h"

constexpr int KEEPOUT_MAX_K = 4;
constexpr int KEEPOUT_MAX_DIM = 16;  // xdim + K, the largest state dimension the solver's kernels take

// a kind-1 description the kernel can run for this state dimension
bool keepout_cstr_valid(const pmpc_scp_cstr *cstr, int xdim);
// the augmented linearisation of M N (particle, stage) units in one launch; X_ref null: X_ref_aug is not written
void launch_keepout_augment(const pmpc_scp_cstr &cstr, int x, int u, int N, int M, const double *X_prev, const double *f, const double *fx,
                            const double *fu, const double *X_ref, double *f_aug, double *fx_aug, double *fu_aug, double *X_prev_aug,
                            double *X_ref_aug, double *xu_aug, hipStream_t s);
// the way back: Xo (rows of x) <- the first x entries of every row of X_aug (rows of x + K), and the SCP residual of (Xo, Xp), (Uo, Up) as
// launch_scp_residual takes it into *out, one launch; zero_out false: the caller vouches that *out is 0
void launch_keepout_strip_residual(const double *X_aug, double *Xo, const double *Xp, const double *Uo, const double *Up, long long rows, int x,
                                   int K, int u, double *out, hipStream_t s, bool zero_out = true);
bool keepout_strip_dims_valid(size_t xdim, int K, size_t udim);  // 1 <= K <= 4, xdim + K <= 16, 1 <= udim <= 16
