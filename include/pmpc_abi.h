/*
 * pmpc_abi.h — C ABI of libpmpc_hip.so, the MI355X-native replacement for the
 * PMPC.jl back end of StanfordASL/pmpc.
 *
 * Part 1 is the DROP-IN boundary: the two symbols the reference's pybind11 module
 * binds (PMPC.jl/pmpcjl/module.cpp:9-23) and the Julia library exports
 * (PMPC.jl/src/c_interface.jl:77-141 `c_lqp_solve`, :146-214 `c_lcone_solve`),
 * with the same argument order, layouts, sentinels and error behaviour.
 *
 * Part 2 is the device-resident extension (no reference counterpart): the same
 * solve with every buffer already in HBM, a persistent workspace, an explicit HIP
 * stream, particle sharding over RCCL and the on-device dynamics linearisation
 * that replaces the user's f_fx_fu_fn callback (pmpc/scp_mpc.py:338-342) for the
 * built-in models.
 *
 * Layouts (column-major, PMPC.jl/src/c_interface.jl:28-46):
 *   x0 (xdim,M)   f, X_prev, X_ref, lx, ux (xdim,N,M)   U_prev, U_ref, lu, uu (udim,N,M)
 *   fx, Q (xdim,xdim,N,M)   fu (xdim,udim,N,M)   R (udim,udim,N,M)
 *   slew_reg (M)   slew_reg0 (M)   slew_um1 (udim,M)
 *   X_out (xdim,N,M)  — steps 1..N, x0 is NOT included (c_interface.jl:138)
 *   U_out (udim,N,M)
 * i.e. particle-major, time-minor arrays of column-major blocks; equivalently the
 * C-order numpy arrays (M,N,d) and (M,N,col,row).
 *
 * Sentinels (c_interface.jl:56-70): any NaN in lx|ux => no state bounds; any NaN in
 * lu|uu => no control bounds; any NaN in slew_reg => 0; any NaN in slew_reg0 or
 * slew_um1 => both ignored.  Nc < 0 => Nc = N (PMPC.jl/src/main.jl:127-128).
 * +-inf entries of a bound array mean "unbounded on that side" (as for OSQP).
 *
 * Errors: void return; on failure X_out/U_out are filled with NaN
 * (PMPC.jl/src/osqp_solver.jl:65-71) which the Python host turns into
 * (None, None, None) (pmpc/scp_mpc.py:391-394).
 *
 * Threading: one caller thread at a time per process (as the reference, which holds
 * the GIL for the whole call, module.cpp:28-72).  Blocking.
 */
#ifndef PMPC_ABI_H
#define PMPC_ABI_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Part 1 — drop-in boundary (host pointers)
 * ------------------------------------------------------------------------------------------- */

/* replaces PMPC.jl/src/c_interface.jl:77-141 (prototype: PMPC.jl/pmpcjl/module.cpp:9-15) */
void c_lqp_solve(double *X_out, double *U_out, size_t xdim, size_t udim, size_t N, size_t M, long long Nc,
                 double *x0, double *f, double *fx, double *fu, double *X_prev, double *U_prev, double *Q,
                 double *R, double *X_ref, double *U_ref, double *lx, double *ux, double *lu, double *uu,
                 double reg_x, double reg_u, double *slew_reg, double *slew_reg0, double *slew_um1,
                 long long verbose);

/* replaces PMPC.jl/src/c_interface.jl:146-214 (prototype: module.cpp:17-23).
 * Minimises the reference's epsilon-anchored epigraph objective (main.jl:204-238, k = M) — see
 * pmpc_lcone_solve_device below.  smooth_alpha = NaN => hard boxes (main.jl:242-244); finite => the boxes enter as
 * -1/alpha sum log(alpha slack) (smooth_cstr = "logbarrier", main.jl:246-262).  `solver` ("ecos" | "cosmo" | "mosek" |
 * "gurobi") only selects the conic back end upstream; all share one optimum (DESIGN.md section 2 notes the one
 * exception, the reference's exponential-cone row order under "ecos", which is not reproduced). */
void c_lcone_solve(double *X_out, double *U_out, size_t xdim, size_t udim, size_t N, size_t M, long long Nc,
                   double *x0, double *f, double *fx, double *fu, double *X_prev, double *U_prev, double *Q,
                   double *R, double *X_ref, double *U_ref, double *lx, double *ux, double *lu, double *uu,
                   double reg_x, double reg_u, double *slew_reg, double *slew_reg0, double *slew_um1,
                   long long verbose, double smooth_alpha, char *solver);

/* Extensions (not in the reference): the two entry points above for callers that hold fx, fu, Q, R as ROW-major blocks —
 * numpy's C-ordered (M, N, row, col) stacks, which the reference's Python side transposes on the host on every call to
 * reach the column-major layout (pmpc/static_backend.py:83-101 via pybind11's f_style cast: ~630 MB at M = 4096, the
 * dominant cost of the call once the solve runs on the GPU).  Bit k of `rowmajor` marks fx (0), fu (1), Q (2), R (3) as
 * row-major; everything else is as above.  The transposition is done in HBM after the upload. */
void pmpc_lqp_solve_host(double *X_out, double *U_out, size_t xdim, size_t udim, size_t N, size_t M, long long Nc,
                         double *x0, double *f, double *fx, double *fu, double *X_prev, double *U_prev, double *Q,
                         double *R, double *X_ref, double *U_ref, double *lx, double *ux, double *lu, double *uu,
                         double reg_x, double reg_u, double *slew_reg, double *slew_reg0, double *slew_um1,
                         long long verbose, unsigned rowmajor);
void pmpc_lcone_solve_host(double *X_out, double *U_out, size_t xdim, size_t udim, size_t N, size_t M, long long Nc,
                           double *x0, double *f, double *fx, double *fu, double *X_prev, double *U_prev, double *Q,
                           double *R, double *X_ref, double *U_ref, double *lx, double *ux, double *lu, double *uu,
                           double reg_x, double reg_u, double *slew_reg, double *slew_reg0, double *slew_um1,
                           long long verbose, double smooth_alpha, unsigned rowmajor, long long cone_k);
/* (cone_k: the reference's `k` setting, see pmpc_problem.cone_k; <= 0 = M) */
/* ... and with `smooth_cstr` (0 logbarrier, 1 squareplus) / `smooth_beta` (see pmpc_problem.smooth_cstr) */
void pmpc_lcone_solve_host_ex(double *X_out, double *U_out, size_t xdim, size_t udim, size_t N, size_t M, long long Nc, double *x0, double *f,
                              double *fx, double *fu, double *X_prev, double *U_prev, double *Q, double *R, double *X_ref, double *U_ref, double *lx,
                              double *ux, double *lu, double *uu, double reg_x, double reg_u, double *slew_reg, double *slew_reg0, double *slew_um1,
                              long long verbose, double smooth_alpha, unsigned rowmajor, long long cone_k, int smooth_cstr, double smooth_beta);

/* ---------------------------------------------------------------------------------------------
 * Part 2 — device-resident extension
 * ------------------------------------------------------------------------------------------- */

/* flags for pmpc_problem.flags */
#define PMPC_HAS_XBOUNDS 1u  /* lx/ux valid (no NaN sentinel) */
#define PMPC_HAS_UBOUNDS 2u  /* lu/uu valid */
#define PMPC_HAS_SLEW 4u     /* slew_reg valid (else treated as 0) */
#define PMPC_HAS_SLEW0 8u    /* slew_reg0 and slew_um1 valid */
#define PMPC_FORCE_GENERIC 16u /* debugging: never take the MFMA fast path */
#define PMPC_SYMMETRIC_COST 32u /* caller guarantees Q_j == Q_j' and R_j == R_j' exactly (OSQP keeps
                                   triu(P); the register-resident path relies on symmetric blocks) */

#define PMPC_COLD_START 64u /* do not start the interior-point iteration from the iterate remembered from the previous
                               solve of the same shape (see "warm start" in DESIGN.md section 2) */
#define PMPC_STATIC_CONS_BOUNDS 128u /* the caller guarantees that the CONTENTS of lu / uu (same device arrays) are those of the
                                       previous solve of this shape, as inside an SCP loop (pmpc/scp_mpc.py passes the same
                                       u_l / u_u every iteration).  The library then reuses (a) its working copy of the control
                                       boxes (the caller's, with global particle 0's on the consensus stages) and (b), sharded,
                                       the consensus bounds it broadcast then instead of two collectives per solve.  This
                                       promise is NOT checked on the device: a caller that changes lu / uu in place between
                                       solves (a moving trust region) must leave the flag off. */
#define PMPC_PREV_IS_LAST_SOLUTION 256u /* the caller guarantees that X_prev / U_prev ARE the X_out / U_out of the previous solve
                                          of this shape, as in an SCP loop (pmpc/scp_mpc.py:313,430: X_prev, U_prev = X, U).
                                          A warm-started solve then takes the linearisation point itself as its first base
                                          point — its dynamics defect is f - X_prev, elementwise — instead of rolling the old
                                          controls out again (one sequential sweep less).  Checked on the device (U_prev must be
                                          the base point of the stored set under the boxes this solve uses): a broken promise
                                          costs time, not correctness. */

#define PMPC_CONE_OBJECTIVE 1024u /* pmpc_scp_loop_device only: the sub-problem of every iteration is the reference's DEFAULT solver path
                                    (solver = "ecos" -> c_lcone_solve, pmpc/static_backend.py:242-253: the eps-anchored epigraph objective of
                                    PMPC.jl/src/main.jl:204-238; barrier_mu > 0: log-barrier smoothing with alpha = 1 / barrier_mu) instead of
                                    the QP of c_lqp_solve */
#define PMPC_F32_MATRICES 512u /* fp32-STORAGE mode (BASELINE config E's "fp32"; the reference is fp64-only, c_interface.jl:6-25): fx, fu,
                                 Q, R point to FLOAT arrays of the same layouts (cast to const double * in the struct).  The
                                 active-set sweeps of an SCP loop's warm-started solves (control boxes and / or stage cones,
                                 Nc <= 1) then stream half the bytes of the dominant arrays and keep their factor records in
                                 fp32; every value is widened on load and ALL arithmetic stays fp64, so the solve is the exact
                                 solve of the fp32-rounded data.  Every other path (cold start, fallbacks, other dims) widens the
                                 four arrays into workspace copies first and runs the fp64 kernels. */

typedef struct pmpc_problem {
  size_t xdim, udim, N, M; /* M = particles held by THIS rank */
  long long Nc;
  unsigned flags;
  double reg_x, reg_u;
  /* device pointers, ABI layouts above; unused ones may be NULL */
  const double *x0, *f, *fx, *fu, *X_prev, *U_prev, *Q, *R, *X_ref, *U_ref;
  const double *lx, *ux, *lu, *uu;
  const double *slew_reg, *slew_reg0, *slew_um1;
  double *X_out, *U_out; /* device, (xdim,N,M) / (udim,N,M) */
  /* optional per-particle cost weights, device (M): minimise sum_i weights_i J_i (the reference's `weights`
   * setting, PMPC.jl/src/main.jl:96-112, and the building block of the cone objective); NULL = all 1 */
  const double *weights;
  /* > 0: log-barrier smoothing of the boxes (the cone path's smooth_cstr = "logbarrier", cone_utils.jl:173-232): the
   * hard boxes are replaced by -barrier_mu * sum log(slack) in the objective, barrier_mu = 1/smooth_alpha; 0 = hard */
  double barrier_mu;
  /* optional second-order cone on the controls of EVERY (particle, stage):  || W u + w0 ||_2 <= v'u + v0  — the
   * structured case of the reference's pyjulia-only `extra_cstrs` (README.md:219-239; config E's thrust cones, SURVEY.md
   * section 8d), which cannot cross its C ABI.  soc_q = rows of W (0 = no cone); all four are DEVICE pointers, W (q x udim)
   * row-major.  soc_u_interior (device, udim): a control strictly inside the boxes and the cone (e.g. hover); the
   * path-following method starts from it on every stage.  Used by pmpc_lsoc_solve_device only. */
  size_t soc_q;
  const double *soc_W, *soc_w0, *soc_v;
  double soc_v0;
  const double *soc_u_interior;
  /* General form of the stage cones (pmpc_lsoc_solve_device; the structured case of the reference's `extra_cstrs` tuples,
   * PMPC.jl/src/main.jl:293-316, that stays inside ONE stage's controls): `cone_count` cones on the controls of every
   * (particle, stage); cone k has cone_sizes[k] + 1 rows — cone_sizes[k] = 0: a linear row s >= 0 (several of them: a
   * stage-wise polytope), >= 1: the second-order cone |s[1..]| <= s[0] —, s = A u + c with the rows of all cones stacked:
   * cone_A (rows x udim, row-major), cone_c (rows), both DEVICE pointers.  cone_per_stage = 0: one (A, c) for every stage;
   * 1: per (particle, stage) data, (M, N, rows, udim) / (M, N, rows) — the consensus stages use particle 0's.  cone_sizes is a
   * HOST array.  At most 4 cones, 8 rows, cone size <= 3.  cone_count = 0: the single cone soc_* above.  Solved by the
   * active-set rounds (kernels_cone.hip) from soc_u_interior (or from U_prev if that is NULL); the general form has no
   * path-following fallback: rounds that do not settle are a failed solve (status 1). */
  size_t cone_count;
  const int *cone_sizes;
  const double *cone_A, *cone_c;
  int cone_per_stage;
  /* cone path only (pmpc_lcone_solve_device): the reference's `k` setting (PMPC.jl/src/main.jl:204-227), the weight
   * (1 - eps) k of the epigraph offset t in  (1 + eps) sum_i y_i + (1 - eps) k t,  J_i <= y_i + t,  y >= 0.  k = M (the
   * default, and the only value its C ABI reaches) is the sum of the particle costs up to the eps-anchoring; k < M is a
   * worst-k objective: only about k (1 - eps) / (1 + eps) costliest particles carry weight.  <= 0 or >= M (all ranks' particles): k = M. */
  long long cone_k;
  /* cone path with smoothing (barrier_mu > 0 = 1 / smooth_alpha): the reference's `smooth_cstr` setting (PMPC.jl/src/main.jl:247-279) —
   * 0 "logbarrier" (the default): -(1/alpha) log(alpha slack) per box side; 1 "squareplus": soft boxes, every side a'z <= b costs
   * beta/2 (v + sqrt(v^2 + 1/alpha^2)), v = a'z - b (smooth_beta = beta, cone_utils.jl:222-228).  Pyjulia-only upstream. */
  int smooth_cstr;
  double smooth_beta;
} pmpc_problem;

typedef struct pmpc_info {
  int status;          /* 0 ok, 1 not converged (outputs NaN), 2 numerical failure (outputs NaN), 3 pmpc_lsoc_solve_device: infeasible start (outputs NaN) */
  int ipm_iters;       /* 0 = the equality-only optimum was feasible */
  int structured_solves; /* Riccati factorisations performed */
  int fast_path;       /* 1 = MFMA register-resident kernels were used; 2 = those kernels on fp32-stored matrices (PMPC_F32_MATRICES) */
  double mu;           /* final complementarity */
  double slack_res;    /* final slack residual (inf-norm) */
  double max_violation;/* bound violation of the equality-only optimum */
  int outer_solves;    /* cone path: weighted QPs solved (active-set + bisection on the threshold particle) */
  int active_set_rounds; /* structured solves spent in the active-set finish of the box interior-point iteration */
} pmpc_info;

/* Opaque solver context: owns the HIP stream, the workspace cache keyed on
 * (xdim,udim,N,M,Nc,flags) and the optional RCCL communicator. */
typedef struct pmpc_ctx pmpc_ctx;

int pmpc_create(pmpc_ctx **ctx, int device);          /* 0 on success */
void pmpc_destroy(pmpc_ctx *ctx);
/* Per-context algorithm switches (0 on success, -1 unknown key).  Every key has an environment variable of the same meaning that
 * sets its DEFAULT when a context is created (so a process-wide override still works): key / variable / default —
 *   as_warm PMPC_AS_WARM 1             warm start of the active-set rounds from the previous solve's set
 *   as_skip PMPC_AS_SKIP 1             settled particles skip the factor sweep of the later rounds
 *   as_defect PMPC_AS_DEFECT 1         no-rollout warm start under PMPC_PREV_IS_LAST_SOLUTION
 *   as_cold_rounds PMPC_AS_COLD 10     rounds of the cold start (0: interior-point iteration at once)
 *   polish_mu PMPC_POLISH_MU 1e-3      relative complementarity at which the interior-point iteration tries the rounds (0: rounds off altogether)
 *   warm_start PMPC_WARM_START 1       interior-point warm start from the remembered early iterate
 *   cone_as PMPC_CONE_AS 1             stage cones inside the rounds (0: path-following iteration)
 *   cone_cold_rounds PMPC_CONE_AS_COLD 16
 *   xbox_as PMPC_XBOX_AS 1             state boxes inside the rounds (0: a binding one sends the solve to the interior-point iteration)
 *   slew_increment_boxes PMPC_SLEW_INCREMENT_BOXES 1   boxed slew problems in increment form on the MFMA path (needs xbox_as)
 *   as_fuse_ctl PMPC_AS_FUSE_CTL 1, as_wave_cons PMPC_AS_WAVE_CONS 1   launch fusions of the rounds (measurement legs)
 *   host_reuse PMPC_HOST_REUSE 1       host ABI: unchanged 8 MB chunks are not uploaded again
 *   warn_slow_path PMPC_WARN_SLOW_PATH 1   one line on stderr when a context first leaves the register-resident path
 *   cone_rank_memory PMPC_CONE_RANK_MEMORY 1   cone objective: the weight assignment the previous solve of the shape settled on is tried first
 *   cone_epigraph    PMPC_CONE_EPIGRAPH    1   cone objective: hard boxes through the epigraph problem in the shared-control space, smoothing through the
 *                                             full-space Newton iteration (any tie pattern); 0: the rank-based weighted-QP iteration everywhere
 *   cond_grouped     PMPC_COND_GROUPED     1   Nc > 1: the condensed consensus Hessians are summed over groups of 8 particles inside the condensing
 *                                             kernel (no per-particle block travels through HBM) whenever nothing downstream needs one particle's block
 *   as_freeze_tol    PMPC_AS_FREEZE_TOL    1e-9  stage-cone rounds with one consensus stage: a step of the free shared controls below this (relative)
 *                                             is taken as zero by every particle, and the settled particles leave the forward sweep at once (0: off)
 *   as_ckpt          PMPC_AS_CKPT          1   the factor sweeps leave their cost-to-go at stages 4, 8, 16, 32, ..; an unsettled particle's factor sweep of a
 *                                             later round starts at the lowest of them at or above its highest changed stage (0: from the terminal cost)
 *   as_sens_min_m    PMPC_AS_SENS_MIN_M    3072  one consensus stage, at least this many particles on the rank: the forward sweep records the sensitivity
 *                                             of every stage to the shared-control step, and settled particles of the later rounds are updated elementwise
 *                                             from it instead of being swept again (0: never)
 *   as_perm_min_m    PMPC_AS_PERM_MIN_M    2048  from that many particles per rank a later round's launches take the UNSETTLED particles first: their long sweeps
 *                                             then spread one per SIMD instead of piling up where their indices fall (0: never)
 *   cone_path        PMPC_CONE_PATH        0   cone objective with hard boxes: which body answers.  0: automatic (the order depends on what the context learnt
 *                                             about the shape: free-particles body first where it worked before, else epigraph path, rank-based iteration,
 *                                             free-particles body last); 1: free-particles body first; 2: epigraph path, free-particles body never; 3: the
 *                                             rank-based weighted-QP iteration alone (two costs on the threshold at most)
 * Setting an option forgets the context's warm-start memory.  The reference has no counterpart (its solver settings travel in
 * `solver_settings`, pmpc/scp_mpc.py:45-66, and never reach the C ABI); kernel launch heuristics stay environment-only. */
int pmpc_set_option(pmpc_ctx *ctx, const char *key, double value);
int pmpc_get_option(pmpc_ctx *ctx, const char *key, double *value);
void *pmpc_stream(pmpc_ctx *ctx);                     /* hipStream_t the solver launches on */
void pmpc_sync(pmpc_ctx *ctx);                        /* hipStreamSynchronize(pmpc_stream) */

/* Solve with all buffers in HBM.  Asynchronous on pmpc_stream() except for one small
 * device->host read per IPM iteration.  Returns pmpc_info.status. */
int pmpc_lqp_solve_device(pmpc_ctx *ctx, const pmpc_problem *prob, pmpc_info *info, int verbose);

/* Cone-path objective of c_lcone_solve with every buffer in HBM (PMPC.jl/src/main.jl:194-354 through the C
 * ABI: k = M, no extra_cstrs): min (1+eps) sum_i y_i + (1-eps) M t  s.t.  J_i <= y_i + t, y >= 0, dynamics, boxes,
 * eps = 1e-3, J_i the particle cost of qp_utils.jl:60-162.  Eliminating (y, t) gives sum_i w_i J_i with w = 1+eps
 * above the threshold particle(s) — solved as a short sequence of weighted QPs.  smooth_alpha = NaN: hard boxes.
 * Sharded runs: equal particle counts per rank; the costs are gathered so that every rank ranks them identically. */
int pmpc_lcone_solve_device(pmpc_ctx *ctx, const pmpc_problem *prob, double smooth_alpha, pmpc_info *info, int verbose);

/* The QP of pmpc_lqp_solve_device plus the stage-wise control cones of pmpc_problem.soc_* (control boxes allowed, state
 * boxes / weights / slew not): feasible primal-dual path following with Nesterov-Todd scaling on the same Riccati
 * kernels, complementarity driven to 1e-12 and — where this iteration alone answers — five centring steps at that value (an
 * off-centre cone pair leaves the controls ~sqrt(mu) off, not ~mu).  Returns status (0 ok, 1 not converged, 2 numerical failure,
 * 3 infeasible start: soc_u_interior is not strictly inside the boxes and the cone — a point ON a box side or on the cone counts
 * as outside; X_out / U_out are filled with NaN as after every failed solve, and the context stays usable). */
int pmpc_lsoc_solve_device(pmpc_ctx *ctx, const pmpc_problem *prob, pmpc_info *info, int verbose);

/* J_out[i] (device, M) = J_i(X, U): per-particle cost of qp_utils.jl:60-162 (1/2 z'Pz + q'z + r), unweighted. */
int pmpc_particle_costs_device(pmpc_ctx *ctx, const pmpc_problem *prob, const double *X, const double *U, double *J_out);

/* Particle sharding over RCCL (one process per GPU).  unique_id is the 128-byte ncclUniqueId
 * produced by pmpc_comm_unique_id on rank 0 and distributed by the host (torch.distributed).
 * With a communicator set, pmpc_lqp_solve_device treats `M` as the local shard and
 * all-reduces the consensus Hessian/gradient and the IPM scalars. */
int pmpc_comm_unique_id(void *unique_id_128);
int pmpc_comm_init(pmpc_ctx *ctx, int rank, int world, const void *unique_id_128);
/* TEST HOOK (tests/test_multirank_gpu.py): an in-process stand-in for the communicator — `world` contexts on ONE device, one
 * host thread each, collectives staged through host memory — so that the world > 1 code paths run on a single-GPU box
 * (RCCL refuses two ranks on one device).  Not for production use. */
int pmpc_comm_init_mock(pmpc_ctx *ctx, int rank, int world, int group);
int pmpc_comm_rank(pmpc_ctx *ctx);
int pmpc_comm_world(pmpc_ctx *ctx);

/* On-device dynamics linearisation (row a2 of SURVEY.md §8: the f_fx_fu_fn callback for the
 * built-in models).  model: 0 = unicycle (reference tests/dubins_car.py:48-90, params (3,M)),
 * 1 = synthetic quadrotor (params (4,M) = [m, Jx, Jy, Jz]), 2 = kinematic bicycle, forward Euler: x = [px, py, theta, v],
 * u = [a, delta] (acceleration, steering angle), params (2,M) = [L, dt] (wheelbase, step):
 *   px+ = px + dt v cos(theta),  py+ = py + dt v sin(theta),  theta+ = theta + dt v tan(delta) / L,  v+ = v + dt a.
 * Any other id: nothing is launched, the call returns 2.  X_prev/U_prev/x0 and outputs in ABI layout. */
int pmpc_linearize_device(pmpc_ctx *ctx, int model, size_t N, size_t M, const double *x0, const double *X_prev,
                          const double *U_prev, const double *params, double *f, double *fx, double *fu);

/* Custom dynamics models: x+ = F(x, u; p) handed over as device code, compiled at run time with forward-mode automatic
 * differentiation for the Jacobians.  `source` is one function template,
 *   template <class T> __device__ void step(const T *x, const T *u, const double *p, T *xn);   // x[XD], u[UD], p[PD] -> xn[XD]
 * with XD, UD, PD defined as macros in front of it.  T is double (rollout, plan shift) or a dual number (linearisation) with
 * + - * / (also against double), unary minus, compound assignment, comparisons by value and
 * sin cos tan exp log sqrt tanh atan atan2 pow(T, double) fabs fmin fmax; at a kink the derivative is that of the value's branch.
 * The function sees per-thread arrays only.
 *   pmpc_model_compile  needs no context and no GPU.  arch: the target id, e.g. "gfx950" (a feature suffix after ':' is dropped).
 *                       0: *code (malloc'd, pmpc_model_free_code) holds *bytes of code object; 1: a bad argument (xdim, udim or pdim
 *                       outside 1 .. 16 — the solver's limits); 2: the runtime compiler (libhiprtc.so) is not available; 3: a compile
 *                       error.  log (log_cap bytes, may be NULL) receives the compiler's text, 0-terminated.
 *   pmpc_model_load     loads a code object on ctx's device and returns its model id >= PMPC_MODEL_CUSTOM0, or a negative value (-1 HIP
 *                       error, -2 bad argument, -3 not a code object of pmpc_model_compile for these dimensions).  The id is known to
 *                       this context only, until pmpc_model_unload (0; 2: not an id of this context) or pmpc_destroy.
 * A loaded id is taken by pmpc_linearize_device, pmpc_rollout_device, pmpc_shift_plan_device and the pmpc_scp_loop_device family
 * (params (M, pdim); dense fp64 Jacobians: refused like an unknown id next to PMPC_F32_MATRICES, and when xdim / udim are not the
 * problem's).  pmpc_linearize_device_f32 and the compact-record entry points know built-in ids only. */
#define PMPC_MODEL_CUSTOM0 1000
int pmpc_model_compile(const char *source, int xdim, int udim, int pdim, const char *arch, void **code, size_t *bytes, char *log,
                       size_t log_cap);
void pmpc_model_free_code(void *code);
int pmpc_model_load(pmpc_ctx *ctx, const void *code, size_t bytes, int xdim, int udim, int pdim);
int pmpc_model_unload(pmpc_ctx *ctx, int id);

/* the same with fx / fu written as FLOAT arrays (PMPC_F32_MATRICES) */
int pmpc_linearize_device_f32(pmpc_ctx *ctx, int model, size_t N, size_t M, const double *x0, const double *X_prev,
                              const double *U_prev, const double *params, double *f, float *fx, float *fu);

/* Nonlinear rollout of a built-in model: X[i, j] = F(X[i, j-1], U[i, j]; params[i]) with X[i, -1] = x0[i] — F is the `f` of
 * pmpc_linearize_device, evaluated alone.  x0 (M, xdim), U (M, N, udim), params (M, ·), X (M, N, xdim), all device, row-major.  A
 * dynamically feasible iterate for pmpc_scp_loop_device, a plant step (N = 1), the tail of a shifted plan.
 * Asynchronous on pmpc_stream().  Returns 0; 2 and launches nothing for an unknown model id, N == 0, M == 0 or a null pointer; 1 on a
 * HIP error. */
int pmpc_rollout_device(pmpc_ctx *ctx, int model, size_t N, size_t M, const double *x0, const double *U, const double *params, double *X);

/* Receding-horizon shift of a plan by s stages, 1 <= s < N, from (X, U) into (X_new, U_new) — never in place: the two trajectory
 * buffer pairs of pmpc_scp_loop_device are the intended source and target.
 *   U_new[i, j] = U[i, j + s],  X_new[i, j] = X[i, j + s]                               for j < N - s
 *   U_new[i, j] = U_tail[i, j - (N - s)]  (U_tail (M, s, udim); NULL: U[i, N - 1], hold) for j >= N - s
 *   X_new[i, j] = F(X_new[i, j - 1], U_new[i, j]; params[i])                            for j >= N - s
 *   um1_new[i]  = U[i, s - 1]  ((M, udim): the control that was applied, for pmpc_problem.slew_um1; NULL: not written)
 * One launch, asynchronous on pmpc_stream().  Returns 0; 2 and launches nothing for an unknown model id, N == 0, M == 0, s outside
 * 1 .. N - 1, X_new == X, U_new == U or a null pointer among the others; 1 on a HIP error.  Overlap beyond equal base pointers is
 * the caller's to avoid. */
int pmpc_shift_plan_device(pmpc_ctx *ctx, int model, size_t N, size_t M, size_t s, const double *X, const double *U,
                           const double *params, const double *U_tail, double *X_new, double *U_new, double *um1_new);

/* The control-box statuses of a plan moved s stages on together with its controls, 1 <= s < N, into the boxes of the stages they
 * arrive at (the boxes do not move with the horizon) — never in place.  act (M, N, udim) ints: 0 free, 1 on the lower, 2 on the upper
 * bound; U, lo, hi (M, N, udim) (lo / hi NULL: no bound on that side); Nc: consensus stages (< 0 or > N: N).  Entry (i, j, r):
 *   source  z = U[i, j + s, r], a = act[i, j + s, r]                                     for j < N - s
 *           z = U_tail[i, j - (N - s), r], a = 0  (U_tail (M, s, udim); NULL: stage N - 1 of U and act, hold)  for j >= N - s
 *           on a consensus stage j < Nc: particle 0's source, and l = lo[0, j, r], h = hi[0, j, r]; else l = lo[i, j, r], h = hi[i, j, r]
 *   l > h or z NaN:  U_new = z, act_new = 0   (the solve's own check refuses such a problem)
 *   else  zc = z < l ? l : (z > h ? h : z);  act_new = 1 if zc == l and (a == 1 or z < l), else 2 if zc == h and (a == 2 or z > h), else 0;
 *         U_new = zc
 * (U_new, act_new) is then a start the no-rollout warm start of the active-set rounds accepts: every held control exactly on its
 * bound, every free one inside its box, the consensus stages uniform over the particles.  pmpc_amd.dynamics.shift_active_set is the
 * specification.  One launch, asynchronous on pmpc_stream().  Returns 0; 2 and launches nothing for N == 0, M == 0, udim == 0, s
 * outside 1 .. N - 1, U_new == U, act_new == act or a null pointer among U, act, U_new, act_new; 1 on a HIP error. */
int pmpc_shift_active_set_device(pmpc_ctx *ctx, size_t N, size_t M, size_t udim, long long Nc, size_t s, const double *U,
                                 const double *U_tail, const int *act, const double *lo, const double *hi, double *U_new, int *act_new);

/* The same launch applied to the set the context's last accepted solve stored: its statuses are moved into a second buffer of the
 * workspace and the two are swapped; U is the plan BEFORE the shift (the source pair of pmpc_shift_plan_device), U_new the shifted
 * plan's controls (written behind that launch on the same stream), lo / hi the lu / uu of the problem.  The next
 * pmpc_scp_loop_device of this shape may then run with first_cold = 0: its first solve takes the warm path of every later one.
 * *shifted = 1 if a set of M N udim statuses was stored; else *shifted = 0, nothing is launched and U_new is untouched (no accepted
 * active-set solve since the context was made or since a solve that ended otherwise; a sharded context).  The stored solution, the
 * predicted round count and every other warm-start memory stay as they are: stage-cone, state-row and epigraph multipliers are NOT
 * moved — a caller with those keeps first_cold = 1.  Returns as above (2 also for shifted == NULL). */
int pmpc_warm_shift_device(pmpc_ctx *ctx, size_t N, size_t M, size_t udim, long long Nc, size_t s, const double *U, const double *U_tail,
                           const double *lo, const double *hi, double *U_new, int *shifted);

/* Copy of the stored statuses into act_out (n ints, device), for tests; asynchronous on pmpc_stream().  Returns 2 if nothing is stored
 * or the stored set does not hold n statuses. */
int pmpc_warm_set_read_device(pmpc_ctx *ctx, int *act_out, size_t n);

/* Compact Jacobian records of a built-in model — what pmpc_scp_loop_device writes into its fx scratch arrays instead of the dense
 * stacks when the coming solve is a warm attempt of the active-set rounds (PMPC_LIN_COMPACT=0 switches that off).  For tests and
 * tools: the linearisation into jc (pmpc_jac_compact_doubles(model, N, M) doubles; f dense), the expansion of jc into the dense
 * fx / fu (orient 0 / 1: through the part of the records the factor / the forward sweep reads; jc must not overlap fx, fu), and the
 * entries the records treat as live (host only, no device needed: fx_mask xdim*xdim, fu_mask xdim*udim bytes, column-major blocks as
 * in fx / fu; returns 100 xdim + udim, -1 for an unknown model). */
int pmpc_linearize_compact_device(pmpc_ctx *ctx, int model, size_t N, size_t M, const double *x0, const double *X_prev,
                                  const double *U_prev, const double *params, double *f, double *jc);
int pmpc_expand_jac_device(pmpc_ctx *ctx, int model, size_t N, size_t M, const double *jc, double *fx, double *fu, int orient);
long long pmpc_jac_compact_doubles(int model, size_t N, size_t M);
int pmpc_jac_live_mask(int model, unsigned char *fx_mask, unsigned char *fu_mask);

/* Which kernel variant an active-set sweep launch would take (pmpc_amd/csrc/as_variant.h) — host only, no device needed; for tests.
 * sweep 0: factor sweep, out[0..4] = {mode, skip, defect, ex, f32}; sweep 1: forward sweep, out[0..4] = {defect, pf2, cone, f32, sens}.
 * flags: which LQArgs fields the launch has set — bit 0 defect, 1 as_settled_in, 2 mat32, 3 cone_H, 4 xb_D, 5 as_uraw, 6 as_T.
 * knobs: {deep2_maxm, deep_maxm, fwd_pf2_maxm}, null = the defaults (the environment is not read).  out[5..7]: whether (xdim, udim)
 * has fp32-storage / cone / state-box sweeps at all (what the solver asks before it sets mat32 / cone_H, as_uraw / xb_D).
 * Returns 1 if the variant is compiled for (xdim, udim), 0 if not, -1 if the pair has no active-set sweeps. */
int pmpc_as_sweep_variant(int sweep, int xdim, int udim, int M, int Nc, unsigned flags, const int *knobs, int *out);

/* Registers and scratch of ONE compiled instantiation of a sweep, as the loaded code object states them (hipFuncGetAttributes: needs a
 * device, launches nothing) — for the test that keeps the sweeps on their occupancy step (tests/test_as_resources_gpu.py).  sweep and
 * variant[0..4]: the record pmpc_as_sweep_variant writes to out[0..4].  out[0..3] = {vector registers per lane (the unified file:
 * architectural + accumulation), scratch ("local") bytes per lane, static LDS bytes, max threads per block}.  Returns 0, -1 for an
 * unknown sweep or a pair without active-set sweeps, -2 if the variant is not compiled for the pair, else the HIP error code. */
int pmpc_as_sweep_resources(int sweep, int xdim, int udim, const int *variant, int *out);

/* How often each variant of a sweep has been launched by this process (every context and dims pair together) since it started or
 * since the last call with reset != 0 — host-side counts of the launcher, for tests that must know which instantiations a solve ran
 * (tests/test_as_variants_gpu.py).  The count of a variant stands at the code of its record:
 *   sweep 0 (factor sweep, 72 codes):  mode + 3 * (skip + 2 * (defect + 2 * (ex + 3 * f32)))
 *   sweep 1 (forward sweep, 32 codes): defect + 2 * pf2 + 4 * cone + 8 * f32 + 16 * sens
 * Writes the first min(n, codes) counts to out (may be NULL), zeroes all counts if reset != 0, returns the number of codes (-1 for
 * an unknown sweep).  A launch is counted when it is enqueued: rounds are enqueued ahead and a sweep that finds the device-side
 * `done` flag set returns at once, so a count says that the instantiation ran, not that it had work to do.
 * pmpc_as_sweep_knobs: out[0..2] = {deep2_maxm, deep_maxm, fwd_pf2_maxm} as this process's launchers read them (PMPC_AS_DEEP2_MAXM,
 * PMPC_AS_DEEP_MAXM, PMPC_AS_FWD_PF2_MAXM; read once per process, at the first launch or this call). */
int pmpc_as_sweep_launches(int sweep, unsigned long long *out, int n, int reset);
void pmpc_as_sweep_knobs(int *out);

/* The same count for the kernels that answer when the active-set rounds do not — the sweeps of the equality solve and of the
 * interior-point iteration (kernels_fast.hip), the condensing kernels and the dense consensus solve —, for the tests that must know
 * which of them a solve ran (tests/test_ipm_dims_gpu.py).  Host-side, every context and dims pair together, counted when enqueued:
 *   kind 0 (k_bwd_fast, 16 codes):      factor + 2 * hxb + 4 * hub + 8 * deep   (factor 0: the vector-only sweep)
 *   kind 1 (condensing, 2 codes):       0 k_cond_fast, 1 k_cond_fast_grouped
 *   kind 2 (launch_cons_solve, 10 codes): variant + 5 * factor, variant 0 k_cons_solve, 1 k_cons_solve_blocked, 2 k_cons_solve_lds,
 *                                       3 k_cons_solve_reg<12>, 4 k_cons_solve_reg<17> (the last two only factor)
 * Kinds 0 and 1 are launches of the register-resident path only.  Kind 2 counts EVERY call of launch_cons_solve — the active-set
 * rounds' and the generic kernels' solves too (both paths share the dense consensus solve) —, so a test that reads it runs nothing
 * else between its reset and its reading.
 * Writes the first min(n, codes) counts to out (may be NULL), zeroes the kind's counts if reset != 0, returns the number of codes
 * (-1 for an unknown kind). */
int pmpc_fast_launches(int kind, unsigned long long *out, int n, int reset);

/* SCP residual of one iteration (pmpc/scp_mpc.py:397-403): *out (device, one double) = max over particles and stages of
 * ||X - X_prev||_2 and ||U - U_prev||_2 (inf if a trajectory holds a NaN); asynchronous on pmpc_stream(). */
int pmpc_scp_residual_device(pmpc_ctx *ctx, size_t xdim, size_t udim, size_t N, size_t M, const double *X, const double *X_prev,
                             const double *U, const double *U_prev, double *out);

/* `steps` iterations of the SCP loop (pmpc/scp_mpc.py:337-430) for a built-in dynamics model with the host out of the loop
 * body: per iteration  linearise about (X_prev, U_prev) -> convex sub-problem (pmpc_lqp_solve_device semantics, or
 * pmpc_lsoc_solve_device if p->soc_u_interior is set) -> SCP residual -> (X_prev, U_prev) <- (X, U).
 *   p          the sub-problem; p->X_prev / p->U_prev hold the start iterate (and are OVERWRITTEN: the two trajectory buffer
 *              pairs (X_prev, U_prev) and (X_out, U_out) swap roles every iteration), p->f / fx / fu are scratch the
 *              linearisation writes (device, caller-allocated), f2 / fx2 / fu2 a second set of the same sizes: the next
 *              linearisation is enqueued behind the sub-problem's rounds BEFORE the host knows they sufficed (if they did
 *              not, it is redone), and must not touch what a continued solve still reads.  What the scratch sets hold on return is
 *              unspecified: for warm solves the loop keeps compact Jacobian records in fx and leaves fu unwritten (see above)
 *   first_cold non-zero: X_prev / U_prev of the first iteration are not the previous solve's outputs (no warm-start promise)
 *   res        device, `steps` doubles: the residual of each iteration (max over ranks when sharded)
 *   infos      host, `steps` entries (may be NULL)
 * The final iterate is in (X_out, U_out) if `steps` is odd, else in (X_prev, U_prev); *last_in_out says which.  Returns the
 * number of iterations completed (== steps unless a sub-problem failed: its status is in infos[returned]; an unknown model
 * id fails the same way, before anything runs: 0, infos[0].status = 2).  The compact records are those of `model`: two models
 * with the same dimensions (0 and 2) keep their own layouts on one context. */
int pmpc_scp_loop_device(pmpc_ctx *ctx, int model, const double *params, const pmpc_problem *p, double *f2, double *fx2, double *fu2,
                         int steps, int first_cold, double *res, pmpc_info *infos, int *last_in_out);

/* Linearised nonlinear costs (the reference's `lin_cost_fn`, pmpc/scp_mpc.py:171-185, 352: the callback returns the cost gradients
 * (cx, cu) at (X_prev, U_prev) and the loop tracks X_ref - Q^-1 cx, U_ref - R^-1 cu for that iteration).
 *
 * pmpc_ref_shift_device: out[r] = ref[r] - A[r]^-1 c[r] for `rows` independent blocks — A (rows, dim, dim) symmetric positive definite
 * blocks in the column-major block layout above (Q with dim = xdim, rows = M N; R with dim = udim), c, ref, out (rows, dim); out may
 * be ref.  Cholesky and two triangular solves per block, fp64; only the lower triangle (row >= column) of a block is read.  A block
 * with a pivot that is not positive (or NaN) gets NaN in its row of `out` and counts in pmpc_ref_shift_bad_pivots; the other rows
 * are not affected.  Asynchronous on pmpc_stream().  Returns 0; 2 and launches nothing if dim is 0 or above 16; 1 on a HIP error.
 * pmpc_ref_shift_bad_pivots: blocks refused since the context was created or the count was last reset (synchronises the stream). */
int pmpc_ref_shift_device(pmpc_ctx *ctx, size_t dim, size_t rows, const double *A, const double *c, const double *ref, double *out);
long long pmpc_ref_shift_bad_pivots(pmpc_ctx *ctx, int reset);

/* A built-in cost for loops that have no Python callable.  kind 1, obstacles: K <= 16 Gaussian bumps shared by all particles,
 *   J_obs = sum_{i,j} sum_k w_k exp(-|x_ij[pos_idx] - c_jk|^2 / (2 sigma_k^2)),
 * x_ij = stage j (0-based: the state after j + 1 steps, row j of X_prev) of particle i; pos_idx: pos_dim = 2 or 3 state indices;
 * centres (device): (K, pos_dim) if per_stage = 0, (N, K, pos_dim) if 1 (moving obstacles); sigma, w (device): (K).
 *
 * kind 2, custom: a runtime-compiled stage cost loaded on the context (pmpc_cost_load below) — `id` its id, `uses_u` as it was compiled,
 * `cparams` (device) its parameters (M, cdim).  The three members share the storage of K, pos_dim and centres, which kind 2 does not
 * use: the struct keeps its size and the offsets of kind 1.  pmpc_obstacle_cost_grad_device / pmpc_obstacle_ref_shift_device answer
 * kind 2 with 2. */
typedef struct pmpc_scp_cost {
  int kind; /* 0 none, 1 obstacles, 2 custom */
  union { int K; int id; };
  union { int pos_dim; int uses_u; };
  int pos_idx[3];
  int per_stage;
  union { const double *centres; const double *cparams; };
  const double *sigma, *w;
} pmpc_scp_cost;
size_t pmpc_abi_scp_cost_size(void); /* sizeof(pmpc_scp_cost) as the library was built (see pmpc_abi_struct_sizes) */

/* cx (device, (xdim, N, M), dense: zero outside pos_idx) = gradient of J_obs at X_prev.  Returns 0; 2 and launches nothing for a cost
 * that is not a valid kind-1 description for this xdim (K, pos_dim, pos_idx out of range, xdim above 16, a null pointer). */
int pmpc_obstacle_cost_grad_device(pmpc_ctx *ctx, const pmpc_scp_cost *cost, size_t xdim, size_t N, size_t M, const double *X_prev,
                                   double *cx);
/* The two in one launch, cx never stored: out = X_ref - Q^-1 cx(X_prev) (out may be X_ref); what pmpc_scp_loop_device_cost enqueues. */
int pmpc_obstacle_ref_shift_device(pmpc_ctx *ctx, const pmpc_scp_cost *cost, size_t xdim, size_t N, size_t M, const double *X_prev,
                                   const double *Q, const double *X_ref, double *out);

/* pmpc_scp_loop_device with a built-in cost (`cost` NULL or kind 0: exactly pmpc_scp_loop_device, launch for launch).  Every
 * iteration's sub-problem tracks X_ref - Q^-1 cx(X_prev) instead of p->X_ref; the shifted reference lives in the context's
 * workspace, two sets of (xdim, N, M) used like the linearisation scratch sets: each linearisation launch — the speculative one
 * behind a sub-problem's rounds included — is followed by the shift into the set that goes with it, so a solve that continues never
 * sees its reference change.  p->X_ref is not written.  Q must hold symmetric positive definite blocks (a block that is not makes
 * its reference NaN, and the sub-problem fails).  Refused before anything runs (0, infos[0].status = 2, as for an unknown model
 * id): an invalid cost description, and a cost together with PMPC_F32_MATRICES (the shift reads Q as doubles). */
int pmpc_scp_loop_device_cost(pmpc_ctx *ctx, int model, const double *params, const pmpc_problem *p, double *f2, double *fx2,
                              double *fu2, int steps, int first_cold, double *res, pmpc_info *infos, int *last_in_out,
                              const pmpc_scp_cost *cost);

/* Custom stage costs: J = sum over particles i and stages j of stage_cost(X[i,j], U[i,j], p_i, j, N), handed over as device code and
 * compiled at run time like a custom model; the gradients (cx, cu) come from forward-mode dual numbers.  `source` is one function template,
 *   template <class T> __device__ T stage_cost(const T *x, const T *u, const double *p, int j, int N);
 * x[XD] = row j of X_prev, u[UD] = row j of U_prev (0-based stage j: the state after j + 1 steps and the control that led to it),
 * p[CD] = this particle's cost parameters, with XD, UD, CD defined as macros in front of it.  T is double or a dual number with the
 * operator and function set of the custom models (above).  p points into global memory (it is not copied per thread): CD may be 1 .. 64;
 * XD, UD in 1 .. 16.  uses_u = 0 promises d/du == 0: cu is not formed, and the loops neither shift U_ref nor read R.
 *   pmpc_cost_compile   as pmpc_model_compile (no context, no GPU): 0 / 1 bad argument / 2 no runtime compiler / 3 compile error;
 *                       pmpc_model_free_code frees *code.
 *   pmpc_cost_load      returns the cost's id >= PMPC_COST_CUSTOM0, or -1 / -2 / -3 as pmpc_model_load.  Costs have a table of their
 *                       own: an id means a cost only where a cost is asked for, it is known to the context that loaded it, until
 *                       pmpc_cost_unload (0; 2: not a cost id of this context) or pmpc_destroy.  A cost and a model are separate
 *                       modules: unloading one leaves the other.
 *   pmpc_custom_cost_grad_device   cx (M, N, xdim), cu (M, N, udim; NULL for a cost compiled with uses_u = 0, which never writes it),
 *                       val (M, N) stage values or NULL, at (X_prev, U_prev), cparams (M, cdim): one launch, asynchronous on
 *                       pmpc_stream().  0; 1 HIP error; 2 and nothing launched: id not of this context, null cx, null cu for a cost
 *                       that uses u.
 * In the pmpc_scp_loop_device family a kind-2 pmpc_scp_cost enqueues behind every linearisation launch (the speculative one included)
 * the gradient kernel into one workspace scratch (cx | cu), pmpc_ref_shift on Q into the X_ref set of that launch and — unless uses_u
 * is 0 — pmpc_ref_shift on R into a U_ref set kept the same way; p->X_ref / p->U_ref are not written; blocks of Q and R that are not
 * positive definite count in pmpc_ref_shift_bad_pivots.  Refused before anything runs (0, infos[0].status = 2): an id that is not this
 * context's, dimensions that are not the problem's, null cparams, PMPC_F32_MATRICES, and a null p->X_ref (or p->U_ref with uses_u):
 * the shift reads the reference it moves. */
#define PMPC_COST_CUSTOM0 1000
int pmpc_cost_compile(const char *source, int xdim, int udim, int cdim, int uses_u, const char *arch, void **code, size_t *bytes, char *log,
                      size_t log_cap);
int pmpc_cost_load(pmpc_ctx *ctx, const void *code, size_t bytes, int xdim, int udim, int cdim, int uses_u);
int pmpc_cost_unload(pmpc_ctx *ctx, int id);
int pmpc_custom_cost_grad_device(pmpc_ctx *ctx, int id, size_t N, size_t M, const double *X_prev, const double *U_prev, const double *cparams,
                                 double *cx, double *cu, double *val);

/* A built-in constraint for loops that have no Python callable.  kind 1, keep-out: every stage j = 0 .. N-1 (0-based: the state after
 * j + 1 steps, row j of X_prev) of every particle i stays outside K balls, 1 <= K <= 4, in the position sub-space pos_idx (pos_dim = 2 or
 * 3 distinct state indices):  |X[i, j, pos_idx] - c_ijk| >= r_k.  About the previous iterate the SCP loop imposes the half-space
 *   n'(p - c) >= r,  n = (pbar - c) / |pbar - c|,  pbar = X_prev[i, j, pos_idx]   (n = the first position axis if |pbar - c| < 1e-12),
 * i.e. the row a_x'x <= h with a_x[pos_idx] = -n, h = -r - n'c; every point of it is outside the ball (Cauchy-Schwarz).
 * centres (device): centre k of (particle i, stage j) is at centres + i centre_stride_particle + j centre_stride_stage + k pos_dim
 * (strides in doubles, >= 0: (0, 0) static obstacles (K, pos_dim); (0, K pos_dim) moving ones (N, K, pos_dim); (N K pos_dim, K pos_dim)
 * per particle and stage (M, N, K, pos_dim)); radius (device): (K).
 *
 * kind 2, custom: a runtime-compiled state constraint loaded on the context (pmpc_cstr_load below) — `K` its row count as it was
 * compiled, `id` its id, `gparams` (device) its parameters (M, pdim).  id and gparams share the storage of pos_dim and centres, which
 * kind 2 does not use: the struct keeps its size and the offsets of kind 1.  pmpc_keepout_augment_device answers kind 2 with 2. */
typedef struct pmpc_scp_cstr {
  int kind; /* 0 none, 1 keep-out, 2 custom */
  int K;
  union { int pos_dim; int id; };
  int pos_idx[3];
  long long centre_stride_particle, centre_stride_stage;
  union { const double *centres; const double *gparams; };
  const double *radius;
} pmpc_scp_cstr;
size_t pmpc_abi_scp_cstr_size(void); /* sizeof(pmpc_scp_cstr) as the library was built (see pmpc_abi_struct_sizes) */

/* The linearised problem with the K rows of every (particle, stage) restated as upper bounds on K auxiliary states that the linearised
 * dynamics produce (state dimension xd = xdim + K; pmpc_amd/extra_cstrs.py keepout_augment is the specification), one launch:
 *   f_aug (M, N, xd)          [f | a_k'f]                       X_prev_aug (M, N, xd)  [X_prev | 0]
 *   fx_aug (M, N, xd, xd)     rows >= xdim: a_k'fx, columns >= xdim: 0     X_ref_aug (M, N, xd)   [X_ref | 0]; not written if X_ref is NULL
 *   fu_aug (M, N, udim, xd)   rows >= xdim: a_k'fu              xu_aug (M, N, xd)      entries xdim + k <- h_k; the first xdim are NOT written
 * in the layouts above (blocks column-major).  The parts that do not change with the iterate (Q with -reg_x on the auxiliary diagonal,
 * x0, the lower bounds -inf, the first xdim upper bounds) are the caller's.  Inputs and outputs must not overlap.  Asynchronous on
 * pmpc_stream().  Returns 0; 2 and launches nothing for K outside 1 .. 4, a bad pos_dim or pos_idx, xdim + K > 16, udim outside
 * 1 .. 16, a negative stride, N == 0, M == 0 or a null pointer (X_ref may be NULL, and X_ref_aug with it); 1 on a HIP error. */
int pmpc_keepout_augment_device(pmpc_ctx *ctx, const pmpc_scp_cstr *cstr, size_t xdim, size_t udim, size_t N, size_t M,
                                const double *X_prev, const double *f, const double *fx, const double *fu, const double *X_ref,
                                double *f_aug, double *fx_aug, double *fu_aug, double *X_prev_aug, double *X_ref_aug, double *xu_aug);

/* The way back from a sub-problem at xd = xdim + K states, one launch: X (M, N, xdim) <- the first xdim entries of every row of X_aug
 * (M, N, xd), and *out (device) <- the SCP residual of (X, X_prev), (U, U_prev) exactly as pmpc_scp_residual_device gives it for the
 * stripped array (the same sums in the same order; *out is zeroed first).  X_aug and X must not overlap.  Asynchronous on pmpc_stream().
 * Returns 0; 2 and launches nothing for a null pointer, K outside 1 .. 4, xdim + K > 16, udim outside 1 .. 16, N == 0 or M == 0; 1 on a
 * HIP error. */
int pmpc_keepout_strip_residual_device(pmpc_ctx *ctx, size_t xdim, int K, size_t udim, size_t N, size_t M, const double *X_aug, double *X,
                                       const double *X_prev, const double *U, const double *U_prev, double *out);

/* The buffers of pmpc_scp_loop_device_cstr at xd = xdim + K states (device, caller-allocated once; the library allocates nothing per call
 * and writes none of the static parts).  Static, the caller's: Q (M, N, xd, xd) = the problem's blocks with -reg_x on the auxiliary
 * diagonal, x0 (M, xd) = [x0 | 0], lx (M, N, xd) = [lx or -inf | -inf], and the first xdim entries of every row of BOTH xu arrays
 * (ux or +inf; no NaN).  Iterate-dependent, two sets used like the linearisation scratch sets (the augmentation enqueued behind a
 * sub-problem's rounds writes the set the running solve does not read): f, X_prev, X_ref, xu (M, N, xd), fx (M, N, xd, xd),
 * fu (M, N, udim, xd) — the loop writes all of them but the first xdim entries of xu's rows.  X_out (M, N, xd): the sub-problem's output. */
typedef struct pmpc_scp_aug {
  const double *Q, *x0, *lx;
  double *f[2], *fx[2], *fu[2], *X_prev[2], *X_ref[2], *xu[2];
  double *X_out;
} pmpc_scp_aug;
size_t pmpc_abi_scp_aug_size(void); /* sizeof(pmpc_scp_aug) as the library was built (see pmpc_abi_struct_sizes) */

/* pmpc_scp_loop_device_cost with a built-in constraint (`cstr` NULL or kind 0: exactly pmpc_scp_loop_device_cost, launch for launch;
 * `aug` is not read then).  With a keep-out constraint an iteration is: dense linearisation at xdim about (X_prev, U_prev) (no compact
 * records) -> the cost's shift, if any -> pmpc_keepout_augment_device's launch into set `cur` of `aug` (its X_ref: this iteration's
 * shifted reference) -> the sub-problem at xd states on aug's Q, x0, lx, xu[cur] with PMPC_PREV_IS_LAST_SOLUTION off in every iteration
 * (X_prev~ holds zeros where the last output holds the rows' values), X_out = aug->X_out, U_out = the loop's -> strip + residual
 * (pmpc_keepout_strip_residual_device's launch) -> swap.  The trajectory pairs, res, infos, *last_in_out and the return value are
 * pmpc_scp_loop_device's, at xdim; on a HIP error aug->X_out is filled with NaN along with the pairs.  Behind a sub-problem's first
 * batch of rounds the loop enqueues the strip, the residual, the next linearisation, its shift and its augmentation (into the other set);
 * if the rounds did not suffice the strip and the residual are redone from the finished output.
 * Refused before anything runs (0, infos[0].status = 2): an invalid description, xdim + K > 16, a null `aug` or a null pointer in it,
 * a stage cone (soc_u_interior / cone_count), PMPC_HAS_SLEW / PMPC_HAS_SLEW0, PMPC_F32_MATRICES, a sharded context, smooth_cstr = 1. */
int pmpc_scp_loop_device_cstr(pmpc_ctx *ctx, int model, const double *params, const pmpc_problem *p, double *f2, double *fx2,
                              double *fu2, int steps, int first_cold, double *res, pmpc_info *infos, int *last_in_out,
                              const pmpc_scp_cost *cost, const pmpc_scp_cstr *cstr, const pmpc_scp_aug *aug);
/* Custom state constraints: g_k(X[i,j]; p_i, j, N) <= 0, k < kdim, on every stage j = 0 .. N-1 (0-based: the state after j + 1 steps, row
 * j of X_prev) of every particle i, handed over as device code and compiled at run time like a custom model or cost.  `source` is one
 * function template,
 *   template <class T> __device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g);
 * x[XD] = the state, p[PD] = this particle's parameters (global memory), g[KD] = the values it writes, with XD, KD, PD defined as macros
 * in front of it; T is double or a dual number with the operator and function set of the custom models.  Limits: XD >= 1, KD in 1 .. 4,
 * XD + KD <= 16, PD in 1 .. 64.  About xbar = X_prev[i, j] the SCP loop imposes the rows a_k'x <= h_k, a_k = grad g_k(xbar),
 * h_k = a_k'xbar - g_k(xbar), the gradients by forward-mode dual numbers.
 *   pmpc_cstr_compile   as pmpc_cost_compile (no context, no GPU): 0 / 1 bad argument / 2 no runtime compiler / 3 compile error;
 *                       pmpc_model_free_code frees *code.
 *   pmpc_cstr_load      returns the constraint's id >= PMPC_CSTR_CUSTOM0, or -1 / -2 / -3 as pmpc_model_load.  Constraints have a table
 *                       of their own, apart from the models' and the costs'; an id is known to the context that loaded it, until
 *                       pmpc_cstr_unload (0; 2: not a constraint id of this context) or pmpc_destroy.
 *   pmpc_custom_cstr_rows_device   a (M, N, K, xdim), h (M, N, K), g (M, N, K) values or NULL, at X_prev (M, N, xdim), gparams (M, pdim):
 *                       one launch, asynchronous on pmpc_stream().  A row whose g_k or gradient holds a non-finite entry gets
 *                       h = +inf and a = 0 (no constraint; never a NaN, the "no state bounds" sentinel of an upper bound) and counts in
 *                       pmpc_cstr_bad_rows.  0; 1 HIP error; 2 and nothing launched: id not of this context, a null pointer (g may be
 *                       NULL), N == 0, M == 0.
 *   pmpc_rows_augment_device   pmpc_keepout_augment_device for K dense rows a (M, N, K, xdim), h (M, N, K) per unit instead of the ball
 *                       geometry: the same outputs in the same layouts (xu_aug: entries xdim + k <- h_k, the first xdim NOT written).
 *                       0; 1 HIP error; 2 and nothing launched: K outside 1 .. 4, xdim + K > 16, udim outside 1 .. 16, N == 0, M == 0,
 *                       a null pointer (X_ref may be NULL, and X_ref_aug with it).
 *   pmpc_cstr_bad_rows  rows refused since the context was created or the count was last reset (synchronises the stream).
 * In pmpc_scp_loop_device_cstr a kind-2 pmpc_scp_cstr enqueues behind every linearisation launch and its shift the rows kernel into a
 * workspace scratch and pmpc_rows_augment_device's launch into set `cur` of `aug`; everything else is the keep-out loop's.  Refused
 * before anything runs (0, infos[0].status = 2): what kind 1 is refused with, an id that is not this context's, a constraint whose xdim
 * or K is not the problem's / the descriptor's, null gparams. */
#define PMPC_CSTR_CUSTOM0 1000
int pmpc_cstr_compile(const char *source, int xdim, int kdim, int pdim, const char *arch, void **code, size_t *bytes, char *log, size_t log_cap);
int pmpc_cstr_load(pmpc_ctx *ctx, const void *code, size_t bytes, int xdim, int kdim, int pdim);
int pmpc_cstr_unload(pmpc_ctx *ctx, int id);
int pmpc_custom_cstr_rows_device(pmpc_ctx *ctx, int id, size_t N, size_t M, const double *X_prev, const double *gparams, double *a, double *h,
                                 double *g);
int pmpc_rows_augment_device(pmpc_ctx *ctx, int K, size_t xdim, size_t udim, size_t N, size_t M, const double *a, const double *h,
                             const double *X_prev, const double *f, const double *fx, const double *fu, const double *X_ref, double *f_aug,
                             double *fx_aug, double *fu_aug, double *X_prev_aug, double *X_ref_aug, double *xu_aug);
long long pmpc_cstr_bad_rows(pmpc_ctx *ctx, int reset);

/* Iterations of pmpc_scp_loop_device* in this process whose follow-up (residual, next linearisation) was taken as enqueued behind the
 * sub-problem's first batch of rounds (out2[0]) / was enqueued after the solve had returned (out2[1]); reset: start counting afresh. */
void pmpc_scp_loop_follow_ups(unsigned long long *out2, int reset);

/* Live kernel timing for bench.py: HIP events on pmpc_stream() around the launches of a class
 * (0 backward+factor, 1 backward vector-only, 2 forward, 3 consensus reduce+solve).
 * level 0 = off, 1 = class 0 only (the dominant kernel; what bench.py's roofline needs), 2 = every class
 * (each event pair costs a few microseconds of launch gap). */
void pmpc_profile_enable(pmpc_ctx *ctx, int level);
void pmpc_profile_read(pmpc_ctx *ctx, double *ms4, long long *n4);
/* Factor sweeps of active-set rounds that skip the settled particles are timed in a class of their own (level 2 only) and
 * never enter class 0, whose launches all process every (particle, stage): totals as of the last pmpc_profile_read. */
void pmpc_profile_read_partial(pmpc_ctx *ctx, double *ms, long long *n);
/* every launch class as of the last pmpc_profile_read: 0 full factor sweep, 1 vector sweep, 2 forward sweep, 3 consensus
 * reduce + solve, 4 factor sweeps that skip settled particles, 5 active-set bookkeeping, 6 linearisation (and the reference shift of a built-in cost), 7 SCP residual */
void pmpc_profile_read_all(pmpc_ctx *ctx, double *ms, long long *launches, int count);

/* Checkpointed restart of the later rounds' factor sweeps (option as_ckpt), counted since the last reset: out4 = {sweeps that
 * started from a checkpoint, stages they ran, sweeps of unsettled particles that started from the terminal cost, stages they ran}.
 * Synchronises the solver's stream.  For tests and bench.py (how much of the horizon the later rounds re-factorise). */
void pmpc_restart_stats(pmpc_ctx *ctx, unsigned long long *out4, int reset);

/* version / build probe used by the loader and the tests */
const char *pmpc_version(void);
/* sizeof(pmpc_problem), sizeof(pmpc_info) as the library was built: a binding that mirrors the structs compares them with its
 * own at load time and refuses a mismatch (a stale .so under a newer binding silently misreads the trailing fields) */
void pmpc_abi_struct_sizes(size_t *problem, size_t *info);

#ifdef __cplusplus
}
#endif
#endif /* PMPC_ABI_H */
