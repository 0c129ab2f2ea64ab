// solver.hip — host side of the device solver and the C ABI of include/pmpc_abi.h: contexts, options, profiling, the structured
// Newton solve, the thin device entries (one launch each) and the entry points of the QP path (fp32-storage protocol, slew increment
// form).  The solve itself — the phases below — is solver_qp.hip (QpSolve, one object per solve); the SCP loop around it is
// solver_scp.hip (ScpLoop), the communicators are comm.hip.
//
// One call = one convex sub-problem of the reference's SCP loop, i.e. what
// PMPC.jl/src/main.jl:115-171 `lqp_solve` does (assemble joint QP -> OSQP -> split), solved here as
//   1. equality-only optimum by ONE structured Newton step (Riccati + consensus condensing),
//   2. if a box constraint is violated: Mehrotra predictor-corrector on the boxes, each Newton
//      system being the same structured solve with modified diagonals.
// The only cross-particle (and therefore cross-GPU) data are the condensed consensus Hessian /
// gradient [Hc | gc] and a handful of IPM scalars -> RCCL all-reduce when a communicator is set.
#include "solver_internal.h"
#include "cost_lin.h"
#include "model_jit.h"
#include "cost_jit.h"
#include "cstr_jit.h"
#include "jit_module.h"

static const struct { const char *key, *env; double dflt; } kPmpcOptions[OPT_COUNT] = {
    {"as_warm", "PMPC_AS_WARM", 1},                // warm start of the active-set rounds from the previous solve's set
    {"as_skip", "PMPC_AS_SKIP", 1},                // settled particles skip the factor sweep of the later rounds
    {"as_defect", "PMPC_AS_DEFECT", 1},            // no-rollout warm start under PMPC_PREV_IS_LAST_SOLUTION
    {"as_cold_rounds", "PMPC_AS_COLD", 10},        // rounds of the cold start (0: straight to the interior-point iteration)
    {"polish_mu", "PMPC_POLISH_MU", 1e-3},         // relative complementarity at which the interior-point iteration tries the rounds (0: never; also switches the warm / cold starts off)
    {"warm_start", "PMPC_WARM_START", 1},          // interior-point warm start from the remembered early iterate
    {"cone_as", "PMPC_CONE_AS", 1},                // stage cones inside the rounds (0: path-following iteration)
    {"cone_cold_rounds", "PMPC_CONE_AS_COLD", 16}, // rounds of the cone cold start
    {"xbox_as", "PMPC_XBOX_AS", 1},                // state boxes inside the rounds (0: interior-point iteration when one binds)
    {"slew_increment_boxes", "PMPC_SLEW_INCREMENT_BOXES", 1},  // boxed slew problems in increment form on the MFMA path (needs xbox_as)
    {"as_fuse_ctl", "PMPC_AS_FUSE_CTL", 1},        // round control rides in the next round's consensus-partials launch
    {"as_wave_cons", "PMPC_AS_WAVE_CONS", 1},      // consensus system solved by every wave of the forward sweep
    {"host_reuse", "PMPC_HOST_REUSE", 1},          // host ABI: unchanged 8 MB chunks are not uploaded again
    {"warn_slow_path", "PMPC_WARN_SLOW_PATH", 1},  // one line on stderr when a context first leaves the register-resident path
    {"cone_rank_memory", "PMPC_CONE_RANK_MEMORY", 1},  // cone objective: the weight assignment the previous solve of the shape settled on is tried first
    {"cone_epigraph", "PMPC_CONE_EPIGRAPH", 1},    // cone objective with hard boxes: epigraph problem in the shared-control space (any tie pattern); 0: weighted-QP fixed point
    {"cond_grouped", "PMPC_COND_GROUPED", 1},      // Nc > 1: condensed Hessians summed over groups of particles inside the condensing kernel
    {"as_freeze_tol", "PMPC_AS_FREEZE_TOL", 1e-9}, // stage-cone rounds: a shared-control step below this (relative) is zero for every particle; settled ones skip the forward sweep
    {"as_ckpt", "PMPC_AS_CKPT", 1},                // factor sweeps checkpoint their cost-to-go at stages 4, 8, 16, 32, ..; the later rounds' sweeps restart at the lowest checkpoint above the highest changed stage
    {"as_sens_min_m", "PMPC_AS_SENS_MIN_M", 3072}, // particles per rank from which the forward sweep records sensitivities to the shared step and settled particles of the later rounds are updated elementwise (one consensus stage; 0: never)
    {"as_perm_min_m", "PMPC_AS_PERM_MIN_M", 2048}, // particles per rank from which a later round's launches take the unsettled particles first (their long sweeps spread one per SIMD); 0: never
    {"cone_path", "PMPC_CONE_PATH", 0},            // cone objective with hard boxes, which body answers: 0 automatic (what the context learnt about the shape decides the order), 1 free-particles body first, 2 epigraph path (free-particles body never), 3 rank-based weighted-QP iteration only
};

namespace pmpc_impl {

// wait until the device has published sequence number `want` into host-coherent memory; stream sync after 2 s of polling
void wait_published(pmpc_ctx *c, volatile unsigned long long *seq, unsigned long long want) {
  if (!spin_until([&] { return *seq == want; })) {
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (*seq != want) {
      fprintf(stderr, "pmpc_hip: device scalars were never published\n");
      throw PmpcHipError{-1, "wait_published", __FILE__, __LINE__};
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
}
void read_scalars(pmpc_ctx *c) {  // sc->status carries the (cross-rank) failure flag of the last exchange
  wait_published(c, &c->mirror->seq, c->seq);
  memcpy(c->sc_host, (const void *)&c->mirror->sc, sizeof(IpmScal));
  *c->fail_host = c->sc_host->status;
}

// one sync point of the IPM: local partials -> exchange table -> (RCCL all-reduce(sum) == all-gather) -> scalars
void exchange(pmpc_ctx *c, int phase) {
  Workspace &w = c->ws;
  IpmScal *sc = (IpmScal *)w.sc.p;
  const int B2 = 2 * PMPC_RED_BLOCKS;
  c->seq++;
  if (!c->multi()) {
    launch_ipm_exchange(phase, true, true, sc, (const int *)w.fail.p, w.xch.d(), 0, 1, w.part_sum.d(), w.part_cnt.d(),
                        w.part_max.d(), B2, c->stream, 0.0, nullptr, &c->mirror_dev->sc, &c->mirror_dev->seq, c->seq);
    return;
  }
  launch_ipm_exchange(phase, true, false, sc, (const int *)w.fail.p, w.xch.d(), c->rank, c->world, w.part_sum.d(),
                      w.part_cnt.d(), w.part_max.d(), B2, c->stream);
  allreduce(c, w.xch.p, (size_t)c->world * 8, ncclFloat64, ncclSum);
  launch_ipm_exchange(phase, false, true, sc, (const int *)w.fail.p, w.xch.d(), c->rank, c->world, w.part_sum.d(),
                      w.part_cnt.d(), w.part_max.d(), B2, c->stream, 0.0, nullptr, &c->mirror_dev->sc, &c->mirror_dev->seq, c->seq);
}

// one structured Newton solve: backward (factor or vector-only) -> reduce -> all-reduce -> dense solve -> forward
void structured_solve(pmpc_ctx *c, LQArgs &a, bool factor, bool fast, bool prep_done) {
  hipStream_t s = c->stream;
  Workspace &w = c->ws;
  const int nc = a.Nc * a.u;
  if (fast && factor && !prep_done) launch_grad_prep(a, s);
  {
    ProfScope ps(c, factor ? ((fast && a.as_settled_in) ? 4 : 0) : 1);
    if (fast && a.as_act) launch_bwd_as(a, s);  // a round of the active-set iteration (kernels_as.hip)
    else if (fast) launch_bwd_fast(a, factor, s);
    else launch_bwd_generic(a, factor, s);
  }
  if (nc > 0) {
    ProfScope ps(c, 3);
    double *Hc = w.Hg.d(), *gc = w.Hg.d() + (size_t)nc * nc;
    // condensed Hessians summed over groups of particles inside the condensing kernel: when nothing downstream looks at ONE particle's
    // H_i again (settled particles of the rounds refresh g_i += H_i delta; consensus weights scale H_i; the cone path's host reads them)
    const bool grouped = fast && factor && a.Nc > 1 && nc * nc + nc > 32 && !a.as_act && !a.as_settled_in && !a.cons_w && c->opt[OPT_COND_GROUPED] != 0.0;
    a.Hc_grp = nullptr;
    if (grouped) {
      w.Hc_grp.ensure((size_t)cond_fast_groups(a.M) * nc * nc * sizeof(double));
      a.Hc_grp = w.Hc_grp.d();
    }
    if (fast && factor) launch_cond_fast(a, s);
    // sharded active-set rounds: the previous round's change counters travel behind [Hc | gc] (one collective per round
    // instead of two); the decision about that round is taken right behind the all-reduce, before this round's forward sweep
    const size_t tail = (a.as_merge && factor) ? 5 : 0;  // {released, activated, bad, failure, open cones}
    double *tl = Hc + (size_t)nc * nc + nc;
    auto merged_exchange = [&]() {
      if (a.as_merge == 2) launch_as_ctl(const_cast<AsCtl *>(a.as_ctl), a.as_cnt, a.M, (const int *)w.fail.p, 1, 0, 0, nullptr, nullptr, 0, s, tl, nullptr, a.as_open);
      else if (a.as_merge == 1) HIP_CHECK(hipMemsetAsync(tl, 0, 5 * sizeof(double), s));
      if (factor) allreduce(c, Hc, (size_t)nc * nc + nc + tail, ncclFloat64, ncclSum);
      else allreduce(c, gc, nc, ncclFloat64, ncclSum);
      if (a.as_merge == 2)
        launch_as_ctl(const_cast<AsCtl *>(a.as_ctl), nullptr, a.M, (const int *)w.fail.p, 0, 1, 0, &c->mirror_dev->ctl, &c->mirror_dev->as_seq, c->as_seq, s, tl);
    };
    const bool wave_solve = c->opt[OPT_AS_WAVE_CONS] != 0.0;
    a.cons_G = 0;
    // consensus weights (cone objective): the reductions read lambda_i (H_i, g_i) from scaled copies; the per-particle arrays stay
    // unweighted (the settled particles' g_i += H_i delta and the host's epigraph solve want them so)
    const double *HcP = a.Hc_part, *gcP = a.gc_part;
    if (a.cons_w) {
      w.Hc_w.ensure((size_t)a.M * nc * nc * sizeof(double)); w.gc_w.ensure((size_t)a.M * nc * sizeof(double));
      launch_cons_scale(a.Hc_part, a.gc_part, a.cons_w, a.M, nc, factor, w.Hc_w.d(), w.gc_w.d(), a.as_act, a.as_big, a.as_act ? nullptr : a.Du,
                        a.as_act ? nullptr : a.wu, a.u, a.owner, s);
      HcP = factor ? w.Hc_w.d() : a.Hc_part; gcP = w.gc_w.d();
    }
    if (fast && a.as_act && factor && !c->multi() && a.Nc == 1 && wave_solve) {
      // active-set round on one rank with one consensus stage: block partials only — every wave of the forward sweep sums
      // them (same order everywhere) and solves the u x u system itself: the second launch of the reduction is gone
      a.cons_G = launch_cons_partials(HcP, gcP, a.M, nc, w.red_tmp.d(), c->as_pend, s);
      c->as_pend.ctl = nullptr;
      a.cons_tH = w.red_tmp.d();
      a.cons_tg = w.red_tmp.d() + (size_t)64 * nc * nc;
    } else if (nc * nc + nc <= 32) {
      const bool solve_now = !c->multi();
      launch_cons_small(HcP, gcP, a.M, nc, factor, Hc, w.red_tmp.d(), solve_now, w.Lc.d(), w.duc.d(), (int *)w.fail.p, s);
      if (!solve_now) {
        merged_exchange();
        if (fast && a.as_act && factor && a.Nc == 1 && wave_solve) {
          // sharded active-set round: the all-reduced [Hc | gc] is ONE partial for the forward sweep's waves to solve
          a.cons_G = 1; a.cons_tH = Hc; a.cons_tg = gc;
        } else {
          launch_cons_solve(Hc, w.Lc.d(), gc, w.duc.d(), nc, factor, (int *)w.fail.p, s);
        }
      }
    } else {
      if (factor && grouped) launch_reduce_particles_hg(a.Hc_grp, gcP, w.red_tmp.d(), Hc, a.M, nc, s, cond_fast_groups(a.M));
      else if (factor) launch_reduce_particles_hg(HcP, gcP, w.red_tmp.d(), Hc, a.M, nc, s);  // (gc sits right behind Hc)
      else launch_reduce_particles(gcP, w.red_tmp.d(), gc, a.M, nc, s);
      merged_exchange();
      launch_cons_solve(Hc, w.Lc.d(), gc, w.duc.d(), nc, factor, (int *)w.fail.p, s);
    }
  }
  ProfScope ps(c, 2);
  if (fast && a.as_act) launch_fwd_as(a, s);
  else if (fast) launch_fwd_fast(a, s);
  else launch_fwd_generic(a, s);
}

// epilogue of a solve that threw (failed HIP / RCCL call, out of memory): forget every warm-start memory, NaN outputs if the
// device still takes work, status 2.  Never throws.
int fail_after_error(pmpc_ctx *c, const pmpc_problem *p, pmpc_info *info) {
  Workspace &w = c->ws;
  w.as_key = w.warm_key = w.soc_key = w.cons_key = w.xb_block_key = w.su_key = -1;
  w.as_U_valid = false;
  w.xb_warm_backoff = w.xb_warm_fails = 0;
  c->cone_rw_key = -1;
  c->xb_ctrl_from = -1;
  c->as_pend.ctl = nullptr;
  c->staged.clear();
  (void)hipGetLastError();
  try {
    if (p && p->X_out && p->U_out) {
      const double nan = std::numeric_limits<double>::quiet_NaN();
      launch_fill(p->X_out, nan, (long long)p->M * p->N * p->xdim, c->stream);
      launch_fill(p->U_out, nan, (long long)p->M * p->N * p->udim, c->stream);
    }
    HIP_WARN(hipStreamSynchronize(c->stream));
  } catch (...) {
  }
  if (info) {
    memset(info, 0, sizeof(*info));
    info->status = 2;
  }
  return 2;
}

void fill_nan_outputs(pmpc_ctx *c, const pmpc_problem *p) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  launch_fill(p->X_out, nan, (long long)p->M * p->N * p->xdim, c->stream);
  launch_fill(p->U_out, nan, (long long)p->M * p->N * p->udim, c->stream);
  HIP_CHECK(hipStreamSynchronize(c->stream));
}

// The counter of blocks the reference shift refused (cost_lin.hip) lives in the workspace, zeroed when it is created.
unsigned *cost_bad_counter(pmpc_ctx *c) {
  if (c->ws.cost_bad.ensure(sizeof(unsigned))) HIP_CHECK(hipMemsetAsync(c->ws.cost_bad.p, 0, sizeof(unsigned), c->stream));
  return (unsigned *)c->ws.cost_bad.p;
}

// A thin device entry, after its own argument checks: the context's device, `body` (the launch) and the check for a refused launch
// timed in `prof_class` if the entry has one; a failed HIP call is the entry's own `hip_error_status`.
template <class F>
static int device_entry(pmpc_ctx *c, int hip_error_status, F body, int prof_class = -1) {
  try {
    HIP_CHECK(hipSetDevice(c->device));
    std::optional<ProfScope> ps;
    if (prof_class >= 0) ps.emplace(c, prof_class);
    body();
    HIP_CHECK(hipGetLastError());
  } catch (const PmpcHipError &) {
    return hip_error_status;
  }
  return 0;
}

}  // namespace pmpc_impl

// =================================================================================================
extern "C" {

const char *pmpc_version(void) { return "pmpc_hip 0.4 (gfx950)"; }
// layout check of the two structs the bindings mirror (a stale library under a newer binding, or the reverse, must fail loudly)
void pmpc_abi_struct_sizes(size_t *problem, size_t *info) { *problem = sizeof(pmpc_problem); *info = sizeof(pmpc_info); }
size_t pmpc_abi_scp_cost_size(void) { return sizeof(pmpc_scp_cost); }

int pmpc_create(pmpc_ctx **out, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) {
    fprintf(stderr, "pmpc_hip: no HIP device %d available (found %d) — this library has no CPU path\n", device, ndev);
    return 1;
  }
  pmpc_ctx *c = new pmpc_ctx();
  c->device = device;
  for (int k = 0; k < OPT_COUNT; k++) {
    const char *e = getenv(kPmpcOptions[k].env);
    c->opt[k] = (e && *e) ? atof(e) : kPmpcOptions[k].dflt;
  }
  try {
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->sc_host = (IpmScal *)calloc(1, sizeof(IpmScal));
    c->fail_host = (int *)calloc(1, sizeof(int));
    HIP_CHECK(hipHostMalloc((void **)&c->mirror, sizeof(pmpc_ctx::ScMirror), hipHostMallocMapped | hipHostMallocCoherent));
    memset(c->mirror, 0, sizeof(pmpc_ctx::ScMirror));
    HIP_CHECK(hipHostGetDevicePointer((void **)&c->mirror_dev, c->mirror, 0));
  } catch (const PmpcHipError &) {
    free(c->sc_host);
    free(c->fail_host);
    delete c;
    return 1;
  }
  *out = c;
  return 0;
}

int pmpc_set_option(pmpc_ctx *c, const char *key, double value) {
  if (!c || !key) return -1;
  for (int k = 0; k < OPT_COUNT; k++)
    if (!strcmp(key, kPmpcOptions[k].key)) {
      c->opt[k] = value;
      c->fp_key = -1;
      c->ws.as_key = c->ws.warm_key = c->cone_rw_key = c->cone_lam_key = c->ws.es_key = -1;  // (a remembered set / iterate / weight assignment was found under the old switches)
      return 0;
    }
  return -1;
}
int pmpc_get_option(pmpc_ctx *c, const char *key, double *value) {
  if (!c || !key || !value) return -1;
  for (int k = 0; k < OPT_COUNT; k++)
    if (!strcmp(key, kPmpcOptions[k].key)) {
      *value = c->opt[k];
      return 0;
    }
  return -1;
}

void pmpc_destroy(pmpc_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  jit_unload_all(c);  // the runtime-compiled models, stage costs and state constraints loaded on this context (jit_module.hip)
  comm_release(c);
  Workspace &w = c->ws;
  DevBuf *all[] = {&w.X, &w.U, &w.dX, &w.dU, &w.dX2, &w.dU2, &w.xm, &w.xd, &w.um, &w.ud, &w.K, &w.Hinv, &w.kff, &w.gc_part, &w.Hc_part, &w.Hc_w, &w.gc_w, &w.cons_w, &w.epi_lam, &w.epi_out, &w.epi_gath, &w.es_Dx, &w.es_wx, &w.es_Du, &w.es_wu, &w.es_xm, &w.es_xd, &w.es_um, &w.es_ud, &w.es_kff2, &w.es_kff3, &w.es_gc2, &w.es_dots, &w.es_coef, &w.es_out2, &w.es_Xt, &w.es_Ut, &w.es_U, &w.es_zero, &w.scratch,
                   &w.red_tmp, &w.Hg, &w.Lc, &w.duc, &w.xch, &w.zeros, &w.zslew, &w.zslew0, &w.zum1, &w.part_sum, &w.part_cnt,
                   &w.part_max, &w.sc, &w.fail, &w.pw, &w.Jc, &w.Jg, &w.part_dev, &w.warmU, &w.lateX, &w.lateU, &w.warm_llu, &w.warm_luu, &w.warm_llx,
                   &w.warm_lux, &w.Hadd, &w.wu_soc, &w.soc_zl, &w.soc_zu, &w.soc_zc, &w.soc_dzl, &w.soc_dzu, &w.soc_dzc, &w.soc_sl, &w.soc_su, &w.soc_sc, &w.soc_dsl,
                   &w.soc_dsu, &w.soc_dsc, &w.soc_cl, &w.soc_cu, &w.soc_cc, &w.soc_wU, &w.soc_wzl, &w.soc_wzu, &w.soc_wzc, &w.as_act, &w.as_cnt, &w.as_cntp, &w.as_settled, &w.cons_lo, &w.cons_hi, &w.as_ctl, &w.as_delta, &w.as_viol, &w.as_ck, &w.as_jhi, &w.ck_stat, &w.Hc_grp, &w.as_T, &w.xb_qmax, &w.as_perm,
                   &w.sa_f, &w.sa_fx, &w.sa_fu, &w.sa_Xp, &w.sa_Up, &w.sa_Q, &w.sa_R, &w.sa_Xr, &w.sa_Ur, &w.sa_lo, &w.sa_hi, &w.sa_Xo, &w.sa_Uo,
                   &w.sa_cl, &w.sa_ch, &w.cone_A, &w.cone_c, &w.cone_z, &w.cone_rec, &w.cone_uraw, &w.as_open, &w.xb_z, &w.xb_st, &w.xb_D, &w.xb_g, &w.m64[0], &w.m64[1], &w.m64[2], &w.m64[3], &w.cost_ref[0], &w.cost_ref[1], &w.cost_uref[0], &w.cost_uref[1], &w.cost_grad, &w.cost_bad, &w.cstr_rows, &w.cstr_bad, &w.as_act2};
  for (DevBuf *b : all) b->release();
  for (SlabBufs *sb : {&w.sx, &w.su})
    for (DevBuf *b : {&sb->lo, &sb->hi, &sb->tl, &sb->tu, &sb->ll, &sb->lu, &sb->cl, &sb->cu, &sb->D, &sb->w}) b->release();
  for (DevBuf &b : c->stage) b.release();
  (void)hipHostFree(c->mirror);
  if (c->pinned) (void)hipHostFree(c->pinned);
  if (c->sm_pinned) (void)hipHostFree(c->sm_pinned);
  c->host_flags.release();
  free(c->sc_host);
  free(c->fail_host);
  (void)hipStreamDestroy(c->stream);
  delete c;
}

void *pmpc_stream(pmpc_ctx *c) { return (void *)c->stream; }
void pmpc_sync(pmpc_ctx *c) { HIP_WARN(hipStreamSynchronize(c->stream)); }

void pmpc_profile_enable(pmpc_ctx *c, int level) { c->prof = level < 0 ? 0 : level; }

// Sums of HIP-event durations (ms) and launch counts per kernel class since the last read:
// 0 backward+factor, 1 backward vector-only, 2 forward sweep, 3 consensus reduce + dense solve.
void pmpc_profile_read(pmpc_ctx *c, double *ms4, long long *n4) {
  HIP_WARN(hipStreamSynchronize(c->stream));
  for (int k = 0; k < 8; k++) {
    ProfCat &pc = c->cat[k];
    for (auto &ev : pc.pending) {
      float t = 0.f;
      HIP_WARN(hipEventElapsedTime(&t, ev.first, ev.second));
      pc.ms += t;
      pc.n++;
      pc.pool.push_back(ev);
    }
    pc.pending.clear();
    if (k < 4) { ms4[k] = pc.ms; n4[k] = pc.n; }
    else if (k == 4) { c->partial_ms = pc.ms; c->partial_n = pc.n; }
    c->last_ms[k] = pc.ms;
    c->last_n[k] = pc.n;
    pc.ms = 0.0;
    pc.n = 0;
  }
}

// every class as of the last pmpc_profile_read (see pmpc_ctx::cat): ms[count], n[count], count <= 8
void pmpc_profile_read_all(pmpc_ctx *c, double *ms, long long *n, int count) {
  for (int k = 0; k < count && k < 8; k++) { ms[k] = c->last_ms[k]; n[k] = c->last_n[k]; }
}

// class 4 (factor sweeps of active-set rounds that skipped the settled particles) as of the last pmpc_profile_read
void pmpc_profile_read_partial(pmpc_ctx *c, double *ms, long long *n) {
  *ms = c->partial_ms;
  *n = c->partial_n;
}

void pmpc_restart_stats(pmpc_ctx *c, unsigned long long *out4, int reset) {
  for (int k = 0; k < 4; k++) out4[k] = 0;
  if (!c || !c->ws.ck_stat.p) return;
  (void)hipSetDevice(c->device);
  HIP_WARN(hipStreamSynchronize(c->stream));
  HIP_WARN(hipMemcpy(out4, c->ws.ck_stat.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (reset) HIP_WARN(hipMemset(c->ws.ck_stat.p, 0, 4 * sizeof(unsigned long long)));
}

int pmpc_comm_rank(pmpc_ctx *c) { return c->rank; }
int pmpc_comm_world(pmpc_ctx *c) { return c->world; }

int pmpc_scp_residual_device(pmpc_ctx *c, size_t xdim, size_t udim, size_t N, size_t M, const double *X, const double *X_prev,
                             const double *U, const double *U_prev, double *out) {
  return device_entry(c, 2, [&] { launch_scp_residual(X, X_prev, U, U_prev, (long long)M * (long long)N, (int)xdim, (int)udim, out, c->stream); }, 7);
}

int pmpc_linearize_device_f32(pmpc_ctx *c, int model, size_t N, size_t M, const double *x0, const double *X_prev,
                              const double *U_prev, const double *params, double *f, float *fx, float *fu) {
  if (!model_known(model)) return 2;  // (built-in ids only: a runtime-compiled model writes fp64 Jacobians)
  return device_entry(c, 2, [&] { launch_linearize(model, (int)N, (int)M, x0, X_prev, U_prev, params, f, (double *)fx, (double *)fu, c->stream, 1); }, 6);
}

int pmpc_linearize_device(pmpc_ctx *c, int model, size_t N, size_t M, const double *x0, const double *X_prev,
                          const double *U_prev, const double *params, double *f, double *fx, double *fu) {
  if (!model_known(c, model)) return 2;
  return device_entry(c, 2, [&] { launch_linearize(model, (int)N, (int)M, x0, X_prev, U_prev, params, f, fx, fu, c->stream); }, 6);
}

// Nonlinear rollout and receding-horizon shift of a built-in or runtime-compiled model (dynamics.hip, model_jit.hip): asynchronous on the context's stream.
int pmpc_rollout_device(pmpc_ctx *c, int model, size_t N, size_t M, const double *x0, const double *U, const double *params, double *X) {
  if (!c || !model_known(c, model) || N == 0 || M == 0 || !x0 || !U || !params || !X) return 2;
  return device_entry(c, 1, [&] { launch_rollout(model, (int)N, (int)M, x0, U, params, X, c->stream); });
}
int pmpc_shift_plan_device(pmpc_ctx *c, int model, size_t N, size_t M, size_t s, const double *X, const double *U, const double *params,
                           const double *U_tail, double *X_new, double *U_new, double *um1_new) {
  if (!c || !model_known(c, model) || N == 0 || M == 0 || s < 1 || s >= N || !X || !U || !params || !X_new || !U_new || X_new == X || U_new == U) return 2;
  return device_entry(c, 1, [&] { launch_shift_plan(model, (int)N, (int)M, (int)s, X, U, params, U_tail, X_new, U_new, um1_new, c->stream); });
}

// The control-box statuses of a plan moved along with its controls (dynamics.hip, k_shift_active_set): on the caller's arrays, and on
// the set the context's last accepted solve stored — what lets the first solve after a plan shift start like every later one of an SCP
// loop (pmpc_scp_loop_device with first_cold = 0).
static bool shift_set_args_ok(const pmpc_ctx *c, size_t N, size_t M, size_t udim, size_t s, const double *U, const double *U_new) {
  return c && N > 0 && M > 0 && udim > 0 && s >= 1 && s < N && U && U_new && U_new != U && M * N * udim < ((size_t)1 << 40) && N * udim < ((size_t)1 << 30);
}
int pmpc_shift_active_set_device(pmpc_ctx *c, size_t N, size_t M, size_t udim, long long Nc, size_t s, const double *U, const double *U_tail, const int *act,
                                 const double *lo, const double *hi, double *U_new, int *act_new) {
  if (!shift_set_args_ok(c, N, M, udim, s, U, U_new) || !act || !act_new || act_new == act) return 2;
  const int nc = Nc < 0 || Nc > (long long)N ? (int)N : (int)Nc;
  return device_entry(c, 1, [&] { launch_shift_active_set((int)N, (int)M, (int)udim, nc, (int)s, U, U_tail, act, lo, hi, U_new, act_new, c->stream); });
}
int pmpc_warm_shift_device(pmpc_ctx *c, size_t N, size_t M, size_t udim, long long Nc, size_t s, const double *U, const double *U_tail, const double *lo,
                           const double *hi, double *U_new, int *shifted) {
  if (!shift_set_args_ok(c, N, M, udim, s, U, U_new) || !shifted) return 2;
  Workspace &w = c->ws;
  *shifted = 0;
  const size_t n = M * N * udim, bytes = n * sizeof(int) + 8;  // (+ 8: the sweeps read the last status as 8 bytes)
  // (a sharded context's shared controls follow global particle 0, which this rank may not hold: its first solve stays cold)
  if (w.as_key == -1 || w.as_count != n || w.as_act.bytes < bytes || c->multi()) return 0;
  const int st = device_entry(c, 1, [&] {
    if (w.as_act2.ensure(w.as_act.bytes)) HIP_CHECK(hipMemsetAsync(w.as_act2.p, 0, w.as_act2.bytes, c->stream));
    launch_shift_active_set((int)N, (int)M, (int)udim, Nc < 0 || Nc > (long long)N ? (int)N : (int)Nc, (int)s, U, U_tail, (const int *)w.as_act.p, lo, hi, U_new,
                            (int *)w.as_act2.p, c->stream);
  });
  if (st != 0) return st;
  std::swap(w.as_act, w.as_act2);  // (same size: the solve's own ensure() finds its buffer as large as before)
  *shifted = 1;
  return 0;
}
int pmpc_warm_set_read_device(pmpc_ctx *c, int *act_out, size_t n) {
  if (!c || !act_out || c->ws.as_key == -1 || c->ws.as_count != n || c->ws.as_act.bytes < n * sizeof(int)) return 2;
  return device_entry(c, 1, [&] { HIP_CHECK(hipMemcpyAsync(act_out, c->ws.as_act.p, n * sizeof(int), hipMemcpyDeviceToDevice, c->stream)); });
}

// Linearised nonlinear costs (cost_lin.hip).
int pmpc_ref_shift_device(pmpc_ctx *c, size_t dim, size_t rows, const double *A, const double *cv, const double *ref, double *out) {
  if (dim < 1 || dim > (size_t)REF_SHIFT_MAX_DIM) return 2;
  return device_entry(c, 1, [&] { launch_ref_shift((int)dim, (long long)rows, A, cv, ref, out, cost_bad_counter(c), c->stream); }, 6);
}
long long pmpc_ref_shift_bad_pivots(pmpc_ctx *c, int reset) {
  if (!c || !c->ws.cost_bad.p) return 0;
  unsigned n = 0;
  (void)hipSetDevice(c->device);
  HIP_WARN(hipStreamSynchronize(c->stream));
  HIP_WARN(hipMemcpy(&n, c->ws.cost_bad.p, sizeof(n), hipMemcpyDeviceToHost));
  if (reset) HIP_WARN(hipMemset(c->ws.cost_bad.p, 0, sizeof(n)));
  return (long long)n;
}
int pmpc_obstacle_cost_grad_device(pmpc_ctx *c, const pmpc_scp_cost *cost, size_t xdim, size_t N, size_t M, const double *X_prev, double *cx) {
  if (!obstacle_cost_valid(cost, (int)xdim)) return 2;
  return device_entry(c, 1, [&] { launch_obstacle_grad(*cost, (int)xdim, (int)N, (int)M, X_prev, cx, c->stream); }, 6);
}
int pmpc_obstacle_ref_shift_device(pmpc_ctx *c, const pmpc_scp_cost *cost, size_t xdim, size_t N, size_t M, const double *X_prev, const double *Q,
                                   const double *X_ref, double *out) {
  if (!obstacle_cost_valid(cost, (int)xdim)) return 2;
  return device_entry(c, 1, [&] { launch_obstacle_ref_shift(*cost, (int)xdim, (int)N, (int)M, X_prev, Q, X_ref, out, cost_bad_counter(c), c->stream); }, 6);
}

int pmpc_custom_cost_grad_device(pmpc_ctx *c, int id, size_t N, size_t M, const double *X_prev, const double *U_prev, const double *cparams, double *cx,
                                 double *cu, double *val) {
  int uses_u = 0;
  if (!c || !custom_cost_known(c, id) || !custom_cost_dims(id, nullptr, nullptr, nullptr, &uses_u) || !cx || (uses_u && !cu)) return 2;
  return device_entry(c, 1, [&] { custom_launch_cost_grad(id, (int)N, (int)M, X_prev, U_prev, cparams, cx, cu, val, c->stream); }, 6);
}

// compact Jacobian records of a built-in model (jac_compact.h), as the SCP loop writes and reads them: the linearisation into jc
// (pmpc_jac_compact_doubles doubles), and the expansion of jc into the dense fx / fu through the column- (orient 0) or row-oriented
// (1) part of the records.  pmpc_jac_live_mask: the entries the records treat as live (host only; returns 100 xdim + udim).
int pmpc_linearize_compact_device(pmpc_ctx *c, int model, size_t N, size_t M, const double *x0, const double *X_prev, const double *U_prev,
                                  const double *params, double *f, double *jc) {
  if (!model_known(model)) return 2;
  return device_entry(c, 2, [&] { launch_linearize_compact(model, (int)N, (int)M, x0, X_prev, U_prev, params, f, jc, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, c->stream); }, 6);
}
int pmpc_expand_jac_device(pmpc_ctx *c, int model, size_t N, size_t M, const double *jc, double *fx, double *fu, int orient) {
  if (!model_known(model)) return 2;
  return device_entry(c, 2, [&] { launch_expand_jac(model, (int)N, (int)M, jc, fx, fu, orient, c->stream); });
}
long long pmpc_jac_compact_doubles(int model, size_t N, size_t M) { return model_known(model) ? jac_compact_doubles(model, (int)N, (int)M) : -1; }
int pmpc_jac_live_mask(int model, unsigned char *fx_mask, unsigned char *fu_mask) { return jac_live_mask(model, fx_mask, fu_mask); }

// -------------------------------------------------------------------------------------------------
// fp32-storage problem -> the same problem with fx, fu, Q, R widened (exactly) into workspace copies, flag cleared
pmpc_problem widened_f32_problem(pmpc_ctx *c, const pmpc_problem *p, bool jacobians) {
  Workspace &w = c->ws;
  const long long rows = (long long)p->M * (long long)p->N, x = (long long)p->xdim, u = (long long)p->udim;
  const long long cnt[4] = {rows * x * x, rows * x * u, rows * x * x, rows * u * u};
  const double *src[4] = {p->fx, p->fu, p->Q, p->R};
  for (int k = jacobians ? 0 : 2; k < 4; k++) {
    w.m64[k].ensure((size_t)cnt[k] * sizeof(double));
    launch_widen_f32((const float *)src[k], w.m64[k].d(), cnt[k], c->stream);
  }
  pmpc_problem q = *p;
  q.flags &= ~(unsigned)PMPC_F32_MATRICES;
  if (jacobians) { q.fx = w.m64[0].d(); q.fu = w.m64[1].d(); }
  q.Q = w.m64[2].d(); q.R = w.m64[3].d();
  return q;
}
static int solve_impl(pmpc_ctx *c, const pmpc_problem *p, pmpc_info *info, int verbose, bool soc) {
  try {
    int st = solve_impl_body(c, p, info, verbose, soc);
    if (st == PMPC_NEEDS_F64) {
      // fp32-storage mode outside the warm-started active-set rounds (first solve of a loop, fallbacks, other dims / consensus
      // horizons): widen fx, fu, Q, R into workspace copies — exact — and run the ordinary solve on them
      const pmpc_problem q = widened_f32_problem(c, p);
      if (verbose) printf("pmpc_hip: fp32-storage problem: widened for the fp64 kernels\n");
      st = solve_impl_body(c, &q, info, verbose, soc);
    }
    HIP_CHECK(hipGetLastError());  // a kernel launch that was refused (bad configuration, lost device) is a failed solve
    return st;
  } catch (const PmpcHipError &) {
    return fail_after_error(c, p, info);
  }
}

int pmpc_lqp_solve_device(pmpc_ctx *c, const pmpc_problem *p, pmpc_info *info, int verbose) {
  return solve_impl(c, p, info, verbose, false);
}
int pmpc_lsoc_solve_device(pmpc_ctx *c, const pmpc_problem *p, pmpc_info *info, int verbose) {
  return solve_impl(c, p, info, verbose, true);
}

// Slew penalties on the MFMA path: restate the problem in control increments (kernels_slew.hip: state [x; u], control
// u_j - u_{j-1}, control boxes -> boxes on the state), solve that plain problem, split the state back into (X, U).
bool slew_increment_form_applies(const pmpc_ctx *c, const pmpc_problem *p, bool soc) {
  if (soc || !(p->flags & (PMPC_HAS_SLEW | PMPC_HAS_SLEW0)) || (p->flags & PMPC_FORCE_GENERIC) || !(p->flags & PMPC_SYMMETRIC_COST))
    return false;
  if (p->N < 2) return false;  // N = 1: the reference's diagonal rule is not the plain penalty (lqp_utils.jl:31-39)
  // With boxes the control boxes become STATE boxes of the restated problem.  Until r03 those met the interior-point iteration only
  // (1.8x - 2.6x slower cold and ~10x slower warm than the generic kernels' active-set rounds), so boxed slew problems stayed on the
  // generic kernels; with the state-box rounds of kernels_xbox.hip the restated form is 2.1x - 5.4x FASTER than the generic kernels cold, 1.45x - 2x warm,
  // and agrees with them to 1e-15 (tools/debug/slew_paths.py, profiles/r03_f_slew_paths.txt, CHANGELOG.md 3.3).  It needs the XBOX instantiation of the
  // factor sweep for (x + u, u); the options slew_increment_boxes = 0 / xbox_as = 0 put boxed slew problems back on the generic kernels.
  const bool with_boxes = c->opt[OPT_SLEW_INCREMENT_BOXES] != 0.0 && c->opt[OPT_XBOX_AS] != 0.0;
  if ((p->flags & (PMPC_HAS_XBOUNDS | PMPC_HAS_UBOUNDS)) && !(with_boxes && xbox_as_dims_supported((int)(p->xdim + p->udim), (int)p->udim))) return false;
  // (barrier mode: the shared controls' boxes carry ONE barrier term — particle 0's — which M state boxes on the u-part would count M times)
  if ((p->flags & (PMPC_HAS_XBOUNDS | PMPC_HAS_UBOUNDS)) && p->barrier_mu > 0.0) return false;
  LQArgs t;
  memset(&t, 0, sizeof(t));
  t.x = (int)(p->xdim + p->udim); t.u = (int)p->udim; t.N = (int)p->N; t.M = (int)p->M; t.sym_cost = 1;
  return lq_fast_supported(t);
}

// the restated problem `q` (state [x; u], control increments; outputs in the workspace) and the augmentation record `g` the split needs
void build_slew_increment_problem(pmpc_ctx *c, const pmpc_problem *p, pmpc_problem &q, SlewAug &g) {
  HIP_CHECK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  Workspace &w = c->ws;
  const int x = (int)p->xdim, u = (int)p->udim, N = (int)p->N, M = (int)p->M, n = x + u;
  const int Nc = p->Nc < 0 ? N : (int)p->Nc;
  const bool has_xb = p->flags & PMPC_HAS_XBOUNDS, has_ub = p->flags & PMPC_HAS_UBOUNDS;
  const bool has_slew = p->flags & PMPC_HAS_SLEW, has_slew0 = p->flags & PMPC_HAS_SLEW0;
  const size_t rows = (size_t)M * N, D8 = sizeof(double);
  w.sa_f.ensure(rows * n * D8); w.sa_fx.ensure(rows * n * n * D8); w.sa_fu.ensure(rows * n * u * D8);
  w.sa_Xp.ensure(rows * n * D8); w.sa_Up.ensure(rows * u * D8); w.sa_Q.ensure(rows * n * n * D8); w.sa_R.ensure(rows * u * u * D8);
  w.sa_Xr.ensure(rows * n * D8); w.sa_Ur.ensure(rows * u * D8); w.sa_Xo.ensure(rows * n * D8); w.sa_Uo.ensure(rows * u * D8);
  const bool boxes = has_xb || has_ub;
  if (boxes) { w.sa_lo.ensure(rows * n * D8); w.sa_hi.ensure(rows * n * D8); }
  if (w.zslew.bytes < (size_t)M * D8 || w.zum1.bytes < (size_t)M * u * D8) {
    w.zslew.ensure((size_t)M * D8); w.zslew0.ensure((size_t)M * D8); w.zum1.ensure((size_t)M * u * D8);
    HIP_CHECK(hipMemsetAsync(w.zslew.p, 0, (size_t)M * D8, s));
    HIP_CHECK(hipMemsetAsync(w.zslew0.p, 0, (size_t)M * D8, s));
    HIP_CHECK(hipMemsetAsync(w.zum1.p, 0, (size_t)M * u * D8, s));
  }
  memset(&g, 0, sizeof(g));
  g.x = x; g.u = u; g.N = N; g.M = M; g.Nc = Nc; g.has_xb = has_xb; g.has_ub = has_ub;
  g.has_um1 = (has_slew0 && Nc >= 1) ? 1 : 0;  // the linear term -s0 u_0'u_{-1} exists only with consensus stages (lqp_utils.jl:165)
  const double reg = std::min(p->reg_x, p->reg_u);  // the one regulariser of the restated problem; the excess goes into the cost blocks
  g.dx = p->reg_x - reg; g.du = p->reg_u - reg;
  g.f = p->f; g.fx = p->fx; g.fu = p->fu; g.Xp = p->X_prev; g.Up = p->U_prev; g.Q = p->Q; g.R = p->R; g.Xr = p->X_ref; g.Ur = p->U_ref;
  g.lx = p->lx; g.ux = p->ux; g.lu = p->lu; g.uu = p->uu;
  g.slew = has_slew ? p->slew_reg : w.zslew.d();
  g.slew0 = has_slew0 ? p->slew_reg0 : w.zslew0.d();
  g.um1 = has_slew0 ? p->slew_um1 : w.zum1.d();
  if (has_ub && Nc > 0) {  // consensus controls: (global) particle 0's boxes, lqp_utils.jl:329-330
    const size_t nc = (size_t)Nc * u;
    w.sa_cl.ensure(nc * D8); w.sa_ch.ensure(nc * D8);
    HIP_CHECK(hipMemcpyAsync(w.sa_cl.p, p->lu, nc * D8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(w.sa_ch.p, p->uu, nc * D8, hipMemcpyDeviceToDevice, s));
    if (c->multi()) {
      broadcast(c, w.sa_cl.p, nc, ncclFloat64, 0);
      broadcast(c, w.sa_ch.p, nc, ncclFloat64, 0);
    }
    g.cons_lo = w.sa_cl.d(); g.cons_hi = w.sa_ch.d();
  }
  g.af = w.sa_f.d(); g.afx = w.sa_fx.d(); g.afu = w.sa_fu.d(); g.aXp = w.sa_Xp.d(); g.aUp = w.sa_Up.d();
  g.aQ = w.sa_Q.d(); g.aR = w.sa_R.d(); g.aXr = w.sa_Xr.d(); g.aUr = w.sa_Ur.d();
  g.alo = boxes ? w.sa_lo.d() : nullptr; g.ahi = boxes ? w.sa_hi.d() : nullptr;
  launch_slew_augment(g, s);

  q = *p;
  q.xdim = (size_t)n;
  q.flags &= ~(PMPC_HAS_SLEW | PMPC_HAS_SLEW0 | PMPC_HAS_UBOUNDS | PMPC_HAS_XBOUNDS | PMPC_PREV_IS_LAST_SOLUTION | PMPC_STATIC_CONS_BOUNDS);
  if (boxes) q.flags |= PMPC_HAS_XBOUNDS;
  q.reg_x = reg;
  q.reg_u = 0.0;
  q.f = g.af; q.fx = g.afx; q.fu = g.afu; q.X_prev = g.aXp; q.U_prev = g.aUp; q.Q = g.aQ; q.R = g.aR; q.X_ref = g.aXr; q.U_ref = g.aUr;
  q.lx = g.alo; q.ux = g.ahi; q.lu = q.uu = nullptr;
  q.slew_reg = q.slew_reg0 = q.slew_um1 = nullptr;
  q.X_out = w.sa_Xo.d(); q.U_out = w.sa_Uo.d();
}

int solve_slew_increment_form(pmpc_ctx *c, const pmpc_problem *p, pmpc_info *info, int verbose) {
  hipStream_t s = c->stream;
  Workspace &w = c->ws;
  const int x = (int)p->xdim, u = (int)p->udim, N = (int)p->N, M = (int)p->M;
  const int Nc = p->Nc < 0 ? N : (int)p->Nc;
  const size_t rows = (size_t)M * N;
  pmpc_problem q;
  SlewAug g;
  build_slew_increment_problem(c, p, q, g);
  pmpc_info inf;
  memset(&inf, 0, sizeof(inf));
  c->xb_ctrl_from = x;
  int st;
  try {
    st = solve_impl_body(c, &q, &inf, verbose, false);
  } catch (...) {
    c->xb_ctrl_from = -1;
    throw;
  }
  c->xb_ctrl_from = -1;
  if (st == 0) launch_slew_split(w.sa_Xo.d(), w.sa_Uo.d(), p->X_out, p->U_out, (long long)rows, x, u, N, (M > 1 || c->multi()) ? Nc : 0, g.cons_lo, g.cons_hi, s);
  else fill_nan_outputs(c, p);
  if (info) *info = inf;
  return st;
}

}  // extern "C"
