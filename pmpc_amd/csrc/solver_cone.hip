// solver_cone.hip — the cone objective of c_lcone_solve (PMPC.jl/src/main.jl:194-354) on the device solver with HARD boxes: particle costs,
// the dispatch (lcone_body: one ConeSolve object per call, one method per phase), the epigraph problem in the shared-control space (its
// Epigraph), the free-particles path (one FreeParticles object), the rank-based weighted-QP iteration as fallback.  Smoothed boxes
// (log barrier / squareplus): solver_cone_smooth.hip.  Split out of solver.hip (r05); shared declarations: solver_internal.h, cone_common.h.
#include "cone_common.h"

extern "C" {

int pmpc_particle_costs_device(pmpc_ctx *c, const pmpc_problem *p0, const double *X, const double *U, double *J_out) {
  HIP_CHECK(hipSetDevice(c->device));
  Workspace &w = c->ws;
  // (the cost kernel reads Q, R as doubles: an fp32-storage problem's blocks are widened first — found by `bench.py --cone --fp32`,
  //  which read the float arrays as doubles, past their end)
  pmpc_problem pw_;
  const pmpc_problem *p = p0;
  if (p0->flags & PMPC_F32_MATRICES) {
    pw_ = widened_f32_problem(c, p0, /*jacobians=*/false);
    p = &pw_;
  }
  const size_t M = p->M, u = p->udim;
  LQArgs a;
  memset(&a, 0, sizeof(a));
  a.x = (int)p->xdim; a.u = (int)u; a.N = (int)p->N; a.M = (int)M;
  a.reg_x = p->reg_x; a.reg_u = p->reg_u;
  a.Q = p->Q; a.R = p->R; a.X_prev = p->X_prev; a.U_prev = p->U_prev; a.X_ref = p->X_ref; a.U_ref = p->U_ref;
  const bool has_slew = p->flags & PMPC_HAS_SLEW, has_slew0 = p->flags & PMPC_HAS_SLEW0;
  ensure_zero_slew(c, M, u);
  a.slew = has_slew ? p->slew_reg : w.zslew.d();
  a.slew0 = has_slew0 ? p->slew_reg0 : w.zslew0.d();
  a.um1 = has_slew0 ? p->slew_um1 : w.zum1.d();
  launch_particle_cost(a, X, U, J_out, c->stream);
  return 0;
}

int pmpc_lcone_solve_device(pmpc_ctx *c, const pmpc_problem *p, double smooth_alpha, pmpc_info *info, int verbose) {
  try {
    return lcone_body(c, p, smooth_alpha, info, verbose);
  } catch (const PmpcHipError &) {
    return fail_after_error(c, p, info);
  }
}

}  // extern "C"

namespace {

constexpr double CONE_EPS = 1e-3;  // COST_ANCHOR_EPS, main.jl:223
constexpr size_t D8 = sizeof(double);

// the reference's `k` (worst-k objective for 0 < k < M; anything else: all M particles)
double cone_k_of(const pmpc_problem *p, size_t M) { return (p->cone_k > 0 && p->cone_k < (long long)M) ? (double)p->cone_k : (double)M; }

// Cone objective with hard boxes when NO inequality of a particle's own is active at the answer (always so with every control shared,
// Nc = N — the reference's default consensus horizon — and no state boxes; often so with loose boxes): each particle's cost, minimised over
// its own free controls, is then an exact quadratic of the shared controls,
//     V_i(u_c) = V_i(base) + g_i'(u_c - base) + 1/2 (u_c - base)' H_i (u_c - base),
// with (H_i, g_i) from ONE unweighted factor sweep (+ condensing) at any base point.  The reference's epigraph program (main.jl:204-239)
// is a problem in the Nc u + 1 unknowns (u_c, t) with M quadratic rows and the box on u_c: solved on the host by a primal active-set
// loop over that box around the epigraph solver of epigraph_host.hip — any number of costs on the threshold, one pass, no iteration on
// rankings (which knows two-way ties only and, for k < M, met four-way ones in tools/fuzz/fuzz_cone.py) and no dependence on how the
// sub-problem solve ended (the epigraph path below needs the state of the active-set rounds: an equality-only optimum has none).
// The particles' own boxes (free controls, states) are CHECKED at the answer: if one is violated the assumption was wrong, nothing
// is returned and the caller goes on with the general paths.  run() returns -1 where it does not apply, else the status.
class FreeParticles {
 public:
  FreeParticles(pmpc_ctx *c_, const pmpc_problem *p_, pmpc_info *info_, int verbose_)
      : c(c_), p(p_), info(info_), verbose(verbose_), w(c_->ws), s(c_->stream), x((int)p_->xdim), u((int)p_->udim), N((int)p_->N), M((int)p_->M),
        Nc(cons_horizon(p_).Nc), nc(cons_horizon(p_).nc), has_ub(p_->flags & PMPC_HAS_UBOUNDS), has_xb(p_->flags & PMPC_HAS_XBOUNDS),
        nx((size_t)M * N * x), nu((size_t)M * N * u), K((1.0 - CONE_EPS) * cone_k_of(p_, p_->M)) {}
  int run() {
    if (!applies()) return -1;
    set_up();
    if (!base_point() || !condensed_quadratics() || !shared_box_active_set() || !own_boxes_hold()) return -1;
    return outputs();
  }

 private:
  static constexpr double cap = 1.0 + CONE_EPS;
  // ---- fixed for the solve ----
  pmpc_ctx *const c;
  const pmpc_problem *const p;
  pmpc_info *const info;
  const int verbose;
  Workspace &w;
  const hipStream_t s;
  const int x, u, N, M, Nc, nc;
  const bool has_ub, has_xb;
  const size_t nx, nu;
  const double K;  // sum of the multipliers of the epigraph rows, (1 - eps) k
  // ---- state the phases hand to each other ----
  LQArgs a;      // applies: the problem's part; set_up: the workspace's; base_point, condensed_quadratics and outputs launch with it
  pmpc_info inf;  // set_up zeroes it; condensed_quadratics and outputs count; outputs hands it to the caller
  // Shared controls and their box.  base_point writes them (ub0: the DEVICE's base point, kept); shared_box_active_set moves ub to the
  // bounds met on the way; outputs reads ub, ub0, lo, hi.
  std::vector<double> ub, ub0, lo, hi;
  // V_i(base) and the condensed quadratics (H_i, g_i) of all particles.  condensed_quadratics writes them; shared_box_active_set reads
  // them and moves them along with the base.
  std::vector<double> J, Hh, gh;
  // shared_box_active_set: held shared controls, multipliers of the epigraph rows, the step from the base, the threshold cost, the host
  // solves it took, the tolerance on a held bound's multiplier; kkt_of_last_solve and outputs read them
  std::vector<unsigned char> held;
  std::vector<double> lam, delta;
  double t = 0.0, tolg = 0.0;
  int it = 0;

  bool applies() {
    if (nc < 1 || c->multi() || c->world != 1 || p->weights || M < 2 || (double)M * nc * nc > 2e7 ||
        (p->flags & (PMPC_HAS_SLEW | PMPC_HAS_SLEW0 | PMPC_FORCE_GENERIC | PMPC_F32_MATRICES)) || p->cone_count > 0 || p->soc_W)
      return false;
    a = lq_args_of(c, p, M, Nc);
    return lq_fast_supported(a);
  }

  void set_up() {
    w.X.ensure(nx * D8); w.U.ensure(nu * D8); w.dX.ensure(nx * D8); w.dU.ensure(nu * D8);
    w.xm.ensure(nx * D8); w.xd.ensure(nx * D8); w.um.ensure(nu * D8); w.ud.ensure(nu * D8);
    w.es_Xt.ensure(nx * D8); w.es_Ut.ensure(nu * D8);
    w.K.ensure((size_t)M * N * 64 * D8); w.Hinv.ensure(nu * u * D8); w.kff.ensure(nu * D8);
    w.gc_part.ensure((size_t)M * nc * D8); w.Hc_part.ensure((size_t)M * nc * nc * D8);
    w.scratch.ensure((size_t)M * 3 * x * nc * D8); w.Jc.ensure((size_t)M * D8); w.duc.ensure((size_t)nc * D8); w.fail.ensure(sizeof(int));
    w.part_max.ensure(2 * PMPC_RED_BLOCKS * D8);
    zero_buffers(c, M, nc, a);
    a.K = w.K.d(); a.Hinv = w.Hinv.d(); a.kff = w.kff.d(); a.gc_part = w.gc_part.d(); a.Hc_part = w.Hc_part.d(); a.scratch = w.scratch.d();
    a.duc = w.es_zero.d(); a.dX = w.dX.d(); a.dU = w.dU.d(); a.fail = (int *)w.fail.p; a.X = w.X.d(); a.U = w.U.d();
    a.xm = w.xm.d(); a.xd = w.xd.d(); a.um = w.um.d(); a.ud = w.ud.d();
    w.as_key = -1; w.warm_key = -1; w.es_key = -1;  // (the workspace's factor records and warm-start memories are overwritten)
    memset(&inf, 0, sizeof(inf));
    inf.fast_path = 1;
  }

  // base point: the previous controls, the shared ones = particle 0's inside their box (the joint problem takes particle 0's bounds on
  // a shared control, lqp_utils.jl:329-330); states by rollout
  bool base_point() {
    ub.assign(nc, 0.0); lo.assign(nc, -1e300); hi.assign(nc, 1e300);
    HIP_CHECK(hipMemcpyAsync(ub.data(), p->U_prev, (size_t)nc * D8, hipMemcpyDeviceToHost, s));
    if (has_ub) {
      HIP_CHECK(hipMemcpyAsync(lo.data(), p->lu, (size_t)nc * D8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(hi.data(), p->uu, (size_t)nc * D8, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    for (int r = 0; r < nc; r++) {
      if (!(lo[r] == lo[r])) lo[r] = -1e300;  // (NaN = no bound)
      if (!(hi[r] == hi[r])) hi[r] = 1e300;
      if (!(lo[r] <= hi[r])) return false;  // (an empty box: the general path reports it as the reference does)
      if (!(ub[r] == ub[r])) return false;
      ub[r] = std::min(std::max(ub[r], lo[r]), hi[r]);
    }
    ub0 = ub;
    HIP_CHECK(hipMemcpyAsync(w.U.p, p->U_prev, nu * D8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(w.U.p, ub.data(), (size_t)nc * D8, hipMemcpyHostToDevice, s));
    launch_share_cons(w.U.d(), M, N, u, Nc, s);
    launch_rollout_fast(a, w.U.d(), w.X.d(), s);
    return true;
  }

  // one unweighted factor sweep at the base point, then V_i(base) and the condensed quadratics (H_i, g_i) to the host
  bool condensed_quadratics() {
    HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
    launch_grad_prep(a, s);
    launch_bwd_fast(a, true, s);
    if (Nc > 1) launch_cond_fast(a, s);
    launch_fwd_fast(a, s);  // (shared step zero: every particle's own optimal response to the base shared controls, in dX / dU)
    launch_step_to(w.X.d(), w.dX.d(), 1.0, w.es_Xt.d(), (long long)nx, s);
    launch_step_to(w.U.d(), w.dU.d(), 1.0, w.es_Ut.d(), (long long)nu, s);
    launch_particle_cost(a, w.es_Xt.d(), w.es_Ut.d(), w.Jc.d(), s);  // V_i(base)
    J.resize(M); Hh.resize((size_t)M * nc * nc); gh.resize((size_t)M * nc);
    int failflag = 0;
    HIP_CHECK(hipMemcpyAsync(J.data(), w.Jc.p, (size_t)M * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(Hh.data(), w.Hc_part.p, Hh.size() * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(gh.data(), w.gc_part.p, gh.size() * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&failflag, w.fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    inf.structured_solves = 1;
    if (failflag) return false;
    for (int i = 0; i < M; i++) mirror_upper(&Hh[(size_t)i * nc * nc], nc);
    return true;
  }

  // primal active-set loop over the box of the shared controls around the epigraph solve
  bool shared_box_active_set() {
    held.assign(nc, 0);
    for (int r = 0; r < nc; r++) held[r] = (ub[r] <= lo[r] || ub[r] >= hi[r]) ? 1 : 0;
    lam.assign(M, K / (double)M); delta.assign(nc, 0.0);
    std::vector<double> Hd(nc);
    double gmax = 0.0;
    for (double v : gh) gmax = std::max(gmax, std::fabs(v));
    tolg = 1e-9 * std::max(1.0, gmax);
    bool done = false;
    for (; it < 20 * nc + 50 && !done; it++) {
      const int est = pmpc_epigraph_solve_host(M, nc, J.data(), Hh.data(), gh.data(), held.data(), K, cap, lam.data(), delta.data(), &t, verbose > 1);
      if (est != 0 && verbose) printf("pmpc_hip: cone objective, free particles: the host solve stopped short of its tolerance\n");
      double al = 1.0;
      int blocking = -1;
      for (int r = 0; r < nc; r++) {
        if (held[r]) { delta[r] = 0.0; continue; }
        const double un = ub[r] + delta[r];
        if (un > hi[r] && delta[r] > 0.0) { const double v = (hi[r] - ub[r]) / delta[r]; if (v < al) { al = v; blocking = r; } }
        if (un < lo[r] && delta[r] < 0.0) { const double v = (lo[r] - ub[r]) / delta[r]; if (v < al) { al = v; blocking = r; } }
      }
      if (blocking >= 0) {  // move the base to the first bound met on the way and hold it there
        al = std::max(0.0, al);
        for (int i = 0; i < M; i++) {
          const double *Hi = &Hh[(size_t)i * nc * nc];
          double *gi = &gh[(size_t)i * nc];
          double gd = 0.0, dHd = 0.0;
          for (int r = 0; r < nc; r++) {
            double acc = 0.0;
            for (int q_ = 0; q_ < nc; q_++) acc += Hi[r + (size_t)nc * q_] * delta[q_];
            Hd[r] = acc;
            gd += gi[r] * delta[r];
            dHd += delta[r] * acc;
          }
          J[i] += al * gd + 0.5 * al * al * dHd;
          for (int r = 0; r < nc; r++) gi[r] += al * Hd[r];
        }
        for (int r = 0; r < nc; r++) ub[r] += al * delta[r];
        ub[blocking] = delta[blocking] > 0.0 ? hi[blocking] : lo[blocking];
        held[blocking] = 1;
        if (verbose) printf("pmpc_hip: cone objective, free particles: shared control %d meets its bound (step fraction %.3e)\n", blocking, al);
        continue;
      }
      // the full step stays inside the box: multipliers of the held bounds = gradient of sum lam_i V_i at base + delta
      int worst = -1;
      double wv = tolg;
      for (int r = 0; r < nc; r++) {
        if (!held[r]) continue;
        double gr = 0.0;
        for (int i = 0; i < M; i++) {
          const double *Hi = &Hh[(size_t)i * nc * nc];
          double acc = gh[(size_t)i * nc + r];
          for (int q_ = 0; q_ < nc; q_++) acc += Hi[r + (size_t)nc * q_] * delta[q_];
          gr += lam[i] * acc;
        }
        const bool at_lo = ub[r] <= lo[r], at_hi = ub[r] >= hi[r];
        const double viol = (at_lo && at_hi) ? 0.0 : (at_lo ? -gr : (at_hi ? gr : std::fabs(gr)));  // (lo == hi: the control stays where it is)
        if (viol > wv) { wv = viol; worst = r; }
      }
      if (worst >= 0) {
        held[worst] = 0;
        if (verbose) printf("pmpc_hip: cone objective, free particles: shared control %d leaves its bound (multiplier %.3e of the wrong sign)\n", worst, wv);
        continue;
      }
      if (est != 0 && !kkt_of_last_solve()) {
        if (verbose) printf("pmpc_hip: cone objective, free particles: the last host solve did not converge and its point fails the KKT check: no answer from this path\n");
        return false;
      }
      done = true;
    }
    if (!done) {
      if (verbose) printf("pmpc_hip: cone objective, free particles: the box active set of the shared controls did not settle\n");
      return false;
    }
    return true;
  }

  // never an unverified iterate: the host solve stopped short of ITS tolerance — with many costs on the threshold its
  // multiplier updates crawl while the point is long exact — so the KKT conditions of the epigraph rows are checked on what it returned:
  // sum lam = K; lam_i = cap above the threshold cost, 0 below, anything on it; stationarity of sum lam_i (g_i + H_i delta) on the free
  // shared controls; t at the breakpoint the multipliers name.
  bool kkt_of_last_solve() const {
    double slam = 0.0, jscale = 1.0;
    std::vector<double> Jn(M), gs(nc, 0.0);
    for (int i = 0; i < M; i++) {
      const double *Hi = &Hh[(size_t)i * nc * nc], *gi = &gh[(size_t)i * nc];
      double lin = 0.0, quad = 0.0;
      for (int r = 0; r < nc; r++) {
        double acc = 0.0;
        for (int q_ = 0; q_ < nc; q_++) acc += Hi[r + (size_t)nc * q_] * delta[q_];
        lin += gi[r] * delta[r];
        quad += delta[r] * acc;
        gs[r] += lam[i] * (gi[r] + acc);
      }
      Jn[i] = J[i] + lin + 0.5 * quad;
      jscale = std::max(jscale, std::fabs(Jn[i]));
      slam += lam[i];
    }
    const double jt = 1e-9 * jscale, lt = 1e-9 * cap;
    bool ok = std::fabs(slam - K) <= 1e-9 * std::max(1.0, K);
    for (int i = 0; i < M && ok; i++) {
      if (lam[i] < -lt || lam[i] > cap + lt) ok = false;
      else if (Jn[i] > t + jt && lam[i] < cap - lt) ok = false;   // above the threshold: full multiplier
      else if (Jn[i] < t - jt && lam[i] > lt) ok = false;         // below: none
    }
    for (int r = 0; r < nc && ok; r++)
      if (!held[r] && std::fabs(gs[r]) > tolg * std::max(1.0, K)) ok = false;
    return ok;
  }

  // The total shared step from the DEVICE's base point, the forward sweep that adds every particle's own response to it — and the
  // assumption: no box of a particle's own is violated at this point.
  bool own_boxes_hold() {
    std::vector<double> dtot(nc);
    for (int r = 0; r < nc; r++) {
      ub[r] = std::min(std::max(ub[r] + delta[r], lo[r]), hi[r]);
      dtot[r] = ub[r] - ub0[r];
    }
    HIP_CHECK(hipMemcpyAsync(w.duc.p, dtot.data(), (size_t)nc * D8, hipMemcpyHostToDevice, s));
    LQArgs a3 = a;
    a3.duc = w.duc.d();
    launch_fwd_fast(a3, s);
    launch_step_to(w.X.d(), w.dX.d(), 1.0, w.es_Xt.d(), (long long)nx, s);
    launch_step_to(w.U.d(), w.dU.d(), 1.0, w.es_Ut.d(), (long long)nu, s);
    HIP_CHECK(hipMemcpyAsync(w.es_Ut.p, ub.data(), (size_t)nc * D8, hipMemcpyHostToDevice, s));  // (a held shared control sits exactly on its bound)
    launch_share_cons(w.es_Ut.d(), M, N, u, Nc, s);
    const int B = PMPC_RED_BLOCKS;
    std::vector<double> pm(2 * B, 0.0);
    HIP_CHECK(hipMemsetAsync(w.part_max.p, 0, 2 * B * D8, s));
    Slab sl;
    memset(&sl, 0, sizeof(sl));
    if (has_xb) { sl.count = (long long)nx; sl.lo = p->lx; sl.hi = p->ux; sl.z = w.es_Xt.d(); launch_violation(sl, w.part_max.d(), s); }
    if (has_ub) { sl.count = (long long)nu; sl.lo = p->lu; sl.hi = p->uu; sl.z = w.es_Ut.d(); launch_violation(sl, w.part_max.d() + B, s); }
    HIP_CHECK(hipMemcpyAsync(pm.data(), w.part_max.p, 2 * B * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    double viol = 0.0;
    for (double v : pm) viol = std::max(viol, v == v ? v : 1e300);
    if (verbose) printf("pmpc_hip: cone objective, free particles: threshold cost %.9e after %d host solves; largest violation of a particle's own box %.3e\n", t, it, viol);
    return !(viol > 1e-9);
  }

  int outputs() {
    HIP_CHECK(hipMemcpyAsync(p->X_out, w.es_Xt.p, nx * D8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(p->U_out, w.es_Ut.p, nu * D8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    c->cone_lam_key = -1;
    inf.outer_solves = it;
    inf.status = 0;
    if (info) *info = inf;
    return 0;
  }
};

int lcone_free_particles_body(pmpc_ctx *c, const pmpc_problem *p, pmpc_info *info, int verbose) { return FreeParticles(c, p, info, verbose).run(); }

class Epigraph;

// One call of lcone_body.  run() is the dispatch; what its phases hand to each other are the members.
class ConeSolve {
 public:
  ConeSolve(pmpc_ctx *c_, const pmpc_problem *p0, double smooth_alpha_, pmpc_info *info_, int verbose_)
      : c(c_), info(info_), verbose(verbose_), smooth_alpha(smooth_alpha_), w(c_->ws), s(c_->stream) {
    // (an fp32-storage problem runs the cone objective on widened copies: its weighted QPs and the particle costs read doubles)
    p = p0;
    if (p0->flags & PMPC_F32_MATRICES) {
      pwide = widened_f32_problem(c, p0);
      p = &pwide;
    }
    // particles are sharded in equal contiguous blocks (bench.py's layout): the ranking of the particle costs is global, so
    // every rank gathers all costs (all-reduce(sum) of a zero-padded vector) and takes the same decisions
    Ml = p->M; M = Ml * (size_t)c->world; off = (size_t)c->rank * Ml;
    w.pw.ensure(Ml * D8); w.Jc.ensure(Ml * D8); w.Jg.ensure(std::max<size_t>(M, 2) * D8);
    user.assign(M, 1.0); pw.resize(Ml); J.resize(M);
    memset(&inf, 0, sizeof(inf));
    memset(&last, 0, sizeof(last));
    // threshold rank of the piecewise-linear epigraph cost in t: the m*-th cheapest particle, m* = ceil(2 eps M / (1+eps))
    // (general k, main.jl:204-227: multipliers lambda_i in [0, 1+eps] of the cone rows sum to (1-eps) k, so the
    // n_hi = floor((1-eps) k / (1+eps)) costliest particles carry 1+eps, the next one the remainder, the rest nothing)
    kk = cone_k_of(p, M);
    n_hi = (long long)std::floor((1.0 - eps) * kk / (1.0 + eps) + 1e-12);
    mstar = std::max<long long>(1, (long long)M - n_hi);
    // floor weight of the weightless particles: they shift the shared controls by O(w_floor (m* - 1) / n_hi) — 1e-4 is harmless for
    // the one-in-500 of k = M, the worst-k objective (half the particles weightless at k = M / 2) needs it smaller
    w_hi = 1.0 + eps; w_thr = (1.0 - eps) * kk - (1.0 + eps) * (double)n_hi; w_floor = kk < (double)M ? 1e-9 : 1e-4;
  }

  int run() {
    if (c->multi() && !equal_shards()) {
      fprintf(stderr, "pmpc_hip: pmpc_lcone_solve_device needs the same number of particles on every rank\n");
      return refuse(2);
    }
    if (p->weights) gather(p->weights, user);
    q = *p;
    q.weights = w.pw.d();
    // smooth_cstr = "logbarrier" (main.jl:246-262): -1/alpha sum log(alpha slack) replaces the hard boxes
    q.barrier_mu = (smooth_alpha == smooth_alpha && smooth_alpha > 0.0) ? 1.0 / smooth_alpha : 0.0;
    if (q.barrier_mu > 0.0 && !(p->flags & (PMPC_HAS_XBOUNDS | PMPC_HAS_UBOUNDS))) q.barrier_mu = 0.0;  // (no boxes: nothing to smooth, main.jl:248)
    if (const std::optional<int> st = smoothed_boxes()) return *st;
    if (const std::optional<int> st = free_particles_first()) return *st;
    if (M == 1) return finish(solve_weighted(std::vector<double>(1, 1.0 - eps)));  // one particle: weight 1 - eps, same minimiser as the QP (k = 1)
    if (const std::optional<int> st = epigraph_path()) return *st;
    return rank_iteration();
  }

 private:
  friend class Epigraph;
  static constexpr double eps = CONE_EPS;
  // ---- fixed for the call ----
  pmpc_ctx *const c;
  pmpc_info *const info;
  const int verbose;
  const double smooth_alpha;
  Workspace &w;
  const hipStream_t s;
  // ---- what the constructor sets and every phase reads ----
  pmpc_problem pwide;     // the widened copy of an fp32-storage problem, else unused
  const pmpc_problem *p;  // the caller's problem, or &pwide
  size_t Ml, M, off;      // particles here, particles in all, global index of this rank's first particle
  // threshold rank and rank weights (rank_weights, cheapest, kink_bisection read them; kk also the Epigraph and the memory key)
  double kk;
  long long n_hi, mstar;
  double w_hi, w_thr, w_floor;
  // ---- state the phases hand to each other ----
  std::vector<double> user;  // the caller's particle weights, ALL particles (1 without): run gathers them; solve_weighted, gather_costs and the Epigraph read them
  std::vector<double> J;     // costs of ALL particles, scaled by `user`: gather_costs writes them; the Epigraph and the rank-based iteration read them
  std::vector<double> pw;    // (scratch of solve_weighted: this rank's weights as uploaded)
  // The weighted QP of the rank-based iteration (weights = w.pw, barrier_mu of the smoothing).  run sets it up; smoothed_boxes and
  // free_particles_first read barrier_mu; sub_solve clears its PREV_IS_LAST_SOLUTION bit.
  pmpc_problem q;
  pmpc_info inf;   // sub_solve: what the last sub-problem solve reported
  pmpc_info last;  // sub_solve copies inf; the Epigraph reads how that solve ended; finish reports it with the totals
  int outer = 0, solves_total = 0, ipm_total = 0;  // sub_solve counts: solves, their structured solves, their interior-point iterations; finish reports them
  // free_particles_first sets both: option cone_path (the Epigraph's condition reads it) and whether the free-particles body may be
  // asked at all (last_resort reads it)
  int forced = 0;
  bool fp_applies = false;

  // global[rank*Ml + i] = local[i] on every rank
  void gather(const double *local_dev, std::vector<double> &global) {
    if (!c->multi()) {
      HIP_CHECK(hipMemcpyAsync(global.data(), local_dev, Ml * D8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      return;
    }
    HIP_CHECK(hipMemsetAsync(w.Jg.p, 0, M * D8, s));
    HIP_CHECK(hipMemcpyAsync(w.Jg.d() + off, local_dev, Ml * D8, hipMemcpyDeviceToDevice, s));
    allreduce(c, w.Jg.p, M, ncclFloat64, ncclSum);
    HIP_CHECK(hipMemcpyAsync(global.data(), w.Jg.p, M * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }

  bool equal_shards() {  // equal shards are assumed by the offsets above
    double cnt[2] = {(double)Ml, -(double)Ml};
    HIP_CHECK(hipMemcpyAsync(w.Jg.p, cnt, 2 * D8, hipMemcpyHostToDevice, s));
    allreduce(c, w.Jg.p, 2, ncclFloat64, ncclMax);
    HIP_CHECK(hipMemcpyAsync(cnt, w.Jg.p, 2 * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return cnt[0] == -cnt[1];
  }

  // a call this path does not take: NaN outputs, nothing but the status in `info`
  int refuse(int status) {
    fill_nan_outputs(c, p);
    if (info) {
      memset(info, 0, sizeof(*info));
      info->status = status;
    }
    return status;
  }

  // `last` with the totals of the call.  (The smoothed and the free-particles bodies write `info` themselves: their answer does not come here.)
  int finish(int status) {
    last.status = status;
    last.outer_solves = outer;
    last.structured_solves = solves_total;
    last.ipm_iters = ipm_total;
    if (status != 0) fill_nan_outputs(c, p);
    if (info) *info = last;
    return status;
  }

  // ---- smoothed boxes: the calls into lcone_smooth_body ----
  std::optional<int> smoothed_boxes() {
    if (p->smooth_cstr == 1 && q.barrier_mu > 0.0) {
      // smooth_cstr = "squareplus" (main.jl:265-279): soft boxes, tau(v) = beta/2 (v + sqrt(v^2 + 1/alpha^2)) per side; only the
      // full-space Newton path has it (mu carries 1/alpha)
      const double sbeta = p->smooth_beta > 0.0 ? p->smooth_beta : 1.0;
      const bool one_particle = M == 1 && !c->multi() && (p->weights || (p->flags & (PMPC_HAS_SLEW | PMPC_HAS_SLEW0)));
      const int st_s = one_particle ? squareplus_one_particle(sbeta) : lcone_smooth_body(c, p, q.barrier_mu, info, verbose, 1, sbeta);
      if (st_s >= 0) return st_s;
      fprintf(stderr, "pmpc_hip: smooth_cstr = \"squareplus\" needs boxes to smooth, M (Nc u)^2 <= 2e7, no fp32 storage, a compiled (xdim, udim) pair and — with slew penalties or particle weights — M = 1 (slew: symmetric costs, N >= 2, a compiled (xdim + udim, udim) pair)\n");
      return refuse(2);
    }
    if (q.barrier_mu > 0.0 && c->opt[OPT_CONE_EPIGRAPH] != 0.0 && M > 1) {
      const int st_s = lcone_smooth_body(c, p, q.barrier_mu, info, verbose);
      if (st_s >= 0) return st_s;
    }
    return std::nullopt;
  }

  // ONE particle (the shape of nearly every reference example): the epigraph row is degenerate, the problem is
  //   min (1 - eps) w J(z) + sum of hinges   <=>   min (1 - eps) J(z) + sum of hinges of slope beta / w      (scale_probs_cost!, main.jl:96-112)
  // and slew penalties go through the increment form of the QP path (state [x; u], control increments: the control boxes — and with
  // them their hinges — become state boxes; one particle, so no shared control is counted twice).  -1: not taken.
  int squareplus_one_particle(double sbeta) {
    double wgt = 1.0;
    if (p->weights) {
      HIP_CHECK(hipMemcpyAsync(&wgt, p->weights, sizeof(double), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
    if (!(wgt > 0.0)) return -1;
    pmpc_problem p1 = *p;
    p1.weights = nullptr;
    // (the cone program takes each particle's cost from qp_repr_Pq, cone_utils.jl:64-95, which keeps the first-step slew term
    //  slew_reg0 |u_0 - u_{-1}|^2 whatever Nc is — the joint QP assembly loses it at Nc = 0, lqp_utils.jl:165; with ONE particle a
    //  consensus horizon of one stage is the same problem and carries the term)
    if (p1.Nc == 0) p1.Nc = 1;
    if (!(p->flags & (PMPC_HAS_SLEW | PMPC_HAS_SLEW0))) return lcone_smooth_body(c, &p1, q.barrier_mu, info, verbose, 1, sbeta / wgt);
    LQArgs t;
    memset(&t, 0, sizeof(t));
    t.x = (int)(p->xdim + p->udim); t.u = (int)p->udim; t.N = (int)p->N; t.M = 1; t.sym_cost = 1;
    if (!(p->N >= 2 && (p->flags & PMPC_SYMMETRIC_COST) && !(p->flags & PMPC_FORCE_GENERIC) && lq_fast_supported(t))) return -1;
    pmpc_problem qa;
    SlewAug g;
    build_slew_increment_problem(c, &p1, qa, g);
    qa.weights = nullptr;
    const int st_s = lcone_smooth_body(c, &qa, q.barrier_mu, info, verbose, 1, sbeta / wgt);
    if (st_s == 0) launch_slew_split(w.sa_Xo.d(), w.sa_Uo.d(), p->X_out, p->U_out, (long long)p->N, (int)p->xdim, (int)p->udim, (int)p->N, 0, g.cons_lo, g.cons_hi, s);
    else if (st_s > 0) fill_nan_outputs(c, p);
    return st_s;
  }

  // The free-particles path (lcone_free_particles_body) is exact for any tie pattern but host-heavy (it gathers every particle's
  // condensed Hessian): it goes FIRST only on a shape where it was needed and worked before; otherwise it is the last resort behind the
  // ranking iteration (measured, config B with Nc = N: 4200 it/s through the ranking, 280 through this path).
  std::optional<int> free_particles_first() {
    // (the key discriminates the raw cone_k and the box flags, not the world: the body runs on one rank only)
    const long long fkey = cone_shape_key(M, p, (long long)p->cone_k + 1, 4, ((p->flags & PMPC_HAS_XBOUNDS) ? 2 : 0) + ((p->flags & PMPC_HAS_UBOUNDS) ? 1 : 0));
    // (option cone_path: which body answers does not have to depend on what the context saw before — 1: the free-particles body first,
    //  2: never, 3: the rank-based iteration alone; tests/test_cone_ties_gpu.py runs the same problems through each)
    forced = (int)c->opt[OPT_CONE_PATH];
    fp_applies = !(q.barrier_mu > 0.0) && c->opt[OPT_CONE_EPIGRAPH] != 0.0 && M > 1 && forced != 2 && forced != 3;
    if ((p->flags & PMPC_COLD_START) || c->fp_key != fkey) { c->fp_key = fkey; c->fp_ok = -1; }
    if (forced == 1) c->fp_ok = 1;
    if (fp_applies && c->fp_ok == 1) {
      const int st_f = lcone_free_particles_body(c, p, info, verbose);
      if (st_f >= 0) return st_f;
      c->fp_ok = 0;
    }
    return std::nullopt;
  }

  // No consistent threshold set within the outer iteration limit (more than two costs on the threshold, typically): the exact path for
  // particles without an active inequality of their own, if that is what they are; else a failed solve (NaN outputs), never an
  // unverified iterate.
  int last_resort() {
    if (verbose) printf("pmpc_hip: cone objective: the threshold set did not settle\n");
    if (fp_applies && c->fp_ok != 0) {
      const int st_f = lcone_free_particles_body(c, p, info, verbose);
      c->fp_ok = st_f == 0 ? 1 : 0;
      if (st_f >= 0) return st_f;
    }
    return finish(1);
  }

  // ---- sub-problem solves ----
  // One sub-problem on the QP path, counted.  The later solves of this call start from THIS solve's set and solution (kept in the
  // workspace), not from the caller's X_prev / U_prev: the caller's promise covers the first one only — whichever problem copy it ran on.
  int sub_solve(pmpc_problem &prob) {
    const int st = pmpc_lqp_solve_device(c, &prob, &inf, verbose > 1);
    prob.flags &= ~(unsigned)PMPC_PREV_IS_LAST_SOLUTION;
    q.flags &= ~(unsigned)PMPC_PREV_IS_LAST_SOLUTION;
    outer++;
    solves_total += inf.structured_solves;
    ipm_total += inf.ipm_iters;
    last = inf;
    return st;
  }

  // costs of the accepted point (w.Jc) of ALL particles on the host; scale_probs_cost! (main.jl:96-112) acts on the costs themselves
  void gather_costs() {
    gather(w.Jc.d(), J);
    for (size_t i = 0; i < M; i++) J[i] *= user[i];
  }

  // the weighted QP with the weights `rankw` (all particles) times the caller's, then the costs at its optimum
  int solve_weighted(const std::vector<double> &rankw) {
    for (size_t i = 0; i < Ml; i++) pw[i] = user[off + i] * rankw[off + i];
    HIP_CHECK(hipMemcpyAsync(w.pw.p, pw.data(), Ml * D8, hipMemcpyHostToDevice, s));
    const int st = sub_solve(q);
    if (st != 0) return st;
    pmpc_particle_costs_device(c, p, p->X_out, p->U_out, w.Jc.d());
    gather_costs();
    return 0;
  }

  std::optional<int> epigraph_path();  // a status: answered; nothing: go on with the rank-based iteration

  // ---- the rank-based iteration ----
  long long memory_key() const { return cone_shape_key(M, p, (long long)kk, 64, c->world); }  // of cone_lam and of cone_rw

  // the (m* - 1) cheapest particles carry no weight in the reference's objective (their trajectories are then not
  // unique); they keep w_floor here so that every particle's sub-problem stays strictly convex
  void rank_weights(const std::vector<size_t> &low, std::vector<double> &rw) const {
    std::fill(rw.begin(), rw.end(), w_hi);
    for (size_t k = 0; k + 1 < low.size(); k++) rw[low[k]] = w_floor;
    rw[low.back()] = std::max(w_thr, w_floor);
  }
  void cheapest(std::vector<size_t> &low) const {  // indices of the m* cheapest particles, ascending cost
    std::vector<size_t> idx(M);
    for (size_t i = 0; i < M; i++) idx[i] = i;
    std::partial_sort(idx.begin(), idx.begin() + mstar, idx.end(), [&](size_t a_, size_t b_) { return J[a_] < J[b_] || (J[a_] == J[b_] && a_ < b_); });
    low.assign(idx.begin(), idx.begin() + mstar);
  }

  // Inside an SCP loop the ranking of the particle costs rarely changes between iterations: the assignment the previous solve of this
  // shape settled on is tried FIRST — if the ranking at its optimum reproduces it, that is the fixed point (the same consistency test
  // as below: weights = multipliers of the epigraph rows, KKT of the reference's problem) after ONE weighted QP instead of two.
  int rank_iteration() {
    const long long rwkey = memory_key();
    int st = 0;
    std::vector<size_t> low;
    std::vector<double> rw(M, w_hi), rw1(M), rw2(M), rw_prev;
    if (c->opt[OPT_CONE_RANK_MEMORY] != 0.0 && !(p->flags & PMPC_COLD_START) && c->cone_rw_key == rwkey && c->cone_rw.size() == M) {
      rw1 = c->cone_rw;
      low.assign(1, 0);  // (only its last entry is read before the first ranking, for the verbose line)
    } else {
      st = solve_weighted(rw);  // uniform weights: the QP optimum ranks the particles
      if (st != 0) return finish(st);
      cheapest(low);
      rank_weights(low, rw1);
    }
    c->cone_rw_key = -1;
    // fixed-point iteration on the WEIGHT assignment the ranking implies (the order inside the floor-weight group is irrelevant)
    bool settled = false;
    for (int it = 0; it < 12 && !settled; it++) {
      rw = rw1;
      st = solve_weighted(rw);
      if (st != 0) return finish(st);
      const size_t thr_old = low.back();
      cheapest(low);
      rank_weights(low, rw2);
      if (verbose) printf("pmpc_hip: cone outer %d  threshold particle %zu -> %zu  J_thr %.9e\n", it + 1, thr_old, low.back(), J[low.back()]);
      if (rw2 == rw1) {
        settled = true;
        c->cone_rw = rw1;  // (a kink's interpolated weights are not remembered: they are no assignment by rank)
        c->cone_rw_key = rwkey;
        break;
      }
      if (!rw_prev.empty() && rw2 == rw_prev) {
        st = kink_bisection(rw1, rw2, rw, settled);
        if (st != 0) return finish(st);
        break;
      }
      rw_prev = rw1;
      rw1 = rw2;
    }
    return settled ? finish(0) : last_resort();
  }

  // 2-cycle between two rankings: the optimum sits on a kink J_a = J_b between the particles a, b whose weights differ
  // most between the two assignments; on the segment rw(theta) = theta rw1 + (1 - theta) rw2 the gap J_a - J_b is
  // monotone in theta (a loses weight as theta grows, so its cost rises relative to b's): bisection.  mstar = 1: a and
  // b share the deficit 2 eps M; mstar > 1: they swap the threshold / floor weights.  Returns a failed solve's status, else 0 with
  // `settled`: the point at the kink passes the KKT test (rw: its weights).
  int kink_bisection(const std::vector<double> &rw1, const std::vector<double> &rw2, std::vector<double> &rw, bool &settled) {
    size_t a_ = 0, b_ = 0;
    double da = 0.0, db = 0.0;
    for (size_t i = 0; i < M; i++) {
      const double dlt = rw1[i] - rw2[i];
      if (dlt < da) { da = dlt; a_ = i; }  // lighter under assignment 1
      if (dlt > db) { db = dlt; b_ = i; }  // lighter under assignment 2
    }
    if (!(da < 0.0 && db > 0.0)) return 0;  // (cannot happen: the assignments differ)
    double lo = 0.0, hi = 1.0;  // theta = 1: assignment 1 (a light, then J_a > J_b), theta = 0: assignment 2
    for (int bis = 0; bis < 60; bis++) {
      const double th = 0.5 * (lo + hi);
      for (size_t i = 0; i < M; i++) rw[i] = th * rw1[i] + (1.0 - th) * rw2[i];
      const int st = solve_weighted(rw);
      if (st != 0) return st;
      const double gap = J[a_] - J[b_];
      if (verbose) printf("pmpc_hip: cone kink bisection %2d  theta %.12f  J_a - J_b %+.3e\n", bis, th, gap);
      if (std::fabs(gap) <= 1e-11 * std::max(1.0, std::fabs(J[a_]))) break;
      if (gap > 0.0) hi = th; else lo = th;
    }
    // accept if the weights are consistent with the ranking at the kink: every particle lighter than the threshold pair is
    // cheaper than it, every full-weight particle costlier (KKT of the epigraph problem, multipliers lambda_i = w_i)
    const double jk = 0.5 * (J[a_] + J[b_]), tolj = 1e-9 * std::max(1.0, std::fabs(jk));
    settled = std::fabs(J[a_] - J[b_]) <= 1e-8 * std::max(1.0, std::fabs(jk));
    for (size_t i = 0; i < M && (settled || verbose); i++) {
      if (i == a_ || i == b_) continue;
      const bool dips = rw[i] >= w_hi && J[i] < jk - tolj;  // a full-weight particle dips below the threshold cost
      const bool rises = rw[i] < w_hi && J[i] > jk + tolj;  // a down-weighted particle rises above it
      // a multiplier strictly between 0 (the floor) and 1 + eps belongs to a row ON the threshold: a third particle that carries the
      // threshold remainder while its cost sits below the kink's is no KKT point (found by tools/fuzz/fuzz_cone.py with k < M: the
      // kink of the two COSTLIEST particles was accepted with the remainder weight on the third)
      const bool off_thr = rw[i] > 2.0 * w_floor && rw[i] < w_hi * (1.0 - 1e-12) && std::fabs(J[i] - jk) > tolj;
      if (dips || rises || off_thr) {
        settled = false;
        if (verbose) printf("pmpc_hip: cone kink: particle %zu (weight %.3e) is on the wrong side of the threshold cost by %.3e (J_thr %.9e)\n", i, rw[i], J[i] - jk, jk);
      }
    }
    return 0;
  }
};

// ---- hard boxes: the epigraph problem in the space of the shared controls (epigraph_host.hip) ------------------------------------
// Scaling a particle's whole cost changes neither its gains nor its active set nor its optimum GIVEN the shared controls, so the
// sweeps run unweighted (a particle of weight zero takes the minimum-cost completion: the limit of the floor weight of the
// weighted-QP iteration, without the floor) and the multipliers lam_i of the M epigraph rows enter only where the particles
// meet: the consensus system sum_i lam_i (H_i, g_i) (LQArgs::cons_w).  Each sub-problem solve leaves the particles' condensed
// quadratics behind; when its costs J_i and the multipliers violate the KKT conditions of the epigraph problem (lam = 1 + eps above
// the threshold cost, 0 below, anything on it), the host solves that problem on those quadratics — ties among any number of
// particles are ordinary degenerate rows there — and the next solve applies the result: one more round if no box changes status.
// (sharded: every rank holds the multipliers of ALL particles, checks the gathered costs on the host and solves the same epigraph problem
//  on the all-gathered quadratics: identical decisions everywhere, as for the rank-based iteration)
class Epigraph {
 public:
  explicit Epigraph(ConeSolve &o_)
      : o(o_), c(o_.c), p(o_.p), verbose(o_.verbose), w(o_.w), s(o_.s), Ml(o_.Ml), M(o_.M), off(o_.off), ncv(cons_horizon(o_.p).nc), epi_multi(o_.c->multi()),
        Ksum((1.0 - CONE_EPS) * o_.kk), lam(o_.M, Ksum / (double)o_.M), cw(o_.Ml), lam_loc(o_.Ml) {
    qq = *p;
    qq.weights = nullptr;
    qq.barrier_mu = 0.0;
    // KKT check of the epigraph rows on the device (k_epi_check): costs of the accepted point, threshold cost, violation — 32 bytes back.
    // Inside pmpc_scp_loop_device both kernels go in BEHIND the first batch of rounds, ahead of the speculative follow-up work (residual,
    // next linearisation), so the answer is there when the host has seen the rounds end.
    if (w.epi_lam.ensure(Ml * D8)) c->epi_lam_host.clear();  // (fresh allocations hold nothing of what the host mirrors remember)
    if (w.cons_w.ensure(Ml * D8)) c->cons_w_host.clear();
    w.epi_out.ensure(4 * D8);
  }

  // The outer loop: solve, check the epigraph rows, solve the epigraph problem on the quadratics the solve left, apply.  A status: answered.
  // Nothing: not settled (or the sub-problem does not end in the active-set rounds) — the caller goes on with the rank-based iteration.
  std::optional<int> run() {
    const long long lkey = o.memory_key();
    if (ncv == 0) return o.finish(solve_cons(false));  // no shared controls: every particle minimises its own cost, whatever its multiplier
    const bool remembered = c->opt[OPT_CONE_RANK_MEMORY] != 0.0 && !(p->flags & PMPC_COLD_START) && c->cone_lam_key == lkey && c->cone_lam.size() == M;
    if (remembered) lam = c->cone_lam;
    c->cone_lam_key = -1;
    int st_ = solve_cons(remembered);
    if (st_ != 0) return o.finish(st_);
    delta.resize(ncv);
    bool settled = false;
    for (int it = 0; it < 30; it++) {
      // KKT of the epigraph rows at (lam, J), from the device: {violation, threshold cost, rows on the threshold}
      const double viol = chk[0], tthr = chk[1];
      if (verbose) printf("pmpc_hip: cone epigraph outer %d: threshold cost %.9e, %d rows on it, KKT violation %.3e\n", it, tthr, (int)chk[2], viol);
      if (viol <= 1e-9 * std::max(1.0, std::fabs(tthr))) { settled = true; break; }
      if (!costs_on_host) o.gather_costs();
      // the particles' quadratics around the accepted point: left by the LAST round of the active-set rounds (gradient at that round's
      // base point, the consensus step it applied).  A solve that ended elsewhere (equality-only optimum, interior-point iteration) is
      // repeated warm: one round that changes nothing.
      for (int rep = 0; rep < 2 && !ended_in_rounds(); rep++) {
        st_ = solve_cons(true);
        if (st_ != 0) return o.finish(st_);
      }
      if (!ended_in_rounds()) {
        if (verbose) printf("pmpc_hip: cone epigraph: the sub-problem does not end in the active-set rounds; weighted-QP iteration instead\n");
        break;
      }
      fetch_quadratics();
      double tpred = 0.0;
      const int est = pmpc_epigraph_solve_host((int)M, ncv, o.J.data(), Hh.data(), gh.data(), held.data(), Ksum, cap, lam.data(), delta.data(), &tpred, verbose);
      if (est != 0 && verbose) printf("pmpc_hip: cone epigraph: the host solve stopped short of its tolerance (the next check decides)\n");
      st_ = solve_cons(true);
      if (st_ != 0) return o.finish(st_);
    }
    // work the caller enqueued behind the first batch of rounds (pmpc_scp_loop_device) saw the final outputs only if that solve was the last
    if (c->scp.fired && hook_solve != n_solves - 1) c->scp.ok = false;
    if (settled) {
      c->cone_lam = lam;
      c->cone_lam_key = lkey;
      return o.finish(0);
    }
    if (verbose) printf("pmpc_hip: cone epigraph: not settled; weighted-QP iteration\n");
    return std::nullopt;
  }

 private:
  static constexpr double cap = 1.0 + CONE_EPS;
  ConeSolve &o;
  pmpc_ctx *const c;
  const pmpc_problem *const p;
  const int verbose;
  Workspace &w;
  const hipStream_t s;
  const size_t Ml, M, off;
  const int ncv;         // shared controls
  const bool epi_multi;  // sharded: the check runs on the host, the quadratics are all-gathered
  const double Ksum;     // sum of the multipliers, (1 - eps) k
  // ---- state the methods hand to each other ----
  pmpc_problem qq;              // the unweighted sub-problem; ConeSolve::sub_solve clears its PREV_IS_LAST_SOLUTION bit
  std::vector<double> lam;      // multipliers of the epigraph rows, ALL particles: run (the remembered ones) and the host solve write them; solve_cons, host_check read them
  std::vector<double> cw, lam_loc;  // (scratch of solve_cons: this rank's consensus weights / multipliers as uploaded)
  double chk[4] = {0.0, 0.0, 0.0, 0.0};  // {violation, threshold cost, rows on it}: solve_cons writes it (device check or host_check), run reads it
  int n_solves = 0, hook_solve = -1;  // solve_cons: solves so far, the one the caller's hook fired in; run tells the caller whether that was the last
  bool costs_on_host = false;         // solve_cons: o.J holds the costs of the accepted point (sharded runs gather them for the check)
  std::vector<double> Hh, gh, delta;  // fetch_quadratics writes (H_i, g_i) of all particles; the host solve reads them and writes the step
  std::vector<unsigned char> held;    // fetch_quadratics: shared controls on a bound

  bool ended_in_rounds() const { return o.last.fast_path && o.last.ipm_iters == 0 && o.last.active_set_rounds >= 1; }

  void enqueue_check() {
    pmpc_particle_costs_device(c, p, p->X_out, p->U_out, w.Jc.d());
    if (!epi_multi) launch_epi_check(w.epi_lam.d(), w.Jc.d(), p->weights, (int)Ml, cap, w.epi_out.d(), s, c->mirror_dev->epi, &c->mirror_dev->epi_seq, ++c->epi_seq);
  }

  // one unweighted sub-problem solve with the consensus weights lam_i (weighted) or 1, times the caller's; then the check of the epigraph rows into chk
  int solve_cons(bool weighted) {
    bool need = p->weights != nullptr || weighted;
    if (need) {
      for (size_t i = 0; i < Ml; i++) cw[i] = (weighted ? lam[off + i] : 1.0) * o.user[off + i];
      if (c->cons_w_host != cw) {  // (unchanged since the last upload — the steady state of an SCP loop: nothing to send)
        HIP_CHECK(hipMemcpyAsync(w.cons_w.p, cw.data(), Ml * D8, hipMemcpyHostToDevice, s));
        c->cons_w_host = cw;
      }
    }
    for (size_t i = 0; i < Ml; i++) lam_loc[i] = lam[off + i];
    if (!epi_multi && c->epi_lam_host != lam_loc) {
      HIP_CHECK(hipMemcpyAsync(w.epi_lam.p, lam_loc.data(), Ml * D8, hipMemcpyHostToDevice, s));
      c->epi_lam_host = lam_loc;
    }
    c->cons_w_active = (need && ncv > 0) ? w.cons_w.d() : nullptr;
    // the caller's hook (pmpc_scp_loop_device), wrapped: the check goes in ahead of its follow-up work.  fired_here and orig live in
    // this frame, which outlives the solve.
    bool fired_here = false;
    std::function<void()> orig;
    if (c->scp.post_batch) {
      orig.swap(c->scp.post_batch);
      c->scp.post_batch = [&]() {
        fired_here = true;
        enqueue_check();
        orig();
      };
    }
    int st_;
    try {
      st_ = o.sub_solve(qq);
    } catch (...) {  // (the hook record is emptied by the scope that filled it: ScpHookGuard)
      c->cons_w_active = nullptr;
      throw;
    }
    c->cons_w_active = nullptr;
    // not fired (the solve did not go through a first batch of rounds): the caller's hook stays for a later solve
    if (c->scp.post_batch) c->scp.post_batch.swap(orig);
    if (fired_here) hook_solve = n_solves;
    n_solves++;
    if (st_ != 0) return st_;
    if (!(fired_here && c->scp.ok)) enqueue_check();  // (what the hook computed saw unfinished outputs, or there was no hook)
    if (epi_multi) {
      // sharded: all costs to every rank (one all-reduce of a zero-padded vector), the same check on the host everywhere
      o.gather_costs();
      costs_on_host = true;
      host_check();
      return 0;
    }
    costs_on_host = false;
    // (polled from the host-coherent mirror: the stream — which may hold the next linearisation behind the check — is not drained)
    wait_published(c, &c->mirror->epi_seq, c->epi_seq);
    memcpy(chk, (const void *)c->mirror->epi, 4 * D8);
    return 0;
  }

  // The KKT check of the epigraph rows at (lam, o.J) on the host, for the sharded runs.  It RESTATES k_epi_check (kernels_generic.hip), which
  // sees one rank's particles only: threshold cost = mean cost of the rows with a multiplier strictly inside (0, cap), else midway
  // between the cheapest full row and the costliest empty one; violation = how far a row is on the wrong side of it.
  void host_check() {
    const std::vector<double> &J = o.J;
    double tsum = 0.0, jmin_full = 1e300, jmax_zero = -1e300, viol = 0.0;
    size_t nfr = 0;
    for (size_t i = 0; i < M; i++) {
      if (lam[i] > 1e-12 && lam[i] < cap - 1e-12) { tsum += J[i]; nfr++; }
      else if (lam[i] >= cap - 1e-12) jmin_full = std::min(jmin_full, J[i]);
      else jmax_zero = std::max(jmax_zero, J[i]);
    }
    const double th = nfr ? tsum / (double)nfr : ((jmin_full < 1e300 && jmax_zero > -1e300) ? 0.5 * (jmin_full + jmax_zero) : (jmin_full < 1e300 ? jmin_full : jmax_zero));
    for (size_t i = 0; i < M; i++) {
      if (!(J[i] == J[i])) viol = 1e300;
      else if (lam[i] > 1e-12 && lam[i] < cap - 1e-12) viol = std::max(viol, std::fabs(J[i] - th));
      else if (lam[i] >= cap - 1e-12) viol = std::max(viol, th - J[i]);
      else viol = std::max(viol, J[i] - th);
    }
    chk[0] = viol; chk[1] = th; chk[2] = (double)nfr;
  }

  // The particles' condensed quadratics (H_i, g_i) around the accepted point, all particles, as the host solve reads them: read back (or
  // all-gathered) from what the last round left, with that round's applied step and particle 0's held shared controls.
  void fetch_quadratics() {
    std::vector<double> dl(ncv);
    std::vector<int> act0(ncv);
    held.resize(ncv);
    Hh.resize(M * (size_t)ncv * ncv); gh.resize(M * (size_t)ncv);
    if (!epi_multi) {
      HIP_CHECK(hipMemcpyAsync(Hh.data(), w.Hc_part.p, Hh.size() * D8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(gh.data(), w.gc_part.p, gh.size() * D8, hipMemcpyDeviceToHost, s));
    } else {  // all-gather through one all-reduce of a zero-padded buffer [H of every particle | g of every particle]
      const size_t nH = (size_t)ncv * ncv, tot = M * (nH + ncv);
      w.epi_gath.ensure(tot * D8);
      HIP_CHECK(hipMemsetAsync(w.epi_gath.p, 0, tot * D8, s));
      HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + off * nH, w.Hc_part.p, Ml * nH * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + M * nH + off * ncv, w.gc_part.p, Ml * (size_t)ncv * D8, hipMemcpyDeviceToDevice, s));
      allreduce(c, w.epi_gath.p, tot, ncclFloat64, ncclSum);
      HIP_CHECK(hipMemcpyAsync(Hh.data(), w.epi_gath.p, M * nH * D8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(gh.data(), w.epi_gath.d() + M * nH, M * (size_t)ncv * D8, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipMemcpyAsync(dl.data(), w.as_delta.p, ncv * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(act0.data(), w.as_act.p, ncv * sizeof(int), hipMemcpyDeviceToHost, s));  // (particle 0's stages < Nc come first)
    HIP_CHECK(hipStreamSynchronize(s));
    for (int r = 0; r < ncv; r++) held[r] = act0[r] != 0 ? 1 : 0;
    for (size_t i = 0; i < M; i++) {
      double *Hi = &Hh[i * (size_t)ncv * ncv], *gi = &gh[i * (size_t)ncv];
      mirror_upper(Hi, ncv);
      if (i == 0)
        for (int r = 0; r < ncv; r++)
          if (held[r]) Hi[r + (size_t)ncv * r] = 1.0;  // (the 1e30 penalty of a held shared control is not part of the cost; the step there is zero)
      for (int r = 0; r < ncv; r++) {  // gradient at the accepted point = gradient at the last round's base + H_i (applied step)
        double acc = 0.0;
        for (int cc = 0; cc < ncv; cc++) acc += (held[cc] ? 0.0 : Hi[r + (size_t)ncv * cc] * dl[cc]);
        gi[r] += acc;
      }
      if (o.user[i] != 1.0) {
        for (size_t e_ = 0; e_ < (size_t)ncv * ncv; e_++) Hi[e_] *= o.user[i];
        for (int r = 0; r < ncv; r++) gi[r] *= o.user[i];
      }
    }
  }
};

std::optional<int> ConeSolve::epigraph_path() {
  const int ncv = cons_horizon(p).nc;
  const bool epi_on = c->opt[OPT_CONE_EPIGRAPH] != 0.0 && forced != 3 && !(q.barrier_mu > 0.0) && (double)M * ncv * ncv <= 2e7 && !(p->flags & PMPC_FORCE_GENERIC);
  if (!epi_on) return std::nullopt;
  return Epigraph(*this).run();
}

}  // namespace

extern "C" int lcone_body(pmpc_ctx *c, const pmpc_problem *p0, double smooth_alpha, pmpc_info *info, int verbose) {
  HIP_CHECK(hipSetDevice(c->device));
  return ConeSolve(c, p0, smooth_alpha, info, verbose).run();
}
