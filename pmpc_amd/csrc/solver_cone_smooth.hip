// solver_cone_smooth.hip — the cone objective of c_lcone_solve with SMOOTHED boxes (log barrier / squareplus, PMPC.jl/src/main.jl:246-279): the
// full-space Newton iteration lcone_smooth_body, called by the dispatch of solver_cone.hip (ConeSolve).  Moved out of solver_cone.hip as it
// stood; shared declarations: solver_internal.h, cone_common.h.
#include "cone_common.h"

extern "C" {

// -------------------------------------------------------------------------------------------------
// cone objective WITH log-barrier smoothing (main.jl:246-262): proximal method of multipliers on the epigraph rows, damped Newton in
// the full space (kernels_epi.hip).  Any number of particles on the threshold — with the barrier a particle's optimum given the shared
// controls depends on its multiplier, so every particle whose cost range brackets the threshold carries a fractional multiplier.
//   F(z, t; lam) = (1 - eps) k t + sum_i psi(J_i(z_i) - t; lam_i) - mu_b sum log(slack),  psi(v; l) = max over m in [0, 1 + eps] of  m v - rho/2 (m - l)^2
// Newton step: per particle the Hessian  m_i grad^2 J_i + grad^2 B_i  (one Riccati factor sweep with cost weight m_i and the barrier
// diagonals) plus, for a row with m_i strictly inside, the rank-one term (1/rho) (grad J_i; -1)(grad J_i; -1)' coupling its variables
// to t: a second sweep with the right-hand side grad J_i gives v_i = K^-1 grad J_i, its condensed gradient and kappa_i = grad J_i' v_i,
// and Sherman-Morrison folds the term into the (Nc u + 1)-dimensional system of the shared controls and t, assembled on the host from
// per-particle scalars.  Returns -1 when the problem is outside what this path covers (the caller takes the weighted-QP iteration).
// -------------------------------------------------------------------------------------------------
int lcone_smooth_body(pmpc_ctx *c, const pmpc_problem *p, double mu_b, pmpc_info *info, int verbose, int smode, double sbeta, bool phase1_start) {
  Workspace &w = c->ws;
  hipStream_t s = c->stream;
  // Sharded particles (equal contiguous blocks, as everywhere): the device work is local — every rank sweeps its own particles —, the host
  // side of the iteration is GLOBAL and identical on every rank: the per-particle scalars, condensed blocks and costs are gathered
  // (all-reduce(sum) of a zero-padded table, one per Newton step + one per trial point), so every rank assembles the same (Nc u + 1)
  // system, finds the same threshold and takes the same decisions.  Ml: particles here, M: particles in all.
  const int x = (int)p->xdim, u = (int)p->udim, N = (int)p->N, Ml = (int)p->M, world = c->multi() ? c->world : 1, M = Ml * world;
  const size_t off = (size_t)(c->multi() ? c->rank : 0) * Ml;
  const int Nc = p->Nc < 0 ? N : (int)std::min<long long>(p->Nc, (long long)N), nc = Nc * u;
  const bool has_xb = p->flags & PMPC_HAS_XBOUNDS, has_ub = p->flags & PMPC_HAS_UBOUNDS;
  // (several consensus stages: the condensed Hessians M (Nc u)^2 are gathered to the host every Newton step — bounded)
  // (M = 1: the epigraph row is degenerate — its multiplier is (1 - eps) k whatever t does — and the iteration is plain damped Newton on
  //  (1 - eps) J + the smoothing terms; taken for the squareplus hinge, which the interior-point iteration of the QP path does not know)
  if (p->weights || (p->flags & (PMPC_HAS_SLEW | PMPC_HAS_SLEW0 | PMPC_FORCE_GENERIC | PMPC_F32_MATRICES)) || M < (smode == 1 ? 1 : 2) ||
      !(has_xb || has_ub) || !(mu_b > 0.0) || (double)M * nc * nc > 2e7 || (size_t)3 * N * (x + u) * sizeof(double) > 56 * 1024 /* k_cost_dots keeps a particle's vectors in LDS */)
    return -1;
  const size_t nx = (size_t)Ml * N * x, nu = (size_t)Ml * N * u, D8 = sizeof(double);
  LQArgs a = lq_args_of(c, p, Ml, Nc);
  if (!lq_fast_supported(a)) return -1;
  const double eps = 1e-3, cap = 1.0 + eps;
  const double kk = (p->cone_k > 0 && p->cone_k < (long long)M) ? (double)p->cone_k : (double)M, K = (1.0 - eps) * kk;
  // workspace
  w.X.ensure(nx * D8); w.U.ensure(nu * D8); w.dX.ensure(nx * D8); w.dU.ensure(nu * D8); w.dX2.ensure(nx * D8); w.dU2.ensure(nu * D8);
  w.xm.ensure(nx * D8); w.xd.ensure(nx * D8); w.um.ensure(nu * D8); w.ud.ensure(nu * D8);
  w.es_xm.ensure(nx * D8); w.es_xd.ensure(nx * D8); w.es_um.ensure(nu * D8); w.es_ud.ensure(nu * D8);
  w.es_Dx.ensure(nx * D8); w.es_wx.ensure(nx * D8); w.es_Du.ensure(nu * D8); w.es_wu.ensure(nu * D8);
  w.es_Xt.ensure(nx * D8); w.es_Ut.ensure(nu * D8);
  w.K.ensure((size_t)Ml * N * 64 * D8); w.Hinv.ensure(nu * u * D8);
  w.kff.ensure(nu * D8); w.es_kff2.ensure(nu * D8); w.es_kff3.ensure(nu * D8);
  w.gc_part.ensure((size_t)Ml * std::max(nc, 1) * D8); w.es_gc2.ensure((size_t)Ml * std::max(nc, 1) * D8); w.Hc_part.ensure((size_t)Ml * std::max(nc * nc, 1) * D8);
  w.scratch.ensure((size_t)Ml * 3 * x * std::max(nc, 1) * D8);
  w.es_dots.ensure((size_t)3 * Ml * D8); w.pw.ensure((size_t)Ml * D8); w.Jc.ensure((size_t)Ml * D8);
  w.es_coef.ensure((size_t)2 * Ml * D8);  // [coefficients | sig (input of k_epi_newton)]
  w.es_out2.ensure(4 * D8);  // {step size | barrier value, smallest slack} + {barrier value, smallest slack} of the first trial point
  // gather table of the sharded runs: [H_i | g_i (b) | g_i (a) | dots | one flag per rank] for ALL particles
  const size_t nH = (size_t)nc * nc, tab_H = 0, tab_gb = tab_H + (size_t)M * nH, tab_ga = tab_gb + (size_t)M * nc, tab_dots = tab_ga + (size_t)M * nc, tab_rank = tab_dots + (size_t)3 * M,
               tab_tot = tab_rank + (size_t)4 * world;
  if (c->multi()) w.epi_gath.ensure(tab_tot * D8);
  w.part_sum.ensure(2 * PMPC_RED_BLOCKS * D8); w.part_max.ensure(2 * PMPC_RED_BLOCKS * D8);
  w.duc.ensure((size_t)std::max(nc, 1) * D8); w.fail.ensure(sizeof(int));
  zero_buffers(c, Ml, nc, a);
  a.K = w.K.d(); a.Hinv = w.Hinv.d(); a.kff = w.kff.d(); a.gc_part = w.gc_part.d(); a.Hc_part = w.Hc_part.d(); a.scratch = w.scratch.d();
  a.duc = w.es_zero.d(); a.dX = w.dX.d(); a.dU = w.dU.d(); a.fail = (int *)w.fail.p; a.X = w.X.d(); a.U = w.U.d();
  a.xm = w.xm.d(); a.xd = w.xd.d(); a.um = w.um.d(); a.ud = w.ud.d();
  a.pw = w.pw.d();
  a.Dx = has_xb ? w.es_Dx.d() : nullptr; a.wx = has_xb ? w.es_wx.d() : nullptr;
  a.Du = has_ub ? w.es_Du.d() : nullptr; a.wu = has_ub ? w.es_wu.d() : nullptr;
  w.as_key = -1;  // (the workspace's factor records and warm-start memories of the QP path are overwritten)
  w.warm_key = -1;
  pmpc_info inf;
  memset(&inf, 0, sizeof(inf));
  inf.fast_path = 1;
  auto finish = [&](int status) {
    inf.status = status;
    if (status == 0) {
      HIP_CHECK(hipMemcpyAsync(p->X_out, w.X.p, nx * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(p->U_out, w.U.p, nu * D8, hipMemcpyDeviceToDevice, s));
    } else {
      fill_nan_outputs(c, p);
      w.es_key = -1;
      c->cone_lam_key = -1;
    }
    if (info) *info = inf;
    return status;
  };
  // ---- host pieces ---------------------------------------------------------------------------------------------------------
  std::vector<double> J(M), Jt(M), lam(M, std::log((K / (double)M) / (cap - K / (double)M))), mu(M), sig(M);
  // the arrays the device copies into / out of every Newton step: pinned, kept with the context
  struct Span {
    double *p;
    double &operator[](size_t i) const { return p[i]; }
    double *data() const { return p; }
  };
  const size_t n_H = (size_t)M * std::max(nc * nc, 1), n_g = (size_t)M * std::max(nc, 1), n_pin = n_H + 2 * n_g + (size_t)3 * M + (size_t)M;
  if (c->sm_pinned_bytes < n_pin * D8) {
    if (c->sm_pinned) HIP_WARN(hipHostFree(c->sm_pinned));
    c->sm_pinned = nullptr;
    c->sm_pinned_bytes = 0;
    HIP_CHECK(hipHostMalloc(&c->sm_pinned, n_pin * D8, hipHostMallocDefault));
    c->sm_pinned_bytes = n_pin * D8;
  }
  double *pin = (double *)c->sm_pinned;
  const Span Hh{pin}, gb{pin + n_H}, ga{pin + n_H + n_g}, dots{pin + n_H + 2 * n_g}, coef{pin + n_H + 2 * n_g + (size_t)3 * M};
  double rho = 1.0, out2[2] = {0.0, 0.0};
  std::vector<double> rk((size_t)4 * world);  // per-rank scalars as gathered
  auto combine_out2 = [&]() {  // rk = (barrier value, smallest slack) per rank -> out2, summed / minimised in rank order
    double v = 0.0, m_ = 1e300;
    for (int r = 0; r < world; r++) {
      v += rk[2 * r];
      m_ = (rk[2 * r + 1] < m_ || rk[2 * r + 1] != rk[2 * r + 1]) ? rk[2 * r + 1] : m_;
    }
    out2[0] = v;
    out2[1] = m_;
  };
  // Entropic proximal term (exponential method of multipliers for multipliers boxed in [0, cap]): with l_i = logit(lam_i / cap)
  //   m_i(v) = cap * sigmoid(l_i + v / rho),   psi(v; l_i) = rho cap [softplus(l_i + v / rho) - softplus(l_i)],   psi'' = m (cap - m) / (rho cap) > 0:
  // every row carries a rank-one term, F is smooth (the quadratic proximal term's clipping makes its second derivative jump between 0
  // and 1/rho — at config D the semismooth Newton iteration then flips a handful of rows in and out of the hinge for ever), and the
  // update l_i += v_i / rho sends the multiplier of a row below the threshold to zero geometrically.  `lam` holds the logits.
  // (beyond |w| = 40 the exponential is below the last bit of 1: no libm call.  At config D all but a few dozen of the 4096 rows are
  //  saturated at every evaluation, and the exponentials of solve_t / Fval were more than half of a Newton step's wall time)
  auto sigm = [](double w_) { return w_ > 40.0 ? 1.0 : (w_ < -40.0 ? std::exp(w_) : (w_ >= 0.0 ? 1.0 / (1.0 + std::exp(-w_)) : std::exp(w_) / (1.0 + std::exp(w_)))); };
  auto softplus = [](double w_) { return w_ > 40.0 ? w_ : (w_ < -40.0 ? std::exp(w_) : (w_ > 0.0 ? w_ + std::log1p(std::exp(-w_)) : std::log1p(std::exp(w_)))); };
  auto mult = [&](int i, const std::vector<double> &Jv, double t) { return cap * sigm(lam[i] + (Jv[i] - t) / rho); };
  double t_guess = std::numeric_limits<double>::quiet_NaN();
  auto solve_t = [&](const std::vector<double> &Jv) {  // sum_i m_i(J_i - t) = K  (smooth, strictly decreasing in t): safeguarded Newton
    double lo = 1e300, hi = -1e300;
    for (int i = 0; i < M; i++) { const double c0 = Jv[i] + rho * lam[i]; lo = std::min(lo, c0); hi = std::max(hi, c0); }
    lo -= 50.0 * rho + 1.0; hi += 50.0 * rho + 1.0;
    double tt = (t_guess == t_guess && t_guess > lo && t_guess < hi) ? t_guess : 0.5 * (lo + hi);
    for (int it = 0; it < 200; it++) {
      double sm = 0.0, ds = 0.0;
      for (int i = 0; i < M; i++) {
        const double m = mult(i, Jv, tt);
        sm += m;
        ds += m * (cap - m);
      }
      const double S = sm - K;
      if (S > 0.0) lo = tt; else hi = tt;
      if (std::fabs(S) <= 1e-13 * K || hi - lo <= 1e-15 * std::max(1.0, std::fabs(lo) + std::fabs(hi))) break;
      ds /= rho * cap;  // = -dS/dt
      double tn = ds > 0.0 ? tt + S / ds : 0.5 * (lo + hi);
      if (!(tn > lo && tn < hi)) tn = 0.5 * (lo + hi);
      tt = tn;
    }
    t_guess = tt;
    return tt;
  };
  auto Fval = [&](const std::vector<double> &Jv, double t, double bval) {
    double f = 0.0;
    for (int i = 0; i < M; i++) f += softplus(lam[i] + (Jv[i] - t) / rho) - softplus(lam[i]);
    return K * t + bval + rho * cap * f;
  };
  // barrier terms + particle costs at (Xe, Ue): -> Jv, out2 = {barrier value, smallest slack}
  auto eval_at = [&](const double *Xe, const double *Ue, std::vector<double> &Jv) {
    launch_bar_prep(Xe, Ue, has_xb ? p->lx : nullptr, has_xb ? p->ux : nullptr, has_ub ? p->lu : nullptr, has_ub ? p->uu : nullptr, w.es_Dx.d(), w.es_wx.d(),
                    w.es_Du.d(), w.es_wu.d(), mu_b, (long long)nx, (long long)nu, u, N, Nc, a.owner, w.part_sum.d(), w.part_max.d(), w.es_out2.d(), s, smode, sbeta);
    launch_particle_cost(a, Xe, Ue, w.Jc.d(), s);
    if (!c->multi()) {
      HIP_CHECK(hipMemcpyAsync(out2, w.es_out2.p, 2 * D8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(Jv.data(), w.Jc.p, (size_t)M * D8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      return;
    }
    // [J of every particle | (barrier value, smallest slack) of every rank]
    const size_t tot = (size_t)M + 2 * world;
    HIP_CHECK(hipMemsetAsync(w.epi_gath.p, 0, tot * D8, s));
    HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + off, w.Jc.p, (size_t)Ml * D8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + M + 2 * c->rank, w.es_out2.p, 2 * D8, hipMemcpyDeviceToDevice, s));
    allreduce(c, w.epi_gath.p, tot, ncclFloat64, ncclSum);
    HIP_CHECK(hipMemcpyAsync(Jv.data(), w.epi_gath.p, (size_t)M * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(rk.data(), w.epi_gath.d() + M, (size_t)2 * world * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    combine_out2();
  };
  // ---- starting point: the previous smoothed solution of this shape (strictly inside the same boxes), else the caller's U_prev pulled inside ----
  const long long skey = ((((((long long)x * 131 + u) * 131 + N) * 1000003 + M) * 131 + Nc) * 4 + (has_xb ? 2 : 0) + (has_ub ? 1 : 0)) * 2 + smode;
  bool warm = (phase1_start || !(p->flags & PMPC_COLD_START)) && w.es_key == skey && w.es_U.bytes >= nu * D8;
  const bool lam_mem = c->opt[OPT_CONE_RANK_MEMORY] != 0.0 && !(p->flags & PMPC_COLD_START) && c->cone_lam_key == -(skey + 7) && (int)c->cone_lam.size() == M;
  if (lam_mem) lam = c->cone_lam;
  c->cone_lam_key = -1;
  for (int attempt = 0; attempt < 2; attempt++) {
    if (warm) {
      HIP_CHECK(hipMemcpyAsync(w.U.p, w.es_U.p, nu * D8, hipMemcpyDeviceToDevice, s));
    } else {
      HIP_CHECK(hipMemcpyAsync(w.U.p, p->U_prev, nu * D8, hipMemcpyDeviceToDevice, s));
      if (has_ub && smode == 0) launch_interior(w.U.d(), p->lu, p->uu, (long long)nu, 0.05, s);
    }
    if (c->multi() && nc > 0) broadcast(c, w.U.p, (size_t)nc, ncclFloat64, 0);  // (global particle 0's shared controls)
    launch_share_cons(w.U.d(), Ml, N, u, Nc, s);
    launch_rollout_fast(a, w.U.d(), w.X.d(), s);
    eval_at(w.X.d(), w.U.d(), J);
    if (out2[1] > 0.0 && out2[0] == out2[0]) break;
    if (warm) { warm = false; continue; }
    if (has_xb && !phase1_start) {
      // the caller's controls roll out to states outside their boxes (nothing pulls a STATE inside): phase 1 = the plain-sum problem with
      // the same barrier (the library's interior-point iteration starts anywhere); its controls are strictly inside everything
      pmpc_problem q1 = *p;
      q1.weights = nullptr;
      q1.barrier_mu = mu_b;
      q1.flags |= PMPC_COLD_START;
      pmpc_info i1;
      const int st1 = pmpc_lqp_solve_device(c, &q1, &i1, 0);
      if (verbose) printf("pmpc_hip: smoothed cone objective: start outside the state boxes (smallest slack %.3e); phase 1 (barrier QP) status %d\n", out2[1], st1);
      if (st1 == 0) {
        w.es_U.ensure(nu * D8);
        HIP_CHECK(hipMemcpyAsync(w.es_U.p, p->U_out, nu * D8, hipMemcpyDeviceToDevice, s));
        w.es_key = skey;
        return lcone_smooth_body(c, p, mu_b, info, verbose, smode, sbeta, true);  // (the QP solve may have moved workspace buffers: start over)
      }
    }
    if (verbose) printf("pmpc_hip: smoothed cone objective: no strictly feasible start (smallest slack %.3e)\n", out2[1]);
    return finish(1);
  }
  w.es_key = -1;
  if (lam_mem) {
    // remembered logits may belong to ANOTHER problem of this shape.  A multiplier saturated at the wrong end of [0, cap] takes
    // |l| rho / |J - t| updates to come back: where the costs at the start rank a particle clearly on the other side of the threshold
    // than its remembered multiplier says, the logit is pulled back to +-12 (inside an SCP loop the sides agree and nothing changes)
    std::vector<int> idx(M);
    for (int i = 0; i < M; i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](int a_, int b_) { return J[a_] > J[b_]; });
    const int n_top = (int)(K / cap);  // about this many rows carry the full multiplier
    for (int r = 0; r < M; r++) {
      const int i = idx[r];
      if (lam[i] > 12.0 && r >= n_top + 2) lam[i] = 12.0;
      if (lam[i] < -12.0 && r < n_top - 1) lam[i] = -12.0;
    }
  }
  {
    double jlo = 1e300, jhi = -1e300;
    for (int i = 0; i < M; i++) { jlo = std::min(jlo, J[i]); jhi = std::max(jhi, J[i]); }
    rho = 1e-6 * std::max(1.0, std::max(std::fabs(jlo), std::fabs(jhi)));
  }
  // proximal parameter rho = width of the smoothed hinge in cost units.  The method converges for ANY rho (the multipliers are exact at
  // its fixed point); a narrow hinge makes one multiplier update nearly exact but its inner problem nearly non-smooth — with few rows
  // strictly inside, every Newton step crosses kinks and the line search cuts it to nothing (measured at config D: steps of 1e-4 below
  // rho ~ 1e-3 max|J|) —, a wide one gives inner problems that settle in a few full steps and more multiplier updates.  Adaptive: start
  // wide, narrow by 3 after an inner solve that took full steps, widen by 3 after one that was damped throughout.
  const double rho_min = rho, rho_max = 1e5 * rho;
  rho = lam_mem ? 3.0 * c->cone_rho : 1e4 * rho_min;
  if (!(rho >= rho_min && rho <= rho_max)) rho = 1e4 * rho_min;
  double bval = out2[0], t = solve_t(J), Fcur = Fval(J, t, bval);
  int newton = 0;
  bool converged = false;
  double dl_prev = 1e300, dl_last = 1e300, rho_floor = 0.0;
  std::vector<double> lam_before(M), dlam_prev(M, 0.0), dlam_cur(M, 0.0);
  bool have_prev_delta = false;
  double quad_c = 1e3;  // contraction constant of the Newton steps in their quadratic regime, |step_{n+1}| ~ quad_c |step_n|^2: the largest ratio seen in this solve
  static const bool quad_on = !(getenv("PMPC_SM_QUAD") && atoi(getenv("PMPC_SM_QUAD")) == 0);  // (A/B switch)
  double r_prev = -1.0, rho_at_prev_delta = -1.0;
  int since_extrap = 2;
  for (int outer = 0; outer < 500 && !converged; outer++) {
    bool inner_ok = false;
    const bool last_stage = true;
    const double step_tol = std::max(1e-9, std::min(1e-5, 1e-3 * dl_prev));  // (the inner problems are solved as sharply as the multipliers are known; looser — 1e-1 dl, cap 1e-3 — measured: no fewer Newton steps)  // (the inner problems are solved as sharply as the multipliers are known)
    int n_damped = 0, n_cut = 0;
    double s_prev = -1.0;  // the previous full Newton step of this inner solve
    for (int it = 0; it < 25; it++) {
      t = solve_t(J);
      Fcur = Fval(J, t, bval);
      double summu = 0.0;
      for (int i = 0; i < M; i++) {
        mu[i] = mult(i, J, t);
        sig[i] = mu[i] * (cap - mu[i]) / (rho * cap);
        summu += mu[i];
        coef[i] = std::max(mu[i], 1e-8);  // (cost weight of the sweeps: a particle of multiplier zero keeps a strictly convex sub-problem)
      }
      HIP_CHECK(hipMemcpyAsync(w.pw.p, coef.data() + off, (size_t)Ml * D8, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(w.es_coef.d() + Ml, sig.data() + off, (size_t)Ml * D8, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
      // right-hand side b: gradient of sum m_i J_i + barrier (the barrier arrays were written by the last eval_at at this point)
      launch_grad_prep(a, s);
      launch_bwd_fast(a, true, s);
      if (Nc > 1) launch_cond_fast(a, s);  // off-diagonal blocks of the condensed Hessians
      // (the particles' own Newton steps p_b = -K^-1 b_i are not formed: all that is needed of them is pi_i = grad J_i . p_b = b_i . (-K^-1 grad J_i),
      //  a dot product with the second solve's direction — one forward sweep less per Newton step)
      // right-hand side a_i = grad J_i (unweighted, no barrier shift), same Hessian
      LQArgs ag = a;
      ag.pw = nullptr; ag.wx = ag.wu = nullptr;
      ag.xm = w.es_xm.d(); ag.xd = w.es_xd.d(); ag.um = w.es_um.d(); ag.ud = w.es_ud.d();
      launch_grad_prep(ag, s);
      LQArgs a2 = a;
      a2.xm = ag.xm; a2.xd = ag.xd; a2.um = ag.um; a2.ud = ag.ud;
      a2.kff = w.es_kff2.d(); a2.gc_part = w.es_gc2.d(); a2.dX = w.dX2.d(); a2.dU = w.dU2.d();
      launch_bwd_fast(a2, true, s);
      launch_fwd_fast(a2, s);  // -> -v_i = -K^-1 grad J_i in dX2 / dU2
      launch_cost_dots(a, w.X.d(), w.U.d(), w.dX2.d(), w.dU2.d(), w.dX2.d(), w.dU2.d(), w.es_dots.d(), s, a.wx, a.wu);  // (at least one of the two exists: the path needs boxes)
      // the (Nc u + 1) system: on the device where it applies (1 <= Nc u <= 8) — no read-back of the condensed blocks, no synchronisation
      // before the direction's sweep; sharded: every rank sums its own particles' terms, ONE all-reduce of those sums (<= 55 doubles,
      // the failure flags among them) instead of the table of every particle's blocks.  PMPC_SM_DEV=0: the host loop, for A/B
      static const bool dev_env = !(getenv("PMPC_SM_DEV") && atoi(getenv("PMPC_SM_DEV")) == 0);
      const bool dev_sys = dev_env && nc >= 1 && nc <= 8;
      int failflag = 0;
      if (dev_sys) {
        if (!c->multi()) {
          launch_epi_newton(w.Hc_part.d(), w.gc_part.d(), w.es_gc2.d(), w.es_dots.d(), w.es_coef.d() + Ml, Ml, nc, K - summu, w.es_coef.d(), w.duc.d(), (int *)w.fail.p, s);
        } else {
          const int n_x = launch_epi_newton(w.Hc_part.d(), w.gc_part.d(), w.es_gc2.d(), w.es_dots.d(), w.es_coef.d() + Ml, Ml, nc, K - summu, w.es_coef.d(), w.duc.d(),
                                            (int *)w.fail.p, s, 1, w.epi_gath.d());
          allreduce(c, w.epi_gath.p, (size_t)n_x, ncclFloat64, ncclSum);
          launch_epi_newton(w.Hc_part.d(), w.gc_part.d(), w.es_gc2.d(), w.es_dots.d(), w.es_coef.d() + Ml, Ml, nc, K - summu, w.es_coef.d(), w.duc.d(), (int *)w.fail.p, s, 2,
                            w.epi_gath.d());
        }
        inf.structured_solves += 2;
      } else {
        if (!c->multi()) {
          if (nc > 0) {
            HIP_CHECK(hipMemcpyAsync(Hh.data(), w.Hc_part.p, (size_t)M * nc * nc * D8, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(gb.data(), w.gc_part.p, (size_t)M * nc * D8, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(ga.data(), w.es_gc2.p, (size_t)M * nc * D8, hipMemcpyDeviceToHost, s));
          }
          HIP_CHECK(hipMemcpyAsync(dots.data(), w.es_dots.p, (size_t)3 * M * D8, hipMemcpyDeviceToHost, s));
          HIP_CHECK(hipMemcpyAsync(&failflag, w.fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
          HIP_CHECK(hipStreamSynchronize(s));
        } else {
          // one table, one all-reduce: every rank gets every particle's condensed blocks and scalars (and every rank's failure flag)
          HIP_CHECK(hipMemcpyAsync(&failflag, w.fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
          HIP_CHECK(hipMemsetAsync(w.epi_gath.p, 0, tab_tot * D8, s));
          if (nc > 0) {
            HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + tab_H + off * nH, w.Hc_part.p, (size_t)Ml * nH * D8, hipMemcpyDeviceToDevice, s));
            HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + tab_gb + off * nc, w.gc_part.p, (size_t)Ml * nc * D8, hipMemcpyDeviceToDevice, s));
            HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + tab_ga + off * nc, w.es_gc2.p, (size_t)Ml * nc * D8, hipMemcpyDeviceToDevice, s));
          }
          HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + tab_dots + 3 * off, w.es_dots.p, (size_t)3 * Ml * D8, hipMemcpyDeviceToDevice, s));
          HIP_CHECK(hipStreamSynchronize(s));  // (the flag is on the host)
          const double ff = (double)failflag;
          HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + tab_rank + 4 * c->rank, &ff, D8, hipMemcpyHostToDevice, s));
          allreduce(c, w.epi_gath.p, tab_tot, ncclFloat64, ncclSum);
          if (nc > 0) {
            HIP_CHECK(hipMemcpyAsync(Hh.data(), w.epi_gath.d() + tab_H, (size_t)M * nH * D8, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(gb.data(), w.epi_gath.d() + tab_gb, (size_t)M * nc * D8, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(ga.data(), w.epi_gath.d() + tab_ga, (size_t)M * nc * D8, hipMemcpyDeviceToHost, s));
          }
          HIP_CHECK(hipMemcpyAsync(dots.data(), w.epi_gath.d() + tab_dots, (size_t)3 * M * D8, hipMemcpyDeviceToHost, s));
          HIP_CHECK(hipMemcpyAsync(rk.data(), w.epi_gath.d() + tab_rank, (size_t)4 * world * D8, hipMemcpyDeviceToHost, s));
          HIP_CHECK(hipStreamSynchronize(s));
          for (int r = 0; r < world; r++) failflag = std::max(failflag, (int)rk[4 * r]);
        }
        inf.structured_solves += 2;
        if (failflag) {
          if (verbose) printf("pmpc_hip: smoothed cone objective: a factor sweep failed (flag %d)\n", failflag);
          return finish(2);
        }
        // (nc + 1) system of the shared controls and t
        const int n1 = nc + 1;
        std::vector<double> A((size_t)n1 * n1, 0.0), rhs(n1, 0.0), sol(n1, 0.0), sp(M), kap(M), pi_(M);
        double cc = 0.0;
        for (int i = 0; i < M; i++) {
          kap[i] = std::max(0.0, -dots[3 * i]);
          pi_[i] = dots[3 * i + 1];
          sp[i] = sig[i] / (1.0 + sig[i] * kap[i]);
          const double *Hi = &Hh[(size_t)i * nc * nc], *gbi = &gb[(size_t)i * nc], *gai = &ga[(size_t)i * nc];
          for (int r = 0; r < nc; r++) {
            for (int q_ = 0; q_ < nc; q_++) A[r + (size_t)n1 * q_] += Hi[(r <= q_ ? r : q_) + (size_t)nc * (r <= q_ ? q_ : r)] + sp[i] * gai[r] * gai[q_];
            A[r + (size_t)n1 * nc] -= sp[i] * gai[r];
            A[nc + (size_t)n1 * r] -= sp[i] * gai[r];
            rhs[r] -= gbi[r] + sp[i] * pi_[i] * gai[r];
          }
          cc += sp[i];
          rhs[nc] += sp[i] * pi_[i];
        }
        rhs[nc] -= K - summu;
        A[nc + (size_t)n1 * nc] = cc > 0.0 ? cc : 1.0;  // (no row strictly inside: t stays — it is re-optimised exactly at the next point)
        if (!(cc > 0.0)) {
          rhs[nc] = 0.0;
          for (int r = 0; r < nc; r++) A[r + (size_t)n1 * nc] = A[nc + (size_t)n1 * r] = 0.0;
        }
        {  // Gaussian elimination with partial pivoting (the matrix is positive definite; n1 = Nc u + 1)
          std::vector<double> Mx = A;
          sol = rhs;
          for (int k = 0; k < n1; k++) {
            int pv = k;
            for (int r = k + 1; r < n1; r++)
              if (std::fabs(Mx[r + (size_t)n1 * k]) > std::fabs(Mx[pv + (size_t)n1 * k])) pv = r;
            if (pv != k) {
              for (int q_ = 0; q_ < n1; q_++) std::swap(Mx[k + (size_t)n1 * q_], Mx[pv + (size_t)n1 * q_]);
              std::swap(sol[k], sol[pv]);
            }
            const double d = Mx[k + (size_t)n1 * k];
            if (!(std::fabs(d) > 0.0)) return finish(2);
            for (int r = k + 1; r < n1; r++) {
              const double fct = Mx[r + (size_t)n1 * k] / d;
              for (int q_ = k; q_ < n1; q_++) Mx[r + (size_t)n1 * q_] -= fct * Mx[k + (size_t)n1 * q_];
              sol[r] -= fct * sol[k];
            }
          }
          for (int k = n1 - 1; k >= 0; k--) {
            double v = sol[k];
            for (int q_ = k + 1; q_ < n1; q_++) v -= Mx[k + (size_t)n1 * q_] * sol[q_];
            sol[k] = v / Mx[k + (size_t)n1 * k];
          }
        }
        const double dt = sol[nc];
        for (int i = 0; i < M; i++) {
          double e_ = pi_[i] - dt;
          for (int r = 0; r < nc; r++) e_ += ga[(size_t)i * nc + r] * sol[r];
          coef[i] = sig[i] * e_ / (1.0 + sig[i] * kap[i]);
        }
        // total direction: feed-forward k_b + c_i k_a, shared step du_c
        HIP_CHECK(hipMemcpyAsync(w.es_coef.p, coef.data() + off, (size_t)Ml * D8, hipMemcpyHostToDevice, s));
        if (nc > 0) HIP_CHECK(hipMemcpyAsync(w.duc.p, sol.data(), (size_t)nc * D8, hipMemcpyHostToDevice, s));
      }
      launch_axpy_particle(w.kff.d(), w.es_kff2.d(), w.es_coef.d(), w.es_kff3.d(), (long long)N * u, (long long)nu, s);
      LQArgs a3 = a;
      a3.kff = w.es_kff3.d(); a3.duc = nc > 0 ? w.duc.d() : w.es_zero.d();
      launch_fwd_fast(a3, s);  // -> direction in dX / dU
      // along the step the particle costs are EXACT quadratics in the step length: J_i(al) = J_i + al s_i + al^2/2 q_i with s_i = grad J_i . d,
      // q_i = d' hess J_i d (one pass); only the barrier has to be evaluated at the trial points
      launch_cost_dots(a, w.X.d(), w.U.d(), w.dX.d(), w.dU.d(), w.dX.d(), w.dU.d(), w.es_dots.d(), s);
      launch_step_to(w.X.d(), w.dX.d(), 1.0, w.es_Xt.d(), (long long)nx, s);
      launch_step_to(w.U.d(), w.dU.d(), 1.0, w.es_Ut.d(), (long long)nu, s);
      launch_scp_residual(w.es_Xt.d(), w.X.d(), w.es_Ut.d(), w.U.d(), (long long)Ml * N, x, u, w.es_out2.d(), s, true);
      // (the barrier at the FULL step — the line search's first trial, nearly always the accepted one — rides in the same read-back)
      launch_bar_prep(w.es_Xt.d(), w.es_Ut.d(), has_xb ? p->lx : nullptr, has_xb ? p->ux : nullptr, has_ub ? p->lu : nullptr, has_ub ? p->uu : nullptr, w.es_Dx.d(), w.es_wx.d(),
                      w.es_Du.d(), w.es_wu.d(), mu_b, (long long)nx, (long long)nu, u, N, Nc, a.owner, w.part_sum.d(), w.part_max.d(), w.es_out2.d() + 2, s, smode, sbeta);
      double stepmax = 0.0, out_first[2] = {0.0, 0.0};
      if (!c->multi()) {
        HIP_CHECK(hipMemcpyAsync(dots.data(), w.es_dots.p, (size_t)3 * M * D8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&stepmax, w.es_out2.p, D8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(out_first, w.es_out2.d() + 2, 2 * D8, hipMemcpyDeviceToHost, s));
        if (dev_sys) HIP_CHECK(hipMemcpyAsync(&failflag, w.fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
      } else {  // [dots of every particle | largest step of every rank | (barrier value, smallest slack) of every rank at the full step]
        const size_t tot = (size_t)3 * M + 3 * world;
        HIP_CHECK(hipMemsetAsync(w.epi_gath.p, 0, tot * D8, s));
        HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + 3 * off, w.es_dots.p, (size_t)3 * Ml * D8, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + 3 * M + c->rank, w.es_out2.p, D8, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + 3 * M + world + 2 * c->rank, w.es_out2.d() + 2, 2 * D8, hipMemcpyDeviceToDevice, s));
        allreduce(c, w.epi_gath.p, tot, ncclFloat64, ncclSum);
        std::vector<double> rs(world);
        HIP_CHECK(hipMemcpyAsync(dots.data(), w.epi_gath.p, (size_t)3 * M * D8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(rs.data(), w.epi_gath.d() + 3 * M, (size_t)world * D8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(rk.data(), w.epi_gath.d() + 3 * M + world, (size_t)2 * world * D8, hipMemcpyDeviceToHost, s));
        if (dev_sys) HIP_CHECK(hipMemcpyAsync(&failflag, w.fail.p, sizeof(int), hipMemcpyDeviceToHost, s));  // (the same on every rank: the flags were summed)
        HIP_CHECK(hipStreamSynchronize(s));
        for (int r = 0; r < world; r++) stepmax = (rs[r] > stepmax || rs[r] != rs[r]) ? rs[r] : stepmax;
        combine_out2();
        out_first[0] = out2[0]; out_first[1] = out2[1];
      }
      if (dev_sys && failflag) {
        if (verbose) printf("pmpc_hip: smoothed cone objective: a factor sweep or the Newton system failed (flag %d)\n", failflag);
        return finish(2);
      }
      newton++;
      auto bar_at = [&](const double *Xe, const double *Ue) {  // barrier arrays + value + smallest slack at a point
        launch_bar_prep(Xe, Ue, has_xb ? p->lx : nullptr, has_xb ? p->ux : nullptr, has_ub ? p->lu : nullptr, has_ub ? p->uu : nullptr, w.es_Dx.d(), w.es_wx.d(),
                        w.es_Du.d(), w.es_wu.d(), mu_b, (long long)nx, (long long)nu, u, N, Nc, a.owner, w.part_sum.d(), w.part_max.d(), w.es_out2.d(), s, smode, sbeta);
        if (!c->multi()) {
          HIP_CHECK(hipMemcpyAsync(out2, w.es_out2.p, 2 * D8, hipMemcpyDeviceToHost, s));
          HIP_CHECK(hipStreamSynchronize(s));
          return;
        }
        HIP_CHECK(hipMemsetAsync(w.epi_gath.p, 0, (size_t)2 * world * D8, s));
        HIP_CHECK(hipMemcpyAsync(w.epi_gath.d() + 2 * c->rank, w.es_out2.p, 2 * D8, hipMemcpyDeviceToDevice, s));
        allreduce(c, w.epi_gath.p, (size_t)2 * world, ncclFloat64, ncclSum);
        HIP_CHECK(hipMemcpyAsync(rk.data(), w.epi_gath.p, (size_t)2 * world * D8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        combine_out2();
      };
      // backtracking: strictly inside the boxes, no increase of F beyond its round-off (t re-optimised at every trial point); a step
      // that is already tiny is taken in full as soon as it is feasible — F cannot resolve it
      const double f_noise = 1e-13 * std::max(1.0, std::fabs(Fcur)) * std::sqrt((double)M);
      double al = 1.0, Ft = 0.0, tt = t, bt = 0.0, al_feas = 0.0;  // al_feas: the first trial step strictly inside the boxes
      bool accepted = false;
      for (int ls = 0; ls < 30; ls++) {
        if (ls > 0) {
          launch_step_to(w.X.d(), w.dX.d(), al, w.es_Xt.d(), (long long)nx, s);
          launch_step_to(w.U.d(), w.dU.d(), al, w.es_Ut.d(), (long long)nu, s);
        }
        if (ls == 0) { out2[0] = out_first[0]; out2[1] = out_first[1]; }
        else bar_at(w.es_Xt.d(), w.es_Ut.d());
        if (out2[1] > 0.0 && out2[0] == out2[0]) {
          if (al_feas == 0.0) al_feas = al;
          for (int i = 0; i < M; i++) Jt[i] = J[i] + al * (dots[3 * i] + 0.5 * al * dots[3 * i + 2]);
          bt = out2[0];
          tt = solve_t(Jt);
          Ft = Fval(Jt, tt, bt);
          if (Ft <= Fcur + f_noise || stepmax * al <= 1e-7) { accepted = true; break; }
        }
        al *= 0.5;
      }
      if (!accepted) {
        bar_at(w.X.d(), w.U.d());  // (restores the barrier arrays of the current point)
        if (verbose) printf("pmpc_hip: smoothed cone objective: line search found no decrease (Newton step %d, step size %.3e)\n", newton, stepmax);
        inner_ok = stepmax <= 1e-6;
        break;
      }
      const double dF = Fcur - Ft;
      HIP_CHECK(hipMemcpyAsync(w.X.p, w.es_Xt.p, nx * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(w.U.p, w.es_Ut.p, nu * D8, hipMemcpyDeviceToDevice, s));
      J = Jt; bval = bt; t = tt; Fcur = Ft;
      if (verbose) printf("pmpc_hip: smoothed cone objective: outer %d (rho %.1e) Newton %d  alpha %.4f  step %.3e  F %.12e  decrease %.3e  t %.9e  rows inside %d\n", outer + 1, rho,
                          newton, al, stepmax * al, Fcur, dF, t, (int)std::count_if(mu.begin(), mu.end(), [&](double v) { return v > 1e-6 && v < cap - 1e-6; }));
      if (al < 0.2) n_damped++;
      if (al == 1.0 && stepmax <= step_tol) { inner_ok = true; break; }
      // Full steps in the quadratic regime: after a step s the iterate is off by ~ quad_c s^2.  Once that is a tenth of the tolerance the
      // step that would only confirm it (1e-9 .. 1e-14 in the traces of config D: a third of all Newton steps, two factor sweeps each) is
      // not taken.  quad_c: measured on this solve's own consecutive full steps (the largest ratio seen; 1e3 until there is one).
      if (quad_on && al == 1.0) {
        if (s_prev > 0.0 && s_prev < 1e-2 && stepmax < s_prev) quad_c = std::max(quad_c == 1e3 ? 1.0 : quad_c, std::min(1e6, stepmax / (s_prev * s_prev)));
        if (stepmax <= 1e-3 && 10.0 * quad_c * stepmax * stepmax <= step_tol) { inner_ok = true; break; }
        s_prev = stepmax;
      } else {
        s_prev = -1.0;
      }
      // a hinge too narrow for this start shows at once: step after step cut to a few per cent (every Newton step crosses kinks).  Four of
      // those in a row end the attempt — the remaining twenty would be spent the same way (measured at config D: 50 such steps before the
      // width was right) — and the hinge widens from where the iterate is now
      // (a step cut by the BOXES — the first feasible trial accepted, or nearly — is the barrier doing its work from a start near a
      //  bound, and recovers; only cuts the decrease test demanded beyond feasibility count)
      n_cut = (al < 0.1 && al <= 0.25 * al_feas) ? n_cut + 1 : 0;
      if (n_cut >= 4 && rho < rho_max) break;
    }
    if (!inner_ok) {  // the inner problem was not solved: the multipliers stay, the hinge widens (a smoother inner problem from the same point)
      if (verbose) printf("pmpc_hip: smoothed cone objective: outer %d: inner iteration limit at rho %.1e, widening\n", outer + 1, rho);
      if (rho >= rho_max) break;
      rho_floor = std::max(rho_floor, 3.0 * rho);
      rho = std::min(rho_max, 10.0 * rho);
      continue;
    }
    // multiplier update of the proximal method
    t = solve_t(J);
    double dl = 0.0;
    lam_before = lam;
    for (int i = 0; i < M; i++) {
      const double m_old = cap * sigm(lam[i]), m_new = mult(i, J, t);
      dl = std::max(dl, std::fabs(m_new - m_old));
      lam[i] = std::min(700.0, std::max(-700.0, lam[i] + (J[i] - t) / rho));
    }
    // The multiplier iteration is a fixed-point map that contracts LINEARLY at a fixed hinge width (rate ~ rho / (rho + curvature)): once
    // the width sits on its floor and two successive updates of the rows INSIDE the hinge point the same way with a steady ratio r, the
    // remaining geometric series is summed at once (Aitken):  l += r / (1 - r) * delta.  (Measured at config D: 50 updates at rate 0.74.)
    // Rows at either end of [0, cap] drift to +-infinity at constant speed in the logits anyway and are left alone.
    {
      double num = 0.0, den = 0.0;
      int nin = 0;
      for (int i = 0; i < M; i++) {
        const double m_new = cap * sigm(lam[i]);
        const bool inside = m_new > 1e-4 * cap && m_new < (1.0 - 1e-4) * cap;
        const double d = inside ? lam[i] - lam_before[i] : 0.0;
        if (inside && have_prev_delta) { num += d * dlam_prev[i]; den += dlam_prev[i] * dlam_prev[i]; nin++; }
        dlam_cur[i] = d;
      }
      const double r = den > 0.0 ? num / den : 0.0;
      const bool same_map = rho == rho_at_prev_delta;
      if (have_prev_delta && same_map && nin > 0 && r > 0.3 && r < 0.985 && std::fabs(r - r_prev) <= 0.1 * r && since_extrap >= 2) {
        const double gain = std::min(r / (1.0 - r), 50.0);
        for (int i = 0; i < M; i++)
          if (dlam_cur[i] != 0.0) lam[i] = std::min(700.0, std::max(-700.0, lam[i] + gain * dlam_cur[i]));
        if (verbose) printf("pmpc_hip: smoothed cone objective: outer %d: multiplier updates contract at %.3f: extrapolated (x %.1f, %d rows inside)\n", outer + 1, r, gain, nin);
        have_prev_delta = false;
        since_extrap = 0;
        r_prev = -1.0;
      } else {
        r_prev = (have_prev_delta && same_map) ? r : -1.0;
        dlam_prev.swap(dlam_cur);
        have_prev_delta = true;
        rho_at_prev_delta = rho;
        since_extrap++;
      }
    }
    if (verbose) printf("pmpc_hip: smoothed cone objective: outer %d done (%d Newton steps so far), multiplier change %.3e%s\n", outer + 1, newton, dl, inner_ok ? "" : " (inner limit)");
    (void)last_stage;
    // converged: the multipliers stand still AND they are the multipliers of these costs — complementarity of every epigraph row at the
    // threshold t (a multiplier saturated at the wrong end of [0, cap] also "stands still": its logit moves, its value does not; found
    // by tools/fuzz/fuzz_sequence.py with multipliers remembered from another problem of the same shape)
    double comp = 0.0;
    for (int i = 0; i < M; i++) {
      const double m_i = cap * sigm(lam[i]), v = J[i] - t;
      comp = std::max(comp, v > 0.0 ? v * (cap - m_i) : -v * m_i);
    }
    const bool kkt_ok = comp <= 1e-8 * cap * std::max(1.0, std::fabs(t));
    if (inner_ok && step_tol <= 1e-9 * 1.0000001 && dl <= 1e-7 * cap && kkt_ok) converged = true;
    dl_prev = dl;
    // (a sharper hinge makes the multiplier updates contract faster — wanted while they are far off or contracting slowly; never below a
    //  width whose inner problem this solve has already failed to solve)
    // (the floor is what a failed inner solve from a FAR start taught; next to the fixed point a sharper hinge is solvable again — Newton
    //  starts inside its basin — so the floor decays while the inner solves take full steps)
    if (inner_ok && n_damped == 0) rho_floor *= 0.5;
    if (inner_ok && n_damped == 0 && (dl > 1e-2 * cap || dl > 0.3 * dl_last)) rho = std::max(std::max(rho_min, rho_floor), rho / 3.0);
    else if (n_damped >= 3) rho = std::min(rho_max, 3.0 * rho);
    dl_last = dl;
    Fcur = Fval(J, solve_t(J), bval);
  }
  inf.ipm_iters = newton;
  inf.outer_solves = newton;
  inf.mu = mu_b;
  if (!converged) {
    if (verbose) printf("pmpc_hip: smoothed cone objective: not converged\n");
    return finish(1);
  }
  w.es_U.ensure(nu * D8);
  HIP_CHECK(hipMemcpyAsync(w.es_U.p, w.U.p, nu * D8, hipMemcpyDeviceToDevice, s));
  w.es_key = skey;
  c->cone_lam = lam;
  c->cone_lam_key = -(skey + 7);
  c->cone_rho = rho;
  return finish(0);
}

}  // extern "C"
