// solver_cone_smooth.hip — the cone objective of c_lcone_solve with SMOOTHED boxes (log barrier / squareplus, PMPC.jl/src/main.jl:246-279): the
// full-space Newton iteration lcone_smooth_body = one SmoothSolve, called by the dispatch of solver_cone.hip (ConeSolve).  The host
// mathematics of the iteration: cone_smooth_math.h; shared declarations: solver_internal.h, cone_common.h.
#include <optional>

#include "cone_common.h"
#pragma GCC visibility push(hidden)  // (the header's inline functions stay inside the library: no new exported name)
#include "cone_smooth_math.h"
#pragma GCC visibility pop

namespace {

using namespace pmpc_smooth;
constexpr size_t D8 = sizeof(double);

// The two A/B switches of this file, both read at the first smoothed solve of the process:
//   PMPC_SM_QUAD=0  every confirming Newton step is taken (QuadRegime is off) — what ADVICE.md's finding on quad_c asks to re-run with;
//   PMPC_SM_DEV=0   the (Nc u + 1) system is assembled and solved on the host at every Nc u, not only above 8.
struct Switches {
  bool quad, dev;
};
bool env_on(const char *name) { return !(getenv(name) && atoi(getenv(name)) == 0); }
const Switches &switches() {
  static const Switches sw{env_on("PMPC_SM_QUAD"), env_on("PMPC_SM_DEV")};
  return sw;
}

// One read-back of the iteration: values of every particle and of every rank, on the host of EVERY rank — the only place that asks
// c->multi().  One rank: the device-to-host copies, one synchronisation.  Several: a zeroed table, each rank's values at its offset, ONE
// all-reduce(sum), unpacked; what the ranks report one value each of is combined in rank order (NaN propagates).  Declare, then run().
struct Gather {
  pmpc_ctx *c;
  int Ml, world;
  struct Seg {
    enum Kind { particles, sum_min, largest, flag, local } kind;
    const void *src;
    size_t n;  // doubles per particle / per rank (local: bytes)
    void *dst;
    size_t at;  // offset in the table
  };
  std::vector<Seg> segs;
  size_t tot = 0, n_rank = 0;
  Gather(pmpc_ctx *c_, int Ml_, int world_) : c(c_), Ml(Ml_), world(world_) {}

  void add(Seg::Kind kind, const void *src, size_t n, void *dst) {
    if (n == 0) return;
    segs.push_back({kind, src, n, dst, tot});
    if (kind == Seg::local) return;
    tot += n * (kind == Seg::particles ? (size_t)Ml * world : (size_t)world);
    if (kind != Seg::particles) n_rank += n * world;
  }
  void particles(const double *src, size_t per, double *dst) { add(Seg::particles, src, per, dst); }  // dst: all particles, in global order
  void sum_min(const double *src, double *dst) { add(Seg::sum_min, src, 2, dst); }  // a rank's {value, smallest} -> {sum, minimum}
  void largest(const double *src, double *dst) { add(Seg::largest, src, 1, dst); }  // -> the largest, starting from *dst
  void flag(const int *src, int *dst) { add(Seg::flag, src, 1, dst); }              // a rank's int -> the largest (goes through the host)
  void local(const void *src, size_t bytes, void *dst) { add(Seg::local, src, bytes, dst); }  // this rank's own bytes, in the same synchronisation

  void run() {
    hipStream_t s = c->stream;
    if (!c->multi()) {
      for (const Seg &g : segs)
        HIP_CHECK(hipMemcpyAsync(g.dst, g.src, g.kind == Seg::local ? g.n : (g.kind == Seg::flag ? sizeof(int) : g.n * (g.kind == Seg::particles ? (size_t)Ml : 1) * D8), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      return;
    }
    DevBuf &tab = c->ws.epi_gath;
    tab.ensure(tot * D8);
    const size_t off = (size_t)c->rank * Ml;
    bool staged = false;
    for (const Seg &g : segs)
      if (g.kind == Seg::flag) { HIP_CHECK(hipMemcpyAsync(g.dst, g.src, sizeof(int), hipMemcpyDeviceToHost, s)); staged = true; }
    HIP_CHECK(hipMemsetAsync(tab.p, 0, tot * D8, s));
    for (const Seg &g : segs) {
      if (g.kind == Seg::particles) HIP_CHECK(hipMemcpyAsync(tab.d() + g.at + off * g.n, g.src, (size_t)Ml * g.n * D8, hipMemcpyDeviceToDevice, s));
      else if (g.kind == Seg::sum_min || g.kind == Seg::largest) HIP_CHECK(hipMemcpyAsync(tab.d() + g.at + g.n * c->rank, g.src, g.n * D8, hipMemcpyDeviceToDevice, s));
    }
    std::vector<double> ff;
    if (staged) {
      HIP_CHECK(hipStreamSynchronize(s));  // (the flags are on the host)
      for (const Seg &g : segs)
        if (g.kind == Seg::flag) ff.push_back((double)*(const int *)g.dst);
      size_t k = 0;
      for (const Seg &g : segs)
        if (g.kind == Seg::flag) HIP_CHECK(hipMemcpyAsync(tab.d() + g.at + c->rank, &ff[k++], D8, hipMemcpyHostToDevice, s));
    }
    allreduce(c, tab.p, tot, ncclFloat64, ncclSum);
    std::vector<double> rk(n_rank);  // per-rank values as gathered
    size_t k = 0;
    for (const Seg &g : segs) {
      if (g.kind == Seg::particles) HIP_CHECK(hipMemcpyAsync(g.dst, tab.d() + g.at, (size_t)Ml * world * g.n * D8, hipMemcpyDeviceToHost, s));
      else if (g.kind == Seg::local) HIP_CHECK(hipMemcpyAsync(g.dst, g.src, g.n, hipMemcpyDeviceToHost, s));
      else { HIP_CHECK(hipMemcpyAsync(&rk[k], tab.d() + g.at, g.n * world * D8, hipMemcpyDeviceToHost, s)); k += g.n * world; }
    }
    HIP_CHECK(hipStreamSynchronize(s));
    k = 0;
    for (const Seg &g : segs) {
      if (g.kind == Seg::particles || g.kind == Seg::local) continue;
      const double *v = &rk[k];
      k += g.n * world;
      if (g.kind == Seg::sum_min) {
        double sum = 0.0, m_ = 1e300;
        for (int r = 0; r < world; r++) {
          sum += v[2 * r];
          m_ = (v[2 * r + 1] < m_ || v[2 * r + 1] != v[2 * r + 1]) ? v[2 * r + 1] : m_;
        }
        ((double *)g.dst)[0] = sum;
        ((double *)g.dst)[1] = m_;
      } else if (g.kind == Seg::largest) {
        double &m_ = *(double *)g.dst;
        for (int r = 0; r < world; r++) m_ = (v[r] > m_ || v[r] != v[r]) ? v[r] : m_;
      } else {
        int &f = *(int *)g.dst;
        for (int r = 0; r < world; r++) f = std::max(f, (int)v[r]);
      }
    }
  }
};

// -------------------------------------------------------------------------------------------------
// cone objective WITH log-barrier smoothing (main.jl:246-262): proximal method of multipliers on the epigraph rows, damped Newton in
// the full space (kernels_epi.hip).  Any number of particles on the threshold — with the barrier a particle's optimum given the shared
// controls depends on its multiplier, so every particle whose cost range brackets the threshold carries a fractional multiplier.
//   F(z, t; lam) = (1 - eps) k t + sum_i psi(J_i(z_i) - t; lam_i) - mu_b sum log(slack),  psi: the smoothed hinge of HingeRows
// Newton step: per particle the Hessian  m_i grad^2 J_i + grad^2 B_i  (one Riccati factor sweep with cost weight m_i and the barrier
// diagonals) plus the rank-one term psi'' (grad J_i; -1)(grad J_i; -1)' coupling its variables to t: a second sweep with the right-hand
// side grad J_i gives v_i = K^-1 grad J_i, its condensed gradient and kappa_i = grad J_i' v_i, and Sherman-Morrison folds the term into
// the (Nc u + 1)-dimensional system of the shared controls and t (NewtonSystem; on the device for 1 <= Nc u <= 8).
//
// Sharded particles (equal contiguous blocks, as everywhere): the device work is local — every rank sweeps its own particles —, the host
// side of the iteration is GLOBAL and identical on every rank: the per-particle scalars, condensed blocks and costs are gathered (Gather:
// one per Newton step + one per trial point), so every rank assembles the same system, finds the same threshold and takes the same
// decisions.  Ml: particles here, M: particles in all.
//
// One call of lcone_smooth_body.  run() is the iteration read top to bottom; what its phases hand to each other are the members.
// -------------------------------------------------------------------------------------------------
class SmoothSolve {
 public:
  SmoothSolve(pmpc_ctx *c_, const pmpc_problem *p_, double mu_b_, pmpc_info *info_, int verbose_, int smode_, double sbeta_, bool phase1_start_)
      : c(c_), p(p_), info(info_), verbose(verbose_), smode(smode_), phase1_start(phase1_start_), mu_b(mu_b_), sbeta(sbeta_), w(c_->ws), s(c_->stream),
        x((int)p_->xdim), u((int)p_->udim), N((int)p_->N), Ml((int)p_->M), world(c_->multi() ? c_->world : 1), M(Ml * world), Nc(cons_horizon(p_).Nc), nc(cons_horizon(p_).nc),
        off((size_t)(c_->multi() ? c_->rank : 0) * Ml), nx((size_t)Ml * N * x), nu((size_t)Ml * N * u), has_xb(p_->flags & PMPC_HAS_XBOUNDS), has_ub(p_->flags & PMPC_HAS_UBOUNDS),
        dev_sys(switches().dev && nc >= 1 && nc <= 8), aitken(M) {}

  // -1: the problem is outside what this path covers (the caller takes the weighted-QP iteration); else the status
  int run() {
    if (!applies()) return -1;
    set_up();
    if (const std::optional<int> st = starting_point()) return *st;
    reconcile_remembered_multipliers();
    initial_width();
    bool converged = false;
    for (outer = 0; outer < 500 && !converged; outer++) {
      step_tol = step_tolerance(dl_prev);
      const Inner in = inner_solve();
      if (in == Inner::failed) return finish(2);
      if (in == Inner::unsolved) {  // the multipliers stay, the hinge widens (a smoother inner problem from the same point)
        if (verbose) printf("pmpc_hip: smoothed cone objective: outer %d: inner iteration limit at rho %.1e, widening\n", outer + 1, rows.rho);
        if (rows.rho >= width.rho_max) break;
        rows.rho = width.widened(rows.rho);
        continue;
      }
      converged = multiplier_update();
      rows.rho = width.adapted(rows.rho, n_damped, dl_prev, cap);
      Fcur = rows.Fval(J, rows.solve_t(J), bval);
    }
    inf.ipm_iters = newton;
    inf.outer_solves = newton;
    inf.mu = mu_b;
    if (!converged) {
      if (verbose) printf("pmpc_hip: smoothed cone objective: not converged\n");
      return finish(1);
    }
    remember();
    return finish(0);
  }

 private:
  static constexpr double eps = 1e-3, cap = 1.0 + eps;
  enum class Inner { solved, unsolved, failed };
  enum class Step { more, solved, stalled, failed };
  // ---- fixed for the solve ----
  pmpc_ctx *const c;
  const pmpc_problem *const p;
  pmpc_info *const info;
  const int verbose, smode;  // smode 1: squareplus hinge of slope sbeta (mu_b carries 1/alpha), 0: log barrier of weight mu_b
  const bool phase1_start;   // the start in w.es_U is phase 1's answer: taken whatever the cold-start flag says, no second phase 1
  const double mu_b, sbeta;
  Workspace &w;
  const hipStream_t s;
  const int x, u, N, Ml, world, M, Nc, nc;
  const size_t off, nx, nu;  // global index of this rank's first particle; doubles of this rank's states / controls
  const bool has_xb, has_ub;
  const bool dev_sys;  // the (Nc u + 1) system on the device
  // ---- what set_up writes and every later phase reads ----
  // Sweep arguments, none depends on the Newton step.  a (applies: the problem's part): Hessian m_i hess J_i + barrier, right-hand side b =
  // gradient of sum m_i J_i + barrier -> kff, gc_part, Hc_part.  ag: the gradients a_i = grad J_i alone (unweighted, no barrier shift) ->
  // es_xm ...  a2: same Hessian, right-hand side a_i -> es_kff2, es_gc2, dX2 / dU2.  a3: the forward sweep of the total direction.
  LQArgs a, ag, a2, a3;
  double K = 0.0;   // sum of the multipliers of the epigraph rows, (1 - eps) k
  long long skey = 0;  // key of what the context remembers of this shape's smoothed solves
  // the arrays the device copies into / out of every Newton step: pinned, kept with the context (c->sm_pinned), all particles
  double *Hh = nullptr, *gb = nullptr, *ga = nullptr, *dots = nullptr, *coef = nullptr;
  pmpc_info inf;  // set_up zeroes it; the Newton steps count; finish hands it to the caller
  // ---- the iterate: w.X / w.U on the device and, on the host, ----
  HingeRows rows;         // logits, hinge width, threshold guess.  set_up: start values / remembered logits; multiplier_update, run: change them
  std::vector<double> J;  // particle costs at the iterate (eval_at at the start, then newton_step's accepted trial point)
  double bval = 0.0, t = 0.0, Fcur = 0.0;  // barrier value, threshold and F there
  std::vector<double> Jt, mu, sig;  // (newton_step: costs at the trial point; multipliers and curvatures of the rows at the iterate)
  double out2[2] = {0.0, 0.0};  // {barrier value, smallest slack} of the last point evaluated: eval_at, line_search write; starting_point, initial_width, line_search read
  bool lam_mem = false;  // the logits are the ones the context remembered (set_up; reconcile_remembered_multipliers, initial_width read)
  // ---- the outer iteration ----
  int outer = 0, newton = 0;  // multiplier updates so far (the trace prints outer + 1), Newton steps so far
  double step_tol = 0.0, dl_prev = 1e300;  // tolerance of this inner solve; multiplier change of the last update
  int n_damped = 0, n_cut = 0;  // inner_solve resets, newton_step counts: steps cut below 0.2; steps in a row cut by the decrease test
  HingeWidth width;
  Aitken aitken;
  QuadRegime quad;

  bool applies() {
    // (several consensus stages: the condensed Hessians M (Nc u)^2 are gathered to the host every Newton step — bounded)
    // (M = 1: the epigraph row is degenerate — its multiplier is (1 - eps) k whatever t does — and the iteration is plain damped Newton on
    //  (1 - eps) J + the smoothing terms; taken for the squareplus hinge, which the interior-point iteration of the QP path does not know)
    if (p->weights || (p->flags & (PMPC_HAS_SLEW | PMPC_HAS_SLEW0 | PMPC_FORCE_GENERIC | PMPC_F32_MATRICES)) || M < (smode == 1 ? 1 : 2) ||
        !(has_xb || has_ub) || !(mu_b > 0.0) || (double)M * nc * nc > 2e7 || (size_t)3 * N * (x + u) * sizeof(double) > 56 * 1024 /* k_cost_dots keeps a particle's vectors in LDS */)
      return false;
    a = lq_args_of(c, p, Ml, Nc);
    return lq_fast_supported(a);
  }

  void set_up() {
    const double kk = (p->cone_k > 0 && p->cone_k < (long long)M) ? (double)p->cone_k : (double)M;
    K = (1.0 - eps) * kk;
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
    // the table of the sharded runs' gathers (the largest: the host system's) — also the exchange buffer of the device system
    if (c->multi()) w.epi_gath.ensure(((size_t)M * ((size_t)nc * nc + 2 * (size_t)nc + 3) + (size_t)4 * world) * D8);
    w.part_sum.ensure(2 * PMPC_RED_BLOCKS * D8); w.part_max.ensure(2 * PMPC_RED_BLOCKS * D8);
    w.duc.ensure((size_t)std::max(nc, 1) * D8); w.fail.ensure(sizeof(int));
    zero_buffers(c, Ml, nc, a);
    a.K = w.K.d(); a.Hinv = w.Hinv.d(); a.kff = w.kff.d(); a.gc_part = w.gc_part.d(); a.Hc_part = w.Hc_part.d(); a.scratch = w.scratch.d();
    a.duc = w.es_zero.d(); a.dX = w.dX.d(); a.dU = w.dU.d(); a.fail = (int *)w.fail.p; a.X = w.X.d(); a.U = w.U.d();
    a.xm = w.xm.d(); a.xd = w.xd.d(); a.um = w.um.d(); a.ud = w.ud.d();
    a.pw = w.pw.d();
    a.Dx = has_xb ? w.es_Dx.d() : nullptr; a.wx = has_xb ? w.es_wx.d() : nullptr;
    a.Du = has_ub ? w.es_Du.d() : nullptr; a.wu = has_ub ? w.es_wu.d() : nullptr;
    ag = a;
    ag.pw = nullptr; ag.wx = ag.wu = nullptr;
    ag.xm = w.es_xm.d(); ag.xd = w.es_xd.d(); ag.um = w.es_um.d(); ag.ud = w.es_ud.d();
    a2 = a;
    a2.xm = ag.xm; a2.xd = ag.xd; a2.um = ag.um; a2.ud = ag.ud;
    a2.kff = w.es_kff2.d(); a2.gc_part = w.es_gc2.d(); a2.dX = w.dX2.d(); a2.dU = w.dU2.d();
    a3 = a;
    a3.kff = w.es_kff3.d(); a3.duc = nc > 0 ? w.duc.d() : w.es_zero.d();
    w.as_key = -1;  // (the workspace's factor records and warm-start memories of the QP path are overwritten)
    w.warm_key = -1;
    memset(&inf, 0, sizeof(inf));
    inf.fast_path = 1;
    const size_t n_H = (size_t)M * std::max(nc * nc, 1), n_g = (size_t)M * std::max(nc, 1), n_pin = n_H + 2 * n_g + (size_t)3 * M + (size_t)M;
    if (c->sm_pinned_bytes < n_pin * D8) {
      if (c->sm_pinned) HIP_WARN(hipHostFree(c->sm_pinned));
      c->sm_pinned = nullptr;
      c->sm_pinned_bytes = 0;
      HIP_CHECK(hipHostMalloc(&c->sm_pinned, n_pin * D8, hipHostMallocDefault));
      c->sm_pinned_bytes = n_pin * D8;
    }
    Hh = (double *)c->sm_pinned; gb = Hh + n_H; ga = gb + n_g; dots = ga + n_g; coef = dots + (size_t)3 * M;
    J.resize(M); Jt.resize(M); mu.resize(M); sig.resize(M);
    rows.cap = cap; rows.K = K;
    // the multipliers: K spread evenly, or — same shape, not a cold start — the logits the last solve ended with
    skey = ((((((long long)x * 131 + u) * 131 + N) * 1000003 + M) * 131 + Nc) * 4 + (has_xb ? 2 : 0) + (has_ub ? 1 : 0)) * 2 + smode;
    lam_mem = c->opt[OPT_CONE_RANK_MEMORY] != 0.0 && !(p->flags & PMPC_COLD_START) && c->cone_lam_key == -(skey + 7) && (int)c->cone_lam.size() == M;
    if (lam_mem) rows.lam = c->cone_lam;
    else rows.lam.assign(M, std::log((K / (double)M) / (cap - K / (double)M)));
    c->cone_lam_key = -1;
  }

  // exactly what the caller gets: outputs and `info`; a failure forgets what the context remembered of this shape
  int finish(int status) {
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
  }

  // what the next solve of this shape starts from: controls, logits, hinge width
  void remember() {
    w.es_U.ensure(nu * D8);
    HIP_CHECK(hipMemcpyAsync(w.es_U.p, w.U.p, nu * D8, hipMemcpyDeviceToDevice, s));
    w.es_key = skey;
    c->cone_lam = rows.lam;
    c->cone_lam_key = -(skey + 7);
    c->cone_rho = rows.rho;
  }

  // barrier arrays (es_Dx ...: read by the next sweeps) + {barrier value, smallest slack} at a point -> es_out2[out_slot ..]
  void barrier_at(const double *Xe, const double *Ue, int out_slot) {
    launch_bar_prep(Xe, Ue, has_xb ? p->lx : nullptr, has_xb ? p->ux : nullptr, has_ub ? p->lu : nullptr, has_ub ? p->uu : nullptr, w.es_Dx.d(), w.es_wx.d(),
                    w.es_Du.d(), w.es_wu.d(), mu_b, (long long)nx, (long long)nu, u, N, Nc, a.owner, w.part_sum.d(), w.part_max.d(), w.es_out2.d() + out_slot, s, smode, sbeta);
  }
  void barrier_to_host(const double *Xe, const double *Ue) {  // -> out2
    barrier_at(Xe, Ue, 0);
    Gather g(c, Ml, world);
    g.sum_min(w.es_out2.d(), out2);
    g.run();
  }
  // barrier terms + particle costs at (Xe, Ue): -> Jv, out2
  void eval_at(const double *Xe, const double *Ue, std::vector<double> &Jv) {
    barrier_at(Xe, Ue, 0);
    launch_particle_cost(a, Xe, Ue, w.Jc.d(), s);
    Gather g(c, Ml, world);
    g.particles(w.Jc.d(), 1, Jv.data());
    g.sum_min(w.es_out2.d(), out2);
    g.run();
  }
  bool strictly_inside() const { return out2[1] > 0.0 && out2[0] == out2[0]; }

  // The previous smoothed solution of this shape (strictly inside the same boxes), else the caller's U_prev pulled inside; where that rolls
  // out of the state boxes, phase 1.  An answer: the solve ends here with it.
  std::optional<int> starting_point() {
    bool warm = (phase1_start || !(p->flags & PMPC_COLD_START)) && w.es_key == skey && w.es_U.bytes >= nu * D8;
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
      if (strictly_inside()) {
        w.es_key = -1;
        return std::nullopt;
      }
      if (warm) { warm = false; continue; }
      break;
    }
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
        return SmoothSolve(c, p, mu_b, info, verbose, smode, sbeta, true).run();  // (the QP solve may have moved workspace buffers: start over)
      }
    }
    if (verbose) printf("pmpc_hip: smoothed cone objective: no strictly feasible start (smallest slack %.3e)\n", out2[1]);
    return finish(1);
  }

  void reconcile_remembered_multipliers() {
    if (lam_mem) rows.pull_back(J);
  }

  // the hinge width's range and first value, and F at the start
  void initial_width() {
    rows.rho = width.start(J, lam_mem ? c->cone_rho : 0.0);
    bval = out2[0];
    t = rows.solve_t(J);
    Fcur = rows.Fval(J, t, bval);
  }

  // damped Newton on F at fixed multipliers and hinge width, to step_tol
  Inner inner_solve() {
    n_damped = n_cut = 0;
    quad.new_inner_solve();
    for (int it = 0; it < 25; it++) {
      const Step st = newton_step();
      if (st == Step::failed) return Inner::failed;
      if (st == Step::solved) return Inner::solved;
      if (st == Step::stalled) return Inner::unsolved;
    }
    return Inner::unsolved;
  }

  Step newton_step() {
    t = rows.solve_t(J);
    Fcur = rows.Fval(J, t, bval);
    const double summu = rows.newton_weights(J, t, mu, sig, coef);
    HIP_CHECK(hipMemcpyAsync(w.pw.p, coef + off, (size_t)Ml * D8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(w.es_coef.d() + Ml, sig.data() + off, (size_t)Ml * D8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
    two_sweeps();
    inf.structured_solves += 2;
    if (dev_sys) newton_system_on_device(K - summu);
    else if (!newton_system_on_host(K - summu)) return Step::failed;
    double stepmax = 0.0, out_first[2] = {0.0, 0.0};
    if (!direction_and_full_step(stepmax, out_first)) return Step::failed;
    newton++;
    double al = 1.0, al_feas = 0.0, Ft = 0.0, tt = t, bt = 0.0;
    if (!line_search(stepmax, out_first, al, al_feas, Ft, tt, bt)) {
      barrier_to_host(w.X.d(), w.U.d());  // (restores the barrier arrays of the current point)
      if (verbose) printf("pmpc_hip: smoothed cone objective: line search found no decrease (Newton step %d, step size %.3e)\n", newton, stepmax);
      return stepmax <= 1e-6 ? Step::solved : Step::stalled;
    }
    const double dF = Fcur - Ft;
    HIP_CHECK(hipMemcpyAsync(w.X.p, w.es_Xt.p, nx * D8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(w.U.p, w.es_Ut.p, nu * D8, hipMemcpyDeviceToDevice, s));
    J = Jt; bval = bt; t = tt; Fcur = Ft;
    if (verbose) printf("pmpc_hip: smoothed cone objective: outer %d (rho %.1e) Newton %d  alpha %.4f  step %.3e  F %.12e  decrease %.3e  t %.9e  rows inside %d\n", outer + 1, rows.rho,
                        newton, al, stepmax * al, Fcur, dF, t, (int)std::count_if(mu.begin(), mu.end(), [&](double v) { return v > 1e-6 && v < cap - 1e-6; }));
    if (al < 0.2) n_damped++;
    if (al == 1.0 && stepmax <= step_tol) return Step::solved;
    if (switches().quad && al == 1.0) {
      if (quad.full_step(stepmax, step_tol)) return Step::solved;
    } else {
      quad.damped_step();
    }
    // a hinge too narrow for this start shows at once: step after step cut to a few per cent (every Newton step crosses kinks).  Four of
    // those in a row end the attempt — the remaining twenty would be spent the same way (measured at config D: 50 such steps before the
    // width was right) — and the hinge widens from where the iterate is now
    // (a step cut by the BOXES — the first feasible trial accepted, or nearly — is the barrier doing its work from a start near a
    //  bound, and recovers; only cuts the decrease test demanded beyond feasibility count)
    n_cut = (al < 0.1 && al <= 0.25 * al_feas) ? n_cut + 1 : 0;
    return (n_cut >= 4 && rows.rho < width.rho_max) ? Step::stalled : Step::more;
  }

  // The factor sweep with right-hand side b (the barrier arrays were written by the last evaluation at this point), and the second solve
  // with right-hand side a_i = grad J_i -> -v_i = -K^-1 grad J_i in dX2 / dU2; es_dots = {-kappa_i, pi_i, .}.
  // (the particles' own Newton steps p_b = -K^-1 b_i are not formed: all that is needed of them is pi_i = grad J_i . p_b = b_i . (-K^-1 grad J_i),
  //  a dot product with the second solve's direction — one forward sweep less per Newton step)
  void two_sweeps() {
    launch_grad_prep(a, s);
    launch_bwd_fast(a, true, s);
    if (Nc > 1) launch_cond_fast(a, s);  // off-diagonal blocks of the condensed Hessians
    launch_grad_prep(ag, s);
    launch_bwd_fast(a2, true, s);
    launch_fwd_fast(a2, s);
    launch_cost_dots(a, w.X.d(), w.U.d(), w.dX2.d(), w.dU2.d(), w.dX2.d(), w.dU2.d(), w.es_dots.d(), s, a.wx, a.wu);  // (at least one of the two exists: the path needs boxes)
  }

  int epi_newton(double k_minus_summu, int mode) {
    return launch_epi_newton(w.Hc_part.d(), w.gc_part.d(), w.es_gc2.d(), w.es_dots.d(), w.es_coef.d() + Ml, Ml, nc, k_minus_summu, w.es_coef.d(), w.duc.d(), (int *)w.fail.p, s, mode,
                             mode == 0 ? nullptr : w.epi_gath.d());
  }
  // No read-back of the condensed blocks, no synchronisation before the direction's sweep; sharded: every rank sums its own particles'
  // terms, ONE all-reduce of those sums (<= 55 doubles, the failure flags among them) instead of the table of every particle's blocks.
  void newton_system_on_device(double k_minus_summu) {
    if (!c->multi()) {
      epi_newton(k_minus_summu, 0);
      return;
    }
    const int n_x = epi_newton(k_minus_summu, 1);
    allreduce(c, w.epi_gath.p, (size_t)n_x, ncclFloat64, ncclSum);
    epi_newton(k_minus_summu, 2);
  }

  // every particle's condensed blocks and scalars (and every rank's failure flag) to the host; coefficients and shared step back.  false: failed
  bool newton_system_on_host(double k_minus_summu) {
    int failflag = 0;
    Gather g(c, Ml, world);
    g.flag((const int *)w.fail.p, &failflag);
    g.particles(w.Hc_part.d(), (size_t)nc * nc, Hh);
    g.particles(w.gc_part.d(), nc, gb);
    g.particles(w.es_gc2.d(), nc, ga);
    g.particles(w.es_dots.d(), 3, dots);
    g.run();
    if (failflag) {
      if (verbose) printf("pmpc_hip: smoothed cone objective: a factor sweep failed (flag %d)\n", failflag);
      return false;
    }
    NewtonSystem sys(M, nc);
    if (!sys.solve(Hh, gb, ga, dots, sig.data(), k_minus_summu, coef)) return false;
    HIP_CHECK(hipMemcpyAsync(w.es_coef.p, coef + off, (size_t)Ml * D8, hipMemcpyHostToDevice, s));
    if (nc > 0) HIP_CHECK(hipMemcpyAsync(w.duc.p, sys.sol.data(), (size_t)nc * D8, hipMemcpyHostToDevice, s));
    return true;
  }

  // Total direction (feed-forward k_b + c_i k_a, shared step du_c) in dX / dU, and one read-back: its slopes and curvatures, its size and
  // the barrier at the FULL step — the line search's first trial, nearly always the accepted one.  false: failed
  bool direction_and_full_step(double &stepmax, double *out_first) {
    launch_axpy_particle(w.kff.d(), w.es_kff2.d(), w.es_coef.d(), w.es_kff3.d(), (long long)N * u, (long long)nu, s);
    launch_fwd_fast(a3, s);
    // along the step the particle costs are EXACT quadratics in the step length: J_i(al) = J_i + al s_i + al^2/2 q_i with s_i = grad J_i . d,
    // q_i = d' hess J_i d (one pass); only the barrier has to be evaluated at the trial points
    launch_cost_dots(a, w.X.d(), w.U.d(), w.dX.d(), w.dU.d(), w.dX.d(), w.dU.d(), w.es_dots.d(), s);
    launch_step_to(w.X.d(), w.dX.d(), 1.0, w.es_Xt.d(), (long long)nx, s);
    launch_step_to(w.U.d(), w.dU.d(), 1.0, w.es_Ut.d(), (long long)nu, s);
    launch_scp_residual(w.es_Xt.d(), w.X.d(), w.es_Ut.d(), w.U.d(), (long long)Ml * N, x, u, w.es_out2.d(), s, true);
    barrier_at(w.es_Xt.d(), w.es_Ut.d(), 2);
    int failflag = 0;
    Gather g(c, Ml, world);
    g.particles(w.es_dots.d(), 3, dots);
    g.largest(w.es_out2.d(), &stepmax);
    g.sum_min(w.es_out2.d() + 2, out_first);
    if (dev_sys) g.local(w.fail.p, sizeof(int), &failflag);  // (sharded: the same on every rank — the device system summed the flags)
    g.run();
    if (failflag) {
      if (verbose) printf("pmpc_hip: smoothed cone objective: a factor sweep or the Newton system failed (flag %d)\n", failflag);
      return false;
    }
    return true;
  }

  // backtracking: strictly inside the boxes, no increase of F beyond its round-off (t re-optimised at every trial point); a step
  // that is already tiny is taken in full as soon as it is feasible — F cannot resolve it.  true: accepted, the trial point in es_Xt /
  // es_Ut, its costs in Jt, F, threshold and barrier value there in Ft, tt, bt; al_feas: the first trial step strictly inside the boxes
  bool line_search(double stepmax, const double *out_first, double &al, double &al_feas, double &Ft, double &tt, double &bt) {
    const double f_noise = 1e-13 * std::max(1.0, std::fabs(Fcur)) * std::sqrt((double)M);
    for (int ls = 0; ls < 30; ls++) {
      if (ls > 0) {
        launch_step_to(w.X.d(), w.dX.d(), al, w.es_Xt.d(), (long long)nx, s);
        launch_step_to(w.U.d(), w.dU.d(), al, w.es_Ut.d(), (long long)nu, s);
      }
      if (ls == 0) { out2[0] = out_first[0]; out2[1] = out_first[1]; }
      else barrier_to_host(w.es_Xt.d(), w.es_Ut.d());
      if (strictly_inside()) {
        if (al_feas == 0.0) al_feas = al;
        for (int i = 0; i < M; i++) Jt[i] = J[i] + al * (dots[3 * i] + 0.5 * al * dots[3 * i + 2]);
        bt = out2[0];
        tt = rows.solve_t(Jt);
        Ft = rows.Fval(Jt, tt, bt);
        if (Ft <= Fcur + f_noise || stepmax * al <= 1e-7) return true;
      }
      al *= 0.5;
    }
    return false;
  }

  // Multiplier update of the proximal method, with the Aitken extrapolation.  true: converged — the multipliers stand still AND they are
  // the multipliers of these costs: complementarity of every epigraph row at the threshold t (a multiplier saturated at the wrong end of
  // [0, cap] also "stands still": its logit moves, its value does not; found by tools/fuzz/fuzz_sequence.py with multipliers remembered
  // from another problem of the same shape)
  bool multiplier_update() {
    t = rows.solve_t(J);
    const std::vector<double> lam_before = rows.lam;
    const double dl = rows.update(J, t);
    const Aitken::Outcome ex = aitken.step(rows.lam, lam_before, rows.rho, cap);
    if (verbose && ex.extrapolated)
      printf("pmpc_hip: smoothed cone objective: outer %d: multiplier updates contract at %.3f: extrapolated (x %.1f, %d rows inside)\n", outer + 1, ex.r, ex.gain, ex.nin);
    if (verbose) printf("pmpc_hip: smoothed cone objective: outer %d done (%d Newton steps so far), multiplier change %.3e\n", outer + 1, newton, dl);
    const bool kkt_ok = rows.complementarity(J, t) <= 1e-8 * cap * std::max(1.0, std::fabs(t));
    dl_prev = dl;
    return step_tol <= 1e-9 * 1.0000001 && dl <= 1e-7 * cap && kkt_ok;
  }
};

}  // namespace

extern "C" {

int lcone_smooth_body(pmpc_ctx *c, const pmpc_problem *p, double mu_b, pmpc_info *info, int verbose, int smode, double sbeta, bool phase1_start) {
  return SmoothSolve(c, p, mu_b, info, verbose, smode, sbeta, phase1_start).run();
}

}  // extern "C"
