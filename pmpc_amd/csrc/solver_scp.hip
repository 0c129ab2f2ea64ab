// solver_scp.hip — the SCP loop with the host out of the loop body (pmpc_scp_loop_device*): one ScpLoop object per call, one method
// per phase.  Host code only; shared declarations: solver_internal.h.
//   run()   per iteration: linearize() unless the previous follow-up did -> sub_problem() -> the solve, with follow_up(true) handed
//           to it through the context's hook record (pmpc_ctx::scp) -> follow_up(false) if what the hook enqueued does not stand
#include "solver_internal.h"
#include "cost_lin.h"
#include "keepout.h"
#include "model_jit.h"
#include "cost_jit.h"
#include "cstr_jit.h"
#include "cstr_rows.h"

static std::atomic<unsigned long long> g_follow_ups[2];  // iterations whose follow-up was taken as enqueued behind the rounds / enqueued after the solve

static bool lin_compact_env() {  // PMPC_LIN_COMPACT=0 switches the compact records off (A/B); read once per process
  static const bool on = !(getenv("PMPC_LIN_COMPACT") && atoi(getenv("PMPC_LIN_COMPACT")) == 0);
  return on;
}
// every pointer of the augmented buffers is there
static bool scp_aug_complete(const pmpc_scp_aug *g) {
  if (!g || !g->Q || !g->x0 || !g->lx || !g->X_out) return false;
  for (int k = 0; k < 2; k++)
    if (!g->f[k] || !g->fx[k] || !g->fu[k] || !g->X_prev[k] || !g->X_ref[k] || !g->xu[k]) return false;
  return true;
}

namespace pmpc_impl {

struct ScpLoop {
  struct Residual { const double *X, *Xp, *U, *Up; double *out; };  // the SCP residual a linearisation launch computes on the side

  // ---- fixed for the loop: the entry's arguments, then what follows from them ----
  pmpc_ctx *const c;
  const int model;
  const double *const params;
  const pmpc_problem *const p0;
  const int steps, first_cold;
  double *const res;
  pmpc_info *const infos;
  const pmpc_scp_cost *const cost;
  const pmpc_scp_cstr *const cstr;
  const pmpc_scp_aug *const aug;
  const int x, u, N, M;
  // Built-in cost: the sub-problem of an iteration tracks X_ref - Q^-1 cx(X_prev).  The shifted reference has two sets in the
  // workspace (Xr), indexed like F below; the shift goes behind every linearisation launch, into the set that launch writes.
  const bool with_cost;
  // Custom cost (kind 2, cost_jit.hip): behind every linearisation launch the gradient kernel writes (cx | cu) into one workspace scratch
  // and launch_ref_shift makes Xr[set] = X_ref - Q^-1 cx and, unless the cost was compiled with uses_u = 0, Ur[set] = U_ref - R^-1 cu,
  // which the sub-problem then tracks; with uses_u = 0 neither cu nor R is touched.
  const bool custom_cost, cost_u;
  // Built-in constraint (keepout.hip): the sub-problem runs at xd = x + K states on the caller's augmented buffers, of which the
  // iterate-dependent ones have two sets, indexed like F; the augmentation goes behind every linearisation launch and its shift.  The
  // trajectory pairs stay at x: the sub-problem's states land in aug->X_out and the follow-up strips them into the pair.
  const bool with_cstr;
  // Custom constraint (kind 2, cstr_jit.hip): behind every linearisation launch and its shift the rows kernel writes (a | h) about the
  // iterate into one workspace scratch and k_rows_augment (cstr_rows.hip) turns them into set `set` of the augmented buffers, where the
  // keep-out kernel does both at once; the sub-problem and the follow-up are the keep-out loop's.
  const bool custom_cstr;
  const int K;
  const bool soc;
  const bool cone_obj;  // the sub-problem is the reference's default path (c_lcone_solve)
  const int jac32;      // (f / fx / fu scratch sets: fx, fu FLOAT arrays then)
  // Compact Jacobian records (jac_compact.h) instead of the dense fx / fu — a third of the bytes of the one kernel of the step that is
  // bound by its write stream — whenever the coming solve is expected to be a warm attempt of the active-set rounds without a rollout
  // (QpSolve::as_start, use_defect), whose sweeps read the records as they are; a solve that takes another turn expands them first
  // (QpSolve::densify).  Never with a constraint: the augmentation reads dense Jacobians.
  const bool compact_ok;
  // trajectory buffers A = (X_prev, U_prev), B = (X_out, U_out); linearisation buffers 0 = (f, fx, fu), 1 = (f2, fx2, fu2)
  double *const XA, *const UA, *const XB, *const UB;
  double *const F[2][3];

  // ---- state of the iteration ----
  double *Xr[2] = {nullptr, nullptr}, *Ur[2] = {nullptr, nullptr}, *cgrad = nullptr;
  unsigned *cost_bad = nullptr, *cstr_bad = nullptr;
  double *crows = nullptr;  // a kind-2 constraint's rows about the iterate: a (M, N, K, x) | h (M, N, K)
  bool compact_set[2] = {false, false};  // what the linearisation buffer sets hold
  int done = 0, cur = 0;
  double *Xp = nullptr, *Up = nullptr, *Xo = nullptr, *Uo = nullptr;  // this iteration's (X_prev, U_prev) and (X_out, U_out) of the pairs
  bool res_dirty = false;  // the slot was zeroed with all the others when the loop started; a repeat must zero it again

  ScpLoop(pmpc_ctx *c_, int model_, const double *params_, const pmpc_problem *p, double *f2, double *fx2, double *fu2, int steps_, int first_cold_,
          double *res_, pmpc_info *infos_, const pmpc_scp_cost *cost_, const pmpc_scp_cstr *cstr_, const pmpc_scp_aug *aug_)
      : c(c_), model(model_), params(params_), p0(p), steps(steps_), first_cold(first_cold_), res(res_), infos(infos_), cost(cost_), cstr(cstr_),
        aug(aug_), x((int)p->xdim), u((int)p->udim), N((int)p->N), M((int)p->M), with_cost(cost_ != nullptr && cost_->kind != 0),
        custom_cost(with_cost && cost_->kind == 2), cost_u(custom_cost && cost_->uses_u != 0),
        with_cstr(cstr_ != nullptr && cstr_->kind != 0), custom_cstr(with_cstr && cstr_->kind == 2), K(with_cstr ? cstr_->K : 0), soc(p->soc_u_interior != nullptr || p->cone_count > 0),
        cone_obj((p->flags & PMPC_CONE_OBJECTIVE) != 0), jac32((p->flags & PMPC_F32_MATRICES) ? 1 : 0),
        compact_ok(lin_compact_env() && !with_cstr && !cone_obj && !jac32 && !c_->multi() && p->Nc >= 0 && p->Nc <= 1 && jac_compact_dims(model_, x, u) &&
                   (p->flags & PMPC_SYMMETRIC_COST) && !(p->flags & (PMPC_HAS_SLEW | PMPC_HAS_SLEW0 | PMPC_FORCE_GENERIC | PMPC_COLD_START)) &&
                   ((p->flags & PMPC_HAS_UBOUNDS) || soc) && !(p->barrier_mu > 0.0) && c_->opt[OPT_AS_DEFECT] != 0.0 && c_->opt[OPT_AS_WARM] != 0.0 &&
                   c_->opt[OPT_POLISH_MU] > 0.0),
        XA(const_cast<double *>(p->X_prev)), UA(const_cast<double *>(p->U_prev)), XB(p->X_out), UB(p->U_out),
        F{{const_cast<double *>(p->f), const_cast<double *>(p->fx), const_cast<double *>(p->fu)}, {f2, fx2, fu2}} {}

  bool warm() const { return done > 0 || !first_cold; }  // this iteration's solve starts from the previous one's

  // nothing runs (the kernels of some other model would read the caller's arrays with ITS dimensions)
  bool refused() const {
    if (!model_known(c, model)) return true;
    // (a runtime-compiled model whose dimensions are not the problem's, or next to fp32-stored matrices: its Jacobians are doubles)
    if (model_custom(model)) {
      int mx = 0, mu = 0;
      if (jac32 || !custom_model_dims(model, &mx, &mu) || mx != x || mu != u) return true;
    }
    // (a cost description the kernels cannot run, and a cost next to fp32-stored matrices — the shift reads Q as doubles)
    if (with_cost && !custom_cost && (jac32 || !obstacle_cost_valid(cost, x))) return true;
    // (a custom cost that is not this context's or not of the problem's dimensions, without parameters, next to fp32-stored matrices, or
    //  without the reference its shift moves: launch_ref_shift reads ref, and the built-in cost's path does not define a null one either)
    if (custom_cost) {
      int cx_ = 0, cu_ = 0, uses = 0;
      if (jac32 || !custom_cost_known(c, cost->id) || !custom_cost_dims(cost->id, &cx_, &cu_, nullptr, &uses) || cx_ != x || cu_ != u ||
          (uses != 0) != cost_u || !cost->cparams || !p0->X_ref || (cost_u && !p0->U_ref))
        return true;
    }
    // (a constraint description the kernels cannot run, incomplete augmented buffers, and a constraint next to what rows on the states are
    //  not solved with: a stage cone, slew penalties, fp32-stored matrices, a sharded context, the squareplus smoothing of the boxes)
    // (a custom constraint that is not this context's, whose dimensions are not the problem's and the descriptor's, or without parameters)
    if (custom_cstr) {
      int gx = 0, gk = 0;
      if (!custom_cstr_known(c, cstr->id) || !custom_cstr_dims(cstr->id, &gx, &gk, nullptr) || gx != x || gk != K || !cstr->gparams) return true;
    }
    return with_cstr && ((!custom_cstr && !keepout_cstr_valid(cstr, x)) || !keepout_strip_dims_valid(p0->xdim, K, p0->udim) || !scp_aug_complete(aug) || soc ||
                         (p0->flags & (PMPC_HAS_SLEW | PMPC_HAS_SLEW0)) || jac32 || c->multi() || p0->smooth_cstr == 1);
  }

  // The linearisation about (X, U) into buffer set `set`, with what rides behind it (the cost's shifted reference, the constraint's
  // augmentation; class 6 with it), and — `fused` — the SCP residual in the same launch.  The one place that chooses the launch form:
  // compact records whenever the solve that reads the set is a warm one (every solve but a cold first).  With a constraint compact_ok
  // is false, so its sets are always dense, as the augmentation needs them.
  void linearize(int set, const double *X, const double *U, const Residual *fused) {
    ProfScope ps(c, 6);
    double *const *f = F[set];
    compact_set[set] = compact_ok && (set != cur || warm());  // (set != cur: the coming iteration's)
    if (compact_set[set] && fused)
      launch_linearize_compact(model, N, M, p0->x0, X, U, params, f[0], f[1], fused->X, fused->Xp, fused->U, fused->Up, x, u, fused->out, c->stream);
    else if (compact_set[set])
      launch_linearize_compact(model, N, M, p0->x0, X, U, params, f[0], f[1], nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, c->stream);
    else if (fused)
      launch_linearize_with_residual(model, N, M, p0->x0, X, U, params, f[0], f[1], f[2], fused->X, fused->Xp, fused->U, fused->Up, x, u, fused->out,
                                     c->stream, jac32);
    else
      launch_linearize(model, N, M, p0->x0, X, U, params, f[0], f[1], f[2], c->stream, jac32);
    if (custom_cost) {
      const long long rows = (long long)M * N;
      double *cu = cost_u ? cgrad + rows * x : nullptr;
      custom_launch_cost_grad(cost->id, N, M, X, U, cost->cparams, cgrad, cu, nullptr, c->stream);
      launch_ref_shift(x, rows, p0->Q, cgrad, p0->X_ref, Xr[set], cost_bad, c->stream);
      if (cost_u) launch_ref_shift(u, rows, p0->R, cu, p0->U_ref, Ur[set], cost_bad, c->stream);
    } else if (with_cost) {
      launch_obstacle_ref_shift(*cost, x, N, M, X, p0->Q, p0->X_ref, Xr[set], cost_bad, c->stream);
    }
    const double *ref = with_cost ? Xr[set] : p0->X_ref;  // (the reference a constraint extends: this iteration's shifted one, else the caller's)
    if (custom_cstr) {
      double *h = crows + (long long)M * N * K * x;
      custom_launch_cstr_rows(cstr->id, N, M, X, cstr->gparams, crows, h, nullptr, cstr_bad, c->stream);
      launch_rows_augment(K, x, u, N, M, crows, h, X, f[0], f[1], f[2], ref, aug->f[set], aug->fx[set], aug->fu[set], aug->X_prev[set], aug->X_ref[set],
                          aug->xu[set], c->stream);
    } else if (with_cstr)
      launch_keepout_augment(*cstr, x, u, N, M, X, f[0], f[1], f[2], ref, aug->f[set], aug->fx[set], aug->fu[set],
                             aug->X_prev[set], aug->X_ref[set], aug->xu[set], c->stream);
  }

  // this iteration's convex sub-problem on linearisation set `set`
  pmpc_problem sub_problem(int set, bool warm_start) const {
    pmpc_problem p = *p0;
    p.f = F[set][0]; p.fx = F[set][1]; p.fu = F[set][2];
    if (with_cost) p.X_ref = Xr[set];
    if (cost_u) p.U_ref = Ur[set];
    p.X_prev = Xp; p.U_prev = Up; p.X_out = Xo; p.U_out = Uo;
    p.flags = p0->flags | PMPC_STATIC_CONS_BOUNDS;
    if (warm_start) p.flags |= PMPC_PREV_IS_LAST_SOLUTION;
    else p.flags &= ~(unsigned)PMPC_PREV_IS_LAST_SOLUTION;
    if (with_cstr) {  // the restated problem: rows on the states as upper bounds on the K auxiliary states
      p.xdim = (size_t)(x + K);
      p.f = aug->f[set]; p.fx = aug->fx[set]; p.fu = aug->fu[set]; p.X_prev = aug->X_prev[set];
      p.X_ref = (with_cost || p0->X_ref) ? aug->X_ref[set] : nullptr;
      p.Q = aug->Q; p.x0 = aug->x0; p.lx = aug->lx; p.ux = aug->xu[set]; p.X_out = aug->X_out;
      // X_prev~ holds zeros where the last output holds the rows' values: the flag's promise does not hold for the augmented arrays
      p.flags = (p.flags | PMPC_HAS_XBOUNDS) & ~(unsigned)PMPC_PREV_IS_LAST_SOLUTION;
    }
    return p;
  }

  // residual of this iteration (+ the next iteration's linearisation, into the other buffer set)
  void follow_up(bool with_next) {
    const bool next = with_next && done + 1 < steps;
    const long long rows = (long long)M * (long long)N;
    if (with_cstr) {  // the strip comes first: the residual and the next linearisation read the stripped states
      {
        ProfScope ps(c, 7);
        launch_keepout_strip_residual(aug->X_out, Xo, Xp, Uo, Up, rows, x, K, u, res + done, c->stream, res_dirty);
        res_dirty = true;
      }
      if (next) linearize(cur ^ 1, Xo, Uo, nullptr);
      return;
    }
    if (next && !res_dirty && !c->multi()) {  // both in ONE launch (independent work)
      const Residual r{Xo, Xp, Uo, Up, res + done};
      linearize(cur ^ 1, Xo, Uo, &r);
      res_dirty = true;
      return;
    }
    {
      ProfScope ps(c, 7);
      launch_scp_residual(Xo, Xp, Uo, Up, rows, x, u, res + done, c->stream, res_dirty);
      res_dirty = true;
    }
    if (c->multi()) allreduce(c, res + done, 1, ncclFloat64, ncclMax);
    if (next) linearize(cur ^ 1, Xo, Uo, nullptr);
  }

  int run() {
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipMemsetAsync(res, 0, (size_t)steps * sizeof(double), c->stream));  // (the residual kernel takes a maximum into its slot)
    if (with_cost) {
      for (DevBuf &b : c->ws.cost_ref) b.ensure((size_t)p0->M * p0->N * p0->xdim * sizeof(double));
      Xr[0] = c->ws.cost_ref[0].d(); Xr[1] = c->ws.cost_ref[1].d();
      cost_bad = cost_bad_counter(c);
    }
    if (custom_cost) {
      const size_t rows = (size_t)p0->M * p0->N;
      c->ws.cost_grad.ensure(rows * (p0->xdim + (cost_u ? p0->udim : 0)) * sizeof(double));
      cgrad = c->ws.cost_grad.d();
      if (cost_u) {
        for (DevBuf &b : c->ws.cost_uref) b.ensure(rows * p0->udim * sizeof(double));
        Ur[0] = c->ws.cost_uref[0].d(); Ur[1] = c->ws.cost_uref[1].d();
      }
    }
    if (custom_cstr) {
      c->ws.cstr_rows.ensure((size_t)p0->M * p0->N * K * (p0->xdim + 1) * sizeof(double));
      crows = c->ws.cstr_rows.d();
      cstr_bad = cstr_bad_counter(c);
    }
    bool lin_ready = false;  // the linearisation of iteration `done` is already enqueued (valid speculation of the previous one)
    for (; done < steps; done++, cur ^= 1) {
      Xp = (done & 1) ? XB : XA; Up = (done & 1) ? UB : UA; Xo = (done & 1) ? XA : XB; Uo = (done & 1) ? UA : UB;
      if (!lin_ready) linearize(cur, Xp, Up, nullptr);
      const pmpc_problem p = sub_problem(cur, warm());
      res_dirty = false;
      // the solve enqueues follow_up(true) right behind its first batch of active-set rounds, and reads compact records as they are
      ScpHookGuard hook{c};
      c->scp = pmpc_ctx::ScpHook{[this] { follow_up(true); }, false, false, compact_set[cur] ? F[cur][1] : nullptr, model};
      pmpc_info inf;
      const int st = cone_obj ? lcone_body(c, &p, p.barrier_mu > 0.0 ? 1.0 / p.barrier_mu : std::numeric_limits<double>::quiet_NaN(), &inf, 0)
                              : (soc ? pmpc_lsoc_solve_device(c, &p, &inf, 0) : pmpc_lqp_solve_device(c, &p, &inf, 0));
      if (infos) infos[done] = inf;
      if (st != 0) {  // (the failed solve left NaN in ITS outputs: with a constraint the states of the pair are not among them)
        if (with_cstr) launch_fill(Xo, std::numeric_limits<double>::quiet_NaN(), (long long)M * N * x, c->stream);
        break;
      }
      lin_ready = c->scp.fired && c->scp.ok;  // residual and next linearisation are in flight behind the accepted rounds
      // (else a speculative copy, if any, was computed from unfinished outputs: redone; the next linearisation is enqueued at the top
      //  of the next iteration, into the other buffer set)
      if (!lin_ready) follow_up(false);
      g_follow_ups[lin_ready ? 0 : 1]++;
    }
    HIP_CHECK(hipGetLastError());
    return done;
  }

  // after a HIP error: status 2 for the iteration it struck, and NaN in both trajectory pairs, which hold unfinished iterates now — as
  // every single-solve entry does with its outputs (res[done..] is undefined).  Never throws.
  void poison() {
    if (infos && done < steps) { memset(&infos[done], 0, sizeof(pmpc_info)); infos[done].status = 2; }
    fail_after_error(c, nullptr, nullptr);
    try {
      const double nan = std::numeric_limits<double>::quiet_NaN();
      const long long ex = (long long)M * N * x, eu = (long long)M * N * u;
      for (double *b : {XA, XB}) if (b) launch_fill(b, nan, ex, c->stream);
      for (double *b : {UA, UB}) if (b) launch_fill(b, nan, eu, c->stream);
      if (with_cstr) launch_fill(aug->X_out, nan, (long long)M * N * (x + K), c->stream);
      HIP_WARN(hipStreamSynchronize(c->stream));
    } catch (...) {
    }
  }
};

}  // namespace pmpc_impl

extern "C" {

void pmpc_scp_loop_follow_ups(unsigned long long *out2, int reset) {
  for (int k = 0; k < 2; k++) {
    if (out2) out2[k] = g_follow_ups[k].load();
    if (reset) g_follow_ups[k].store(0);
  }
}
size_t pmpc_abi_scp_aug_size(void) { return sizeof(pmpc_scp_aug); }

int pmpc_scp_loop_device(pmpc_ctx *c, int model, const double *params, const pmpc_problem *p0, double *f2, double *fx2, double *fu2,
                         int steps, int first_cold, double *res, pmpc_info *infos, int *last_in_out) {
  return pmpc_scp_loop_device_cstr(c, model, params, p0, f2, fx2, fu2, steps, first_cold, res, infos, last_in_out, nullptr, nullptr, nullptr);
}
int pmpc_scp_loop_device_cost(pmpc_ctx *c, int model, const double *params, const pmpc_problem *p0, double *f2, double *fx2, double *fu2,
                              int steps, int first_cold, double *res, pmpc_info *infos, int *last_in_out, const pmpc_scp_cost *cost) {
  return pmpc_scp_loop_device_cstr(c, model, params, p0, f2, fx2, fu2, steps, first_cold, res, infos, last_in_out, cost, nullptr, nullptr);
}
int pmpc_scp_loop_device_cstr(pmpc_ctx *c, int model, const double *params, const pmpc_problem *p0, double *f2, double *fx2, double *fu2,
                              int steps, int first_cold, double *res, pmpc_info *infos, int *last_in_out, const pmpc_scp_cost *cost,
                              const pmpc_scp_cstr *cstr, const pmpc_scp_aug *aug) {
  ScpLoop loop(c, model, params, p0, f2, fx2, fu2, steps, first_cold, res, infos, cost, cstr, aug);
  if (loop.refused()) {
    if (infos && steps > 0) { memset(&infos[0], 0, sizeof(pmpc_info)); infos[0].status = 2; }
    if (last_in_out) *last_in_out = 0;
    return 0;
  }
  try {
    loop.run();
  } catch (const PmpcHipError &) {
    loop.poison();
  }
  if (last_in_out) *last_in_out = loop.done & 1;
  return loop.done;
}

}  // extern "C"
