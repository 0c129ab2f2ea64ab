// solver_qp.hip — one convex sub-problem on the QP path (solve_impl_body): what solver.hip's header describes, as a per-solve
// object with one method per phase.  Host code only; shared declarations: solver_internal.h.
//   run()                 refusals, workspace, control boxes, cones, keys, then the dispatch:
//   run_cone_dispatch()   stage cones: warm rounds -> cold rounds -> path following (+ rounds from its iterate)
//   run_box_dispatch()    boxes: warm rounds -> equality-only optimum -> cold rounds -> interior-point iteration (warm, then cold)
#include "solver_internal.h"

namespace {

constexpr int GO_ON = -1000;  // a setup phase that does not end the solve (every other value is the solve's return value)

// One attempt of the active-set rounds on the register-resident path (active_set_fast): what as_blocks builds, as_start decides
// and as_rounds leaves for as_accept.  Plain data.
struct AsAttempt {
  double dual_scale;
  int mode, max_rounds;
  LQArgs b;     // the sweeps' arguments: a copy of QpSolve::a as the dispatch left it, plus the rounds' own fields
  ConeArgs ca;  // stage cones (kernels_cone.hip), if `cone`
  XboxArgs xa;  // state rows (kernels_xbox.hip), if `xbox`
  int *act;
  AsCtl *ctl;
  bool cone, xbox;
  bool refused;     // as_blocks: a buffer the warm start reads was reallocated — nothing to start from
  bool use_defect;  // as_start: the no-rollout warm start (the dynamics defect rides through the first round's sweeps)
  AsCtl h;          // as_rounds: the control block as last published
  int round;        // as_rounds: rounds run
  int n_batches_at_hook;  // as_rounds: batches waited for since the speculation hook fired
};

class QpSolve {
 public:
  QpSolve(pmpc_ctx *c_, const pmpc_problem *p_, pmpc_info *info_, int verbose_, bool soc_)
      : c(c_), p(p_), info(info_), verbose(verbose_), soc(soc_), w(c_->ws), s(c_->stream), f32((p_->flags & PMPC_F32_MATRICES) != 0),
        x((int)p_->xdim), u((int)p_->udim), N((int)p_->N), M((int)p_->M),
        Nc(p_->Nc < 0 ? N : (int)std::min<long long>(p_->Nc, (long long)N)),  // main.jl:127-128 (Nc > N is refused by check_args)
        nc(Nc * u), has_xb(p_->flags & PMPC_HAS_XBOUNDS), has_ub(p_->flags & PMPC_HAS_UBOUNDS), has_slew(p_->flags & PMPC_HAS_SLEW),
        has_slew0(p_->flags & PMPC_HAS_SLEW0), nx((size_t)M * N * x), nu((size_t)M * N * u) {
    memset(&inf, 0, sizeof(inf));
  }
  int run();

 private:
  static constexpr size_t D8 = sizeof(double);
  static constexpr int B = PMPC_RED_BLOCKS;

  // ---- fixed for the solve (holds references into the context only: nothing here needs a destructor) ----
  pmpc_ctx *const c;
  const pmpc_problem *const p;
  pmpc_info *const info;
  const int verbose;
  const bool soc;
  Workspace &w;
  const hipStream_t s;
  const bool f32;
  const int x, u, N, M, Nc, nc;
  const bool has_xb, has_ub, has_slew, has_slew0;
  const size_t nx, nu;
  // set once by the setup phases, in this order
  long long as_prev = -1;  // setup_workspace: accepted active set + solution of the previous solve (valid only if nothing ran since)
  bool fast = false;       // setup_workspace: the register-resident MFMA path
  IpmScal *sc = nullptr;
  double mu_target = 0.0;  // barrier mode
  int ncones = 0, cone_rows = 0;          // setup_cones
  bool cone_as = false, xbox_as = false;  // setup_cones: stage cones / state boxes inside the active-set rounds
  long long as_key = -1, warm_key = -1;   // setup_keys
  double polish_mu = 0.0;                 // setup_keys: option snapshot (0 switches both uses of the rounds off)
  bool as_warm_on = false, as_skip_on = false, as_defect_on = false, polish_on = false, warm_disabled = false;

  // ---- state the phases hand to each other ----
  // Kernel arguments.  setup_workspace fills them.  Dx/wx/Du/wu/du_full/dX/dU are the hand-over: equality_solve nulls the diagonal
  // terms, soc_interior_point and interior_point point them at their own and leave them so, the dispatch nulls them again before
  // rounds that copy `a` (as_blocks, active_set_solve) run.
  LQArgs a;
  // Slabs of the bounded states / controls.  setup_control_boxes (and setup_cones, for working copies) write them; every phase reads
  // them; interior_point sets dz2 around its corrector and clears it again.
  Slab sx, su;
  // What *info receives.  Every phase counts into it; finish() writes it out; run_cone_dispatch snapshots it around the rounds that
  // follow the path-following iteration.
  pmpc_info inf;
  // reset_scalars() is lazy: the warm rounds of the register-resident path never call it.  Written by reset_scalars only.
  bool scalars_reset = false;
  // An accepted active-set point is already in the caller's outputs.  Set by as_accept / active_set_solve, cleared by the dispatch
  // when a later phase rejects that point, read by finish().
  bool outputs_written = false;

  // hash of the problem's shape (x_ = 0: of the controls' shape alone) and of `extra` < `range`: what else the remembered data depend on
  long long shape_key(int x_, long long extra, long long range) const {
    return (((((long long)x_ * 131 + u) * 131 + N) * 1000003 + M) * 131 + Nc) * range + extra;
  }

  int check_args();
  int setup_workspace();
  void setup_slab(Slab &sl, SlabBufs &b, size_t cnt, int d, bool is_u, const double *lo, const double *hi, double *z, double *dz);
  void setup_control_boxes();
  int setup_cones();
  void setup_keys();
  void reset_scalars();
  void densify();
  void equality_solve();
  int finish(int status);
  int equality_phase();
  int soc_interior_point(bool finish_now);
  int interior_point(bool warm);
  int active_set_solve(double dual_scale, int mode, int max_rounds, int xb = 1);
  int active_set_fast(double dual_scale, int mode, int max_rounds, int xb = 1);
  AsAttempt as_blocks(double dual_scale, int mode, int max_rounds, int xb);
  bool as_start(AsAttempt &t);
  void as_rounds(AsAttempt &t);
  int as_accept(AsAttempt &t);
  void dump_state_rows(int round);
  void dump_cone_records();
  int run_cone_dispatch();
  int run_box_dispatch();
};

// refusals and the hand-over to the slew increment form; GO_ON: an ordinary solve follows
int QpSolve::check_args() {
  if (f32 && (p->flags & (PMPC_HAS_SLEW | PMPC_HAS_SLEW0 | PMPC_HAS_XBOUNDS | PMPC_FORCE_GENERIC))) return PMPC_NEEDS_F64;
  if (p->xdim > 0 && p->udim > 0 && p->N > 0 && p->M > 0 && p->Nc <= (long long)p->N && slew_increment_form_applies(c, p, soc))
    return solve_slew_increment_form(c, p, info, verbose);
  HIP_CHECK(hipSetDevice(c->device));
  if (x <= 0 || u <= 0 || N <= 0 || M <= 0 || p->Nc > (long long)N) {
    // Nc > N: the reference indexes U[:, 1:Nc] out of bounds (lqp_utils.jl:17-61 -> BoundsError); here: a failed solve
    if (p->Nc > (long long)N) fprintf(stderr, "pmpc_hip: consensus horizon Nc = %lld exceeds N = %d\n", p->Nc, N);
    inf.status = 2;
    if (x > 0 && u > 0 && N > 0 && M > 0 && p->X_out && p->U_out) fill_nan_outputs(c, p);
    if (info) *info = inf;
    return inf.status;
  }
  return GO_ON;
}

// kernel arguments `a`, workspace buffers, the path (fast) and the fp32-storage gate
int QpSolve::setup_workspace() {
  memset(&a, 0, sizeof(a));
  a.x = x; a.u = u; a.N = N; a.M = M; a.Nc = Nc;
  a.w = has_slew ? u : 0;  // a zero slew vector still takes the augmented path: correct, only slower
  a.n = x + a.w;
  a.reg_x = p->reg_x; a.reg_u = p->reg_u;
  a.f = p->f; a.fx = p->fx; a.fu = p->fu; a.Q = p->Q; a.R = p->R;
  a.jac_compact = (c->scp.compact_fx && c->scp.compact_fx == p->fx) ? c->scp.compact_model + 1 : 0;  // (the SCP loop linearised into compact records of that model: densify())
  a.X_prev = p->X_prev; a.U_prev = p->U_prev; a.X_ref = p->X_ref; a.U_ref = p->U_ref;
  a.owner = (c->rank == 0);
  a.any_slew = (has_slew || has_slew0) ? 1 : 0;
  a.sym_cost = (p->flags & PMPC_SYMMETRIC_COST) ? 1 : 0;
  a.pw = p->weights;
  a.cons_w = c->cons_w_active;  // (set by lcone_body around its sub-problem solves; null otherwise)

  // ---- workspace ---------------------------------------------------------------------------------
  w.X.ensure(nx * D8); w.U.ensure(nu * D8); w.dX.ensure(nx * D8); w.dU.ensure(nu * D8);
  w.dX2.ensure(nx * D8); w.dU2.ensure(nu * D8);
  {  // generic path: K (u x n) per stage; fast path: one 64-double factor record per stage
    size_t kb = nu * a.n * D8, rb = (size_t)M * N * 64 * D8;
    w.K.ensure(kb > rb ? kb : rb);
  }
  w.Hinv.ensure(nu * u * D8);
  w.kff.ensure(nu * D8);
  w.gc_part.ensure((size_t)M * nc * D8); w.Hc_part.ensure((size_t)M * nc * nc * D8);
  w.scratch.ensure((size_t)M * 3 * a.n * nc * D8);
  w.red_tmp.ensure((size_t)64 * ((size_t)nc * nc + nc) * D8);
  w.Hg.ensure(((size_t)nc * nc + nc + 5) * D8);  // (+ 4: change counters of the active-set rounds, sharded runs)
  w.Lc.ensure(((size_t)nc * nc + (size_t)((nc + 15) / 16) * 272) * D8);  // (+ the inverse diagonal blocks of k_cons_solve_lds)
  w.duc.ensure((size_t)nc * D8);
  w.sc.ensure(sizeof(IpmScal)); w.fail.ensure(sizeof(int)); w.xch.ensure((size_t)c->world * 8 * D8);
  const bool fresh_parts = w.part_sum.bytes == 0;
  w.part_sum.ensure(2 * PMPC_RED_BLOCKS * D8); w.part_cnt.ensure(2 * PMPC_RED_BLOCKS * D8);
  w.part_max.ensure(2 * PMPC_RED_BLOCKS * D8);
  if (fresh_parts) {
    HIP_CHECK(hipMemsetAsync(w.part_sum.p, 0, 2 * PMPC_RED_BLOCKS * D8, s));
    HIP_CHECK(hipMemsetAsync(w.part_cnt.p, 0, 2 * PMPC_RED_BLOCKS * D8, s));
    HIP_CHECK(hipMemsetAsync(w.part_max.p, 0, 2 * PMPC_RED_BLOCKS * D8, s));
  }
  as_prev = w.as_key;  // accepted active set + solution of the previous solve (valid only if nothing ran since)
  w.as_key = -1;
  if (!has_slew || !has_slew0) {
    if (w.zslew.bytes < (size_t)M * D8 || w.zum1.bytes < (size_t)M * u * D8) {
      w.zslew.ensure((size_t)M * D8); w.zslew0.ensure((size_t)M * D8); w.zum1.ensure((size_t)M * u * D8);
      HIP_CHECK(hipMemsetAsync(w.zslew.p, 0, (size_t)M * D8, s));
      HIP_CHECK(hipMemsetAsync(w.zslew0.p, 0, (size_t)M * D8, s));
      HIP_CHECK(hipMemsetAsync(w.zum1.p, 0, (size_t)M * u * D8, s));
    }
  }
  a.slew = has_slew ? p->slew_reg : w.zslew.d();
  a.slew0 = has_slew0 ? p->slew_reg0 : w.zslew0.d();
  a.um1 = has_slew0 ? p->slew_um1 : w.zum1.d();
  a.K = w.K.d(); a.Hinv = w.Hinv.d(); a.kff = w.kff.d();
  a.gc_part = w.gc_part.d(); a.Hc_part = w.Hc_part.d(); a.scratch = w.scratch.d(); a.duc = w.duc.d();
  a.dX = w.dX.d(); a.dU = w.dU.d(); a.fail = (int *)w.fail.p;
  a.X = w.X.d(); a.U = w.U.d();
  fast = !(p->flags & PMPC_FORCE_GENERIC) && lq_fast_supported(a);
  if (!fast && !(p->flags & PMPC_FORCE_GENERIC) && c->opt[OPT_WARN_SLOW_PATH] != 0.0 && !c->warned_slow_path) {
    // a caller who forgets symmetric_cost = True (or picks dimensions nothing is compiled for) would get a several times slower solver
    // silently: say so once per context
    c->warned_slow_path = true;
    const char *why = !a.sym_cost ? "Q, R are not declared symmetric (flag PMPC_SYMMETRIC_COST / DeviceSolver(symmetric_cost=True))"
                      : a.any_slew ? "slew penalties whose increment form (xdim + udim, udim) is not a compiled pair (or N = 1)"
                      : ((size_t)M * N * (size_t)std::max(x, u) * D8 >= (1ull << 31)) ? "the problem exceeds the 2 GiB per-array addressing of the register-resident kernels"
                                                                                       : "(xdim, udim) is not a compiled pair (fast_common.h, PMPC_FAST_DIMS)";
    fprintf(stderr, "pmpc_hip: note: this problem (xdim %d, udim %d) runs on the generic kernels, several times slower than the register-resident MFMA path: %s. "
                    "Said once per context; pmpc_set_option(ctx, \"warn_slow_path\", 0) or PMPC_WARN_SLOW_PATH=0 silences it.\n", x, u, why);
  }
  if (f32) {
    // fp32-storage mode: only the warm-started active-set rounds of an SCP loop (no rollout, no equality phase) read the float
    // arrays; everything else asks the caller (solve_impl) for widened copies
    const bool f32_defect_on = c->opt[OPT_AS_DEFECT] != 0.0;
    if (!(fast && f32_as_dims_supported(x, u) && Nc <= 1 && (p->flags & PMPC_PREV_IS_LAST_SOLUTION) && !(p->flags & PMPC_COLD_START) &&
          f32_defect_on && !(p->barrier_mu > 0.0))) {
      w.as_key = as_prev;  // (nothing ran: the warm-start memory stands for the widened solve)
      return PMPC_NEEDS_F64;
    }
    a.mat32 = 1;
  }
  if (w.zeros.bytes == 0) {
    w.zeros.ensure(64 * D8);
    HIP_CHECK(hipMemsetAsync(w.zeros.p, 0, 64 * D8, s));
  }
  a.zeros = w.zeros.d();
  if (fast) {
    w.xm.ensure(nx * D8); w.xd.ensure(nx * D8); w.um.ensure(nu * D8); w.ud.ensure(nu * D8);
    a.xm = w.xm.d(); a.xd = w.xd.d(); a.um = w.um.d(); a.ud = w.ud.d();
  }
  inf.fast_path = fast ? (f32 ? 2 : 1) : 0;  // (2: the active-set sweeps on fp32-stored matrices — set back to 1 by the widened re-solve)
  sc = (IpmScal *)w.sc.p;

  // ---- 1. equality-only optimum: one Newton step from a dynamics-consistent base point -----------
  mu_target = (p->barrier_mu > 0.0 && (has_xb || has_ub)) ? p->barrier_mu : 0.0;
  if (mu_target > 0.0 && w.part_dev.bytes == 0) {
    w.part_dev.ensure(2 * PMPC_RED_BLOCKS * D8);
    HIP_CHECK(hipMemsetAsync(w.part_dev.p, 0, 2 * PMPC_RED_BLOCKS * D8, s));
  }
  return GO_ON;
}

// failure flag and interior-point scalars: reset lazily — the warm-started active-set rounds (the path an SCP loop takes)
// clear the flag in their own first kernel and never touch the scalars
void QpSolve::reset_scalars() {
  if (scalars_reset) return;
  scalars_reset = true;
  HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
  launch_ipm_exchange(0, false, false, sc, (const int *)w.fail.p, w.xch.d(), c->rank, c->world, nullptr, nullptr, nullptr, 0, s,
                      mu_target, w.part_dev.d());
}

// Compact Jacobian records (jac_compact.h) -> the dense fx / fu the ABI describes, in the caller's own arrays.  Only the sweeps of a warm
// attempt of the active-set rounds (no rollout, Nc <= 1) read the records as they are; every other phase calls this first.  Rare (a solve
// that leaves the warm path): the records are copied aside, then expanded — the dense stacks overlap them.
void QpSolve::densify() {
  if (!a.jac_compact) return;
  ProfScope ps(c, 5);
  const int model = c->scp.compact_model;
  const size_t bytes = (size_t)jac_compact_doubles(model, N, M) * D8;
  w.jac_tmp.ensure(bytes);
  HIP_CHECK(hipMemcpyAsync(w.jac_tmp.p, p->fx, bytes, hipMemcpyDeviceToDevice, s));
  launch_expand_jac(model, N, M, w.jac_tmp.d(), const_cast<double *>(p->fx), const_cast<double *>(p->fu), 0, s);
  a.jac_compact = 0;
  c->scp.compact_fx = nullptr;
  if (verbose) printf("pmpc_hip: compact Jacobian records expanded (the solve left the warm active-set path)\n");
}

void QpSolve::equality_solve() {
  launch_init_base(w.U.d(), p->U_prev, M, N, u, Nc, s);
  if (fast) launch_rollout_fast(a, w.U.d(), w.X.d(), s);
  else launch_rollout(a, w.U.d(), w.X.d(), s);
  a.Dx = a.Du = a.wx = a.wu = nullptr;
  structured_solve(c, a, true, fast);
  inf.structured_solves++;
  launch_axpy(w.X.d(), w.dX.d(), 1.0, (long long)nx, s);
  launch_axpy(w.U.d(), w.dU.d(), 1.0, (long long)nu, s);
}

int QpSolve::finish(int status) {
  inf.status = status;
  if (status == 0) {
    if (!outputs_written) {  // (an accepted active-set point is written to the outputs by its own kernel)
      HIP_CHECK(hipMemcpyAsync(p->X_out, w.X.p, nx * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(p->U_out, w.U.p, nu * D8, hipMemcpyDeviceToDevice, s));
    }
  } else {
    fill_nan_outputs(c, p);
  }
  if (info) *info = inf;
  return status;
}

// ---- slabs of bounded variables ----------------------------------------------------------------
void QpSolve::setup_slab(Slab &sl, SlabBufs &b, size_t cnt, int d, bool is_u, const double *lo, const double *hi, double *z, double *dz) {
  for (DevBuf *q : {&b.tl, &b.tu, &b.ll, &b.lu, &b.cl, &b.cu, &b.D, &b.w}) q->ensure(cnt * D8);
  sl.count = (long long)cnt; sl.d = d; sl.N = N; sl.Nc = Nc; sl.is_u = is_u ? 1 : 0; sl.owner = a.owner;
  sl.lo = lo; sl.hi = hi; sl.z = z; sl.dz = dz;
  sl.tl = b.tl.d(); sl.tu = b.tu.d(); sl.ll = b.ll.d(); sl.lu = b.lu.d(); sl.cl = b.cl.d(); sl.cu = b.cu.d();
  sl.D = b.D.d(); sl.w = b.w.d();
}

void QpSolve::setup_control_boxes() {
  memset(&sx, 0, sizeof(sx));
  memset(&su, 0, sizeof(su));
  if (has_xb) setup_slab(sx, w.sx, nx, x, false, p->lx, p->ux, w.X.d(), w.dX.d());
  if (has_ub) {
    const double *lo = p->lu, *hi = p->uu;
    const long long sukey = shape_key(0, soc ? 1 : 0, 2);  // (the cone solver's copy drops a box side)
    if (Nc > 0 && (M > 1 || c->multi()) && (p->flags & PMPC_STATIC_CONS_BOUNDS) && w.su_key == sukey && w.su_src_lo == p->lu &&
        w.su_src_hi == p->uu && w.su.lo.bytes >= nu * D8) {
      // the caller vouches EXPLICITLY (PMPC_STATIC_CONS_BOUNDS, on any rank count) that the CONTENTS of lu / uu are those of the
      // previous solve of this shape, as inside an SCP loop: the working copy made then — the caller's boxes with particle 0's on
      // the consensus stages — still stands: two 6.5 MB copies and a kernel per solve saved.  Nothing on the device compares
      // contents, so without the flag the copy is remade (a caller that moves a trust region in place just leaves the flag off).
      lo = w.su.lo.d(); hi = w.su.hi.d();
    } else if (Nc > 0 && (M > 1 || c->multi())) {  // consensus bounds = global particle 0's (lqp_utils.jl:329-330)
      w.su_key = -1;  // (valid again only once every copy below is enqueued: a throw in between must not leave a half-built copy trusted)
      w.su.lo.ensure(nu * D8); w.su.hi.ensure(nu * D8);
      HIP_CHECK(hipMemcpyAsync(w.su.lo.p, p->lu, nu * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(w.su.hi.p, p->uu, nu * D8, hipMemcpyDeviceToDevice, s));
      if (c->multi()) {
        // rank 0's bounds of the consensus controls reach every rank: two small broadcasts — or, when the caller vouches that
        // they are the previous solve's (PMPC_STATIC_CONS_BOUNDS: an SCP loop), the copy kept from then (each tiny
        // collective costs tens of microseconds over xGMI, a tenth of a sharded solve)
        const long long bkey = shape_key(0, 0, 1);
        if ((p->flags & PMPC_STATIC_CONS_BOUNDS) && w.cons_key == bkey) {
          HIP_CHECK(hipMemcpyAsync(w.su.lo.p, w.cons_lo.p, (size_t)nc * D8, hipMemcpyDeviceToDevice, s));
          HIP_CHECK(hipMemcpyAsync(w.su.hi.p, w.cons_hi.p, (size_t)nc * D8, hipMemcpyDeviceToDevice, s));
        } else {
          broadcast(c, w.su.lo.p, (size_t)nc, ncclFloat64, 0);
          broadcast(c, w.su.hi.p, (size_t)nc, ncclFloat64, 0);
          w.cons_lo.ensure((size_t)nc * D8); w.cons_hi.ensure((size_t)nc * D8);
          HIP_CHECK(hipMemcpyAsync(w.cons_lo.p, w.su.lo.p, (size_t)nc * D8, hipMemcpyDeviceToDevice, s));
          HIP_CHECK(hipMemcpyAsync(w.cons_hi.p, w.su.hi.p, (size_t)nc * D8, hipMemcpyDeviceToDevice, s));
          w.cons_key = bkey;
        }
      }
      launch_cons_bounds(w.su.lo.d(), w.su.hi.d(), M, N, u, Nc, s);
      lo = w.su.lo.d(); hi = w.su.hi.d();
      w.su_key = sukey; w.su_src_lo = p->lu; w.su_src_hi = p->uu;
    }
    setup_slab(su, w.su, nu, u, true, lo, hi, w.U.d(), w.dU.d());
  }
}

// stage cones: validation, the cone_as / xbox_as decisions, the control boxes' working copies they need, the cone data block
int QpSolve::setup_cones() {
  // general form of the stage cones (pmpc_problem.cone_count > 0): several cones / linear rows per stage, optionally stage-dependent data
  ncones = soc ? (int)p->cone_count : 0;
  cone_rows = 0;
  bool cones_ok = true;
  if (ncones > 0) {
    cones_ok = ncones <= 4 && p->cone_sizes && p->cone_A && p->cone_c;
    for (int k = 0; cones_ok && k < ncones; k++) {
      cones_ok = p->cone_sizes[k] >= 0 && p->cone_sizes[k] <= 3;
      cone_rows += p->cone_sizes[k] + 1;
    }
    cones_ok = cones_ok && cone_rows <= 8;
  }
  if (soc && (has_xb || a.any_slew || (ncones == 0 && p->soc_u_interior == nullptr) || (ncones == 0 && p->soc_q > 0 && (!p->soc_W || !p->soc_w0 || !p->soc_v)) ||
              u > 8 || p->soc_q > 4 || !cones_ok)) {
    fprintf(stderr, "pmpc_hip: pmpc_lsoc_solve_device supports control boxes + stage cones (udim <= 8; one cone soc_q <= 4 with soc_u_interior, or "
                    "the general form: <= 4 cones of size <= 3, <= 8 rows), no state boxes / slew\n");
    return finish(2);
  }
  // Stage cones inside the active-set rounds (kernels_cone.hip: semismooth Newton on the cones' natural map, boxes by the
  // primal-dual active-set rule) — warm-started from the previous solve's set and multipliers, cold-started from soc_u_interior;
  // the path-following iteration below is the fallback.  PMPC_CONE_AS=0 switches it off.
  const bool cone_as_env = c->opt[OPT_CONE_AS] != 0.0;
  cone_as = soc && cone_as_env && fast && cone_as_dims_supported(x, u) &&
                       (ncones > 0 ? cone_as_supported(u, 0) : (p->soc_q > 0 && cone_as_supported(u, (int)p->soc_q)));
  if (soc && ncones > 0 && !cone_as) {
    fprintf(stderr, "pmpc_hip: the general form of the stage cones needs the register-resident path (symmetric cost, compiled dims with udim 2..4)\n");
    return finish(2);
  }
  if (ncones == 0 && soc && p->soc_q > 0) cone_rows = (int)p->soc_q + 1;
  // State boxes inside the active-set rounds (kernels_xbox.hip); PMPC_XBOX_AS=0 switches them off (then a binding state box sends
  // the solve to the interior-point iteration, as before r03).
  const bool xbox_as_env = c->opt[OPT_XBOX_AS] != 0.0;
  xbox_as = !soc && has_xb && xbox_as_env && fast && !f32 && xbox_as_dims_supported(x, u);
  if ((soc && !has_ub && cone_as) || (xbox_as && !has_ub)) {  // no control boxes: the active-set sweeps still read them — unbounded working copies
    w.su.lo.ensure(nu * D8); w.su.hi.ensure(nu * D8);
    w.su_key = -1;
    launch_fill(w.su.lo.d(), -std::numeric_limits<double>::infinity(), (long long)nu, s);
    launch_fill(w.su.hi.d(), std::numeric_limits<double>::infinity(), (long long)nu, s);
    setup_slab(su, w.su, nu, u, true, w.su.lo.d(), w.su.hi.d(), w.U.d(), w.dU.d());
  }
  if (soc && has_ub) {
    // working copy of the control boxes on every path of the cone solver: particle 0's on the consensus stages, and a lower
    // side that the cone implies (thrust >= 0 next to the thrust cone) dropped — see k_cone_drop_lo
    if (su.lo == p->lu) {
      w.su.lo.ensure(nu * D8); w.su.hi.ensure(nu * D8);
      w.su_key = -1;
      HIP_CHECK(hipMemcpyAsync(w.su.lo.p, p->lu, nu * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(w.su.hi.p, p->uu, nu * D8, hipMemcpyDeviceToDevice, s));
      su.lo = w.su.lo.d(); su.hi = w.su.hi.d();
    }
  }
  if (soc && ncones == 0 && p->soc_q > 0) {  // cone data as one block A = [v'; W], c = (v0, w0) for kernels_cone.hip
    w.cone_A.ensure((size_t)(p->soc_q + 1) * u * D8); w.cone_c.ensure((size_t)(p->soc_q + 1) * D8);
    HIP_CHECK(hipMemcpyAsync(w.cone_A.p, p->soc_v, (size_t)u * D8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(w.cone_A.d() + u, p->soc_W, (size_t)p->soc_q * u * D8, hipMemcpyDeviceToDevice, s));
    launch_fill(w.cone_c.d(), p->soc_v0, 1, s);  // (by value: no asynchronous read of the caller's struct)
    HIP_CHECK(hipMemcpyAsync(w.cone_c.d() + 1, p->soc_w0, (size_t)p->soc_q * D8, hipMemcpyDeviceToDevice, s));
    if (has_ub) launch_cone_drop_redundant_lo(w.su.lo.d(), w.cone_A.d(), w.cone_c.d(), (int)p->soc_q, (long long)M * N, u, s);
  }
  return GO_ON;
}

// keys of the remembered sets / iterates and the option snapshot of the active-set rounds
void QpSolve::setup_keys() {
  as_key = shape_key(x, ((fast ? 2 : 0) + (has_xb ? 1 : 0)) * 64 + (soc ? 1 + (long long)p->soc_q + 8 * (long long)cone_rows : 0), 256);
  polish_mu = c->opt[OPT_POLISH_MU];  // 0 switches both uses off
  as_warm_on = c->opt[OPT_AS_WARM] != 0.0; as_skip_on = c->opt[OPT_AS_SKIP] != 0.0; as_defect_on = c->opt[OPT_AS_DEFECT] != 0.0;
  // State boxes: a state cannot be held on its bound this way, but boxes that are there and INACTIVE at the optimum (loose
  // limits, e.g. x in +-20 of the reference's tests/pmpcjl_test.py:164-219) change nothing: the accepted point only has to
  // be checked against them.  A violated state box sends the solve (and later solves of this shape) to the interior-point path.
  polish_on = polish_mu > 0.0 && (has_ub || xbox_as) && mu_target == 0.0 && !(has_xb && !xbox_as && w.xb_block_key == as_key);
  warm_disabled = c->opt[OPT_WARM_START] == 0.0;
  warm_key = shape_key(x, (has_xb ? 2 : 0) + (has_ub ? 1 : 0), 4);
}

// (finish_now = false: the caller finishes — it may replace the last digits by cone rounds started from this iterate, see the dispatch)
int QpSolve::soc_interior_point(bool finish_now) {
  reset_scalars();
  // ---- stage-wise control cones: primal-dual path following on the same Riccati kernels (kernels_soc.hip) ----------
  const int q = (int)p->soc_q;
  w.Hadd.ensure(nu * u * D8); w.wu_soc.ensure(nu * D8);
  const size_t ncz = (size_t)M * N * (q + 1);
  for (DevBuf *b : {&w.soc_zl, &w.soc_zu, &w.soc_dzl, &w.soc_dzu, &w.soc_sl, &w.soc_su, &w.soc_dsl, &w.soc_dsu, &w.soc_cl, &w.soc_cu}) {
    b->ensure(nu * D8);
    HIP_CHECK(hipMemsetAsync(b->p, 0, nu * D8, s));
  }
  for (DevBuf *b : {&w.soc_zc, &w.soc_dzc, &w.soc_sc, &w.soc_dsc, &w.soc_cc}) {
    b->ensure(ncz * D8);
    HIP_CHECK(hipMemsetAsync(b->p, 0, ncz * D8, s));
  }
  SocArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.M = M; sa.N = N; sa.u = u; sa.Nc = Nc; sa.q = q; sa.owner = a.owner;
  sa.U = w.U.d(); sa.dU = w.dU.d(); sa.dU2 = w.dU2.d();
  sa.cl = w.soc_cl.d(); sa.cu = w.soc_cu.d(); sa.cc = w.soc_cc.d();
  sa.lo = has_ub ? su.lo : nullptr; sa.hi = has_ub ? su.hi : nullptr;
  sa.W = p->soc_W; sa.w0 = p->soc_w0; sa.v = p->soc_v; sa.v0 = p->soc_v0;
  sa.zl = w.soc_zl.d(); sa.zu = w.soc_zu.d(); sa.zc = w.soc_zc.d();
  sa.dzl = w.soc_dzl.d(); sa.dzu = w.soc_dzu.d(); sa.dzc = w.soc_dzc.d();
  sa.sl = w.soc_sl.d(); sa.su = w.soc_su.d(); sa.sc = w.soc_sc.d();
  sa.dsl = w.soc_dsl.d(); sa.dsu = w.soc_dsu.d(); sa.dsc = w.soc_dsc.d();
  sa.Hadd = w.Hadd.d(); sa.wu = w.wu_soc.d(); sa.fail = (int *)w.fail.p;
  a.Dx = a.wx = nullptr;
  a.Du = w.Hadd.d();  // full u x u blocks
  a.du_full = 1;
  a.wu = w.wu_soc.d();
  const unsigned long long one_bits = 0x4000000000000000ull;  // 2.0: upper end of the step kernel's search
  std::vector<double> hs(PMPC_RED_BLOCKS), hc(PMPC_RED_BLOCKS);
  double cone_cnt = 1.0;  // number of cones (degree of the complementarity measure), all ranks
  struct { unsigned long long amin; int fail; } host_rd;
  // complementarity mu = sum s'z / (number of cones: one per finite box side, one per stage cone), measured on the
  // device by the prepare kernel; cross-rank: summed
  auto measure = [&](int nblk, double &mu_out) -> int {
    HIP_CHECK(hipMemcpyAsync(hs.data(), w.part_sum.p, nblk * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(hc.data(), w.part_cnt.p, nblk * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&host_rd.fail, w.fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    double sum = 0.0, cnt = 0.0;
    for (int k = 0; k < nblk; k++) { sum += hs[k]; cnt += hc[k]; }
    if (c->multi()) {  // tiny host-staged all-reduce through the device (two doubles)
      double pair[2] = {sum, cnt};
      HIP_CHECK(hipMemcpyAsync(w.xch.p, pair, 2 * D8, hipMemcpyHostToDevice, s));
      allreduce(c, w.xch.p, 2, ncclFloat64, ncclSum);
      allreduce(c, w.fail.p, 1, ncclInt32, ncclMax);
      HIP_CHECK(hipMemcpyAsync(pair, w.xch.p, 2 * D8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(&host_rd.fail, w.fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      sum = pair[0]; cnt = pair[1];
    }
    cone_cnt = std::max(cnt, 1.0);
    mu_out = sum / cone_cnt;
    return host_rd.fail;
  };
  const double mu_tol = 1e-12;  // (C mu with C ~ 3e3 on these problems: trajectories within ~3e-9)
  double mu = 1.0;
  int status = 1, newton = 0;
  // warm start as on the box path: the early iterate (mu <= 0.5) of the previous solve of this
  // shape — controls and duals; the slacks are recomputed from the new data — if it is strictly feasible for them
  const bool soc_warm_off = c->opt[OPT_WARM_START] == 0.0;
  const long long skey = shape_key(x, q * 2 + (has_ub ? 1 : 0), 16);
  bool warm = !soc_warm_off && !(p->flags & PMPC_COLD_START) && w.soc_key == skey, remembered = false;
  int nblk, fl;
soc_restart:
  sa.mu = 1.0; sa.sigmu = 0.0;
  if (warm) {
    HIP_CHECK(hipMemcpyAsync(w.U.p, w.soc_wU.p, nu * D8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(sa.zl, w.soc_wzl.p, nu * D8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(sa.zu, w.soc_wzu.p, nu * D8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(sa.zc, w.soc_wzc.p, ncz * D8, hipMemcpyDeviceToDevice, s));
  } else {
    launch_soc_fill_u(w.U.d(), p->soc_u_interior, (long long)nu, u, s);
  }
  if (fast) launch_rollout_fast(a, w.U.d(), w.X.d(), s);
  else launch_rollout(a, w.U.d(), w.X.d(), s);
  nblk = launch_soc_prepare(sa, warm ? 2 : 0, w.part_sum.d(), w.part_cnt.d(), s);  // cold: z = mu0 s^-1, a centred start
  fl = measure(nblk, mu);
  if (fl && warm) {  // the remembered controls are not strictly inside the new boxes / cones
    if (verbose) printf("pmpc_hip: stage cones: remembered iterate rejected, cold start\n");
    warm = false;
    w.soc_key = -1;
    HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
    goto soc_restart;
  }
  if (fl) return finish(fl == 3 ? 3 : 2);
  // the prepare pass above (cold / warm start) measured mu; from here on the pass that follows every update both
  // measures mu and builds the predictor system of the next iteration (a.corr = 0, sigma = 0)
  sa.corr = 0; sa.sigmu = 0.0;
  nblk = launch_soc_prepare(sa, 1, w.part_sum.d(), w.part_cnt.d(), s);
  fl = measure(nblk, mu);
  if (fl) { status = fl == 3 ? 3 : 2; }
  auto read_step = [&](double &amax) -> int {  // step length of the last step kernel (+ failure flag), across ranks
    if (c->multi()) allreduce(c, &sc->amin_bits, 1, ncclFloat64, ncclMin);  // bit pattern of a non-negative double
    HIP_CHECK(hipMemcpyAsync(&host_rd.amin, &sc->amin_bits, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&host_rd.fail, w.fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    memcpy(&amax, &host_rd.amin, sizeof(double));
    return host_rd.fail;
  };
  // Centring steps at the end, where this iteration alone answers (finish_now): mu <= mu_tol says that s'z is small, not that every cone pair is
  // centred — and for a cone with q >= 2 the tangential part of s o z enters s'z only to second order, so an off-centre pair at mu = 1e-12 leaves
  // its dual up to ~sqrt(mu) off in direction and the controls with it (1e-7 .. 1e-6 against the cone oracle; q = 1 and boxes are polyhedral and
  // do not show it).  Pure Newton steps towards s o z = mu e at the mu reached (sigma = 1, no second-order term) remove that part; mu stays.  Worst
  // error over the cases of tests/test_soc_path_gpu.py after 0 / 2 / 3 / 5 / 8 such steps: 1.1e-6 / 2.9e-7 / 3.1e-8 / 1.6e-10 / 1.6e-11 (the first ones
  // are damped by the 0.99 rule, then the iteration converges as Newton's method does).  Before the rounds (mode 5) none: they replace these digits.
  int centre_left = finish_now ? 5 : 0;
  bool centring = false;
  for (int it = 0; it < 100 && status == 1; it++) {
    // ---- predictor: factorisation, affine step, step polynomial, second-order terms -------------------------------
    a.dX = w.dX.d(); a.dU = w.dU.d();
    structured_solve(c, a, true, fast);
    inf.structured_solves++;
    HIP_CHECK(hipMemcpyAsync(&sc->amin_bits, &one_bits, sizeof(one_bits), hipMemcpyHostToDevice, s));
    sa.corr = 0; sa.sigmu = 0.0;
    nblk = launch_soc_step(sa, &sc->amin_bits, w.part_sum.d(), w.part_cnt.d(), s);
    HIP_CHECK(hipMemcpyAsync(hs.data(), w.part_sum.p, nblk * D8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(hc.data(), w.part_cnt.p, nblk * D8, hipMemcpyDeviceToHost, s));
    double a_aff;
    if (read_step(a_aff)) { status = centring ? 0 : 2; break; }  // (centring: the iterate reached stands)
    if (centring) {  // no second-order term: the step aims at the centre of the iterate, not past an affine step
      HIP_CHECK(hipMemsetAsync(sa.cl, 0, nu * D8, s));
      HIP_CHECK(hipMemsetAsync(sa.cu, 0, nu * D8, s));
      HIP_CHECK(hipMemsetAsync(sa.cc, 0, ncz * D8, s));
    }
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < nblk; k++) { s1 += hs[k]; s2 += hc[k]; }
    if (c->multi()) {
      double pair[2] = {s1, s2};
      HIP_CHECK(hipMemcpyAsync(w.xch.p, pair, 2 * D8, hipMemcpyHostToDevice, s));
      allreduce(c, w.xch.p, 2, ncclFloat64, ncclSum);
      HIP_CHECK(hipMemcpyAsync(pair, w.xch.p, 2 * D8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      s1 = pair[0]; s2 = pair[1];
    }
    a_aff = std::min(1.0, a_aff);
    const double mu_aff = mu + a_aff * (s1 + a_aff * s2) / cone_cnt;  // (S0 + a S1 + a^2 S2) / deg
    double sigma = mu_aff / mu;
    sigma = centring ? 1.0 : std::min(1.0, std::max(0.0, sigma * sigma * sigma));
    // ---- corrector: difference step on the same factorisation -----------------------------------------------------
    sa.corr = 1; sa.sigmu = sigma * mu;
    launch_soc_prepare(sa, 1, w.part_sum.d(), w.part_cnt.d(), s);
    a.dX = w.dX2.d(); a.dU = w.dU2.d();
    structured_solve(c, a, false, fast);
    a.dX = w.dX.d(); a.dU = w.dU.d();
    HIP_CHECK(hipMemcpyAsync(&sc->amin_bits, &one_bits, sizeof(one_bits), hipMemcpyHostToDevice, s));
    launch_soc_step(sa, &sc->amin_bits, w.part_sum.d(), w.part_cnt.d(), s);
    double amax;
    if (read_step(amax)) { status = centring ? 0 : 2; break; }
    const double alpha = std::min(1.0, 0.99 * amax);  // strictly inside the cones, also when the boundary is just beyond 1
    if (!(alpha > 0.0)) { status = centring ? 0 : 2; break; }
    launch_soc_update(sa, alpha, w.X.d(), w.dX.d(), w.dX2.d(), w.U.d(), (long long)nx, (long long)nu, (long long)ncz, s);
    newton++;
    // ---- complementarity of the new iterate + the next predictor system ------------------------------------------
    sa.corr = 0; sa.sigmu = 0.0;
    nblk = launch_soc_prepare(sa, 1, w.part_sum.d(), w.part_cnt.d(), s);
    double mu_new;
    fl = measure(nblk, mu_new);
    if (fl) {  // round-off pushed a pair onto its cone boundary: accept what has been reached if that is the end game
      status = (mu <= 1e2 * mu_tol) ? 0 : (fl == 3 ? 3 : 2);
      break;
    }
    if (verbose) printf("pmpc_hip: soc it %3d  mu %9.3e -> %9.3e  alpha_aff %6.4f  sigma %8.2e  alpha %6.4f\n", newton, mu, mu_new, a_aff, sigma, alpha);
    const bool stalled = alpha < 1e-3 && mu <= 1e2 * mu_tol;  // at the precision floor
    mu = mu_new;
    if (!remembered && !soc_warm_off && mu <= 0.5) {
      for (DevBuf *b : {&w.soc_wU, &w.soc_wzl, &w.soc_wzu}) b->ensure(nu * D8);
      w.soc_wzc.ensure(ncz * D8);
      HIP_CHECK(hipMemcpyAsync(w.soc_wU.p, w.U.p, nu * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(w.soc_wzl.p, sa.zl, nu * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(w.soc_wzu.p, sa.zu, nu * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(w.soc_wzc.p, sa.zc, ncz * D8, hipMemcpyDeviceToDevice, s));
      w.soc_key = skey;
      remembered = true;
    }
    if (centring) {
      if (--centre_left <= 0 || stalled) { status = 0; break; }
    } else if (stalled || (mu <= mu_tol && centre_left <= 0)) {
      status = 0;
      break;
    } else if (mu <= mu_tol) {
      centring = true;
    }
  }
  if (status != 0 && warm) {  // a warm-started run that fails is repeated cold
    if (verbose) printf("pmpc_hip: stage cones: warm-started run failed (status %d), cold start\n", status);
    warm = false; remembered = false; status = 1; newton = 0;
    w.soc_key = -1;
    HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
    goto soc_restart;
  }
  inf.ipm_iters = newton;
  inf.mu = mu;
  if (verbose) printf("pmpc_hip: stage cones: status %d after %d Newton steps\n", status, newton);
  return (finish_now || status != 0) ? finish(status) : 0;
}

// returns 0: the equality-only optimum satisfies every box (done), 1: boxes violated (interior-point phase), 2: failure
int QpSolve::equality_phase() {
  reset_scalars();
  equality_solve();
  if (has_xb) launch_violation(sx, w.part_max.d(), s);
  if (has_ub) launch_violation(su, w.part_max.d() + B, s);
  exchange(c, 1);  // (without boxes: only for the failure flag)
  read_scalars(c);
  inf.max_violation = c->sc_host->viol_max;
  if (*c->fail_host || !(c->sc_host->viol_max == c->sc_host->viol_max)) return 2;
  if (verbose) printf("pmpc_hip: equality-only optimum, max bound violation %.3e\n", c->sc_host->viol_max);
  if (!has_xb && !has_ub) return 0;
  if (c->sc_host->viol_max <= 0.0 && mu_target == 0.0) return 0;  // (a barrier acts on feasible points too)
  return 1;
}

// ---- primal-dual active-set iteration on the control boxes (kernels_ipm.hip, k_as_*) -----------------------------------
// Given a guess of the active set, ONE structured solve from a base point with those controls ON their bounds gives the
// exact optimum on that set; a check pass verifies the KKT signs and, where they fail, applies the primal-dual active-set
// update (release negative multipliers, hold violated boxes).  An unchanged set is the optimum of the QP, complementarity
// exactly zero.  Three uses: (a) WARM START — the accepted set and solution of the previous solve of this shape (consecutive
// SCP sub-problems differ in a few hundred to a few thousand of ~1e6 entries) start the next solve directly: no equality-only
// phase, no interior-point iteration; (b) COLD START — without one, the boxes the equality-only optimum violates are the
// first guess; (c) FINISH of the interior-point iteration — once mu <= polish_mu * mu_peak its iterate names the set
// (l > slack), which replaces the last predictor-corrector iterations (4 sweeps each) by a few factor + forward sweeps.
// If the set does not settle the interior-point iteration runs (on), its state untouched.  The rounds act on the control
// boxes (a state cannot be moved onto its bound without leaving the dynamics; state boxes that do not bind are verified at
// acceptance, see below); not in barrier mode.  DESIGN.md section 2.4.
// mode 1: guess from the interior-point iterate in (w.U, slacks, multipliers); mode 0: the stored set, base point = w.U
// (the previous solution).  Returns 0 accepted (w.X, w.U hold the optimum), 1 not settled, 2 numerical failure.
// Fast path: the rounds run on the device's own decisions (k_as_ctl); the host enqueues as many rounds as the previous
// solve of this shape took before it reads anything back, every kernel of a round that is no longer needed returns at once.
// The base point lives in the caller's output buffers (the forward sweep writes base + step there), so an accepted round
// leaves nothing to copy.  Returns 0 accepted, 1 not settled, 2 numerical failure.
// xb (problems with state boxes on the XBOX sweeps): 1 state rows on, from the stored statuses / multipliers (mode 0), the
// interior-point iterate (mode 1) or nothing (mode 2); 0 state boxes IGNORED (first phase of a cold start, see below); 2 on, nothing
// stored.  mode 4: continue from the point an accepted attempt left in the output buffers (second phase of that cold start).
int QpSolve::active_set_fast(double dual_scale, int mode, int max_rounds, int xb) {
  // (compact Jacobian records serve the no-rollout warm start alone — as_start's use_defect —: every other start rolls out)
  if (!(mode == 0 && as_defect_on && (p->flags & PMPC_PREV_IS_LAST_SOLUTION) && Nc <= 1)) densify();
  AsAttempt t = as_blocks(dual_scale, mode, max_rounds, xb);
  if (t.refused || !as_start(t)) return 1;
  as_rounds(t);
  return as_accept(t);
}

// the argument blocks of an attempt: sweeps (b), stage cones (ca), state rows (xa) — and the buffers behind them
AsAttempt QpSolve::as_blocks(double dual_scale, int mode, int max_rounds, int xb) {
  AsAttempt t;
  memset(&t, 0, sizeof(t));
  t.dual_scale = dual_scale; t.mode = mode; t.max_rounds = max_rounds;
  LQArgs &b = t.b;
  ConeArgs &ca = t.ca;
  XboxArgs &xa = t.xa;
  const double big = 1e30, tol_p = 1e-13;
  w.as_act.ensure(nu * sizeof(int) + 8); w.as_cntp.ensure((size_t)M * 3 * sizeof(int)); w.as_settled.ensure((size_t)M * sizeof(int));
  w.as_ctl.ensure(sizeof(AsCtl)); w.as_delta.ensure((size_t)std::max(nc, 1) * D8);
  int *act = t.act = (int *)w.as_act.p;
  AsCtl *ctl = t.ctl = (AsCtl *)w.as_ctl.p;
  b = a;
  b.Dx = b.wx = b.Du = b.wu = nullptr; b.du_full = 0;
  b.as_act = act; b.as_lo = su.lo; b.as_hi = su.hi; b.as_cnt = (int *)w.as_cntp.p; b.as_big = big; b.as_tol_p = tol_p;
  b.as_settled_out = (int *)w.as_settled.p; b.as_delta = w.as_delta.d(); b.as_ctl = ctl; b.done = &ctl->done;
  w.as_viol.ensure((size_t)M * D8);
  b.as_viol = w.as_viol.d();
  b.Xb = p->X_out; b.Ub = p->U_out; b.Xo = p->X_out; b.Uo = p->U_out;
  {  // checkpointed restart of the later rounds' factor sweeps (kernels_as.hip)
    int slots = 0;  // stages FIRST << k <= N - 1
    if (c->opt[OPT_AS_CKPT] != 0.0 && as_skip_on && nc <= 32)
      while ((PMPC_AS_CK_FIRST << slots) <= N - 1) slots++;
    if (slots > 0) {
      const int ks = (x + 3) / 4;
      w.as_ck.ensure((size_t)M * slots * (64 * ks + 32) * D8);
      w.as_jhi.ensure((size_t)M * sizeof(int));
      if (w.ck_stat.ensure(4 * sizeof(unsigned long long))) HIP_CHECK(hipMemsetAsync(w.ck_stat.p, 0, 4 * sizeof(unsigned long long), s));
      b.as_ck = w.as_ck.d(); b.as_jhi = (int *)w.as_jhi.p; b.ck_slots = slots; b.ck_stat = (unsigned long long *)w.ck_stat.p;
    }
  }
  w.as_key = -1;
  // stage cones (mode 0 warm / 3 cold): Newton terms per round from kernels_cone.hip, see the header there
  const bool cone = t.cone = cone_as && (mode == 0 || mode == 3 || mode == 5);
  b.as_freeze_tol = (cone && Nc == 1) ? c->opt[OPT_AS_FREEZE_TOL] : 0.0;
  if (cone) {
    const int q = (int)p->soc_q;
    const size_t rows = (size_t)M * N;
    w.Hadd.ensure(nu * u * D8); w.wu_soc.ensure(nu * D8); w.cone_uraw.ensure(nu * D8); w.as_open.ensure((size_t)M * sizeof(int));
    const bool z_new = w.cone_z.ensure(rows * cone_rows * D8), rec_new = w.cone_rec.ensure(rows * std::max(ncones, 1) * PMPC_CONE_REC * D8);
    if (z_new || rec_new) w.as_key = -1;
    b.cone_H = w.Hadd.d(); b.cone_g = w.wu_soc.d(); b.as_uraw = w.cone_uraw.d(); b.as_open = (int *)w.as_open.p;
    ca.M = M; ca.N = N; ca.u = u; ca.q = q; ca.Nc = Nc; ca.owner = a.owner;
    ca.rows = cone_rows;
    if (ncones > 0) {
      ca.ncones = ncones; ca.per_stage = p->cone_per_stage ? 1 : 0;
      for (int k = 0; k < ncones; k++) ca.qs[k] = p->cone_sizes[k];
      ca.A = p->cone_A; ca.c = p->cone_c;
    } else {
      ca.ncones = 1; ca.qs[0] = q; ca.per_stage = 0;
      ca.A = w.cone_A.d(); ca.c = w.cone_c.d();
    }
    ca.R = p->R; ca.r32 = a.mat32; ca.reg_u = p->reg_u; ca.rho_scale = 1e7;
    ca.z = w.cone_z.d(); ca.rec = w.cone_rec.d(); ca.H = w.Hadd.d(); ca.g = w.wu_soc.d();
    ca.cnt = (int *)w.as_cntp.p; ca.settled = (int *)w.as_settled.p; ca.open = (int *)w.as_open.p; ca.done = &ctl->done; ca.ctl = ctl;
    ca.jhi = b.as_jhi;
    // (measured at config E: 1e-6 .. 1e-3 changes the round count by 7.25 -> 6.75 only — the rounds behind the last status change are the Newton iteration itself)
    ca.tol_step = 1e-6; ca.tol_phi = 1e-9;
    ca.dual_scale = dual_scale;
  }
  // state boxes: penalty + multiplier terms per round from kernels_xbox.hip, see the header there
  const bool xbox = t.xbox = xbox_as && xb != 0;
  {  // sensitivity records of the forward sweep (k_fwd_as<.., SENS>): worth their stores when later rounds are expected and the sweeps are
     // issue-bound (many waves per SIMD); a small shard's rounds sit at one wave's latency whatever the settled particles do
    const int min_m = (int)c->opt[OPT_AS_SENS_MIN_M];
    if (min_m > 0 && M >= min_m && as_skip_on && Nc == 1 && (mode != 0 || w.as_pred_rounds >= 2)) {
      w.as_T.ensure((size_t)M * N * 64 * D8);
      b.as_T = w.as_T.d();
    }
  }
  if (xbox) {
    w.as_open.ensure((size_t)M * sizeof(int)); w.xb_D.ensure(nx * D8); w.xb_g.ensure(nx * D8);
    const bool z_new = w.xb_z.ensure(nx * D8), st_new = w.xb_st.ensure(nx * sizeof(int));
    if ((z_new || st_new) && mode == 0) { t.refused = true; return t; }
    if (mode == 2 || xb == 2) {  // cold: nothing held, no multipliers — the first pass holds what the base point violates
      HIP_CHECK(hipMemsetAsync(w.xb_z.p, 0, nx * D8, s));
      HIP_CHECK(hipMemsetAsync(w.xb_st.p, 0, nx * sizeof(int), s));
    } else if (mode == 1) {
      launch_xbox_from_ipm(sx, (int *)w.xb_st.p, w.xb_z.d(), s);
    }
    b.xb_D = w.xb_D.d(); b.xb_g = w.xb_g.d(); b.as_open = (int *)w.as_open.p;  // (the merged exchange of a sharded run carries the open rows: tail[4])
    xa.M = M; xa.N = N; xa.x = x; xa.lo = p->lx; xa.hi = p->ux; xa.Q = p->Q; xa.pw = p->weights; xa.reg_x = p->reg_x; xa.rho_scale = 1e7;  // (measured, bench.py --vmax: 1e5 .. 1e2 only add rounds)
    w.xb_qmax.ensure((size_t)M * D8);
    xa.qmax = w.xb_qmax.d();
    xa.z = w.xb_z.d(); xa.st = (int *)w.xb_st.p; xa.D = w.xb_D.d(); xa.g = w.xb_g.d();
    xa.cnt = (int *)w.as_cntp.p; xa.settled = (int *)w.as_settled.p; xa.open = (int *)w.as_open.p; xa.done = &ctl->done; xa.ctl = ctl;
    xa.jhi = b.as_jhi;
    xa.tol = 1e-9; xa.dual_scale = dual_scale;
    // (a held row stays open while |s| > tol; its multiplier moves by rho s, so the second test only matters for rows with a small multiplier.
    //  Measured, bench.py --vmax 3 / 2: 1e-6 costs one more round per solve than 1e-3 (709 -> 777 it/s, 267 -> 295), same answers to 1e-9)
    xa.z_tol = 1e-3;
    // (measured on bench.py --vmax 2: 302 it/s with both, 175 without the first, 302 -> 396 and no interior-point iteration at all with the second)
    // — for genuine state rows (a velocity limit violated over a window of stages).  In the increment form of a slew problem the boxes on
    // the u-part of the state are the control boxes, each moved by its own increment: there the plain rule (hold everything violated) settles in 7-11 rounds
    // and partial activation only delays it (tools/debug/slew_paths.py: cold start back on the interior-point iteration)
    xa.keep_on_clamp = 1;
    xa.act_frac = 0.5;
    xa.ctrl_from = c->xb_ctrl_from >= 0 ? c->xb_ctrl_from : x;
  }
  return t;
}

// control block of the attempt and its first base point, by mode; false: fp32 storage and a start that needs a rollout
bool QpSolve::as_start(AsAttempt &t) {
  LQArgs &b = t.b;
  ConeArgs &ca = t.ca;
  XboxArgs &xa = t.xa;
  const int mode = t.mode, max_rounds = t.max_rounds;
  const double dual_scale = t.dual_scale, big = b.as_big;
  const bool cone = t.cone, xbox = t.xbox;
  int *act = t.act;
  AsCtl *ctl = t.ctl;
  // (a cold start on genuine state rows that does not contract is not worth its rounds: the interior-point iteration takes over and
  //  names a better first set; the control boxes of a slew problem in increment form do settle, in 7-11 rounds that need not contract one by one)
  launch_as_begin(ctl, (int *)w.fail.p, max_rounds, dual_scale, s, cone ? 8 : (xbox ? (c->xb_ctrl_from >= 0 ? 8 : (mode == 0 ? 6 : 3)) : 2));  // control block of this attempt (+ cleared failure flag)
  // warm start inside an SCP loop (PMPC_PREV_IS_LAST_SOLUTION): the base point is the linearisation point itself, whose
  // dynamics defect f - X_prev is elementwise and rides through the first round's sweeps — no sequential rollout, nothing
  // written before the sweep.  The forward sweep verifies that U_prev IS the base point of the stored set.
  // (with several consensus stages the condensed gradient of stage j also needs Y_j d_{j-1}, d = the defect propagated
  // FORWARD through the earlier consensus stages — a term no backward sweep can form: the condensing kernel, which walks
  // those stages forward anyway, carries d as one more column (k_cond_fast).  Found by the config-B full-consensus test,
  // which a single accepted round without the term got wrong by 8 %)
  const bool use_defect = t.use_defect = mode == 0 && as_defect_on && (p->flags & PMPC_PREV_IS_LAST_SOLUTION);
  if (a.mat32 && !use_defect) return false;  // (fp32 storage: no rollout kernel reads the float arrays)
  if (mode == 3) {  // cold start of the cone rounds: every control at the caller's interior point, nothing held, no multipliers
    ProfScope ps(c, 5);
    HIP_CHECK(hipMemsetAsync(act, 0, nu * sizeof(int) + 8, s));
    HIP_CHECK(hipMemsetAsync(w.cone_z.p, 0, (size_t)M * N * cone_rows * D8, s));
    if (p->soc_u_interior) launch_soc_fill_u(p->U_out, p->soc_u_interior, (long long)nu, u, s);
    else launch_init_base(p->U_out, p->U_prev, M, N, u, Nc, s);  // (any start will do for the rounds; the shared controls need ONE base value: 0)
    launch_rollout_fast(b, p->U_out, p->X_out, s);
  } else if (mode == 4) {
    // the base point is what the attempt that just ended left in the outputs: its controls on their bounds, its states rolled out
  } else if (!use_defect) {  // first base point: controls snapped into their boxes / onto their bounds, states by rollout
    ProfScope ps(c, 5);
    Slab st = su;
    // the previous solution: this context's copy, or — a caller inside an SCP loop that hands it back as U_prev (promise flag;
    // no copy was kept then) with a consensus horizon the no-rollout start above does not cover — the caller's U_prev
    st.z = (mode == 0 && !w.as_U_valid) ? const_cast<double *>(p->U_prev) : w.U.d();
    st.D = nullptr; st.w = nullptr;
    if (mode == 5) {  // finish of the cone path-following iteration: box statuses from ITS duals, cone multipliers = its cone duals
      st.ll = w.soc_zl.d(); st.lu = w.soc_zu.d();
      HIP_CHECK(hipMemcpyAsync(w.cone_z.p, w.soc_zc.p, (size_t)M * N * cone_rows * D8, hipMemcpyDeviceToDevice, s));
    }
    launch_as_setup(st, mode == 5 ? 1 : mode, 0, act, p->U_out, big, s);
    launch_rollout_fast(b, p->U_out, p->X_out, s);
  }
  c->as_pend.ctl = nullptr;
  if (xbox) {  // terms of the first round, from the first base point and the stored statuses / multipliers
    ProfScope ps(c, 5);
    xa.finish = 0;
    xa.X = use_defect ? p->X_prev : p->X_out;
    launch_xbox_step(xa, s);
  }
  if (cone) {  // Newton terms of the first round, from the first base point and the stored multipliers
    ProfScope ps(c, 5);
    ca.finish = 0;
    ca.U = use_defect ? p->U_prev : p->U_out;
    launch_cone_step(ca, s);
  }
  return true;
}

// the round loop: batches of rounds enqueued ahead of their read-back; leaves the control block (t.h), the rounds run and the
// batches waited for since the speculation hook fired
void QpSolve::as_rounds(AsAttempt &t) {
  LQArgs &b = t.b;
  ConeArgs &ca = t.ca;
  XboxArgs &xa = t.xa;
  const int mode = t.mode, max_rounds = t.max_rounds;
  const bool cone = t.cone, xbox = t.xbox, use_defect = t.use_defect;
  AsCtl *ctl = t.ctl;
  AsCtl &h = t.h;
  int &round = t.round, &n_batches_at_hook = t.n_batches_at_hook;
  // (same conditions as the in-wave consensus solve of structured_solve: one rank, one consensus stage)
  const bool fuse_env = c->opt[OPT_AS_FUSE_CTL] != 0.0 && c->opt[OPT_AS_WAVE_CONS] != 0.0;
  const bool fuse_ctl = fuse_env && !c->multi() && Nc == 1;
  const int *open_part = (cone || xbox) ? (const int *)w.as_open.p : nullptr;
  const int perm_min_m = (int)c->opt[OPT_AS_PERM_MIN_M];
  round = 0;
  int depth = mode == 0 ? std::max(1, std::min(w.as_pred_rounds, max_rounds)) : std::min(3, max_rounds);
  if (verbose > 1 && xbox) depth = 1;  // (the debugging dump below wants every round)
  static const bool duc_trace = getenv("PMPC_DUC_TRACE") != nullptr;
  if (duc_trace) depth = 1;
  n_batches_at_hook = -1000;  // batches waited for since the speculation hook fired (in THIS attempt)
  memset(&h, 0, sizeof(h));
  while (true) {
    const int batch = std::min(depth, max_rounds - round);
    for (int k = 0; k < batch; k++) {
      const int r = round + k;
      b.defect = (use_defect && r == 0) ? p->f : nullptr;
      // particles without a status change in the previous round keep their factors, their condensed Hessian H_i and their
      // conditional optimum: no factor sweep for them — g_i follows the applied consensus step, g_i += H_i delta
      const bool skip = as_skip_on && r > 0 && nc <= 32;
      b.as_settled_in = skip ? (const int *)w.as_settled.p : nullptr;
      // the unsettled particles first: their sweeps are the launch's long waves (kernels_as.hip, k_as_perm)
      b.as_perm = nullptr;
      if (skip && perm_min_m > 0 && M >= perm_min_m && b.as_T) {  // (with every particle sweeping the index order is the better one: memory locality)
        ProfScope pp(c, 5);
        if (w.as_perm.ensure((size_t)M * sizeof(int)) || w.as_perm_m != M) {  // (what the buffer holds must be a permutation of 0 .. M-1 at any time)
          std::vector<int> id(M);
          for (int q_ = 0; q_ < M; q_++) id[q_] = q_;
          HIP_CHECK(hipMemcpyAsync(w.as_perm.p, id.data(), (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
          HIP_CHECK(hipStreamSynchronize(s));
          w.as_perm_m = M;
        }
        static const bool perm_fused = !(getenv("PMPC_AS_PERM_FUSED") && atoi(getenv("PMPC_AS_PERM_FUSED")) == 0);  // (A/B switch)
        if (c->as_pend.ctl && perm_fused) {
          // the round control of the round before rides in this round's consensus-partials launch (between the factor and the forward
          // sweep): the order is computed there, one launch less per round — the forward sweep gets it fresh, the factor sweep (short
          // restarted sweeps) runs in the order of the round before
          c->as_pend.settled = (const int *)w.as_settled.p;
          c->as_pend.perm = (int *)w.as_perm.p;
        } else {
          launch_as_perm((const int *)w.as_settled.p, M, (int *)w.as_perm.p, &ctl->done, s);
        }
        b.as_perm = (const int *)w.as_perm.p;
      }
      const bool last = k == batch - 1;
      // sharded with a consensus horizon: {released, activated, bad, failure} of round r ride in round r + 1's consensus
      // all-reduce (structured_solve), the decision about round r follows it there; only the last round of a batch needs a
      // collective of its own.  Every rank takes the same decisions from the same sums.
      const bool merge = c->multi() && nc > 0;
      b.as_merge = merge ? (k == 0 ? 1 : 2) : 0;  // (the first round of a batch carries nothing: the previous batch closed its last round)
      c->as_seq++;
      structured_solve(c, b, true, true, /*prep_done=*/true);
      ProfScope ps(c, 5);
      if (cone) {  // finish this round's cones (multipliers, cases, counters — BEFORE the round control reads them), prepare the next
        ca.finish = 1;
        ca.U = p->U_out; ca.Uraw = w.cone_uraw.d();
        launch_cone_step(ca, s);
      }
      if (xbox) {
        xa.finish = 1;
        xa.X = p->X_out;
        launch_xbox_step(xa, s);
      }
      if (merge) {
        if (last) {
          double *tl = w.Hg.d() + (size_t)nc * nc + nc;
          launch_as_ctl(ctl, (const int *)w.as_cntp.p, M, (const int *)w.fail.p, 1, 0, 0, nullptr, nullptr, 0, s, tl, nullptr, open_part);
          allreduce(c, tl, 5, ncclFloat64, ncclSum);
          launch_as_ctl(ctl, nullptr, M, (const int *)w.fail.p, 0, 1, 1, &c->mirror_dev->ctl, &c->mirror_dev->as_seq, c->as_seq, s, tl);
        }
      } else if (c->multi()) {  // no consensus exchange to ride on: one sum for all five (open cones + the four counters: contiguous)
        launch_as_ctl(ctl, (const int *)w.as_cntp.p, M, (const int *)w.fail.p, 1, 0, 0, nullptr, nullptr, 0, s, nullptr, nullptr, open_part);
        allreduce(c, &ctl->open, 5, ncclInt32, ncclSum);
        launch_as_ctl(ctl, nullptr, M, (const int *)w.fail.p, 0, 1, last ? 1 : 0, &c->mirror_dev->ctl, &c->mirror_dev->as_seq, c->as_seq, s);
      } else if (!last && fuse_ctl) {
        // the decision about this round rides in the next round's consensus-partials launch (structured_solve): its factor
        // sweep does not need it (settled particles leave it at once), its forward sweep sees it
        c->as_pend = AsCtlCall{ctl, (const int *)w.as_cntp.p, M, (const int *)w.fail.p, &c->mirror_dev->ctl, &c->mirror_dev->as_seq, c->as_seq,
                               b.as_viol, open_part, nullptr, nullptr};
      } else {
        launch_as_ctl(ctl, (const int *)w.as_cntp.p, M, (const int *)w.fail.p, 1, 1, last ? 1 : 0, &c->mirror_dev->ctl, &c->mirror_dev->as_seq, c->as_seq, s,
                      nullptr, b.as_viol, open_part);
      }
    }
    if (round == 0 && c->scp.post_batch) {  // the caller's follow-up work goes in behind the rounds before anything is read back
      std::function<void()> hook;
      hook.swap(c->scp.post_batch);
      c->scp.fired = true;
      n_batches_at_hook = 0;
      hook();
    }
    n_batches_at_hook++;
    // the control block is published when the rounds are over (done) or at the end of the batch, whichever comes first,
    // with the sequence number of the round that published it: wait for any of this batch's numbers
    {
      const unsigned long long lo_seq = c->as_seq - (unsigned long long)batch + 1, hi_seq = c->as_seq;
      const bool seen = spin_until([&] {
        const unsigned long long v = *(volatile unsigned long long *)&c->mirror->as_seq;
        return v >= lo_seq && v <= hi_seq;
      });
      if (!seen) {
        HIP_CHECK(hipStreamSynchronize(s));
        const unsigned long long v = *(volatile unsigned long long *)&c->mirror->as_seq;
        if (!(v >= lo_seq && v <= hi_seq)) throw PmpcHipError{-1, "active-set control block never published", __FILE__, __LINE__};
      }
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      memcpy(&h, (const void *)&c->mirror->ctl, sizeof(h));
    }
    if (verbose)
      for (int r = round; r < h.round && r < 16; r++)
        printf("pmpc_hip: active set (%s) round %d: %d released, %d activated (largest violation behind a change %.2e)\n",
               mode == 5 ? "finish" : (mode == 4 ? "state rows" : (mode >= 2 ? "cold" : (mode ? "finish" : "warm"))), r + 1, h.hist[r][0], h.hist[r][1], h.worst[r]);
    if (verbose && cone) printf("pmpc_hip: active set: %d stage cones still open after round %d\n", h.open, h.round);
    if (duc_trace && nc > 0 && !a.cons_G) {
      std::vector<double> hd(nc);
      HIP_CHECK(hipMemcpy(hd.data(), w.as_delta.p, nc * D8, hipMemcpyDeviceToHost));  // (the step of the shared controls as APPLIED by the round's forward sweep)
      double m = 0.0;
      for (double v : hd) m = std::max(m, std::fabs(v));
      int nset = 0;
      { std::vector<int> hs(M); HIP_CHECK(hipMemcpy(hs.data(), w.as_settled.p, M * sizeof(int), hipMemcpyDeviceToHost)); for (int v : hs) nset += v; }
      printf("pmpc_hip: trace: round %d max |du_c| %.3e, %d of %d particles settled\n", h.round, m, nset, M);
      if (b.as_jhi) {  // histogram of the highest changed stage among the unsettled particles
        std::vector<int> hj(M), hs(M), hist(N + 1, 0);
        HIP_CHECK(hipMemcpy(hj.data(), w.as_jhi.p, M * sizeof(int), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(hs.data(), w.as_settled.p, M * sizeof(int), hipMemcpyDeviceToHost));
        for (int q = 0; q < M; q++) if (!hs[q]) hist[hj[q] < 0 ? N : hj[q]]++;
        printf("pmpc_hip: trace:   highest changed stage:");
        for (int q = 0; q <= N; q++) if (hist[q]) printf(" %d:%d", q == N ? -1 : q, hist[q]);
        printf("\n");
      }
    }
  if (verbose > 1 && xbox) dump_state_rows(h.round);
  if (verbose > 1 && cone) dump_cone_records();
    inf.structured_solves += h.round - round;
    inf.active_set_rounds += h.round - round;
    round = h.round;
    if (h.done || round >= max_rounds) break;
    depth = 1;
  }
}

// debugging aid (verbose > 1): the state rows after a batch — held rows, largest multiplier, largest |x|, per worst particle
void QpSolve::dump_state_rows(int round) {
    HIP_CHECK(hipStreamSynchronize(s));
    std::vector<double> hz(nx), hX(nx), hU(nu);
    std::vector<int> hs(nx), hact(nu);
    HIP_CHECK(hipMemcpy(hz.data(), w.xb_z.p, nx * D8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hs.data(), w.xb_st.p, nx * sizeof(int), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hX.data(), p->X_out, nx * D8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hU.data(), p->U_out, nu * D8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hact.data(), w.as_act.p, nu * sizeof(int), hipMemcpyDeviceToHost));
    int held = 0, uheld = 0, wi = 0;
    double zmax = 0.0, xmax = 0.0;
    for (size_t k = 0; k < nx; k++) {
      held += hs[k] != 0;
      if (hz[k] > zmax) { zmax = hz[k]; wi = (int)(k / ((size_t)N * x)); }
      xmax = std::max(xmax, std::fabs(hX[k]));
    }
    for (size_t k = 0; k < nu; k++) uheld += hact[k] != 0;
    printf("   state rows after round %d: %d held, %d controls held, largest multiplier %.3e (particle %d), largest |x| %.3e\n", round, held, uheld, zmax, wi, xmax);
    if (getenv("PMPC_XB_DUMP")) {
      const int pi = atoi(getenv("PMPC_XB_DUMP"));
      for (int j = 0; j < N; j++) {
        printf("     p%d j%2d st", pi, j);
        for (int r = 0; r < x; r++) printf(" %d", hs[((size_t)pi * N + j) * x + r]);
        printf(" | act");
        for (int r = 0; r < u; r++) printf(" %d", hact[((size_t)pi * N + j) * u + r]);
        printf(" | v");
        for (int r = 3; r < 6 && r < x; r++) printf(" %+.4f", hX[((size_t)pi * N + j) * x + r]);
        printf(" | z");
        for (int r = 3; r < 6 && r < x; r++) printf(" %.3e", hz[((size_t)pi * N + j) * x + r]);
        printf(" | u");
        for (int r = 0; r < u; r++) printf(" %+.4f", hU[((size_t)pi * N + j) * u + r]);
        printf("\n");
      }
    }
}

// debugging aid (verbose > 1): the active cones' records (small problems only)
void QpSolve::dump_cone_records() {
    HIP_CHECK(hipStreamSynchronize(s));
    const int q1 = cone_rows;
    std::vector<double> hz((size_t)M * N * q1), hr((size_t)M * N * std::max(ncones, 1) * PMPC_CONE_REC), hu(nu), hraw(nu), hg(nu);
    HIP_CHECK(hipMemcpy(hz.data(), w.cone_z.p, hz.size() * D8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hr.data(), w.cone_rec.p, hr.size() * D8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hu.data(), p->U_out, nu * D8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hraw.data(), w.cone_uraw.p, nu * D8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hg.data(), w.wu_soc.p, nu * D8, hipMemcpyDeviceToHost));
    {
      std::vector<int> hcnt((size_t)M * 3);
      HIP_CHECK(hipMemcpy(hcnt.data(), w.as_cntp.p, hcnt.size() * sizeof(int), hipMemcpyDeviceToHost));
      std::vector<int> hact(nu);
      HIP_CHECK(hipMemcpy(hact.data(), w.as_act.p, nu * sizeof(int), hipMemcpyDeviceToHost));
      printf("   act:");
      for (size_t k = 0; k < nu && k < 24; k++) printf(" %d", hact[k]);
      printf("\n   as_cnt:");
      for (int v : hcnt) printf(" %d", v);
      printf(" | U of particle 0:");
      for (int k = 0; k < N * u && k < 12; k++) printf(" %.6e", hu[k]);
      printf(" | uraw:");
      for (int k = 0; k < N * u && k < 12; k++) printf(" %.6e", hraw[k]);
      printf(" | cone_g:");
      for (int k = 0; k < N * u && k < 12; k++) printf(" %.3e", hg[k]);
      printf("\n");
    }
    int shown = 0;
    for (size_t k = 0; k < (size_t)M * N && shown < 6; k++) {
      if (M > 64 ? hr[k * PMPC_CONE_REC + 11] < 3.0 : hr[k * PMPC_CONE_REC] == 0.0) continue;  // (large problems: the cones that keep changing case)
      printf("   [flips %g]", hr[k * PMPC_CONE_REC + 11]);
      shown++;
      printf("   cone (%zu,%zu) case %g rho %.3e curv %.3e nu %.6e | s_b", k / N, k % N, hr[k * PMPC_CONE_REC], hr[k * PMPC_CONE_REC + 1], hr[k * PMPC_CONE_REC + 2], hr[k * PMPC_CONE_REC + 3]);
      for (int r = 0; r < q1; r++) printf(" %.9e", hr[k * PMPC_CONE_REC + 4 + (q1 - 1) + r]);
      printf(" | z");
      for (int r = 0; r < q1; r++) printf(" %.9e", hz[k * q1 + r]);
      printf(" | u");
      for (int r = 0; r < u; r++) printf(" %.9e", hu[k * u + r]);
      printf(" | uraw");
      for (int r = 0; r < u; r++) printf(" %.9e", hraw[k * u + r]);
      printf(" | g");
      for (int r = 0; r < u; r++) printf(" %.3e", hg[k * u + r]);
      {
        std::vector<double> hk(u), hH((size_t)u * u);
        std::vector<int> ha(u);
        HIP_CHECK(hipMemcpy(hk.data(), w.kff.d() + k * u, u * D8, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(ha.data(), (int *)w.as_act.p + k * u, u * sizeof(int), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(hH.data(), w.Hadd.d() + k * u * u, (size_t)u * u * D8, hipMemcpyDeviceToHost));
        printf(" | kff");
        for (int r = 0; r < u; r++) printf(" %.3e", hk[r]);
        printf(" | act");
        for (int r = 0; r < u; r++) printf(" %d", ha[r]);
        printf(" | Hdiag");
        for (int r = 0; r < u; r++) printf(" %.3e", hH[r * (u + 1)]);
      }
      printf("\n");
    }
}

// acceptance of a settled attempt: state boxes outside the rounds are verified, set and solution kept for the next warm start
int QpSolve::as_accept(AsAttempt &t) {
  const AsCtl &h = t.h;
  const int mode = t.mode, round = t.round, n_batches_at_hook = t.n_batches_at_hook;
  const double dual_scale = t.dual_scale;
  const bool xbox = t.xbox;
  if (verbose && (h.cnt[2] || h.cnt[3])) printf("pmpc_hip: active set: numerical failure / broken promise (bad %d, fail %d)\n", h.cnt[2], h.cnt[3]);
  if (!h.done) return 1;
  if (h.status != 0) return h.status;
  if (has_xb && !xbox_as) {  // the candidate's states against their boxes
    reset_scalars();
    HIP_CHECK(hipMemsetAsync(w.part_max.p, 0, 2 * PMPC_RED_BLOCKS * D8, s));
    Slab sc2 = sx;
    sc2.z = p->X_out;
    launch_violation(sc2, w.part_max.d(), s);
    exchange(c, 1);
    read_scalars(c);
    if (*c->fail_host || !(c->sc_host->viol_max <= 1e-13)) {
      if (verbose) printf("pmpc_hip: active set settled but a state box is violated by %.3e: interior-point path\n", c->sc_host->viol_max);
      w.xb_block_key = as_key;
      return 1;
    }
  }
  // the next solve's warm start: a caller inside an SCP loop (promise flag) hands the solution back as U_prev, which is then
  // the base point itself — no copy; any other caller's next warm start snaps THIS copy into its boxes
  // (sharded with several consensus stages: neither the no-rollout start nor the caller's U_prev serves — see the warm attempt
  //  below — so the copy is kept there too)
  w.as_U_valid = !(p->flags & PMPC_PREV_IS_LAST_SOLUTION) || (c->multi() && Nc > 1);
  if (w.as_U_valid) HIP_CHECK(hipMemcpyAsync(w.U.p, p->U_out, nu * D8, hipMemcpyDeviceToDevice, s));
  outputs_written = true;
  w.as_key = as_key;  // the stored set (+ w.U) start the next solve of this shape
  w.as_scale = dual_scale;
  w.as_count = nu;
  if (mode == 0) w.as_pred_rounds = round;
  c->scp.ok = n_batches_at_hook == 1 && !(has_xb && !xbox);  // (with state boxes ignored, a second phase follows)  // what was enqueued behind the first batch saw the final outputs
  return 0;
}

int QpSolve::active_set_solve(double dual_scale, int mode, int max_rounds, int xb) {
  if (fast) return active_set_fast(dual_scale, mode, max_rounds, xb);
  reset_scalars();
  // generic kernels: a check pass + rollout per round, decisions on the host.  `big` never meets a normal-sized term in a sum (the penalty's target is a ZERO step), so it only has to dwarf every
  // H_uu entry: gains, H_uu^-1 and the step of a held control come out ~1e-30 relative and -big du_b is its multiplier
  const double big = 1e30, tol_p = 1e-13;
  w.as_act.ensure(nu * sizeof(int) + 8); w.as_cnt.ensure(4 * sizeof(int) + 8);
  int *act = (int *)w.as_act.p, *cnt = (int *)w.as_cnt.p;
  unsigned long long *worst_dev = (unsigned long long *)(cnt + 4);
  double *Xtry = w.dX2.d(), *Utry = w.dU2.d();  // (free here: the corrector's difference step is already applied)
  LQArgs b = a;
  b.X = Xtry; b.U = Utry; b.Dx = b.wx = nullptr; b.Du = su.D; b.wu = su.w; b.dX = w.dX.d(); b.dU = w.dU.d();
  Slab st = su;
  st.z = w.U.d(); st.dz = w.dU.d(); st.dz2 = nullptr;
  int last_add = 1, last_changes = 0x7fffffff, stalls = 0;
  w.as_key = -1;
  for (int round = 0; round < max_rounds; round++) {
    // anti-cycling on (nearly) degenerate boxes — a control at its bound with a multiplier of a few ulps flips for ever —:
    // the sign tolerance of the multipliers widens tenfold per round after the fourth, up to 1e-8 of the dual scale
    const double tol_l = dual_scale * std::min(1e-8, 1e-11 * std::pow(10.0, std::max(0, round - 3)));
    {
      // a round that only RELEASED controls keeps its base point (a released control may start from its bound): no new
      // rollout; only D changes
      const bool same_base = round > 0 && last_add == 0;
      launch_as_setup(st, round == 0 ? mode : 0, same_base, act, Utry, big, s);
      if (!same_base) launch_rollout(b, Utry, Xtry, s);
      structured_solve(c, b, true, false);
      HIP_CHECK(hipMemsetAsync(cnt, 0, 4 * sizeof(int) + 8, s));
      launch_as_check(st, act, Utry, big, tol_p, tol_l, cnt, worst_dev, s);
      launch_as_publish(cnt, (const int *)w.fail.p, c->multi() ? nullptr : c->mirror_dev->as_cnt, &c->mirror_dev->as_seq, ++c->as_seq, s);
    }
    inf.structured_solves++;
    inf.active_set_rounds++;
    if (c->multi()) {  // {released, activated, NaN, failure}: one sum for all four
      allreduce(c, cnt, 4, ncclInt32, ncclSum);
      launch_as_publish(cnt, nullptr, c->mirror_dev->as_cnt, &c->mirror_dev->as_seq, c->as_seq, s);
    }
    wait_published(c, &c->mirror->as_seq, c->as_seq);
    struct { int rel, add, bad, fail; unsigned long long worst; } hc;
    memcpy(&hc, (const void *)c->mirror->as_cnt, 4 * sizeof(int));
    hc.worst = 0;
    if (verbose) {  // (diagnostic of the check pass only)
      HIP_CHECK(hipMemcpyAsync(&hc.worst, worst_dev, 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
    double worst;
    memcpy(&worst, &hc.worst, sizeof(double));
    if (verbose)
      printf("pmpc_hip: active set (%s) round %d: %d released, %d activated (largest %.2e)%s\n", mode == 2 ? "cold" : (mode ? "finish" : "warm"), round + 1,
             hc.rel, hc.add, worst, (hc.bad || hc.fail) ? " (numerical failure)" : "");
    if (hc.bad || hc.fail) return 2;
    last_add = hc.add;
    const int changes = hc.rel + hc.add;
    if (changes == 0) {
      if (has_xb) {  // the candidate's states against their boxes, before anything of the interior-point state is overwritten
        HIP_CHECK(hipMemsetAsync(w.part_max.p, 0, 2 * PMPC_RED_BLOCKS * D8, s));
        launch_violation_sum(sx, Xtry, w.dX.d(), w.part_max.d(), s);
        exchange(c, 1);
        read_scalars(c);
        if (*c->fail_host || !(c->sc_host->viol_max <= 1e-13)) {
          if (verbose) printf("pmpc_hip: active set settled but a state box is violated by %.3e: interior-point path\n", c->sc_host->viol_max);
          w.xb_block_key = as_key;
          return 1;
        }
      }
      launch_as_accept_all(st, act, Utry, p->U_out, Xtry, w.dX.d(), (long long)nx, w.X.d(), p->X_out, s);
      w.as_U_valid = true;  // (the acceptance pass wrote the controls into the warm-start memory)
      outputs_written = true;
      w.as_key = as_key;  // act + w.U start the next solve of this shape
      w.as_scale = dual_scale;
      w.as_count = nu;
      return 0;
    }
    if (changes * 2 > last_changes && ++stalls >= 2) return 1;  // not contracting: leave it to the interior-point iteration
    last_changes = changes;
  }
  return 1;
}

// ---- 2. Mehrotra predictor-corrector on the boxes ----------------------------------------------
// Warm start: consecutive sub-problems of an SCP / MPC loop are close, so the EARLY iterate of the previous solve of
// this shape (first iterate with mu <= 0.5: interior, centred, far from its boxes — a late iterate jams) is a better
// start than the clipped equality-only optimum: 11 -> 9.3 iterations at config D, 11 -> 7.1 on the unicycle.  It is
// used only if it is strictly inside the new boxes, and a warm-started iteration that fails is repeated cold.
// one interior-point run from a warm (remembered iterate) or cold (clipped equality-only optimum) start; returns the
// status (0 converged, 1 not converged, 2 numerical failure) or -1: the remembered iterate does not fit the new boxes
int QpSolve::interior_point(const bool warm) {
  // complementarity (1e-10 leaves ~3e-7 relative trajectory error on the quadrotor: too close to the 1e-6 bar).  State boxes WITHOUT the
  // state-row rounds (generic kernels, or xbox_as = 0) have nothing that finishes the iteration exactly: 1e-12 left up to 1.9e-6 on
  // slew problems with ~15 % of the state entries binding (tools/debug/fuzz_xbox.py), 1e-14 leaves 8e-8 — a breakdown on the way
  // there returns the last good iterate (see below)
  const double tol = (has_xb && !xbox_as) ? 1e-14 : 1e-12;
  const int max_iter = 80;
  // slabs as the fused per-iteration pass sees them (an unbounded slab still takes the step and feeds the
  // gradient pre-pass)
  SlabEx ex, eu;
  memset(&ex, 0, sizeof(ex));
  memset(&eu, 0, sizeof(eu));
  ex.s = sx; eu.s = su;
  if (!has_xb) { ex.s.count = (long long)nx; ex.s.d = x; ex.s.N = N; ex.s.Nc = Nc; ex.s.owner = a.owner; ex.s.z = w.X.d(); ex.s.dz = w.dX.d(); }
  if (!has_ub) { eu.s.count = (long long)nu; eu.s.d = u; eu.s.N = N; eu.s.Nc = Nc; eu.s.owner = a.owner; eu.s.is_u = 1; eu.s.z = w.U.d(); eu.s.dz = w.dU.d(); }
  ex.bounded = has_xb; eu.bounded = has_ub;
  ex.s.dz2 = w.dX2.d(); eu.s.dz2 = w.dU2.d();
  ex.pw = eu.pw = p->weights; ex.per = (long long)N * x; eu.per = (long long)N * u;
  ex.ref = p->X_ref; ex.prev = p->X_prev; ex.reg = p->reg_x; ex.gm = fast ? w.xm.d() : nullptr; ex.gd = fast ? w.xd.d() : nullptr;
  eu.ref = p->U_ref; eu.prev = p->U_prev; eu.reg = p->reg_u; eu.gm = fast ? w.um.d() : nullptr; eu.gd = fast ? w.ud.d() : nullptr;
  auto rollout = [&]() {
    if (fast) launch_rollout_fast(a, w.U.d(), w.X.d(), s);
    else launch_rollout(a, w.U.d(), w.X.d(), s);
  };
  bool remembered = false;  // this run has stored its early iterate
  if (warm) {
    HIP_CHECK(hipMemcpyAsync(w.U.p, w.warmU.p, nu * D8, hipMemcpyDeviceToDevice, s));
    rollout();
    if (has_xb) launch_violation(sx, w.part_max.d(), s);  // the remembered controls must be inside the NEW boxes,
    if (has_ub) launch_violation(su, w.part_max.d() + B, s);  // and so must the states they roll out to
    exchange(c, 1);
    read_scalars(c);
    if (*c->fail_host || !(c->sc_host->viol_max <= 0.0)) {
      if (verbose) printf("pmpc_hip: remembered iterate is outside the new boxes: cold start\n");
      return -1;
    }
  } else if (has_ub) {
    launch_ipm_clip(su, s);
    rollout();
  }
  a.Dx = has_xb ? sx.D : nullptr; a.wx = has_xb ? sx.w : nullptr;
  a.Du = has_ub ? su.D : nullptr; a.wu = has_ub ? su.w : nullptr;
  if (has_xb) launch_ipm_init_slack(sx, 1.0, s, warm ? 1e-9 : 1e-2);
  if (has_ub) launch_ipm_init_slack(su, 1.0, s, warm ? 1e-9 : 1e-2);
  if (warm) {  // multipliers of the remembered iterate (slacks follow from the controls and the new boxes)
    if (has_xb) {
      HIP_CHECK(hipMemcpyAsync(sx.ll, w.warm_llx.p, nx * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(sx.lu, w.warm_lux.p, nx * D8, hipMemcpyDeviceToDevice, s));
    }
    if (has_ub) {
      HIP_CHECK(hipMemcpyAsync(su.ll, w.warm_llu.p, nu * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(su.lu, w.warm_luu.p, nu * D8, hipMemcpyDeviceToDevice, s));
    }
  }
  int status = 1;
  double mu_peak = 1.0;  // dual scale: on badly scaled problems mu first GROWS by orders of magnitude; the
                         // complementarity tolerance is relative to that peak (1e-12 absolute is then below round-off)
  // try the active-set finish once mu <= polish_next * mu_peak (relative, like `tol`).  With state rows the iterate has to name the
  // set more sharply (measured, tools/debug/xbox_check.py: attempts at 1e-3 fail two times in three, at 1e-6 .. 1e-8 they settle)
  double polish_next = xbox_as ? 1e-3 * polish_mu : polish_mu;
  bool advanced = false;  // this iteration's elementwise pass is already in flight (launched behind the last exchange)
  double late_mu = -1.0;  // complementarity of the iterate kept in w.lateX / w.lateU (< 0: none)
  for (int it = 1; it <= max_iter; it++) {
    // previous corrector step (it > 1), predictor preparation and gradient pre-pass in ONE pass
    if (!advanced) launch_ipm_advance(ex, eu, it > 1, sc, w.part_sum.d(), w.part_cnt.d(), w.part_max.d(), s);
    advanced = false;
    if (it == 1 || mu_target > 0.0) {  // later iterates get mu / residual from the corrector's step polynomial (phase 4);
      exchange(c, 2);                    // barrier mode re-measures them together with the centrality deviation
      read_scalars(c);
    }
    const IpmScal &h = *c->sc_host;
    if (verbose)
      printf("pmpc_hip: ipm it %2d  mu %9.3e  slack_res %9.3e  nu %9.3e  alpha %6.4f  sigma %8.2e  dev %8.2e\n", it, h.mu, h.res_max,
             h.nu, h.alpha, h.sigma, h.dev_max);
    inf.mu = h.mu; inf.slack_res = h.res_max; inf.ipm_iters = it - 1;
    if (*c->fail_host || !(h.mu == h.mu)) {
      // With thousands of binding state rows the iteration can break down numerically between mu ~ 1e-12 mu_peak and the
      // convergence test at 1e-12 (slack / multiplier ratios of 1e14 in the cost-to-go; seen at config D with |v| <= 2 m/s and the
      // state-row rounds switched off: mu 7.9e-10 -> 1.3e-12 -> NaN).  The last iterate with mu <= 1e-10 mu_peak and small
      // residuals is a certified near-optimal point (duality gap <= n mu): returned instead of a failed solve.
      if (late_mu >= 0.0 && mu_target == 0.0) {
        // (said on stderr whatever `verbose` is: the status is 0, and only info.mu tells this iterate from a converged one)
        fprintf(stderr, "pmpc_hip: note: interior-point iteration broke down numerically at iteration %d; returning the kept iterate (complementarity %.3e, convergence test %.3e)\n", it, late_mu, tol * mu_peak);
        HIP_CHECK(hipMemcpyAsync(w.X.p, w.lateX.p, nx * D8, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpyAsync(w.U.p, w.lateU.p, nu * D8, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
        *c->fail_host = 0;
        inf.mu = late_mu;
        status = 0;
        break;
      }
      status = 2;
      break;
    }
    if (mu_target == 0.0 && h.mu <= 1e-10 * std::max(mu_peak, h.mu) && h.res_max <= 1e-10 && h.nu <= 1e-8) {
      w.lateX.ensure(nx * D8); w.lateU.ensure(nu * D8);
      HIP_CHECK(hipMemcpyAsync(w.lateX.p, w.X.p, nx * D8, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(w.lateU.p, w.U.p, nu * D8, hipMemcpyDeviceToDevice, s));
      late_mu = h.mu;
    }
    const bool barrier_done = mu_target > 0.0 && h.dev_max <= 1e-9 * mu_target && h.res_max <= 1e-10 && h.nu <= 1e-8;
    if (!warm_disabled && ((!remembered && mu_target == 0.0 && it > 1 && h.mu <= 0.5) || barrier_done)) {
      // (the step that produced this iterate is already applied: the pass behind the last exchange is in flight)
      w.warmU.ensure(nu * D8);
      HIP_CHECK(hipMemcpyAsync(w.warmU.p, w.U.p, nu * D8, hipMemcpyDeviceToDevice, s));
      if (has_ub) {
        w.warm_llu.ensure(nu * D8); w.warm_luu.ensure(nu * D8);
        HIP_CHECK(hipMemcpyAsync(w.warm_llu.p, su.ll, nu * D8, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpyAsync(w.warm_luu.p, su.lu, nu * D8, hipMemcpyDeviceToDevice, s));
      }
      if (has_xb) {
        w.warm_llx.ensure(nx * D8); w.warm_lux.ensure(nx * D8);
        HIP_CHECK(hipMemcpyAsync(w.warm_llx.p, sx.ll, nx * D8, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpyAsync(w.warm_lux.p, sx.lu, nx * D8, hipMemcpyDeviceToDevice, s));
      }
      w.warm_key = warm_key;
      w.warm_mu = mu_target;
      remembered = true;
    }
    if (h.mu > mu_peak) mu_peak = h.mu;
    if (mu_target > 0.0) {  // centred AT mu_target: every complementarity product equals it
      if (barrier_done) { status = 0; break; }
    } else if (h.mu <= tol * mu_peak && h.res_max <= 1e-10 && h.nu <= 1e-8) {
      status = 0;
      // converged on its own (every finish attempt on the way failed, or none was due): one more attempt from the
      // converged iterate — it names the set as sharply as it ever will; a settled attempt takes the answer from ~1e-7 to round-off and
      // leaves the set and multipliers for the next solve's warm start; a failed one changes nothing (the rounds work in the outputs)
      if (polish_on && !(has_xb && !xbox_as && w.xb_block_key == as_key)) {
        const int r = active_set_solve(std::max(1.0, mu_peak), 1, xbox_as ? 10 : 6);
        if (r == 0) inf.mu = 0.0;
        else if (r == 2) HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
      }
      break;
    }
    if (it == max_iter) {
      // out of iterations between the kept iterate (mu <= 1e-10 mu_peak, small residuals) and the convergence test: that iterate
      // is a certified near-optimal point, returned as the breakdown case above returns it — not a failed solve
      if (late_mu >= 0.0 && mu_target == 0.0) {
        fprintf(stderr, "pmpc_hip: note: interior-point iteration out of iterations above its tolerance; returning the kept iterate (complementarity %.3e, convergence test %.3e)\n", late_mu, tol * mu_peak);
        HIP_CHECK(hipMemcpyAsync(w.X.p, w.lateX.p, nx * D8, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpyAsync(w.U.p, w.lateU.p, nu * D8, hipMemcpyDeviceToDevice, s));
        inf.mu = late_mu;
        status = 0;
      }
      break;
    }
    if (polish_on && it > 1 && h.mu <= polish_next * mu_peak && !(has_xb && !xbox_as && w.xb_block_key == as_key)) {
      const double mu_now = h.mu;  // (h aliases the host snapshot)
      const int r = active_set_solve(std::max(1.0, mu_peak), 1, xbox_as ? 10 : 6);
      if (r == 0) { inf.mu = 0.0; status = 0; break; }
      // not settled: the interior-point state (U, X, slacks, multipliers) is untouched; rebuild what the attempt
      // overwrote (D, w, gradient pre-pass arrays) and go on; try again two orders of magnitude further down
      if (verbose) printf("pmpc_hip: active-set finish not settled (%d): continuing the interior-point iteration\n", r);
      polish_next = mu_now / mu_peak * (xbox_as ? 1e-4 : 1e-2);  // (a failed attempt with state rows costs up to ten rounds)
      if (r == 2) HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
      launch_ipm_advance(ex, eu, 0, sc, w.part_sum.d(), w.part_cnt.d(), w.part_max.d(), s);
    }
    // predictor (factorisation) ...
    structured_solve(c, a, true, fast, /*prep_done=*/true);
    inf.structured_solves++;
    if (has_xb) launch_ipm_step(sx, 0, sc, w.part_sum.d(), w.part_cnt.d(), s);
    if (has_ub) launch_ipm_step(su, 0, sc, w.part_sum.d() + B, w.part_cnt.d() + B, s);
    exchange(c, 3);
    // ... corrector (vector sweeps only, same factorisation; solves for the difference step)
    if (has_xb) launch_ipm_prepare(sx, 1, sc, nullptr, nullptr, nullptr, s);
    if (has_ub) launch_ipm_prepare(su, 1, sc, nullptr, nullptr, nullptr, s);
    a.dX = w.dX2.d(); a.dU = w.dU2.d();  // the sweeps never read-modify-write: step = dz + dz2
    structured_solve(c, a, false, fast);
    a.dX = w.dX.d(); a.dU = w.dU.d();
    sx.dz2 = w.dX2.d(); su.dz2 = w.dU2.d();
    if (has_xb) launch_ipm_step(sx, 1, sc, w.part_sum.d(), w.part_cnt.d(), s);
    if (has_ub) launch_ipm_step(su, 1, sc, w.part_sum.d() + B, w.part_cnt.d() + B, s);
    sx.dz2 = su.dz2 = nullptr;
    exchange(c, 4);
    if (mu_target == 0.0) {
      // phase 4 already predicts the next iterate's scalars (step polynomial) and publishes them: enqueue the next
      // elementwise pass BEHIND it before polling — it has to run whether or not that iterate turns out to be converged
      // (it applies the step), and it keeps the GPU busy while the host decides and enqueues the next factor sweep
      launch_ipm_advance(ex, eu, 1, sc, w.part_sum.d(), w.part_cnt.d(), w.part_max.d(), s);
      advanced = true;
    }
    read_scalars(c);
  }
  return status;
}

// stage cones: warm rounds -> cold rounds -> path-following iteration, whose iterate starts one more attempt of the rounds
int QpSolve::run_cone_dispatch() {
  if (cone_as) {
    const int cone_cold_rounds = (int)c->opt[OPT_CONE_COLD_ROUNDS];
    const bool can_defect = as_defect_on && (p->flags & PMPC_PREV_IS_LAST_SOLUTION);
    const bool prev_is_base = !c->multi() && (p->flags & PMPC_PREV_IS_LAST_SOLUTION);
    int r = 1;
    if (as_warm_on && !(p->flags & PMPC_COLD_START) && as_prev == as_key && (w.as_U_valid || can_defect || prev_is_base)) {
      r = active_set_fast(w.as_scale, 0, 14);
      if (r == 0) return finish(0);
      if (verbose) printf("pmpc_hip: warm cone rounds not settled (%d): cold start\n", r);
    }
    densify();
    if (f32) return PMPC_NEEDS_F64;
    if (cone_cold_rounds > 0) {
      if (r == 2) HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
      r = active_set_fast(1.0, 3, cone_cold_rounds);
      if (r == 0) return finish(0);
      if (verbose) printf("pmpc_hip: cold cone rounds not settled (%d): path-following iteration\n", r);
    }
    HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
  }
  densify();
  if (f32) return PMPC_NEEDS_F64;
  if (ncones > 0) {  // the general form has no path-following fallback
    if (verbose) printf("pmpc_hip: stage cones (general form): the rounds did not settle\n");
    return finish(1);
  }
  // the path-following iteration, then — one shared cone on the register-resident path — cone rounds started from its iterate (box
  // statuses from its duals, cone multipliers = its cone duals): they replace its last digits (5e-7 -> round-off against the cone
  // oracle, tools/debug/fuzz_soc.py) and leave set and multipliers for the next solve's warm start; if they do not settle the
  // iterate itself is the answer, as before
  if (!cone_as) return soc_interior_point(true);
  const int st_pf = soc_interior_point(false);
  if (st_pf != 0) return st_pf;  // (failed: already finished, NaN outputs)
  const pmpc_info pf = inf;
  a.Du = nullptr; a.wu = nullptr; a.du_full = 0;
  const int r5 = active_set_fast(1.0, 5, 10);
  if (r5 != 0) {
    if (r5 == 2) HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
    outputs_written = false;
  }
  inf.ipm_iters = pf.ipm_iters;
  inf.mu = r5 == 0 ? 0.0 : pf.mu;
  return finish(0);
}

// boxes: warm rounds -> equality-only optimum -> cold rounds -> interior-point iteration (from the remembered iterate, then cold)
int QpSolve::run_box_dispatch() {
  const bool as_can_defect = as_defect_on && (p->flags & PMPC_PREV_IS_LAST_SOLUTION) && fast;
  // (the caller's U_prev is the stored set's solution; one rank only: the shared controls' base must be the same on every rank,
  //  which only this context's own copy guarantees when a caller breaks its promise)
  const bool as_prev_is_base = fast && !c->multi() && (p->flags & PMPC_PREV_IS_LAST_SOLUTION);
  // (state rows: a warm start that did not settle — hundreds of rows changing at once, see kernels_xbox.hip — would not settle for the
  //  next, similar problem either: the next 1, 2, 4 solves of the shape skip it, by the number of failures in a row)
  const bool xb_backoff = xbox_as && w.xb_warm_backoff > 0;
  if (xb_backoff) w.xb_warm_backoff--;
  if (polish_on && as_warm_on && !xb_backoff && !(p->flags & PMPC_COLD_START) && as_prev == as_key && (w.as_U_valid || as_can_defect || as_prev_is_base)) {
    a.Dx = a.wx = nullptr;
    const int r = active_set_solve(w.as_scale, 0, xbox_as ? 14 : 8);
    if (r == 0) {
      w.xb_warm_fails = 0;
      return finish(0);
    }
    if (xbox_as) {
      w.xb_warm_fails = std::min(w.xb_warm_fails + 1, 3);
      w.xb_warm_backoff = 1 << (w.xb_warm_fails - 1);
    }
    if (verbose) printf("pmpc_hip: warm active-set iteration not settled (%d): interior-point path\n", r);
    if (r == 2) HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
  }
  densify();  // (nothing below reads compact Jacobian records)
  if (f32) return PMPC_NEEDS_F64;
  // Warm start (see below): when the previous solve of this shape ended in the interior-point phase, go there directly —
  // the equality-only solve (one factorisation + forward sweep) would only tell us that the boxes are active again; it
  // is done later if the warm attempt is rejected or fails
  // (barrier mode, r03: the previous solve's FINAL iterate — centred at the same mu for a nearby problem — is the start: a few Newton
  //  iterations instead of ~10 from the clipped equality-only optimum)
  const bool try_warm = !warm_disabled && !(p->flags & PMPC_COLD_START) && (has_xb || has_ub) && w.warm_key == warm_key && w.warm_mu == mu_target;
  if (!try_warm) {
    const int r = equality_phase();
    if (r != 1) return finish(r);
    // cold start of the active-set iteration: the boxes the equality-only optimum violates are the first guess (the classical
    // start of the primal-dual active-set method); the interior-point iteration below only runs if that does not settle
    const int cold_as_rounds = (int)c->opt[OPT_AS_COLD_ROUNDS];
    if (polish_on && cold_as_rounds > 0) {
      // with state boxes, in two phases: the control boxes alone first (the primal-dual active-set rule is at home there, whatever
      // the start), then the state rows from that optimum — which violates about the rows that bind, where the equality-only optimum
      // clipped into its control boxes violates many more (a start the state rows' Newton iteration does not recover from)
      // (no control boxes — e.g. a boxed slew problem in increment form —: the first phase would be the equality-only optimum again)
      const bool two_phase = xbox_as && has_ub;
      int q = active_set_solve(1.0, 2, (xbox_as && !two_phase) ? std::max(cold_as_rounds, 14) : cold_as_rounds, two_phase ? 0 : 1);
      if (q == 0 && two_phase) {
        q = active_set_fast(1.0, 4, 14, 2);
        if (q != 0) outputs_written = false;  // (the first phase's point is not the answer)
      }
      if (q == 0) return finish(0);
      if (q == 2) HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
      // (w.U still holds the equality-only optimum: the rounds work in their own buffers)
    }
  }

  reset_scalars();
  int status = try_warm ? interior_point(true) : interior_point(false);
  if (try_warm && status != 0) {  // rejected or failed: fresh scalars, the equality-only optimum after all, cold start
    if (verbose && status > 0) printf("pmpc_hip: warm-started iteration failed (status %d): repeating from a cold start\n", status);
    w.warm_key = -1;
    HIP_CHECK(hipMemsetAsync(w.fail.p, 0, sizeof(int), s));
    launch_ipm_exchange(0, false, false, sc, (const int *)w.fail.p, w.xch.d(), c->rank, c->world, nullptr, nullptr, nullptr, 0, s,
                        mu_target, w.part_dev.d());
    const int r = equality_phase();
    if (r != 1) return finish(r);
    status = interior_point(false);
  }
  if (verbose && status != 0) printf("pmpc_hip: interior-point iteration did not converge (status %d)\n", status);
  return finish(status);
}

int QpSolve::run() {
  int r = check_args();
  if (r == GO_ON) r = setup_workspace();
  if (r != GO_ON) return r;
  setup_control_boxes();
  r = setup_cones();
  if (r != GO_ON) return r;
  setup_keys();
  if (!fast || Nc > 1 || f32) densify();  // (the generic kernels' rounds and the condensing kernels read the dense stacks)
  return soc ? run_cone_dispatch() : run_box_dispatch();
}

}  // namespace

extern "C" int solve_impl_body(pmpc_ctx *c, const pmpc_problem *p, pmpc_info *info, int verbose, bool soc) {
  return QpSolve(c, p, info, verbose, soc).run();
}
