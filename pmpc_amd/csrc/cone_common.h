// cone_common.h — what the bodies of the cone objective (solver_cone.hip, solver_cone_smooth.hip) set up alike, each written once.
#pragma once
#include "solver_internal.h"

namespace pmpc_impl {

// consensus horizon of a problem: stages whose controls are shared (Nc < 0: all of them) and how many shared controls that makes
struct ConsHorizon {
  int Nc, nc;
};
static inline ConsHorizon cons_horizon(const pmpc_problem *p) {
  const int Nc = p->Nc < 0 ? (int)p->N : (int)std::min<long long>(p->Nc, (long long)p->N);
  return {Nc, Nc * (int)p->udim};
}

// What the sweeps of the register-resident path read of a problem without slew penalties: dimensions, dynamics, cost blocks, previous
// point and references.  Ml: particles of this rank; the owner of the consensus boxes is the rank of global particle 0.
static inline LQArgs lq_args_of(const pmpc_ctx *c, const pmpc_problem *p, int Ml, int Nc) {
  LQArgs a;
  memset(&a, 0, sizeof(a));
  a.x = (int)p->xdim; a.u = (int)p->udim; a.N = (int)p->N; a.M = Ml; a.Nc = Nc; a.w = 0; a.n = (int)p->xdim;
  a.reg_x = p->reg_x; a.reg_u = p->reg_u;
  a.f = p->f; a.fx = p->fx; a.fu = p->fu; a.Q = p->Q; a.R = p->R;
  a.X_prev = p->X_prev; a.U_prev = p->U_prev; a.X_ref = p->X_ref; a.U_ref = p->U_ref;
  a.owner = (!c->multi() || c->rank == 0) ? 1 : 0; a.any_slew = 0; a.sym_cost = (p->flags & PMPC_SYMMETRIC_COST) ? 1 : 0;
  return a;
}

// zero slew weights / zero u_{-1} for M particles (the kernels read them unconditionally): grown and cleared when too small
static inline void ensure_zero_slew(pmpc_ctx *c, size_t M, size_t u) {
  Workspace &w = c->ws;
  const size_t D8 = sizeof(double);
  if (w.zslew.bytes < M * D8 || w.zum1.bytes < M * u * D8) {
    w.zslew.ensure(M * D8); w.zslew0.ensure(M * D8); w.zum1.ensure(M * u * D8);
    HIP_CHECK(hipMemsetAsync(w.zslew.p, 0, M * D8, c->stream));
    HIP_CHECK(hipMemsetAsync(w.zslew0.p, 0, M * D8, c->stream));
    HIP_CHECK(hipMemsetAsync(w.zum1.p, 0, M * u * D8, c->stream));
  }
}

// the zero buffers of a slew-free sweep: es_zero (max(64, nc) doubles: a zero consensus step), zeros, the zero slew terms — into `a`
static inline void zero_buffers(pmpc_ctx *c, int Ml, int nc, LQArgs &a) {
  Workspace &w = c->ws;
  const size_t D8 = sizeof(double);
  if (w.es_zero.ensure((size_t)std::max(64, nc) * D8)) HIP_CHECK(hipMemsetAsync(w.es_zero.p, 0, w.es_zero.bytes, c->stream));
  if (w.zeros.bytes == 0) {
    w.zeros.ensure(64 * D8);
    HIP_CHECK(hipMemsetAsync(w.zeros.p, 0, 64 * D8, c->stream));
  }
  ensure_zero_slew(c, (size_t)Ml, (size_t)a.u);
  a.slew = w.zslew.d(); a.slew0 = w.zslew0.d(); a.um1 = w.zum1.d();
  a.zeros = w.zeros.d();
}

// condensed Hessian of a particle, n x n column-major: the off-diagonal blocks live in the upper triangle
static inline void mirror_upper(double *H, int n) {
  for (int r = 0; r < n; r++)
    for (int q = r + 1; q < n; q++) H[q + (size_t)n * r] = H[r + (size_t)n * q];
}

// Key of what a context remembers about the cone objective of a shape: particles in all, dimensions, consensus horizon, `k`, and
// `tail` < `span` — whatever else the memory depends on.  Compared only with what the same context stored.
static inline long long cone_shape_key(size_t M, const pmpc_problem *p, long long k, long long span, long long tail) {
  return ((((((long long)M * 1000003 + (long long)p->N) * 131 + (long long)p->xdim) * 131 + (long long)p->udim) * 131 + p->Nc + 2) * 1000003 + k) * span + tail;
}

}  // namespace pmpc_impl
