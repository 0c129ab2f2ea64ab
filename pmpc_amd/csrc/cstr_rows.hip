// cstr_rows.hip — dense rows on the states in the SCP loop (built-in constraint kind 2, include/pmpc_abi.h pmpc_scp_cstr): every (particle,
// stage) unit carries K rows  a_k'x <= h_k  over all x states, as pmpc_jit_cstr_rows (cstr_kernels.h) linearises a custom constraint into.
// The solver holds them the way it holds the keep-out rows (keepout.hip): as upper bounds on K auxiliary states that the linearised
// dynamics produce.  numpy specification: pmpc_amd/extra_cstrs.py rows_augment.
//
//   k_rows_augment   (a, h, X_prev, f, fx, fu [, X_ref]) -> (f~, fx~, fu~, X_prev~ [, X_ref~], x_u~[x .. xd))  for M N units
//
// The walk is k_keepout_augment's, layout for layout (see the picture there): a workgroup takes UNITS consecutive units, loads their
// K x <= 48 row entries each into LDS (consecutive lanes, consecutive doubles; the stride per unit is odd, so the lanes of augmented
// rows of neighbouring units read different banks), and then ALL threads walk the workgroup's range of each OUTPUT array, consecutive
// lanes storing consecutive doubles.  The value of an augmented entry is an x-long fma chain in entry order.  An output index is split
// into (unit, column, row) with multiply-high by constants of the launch: no integer division in the loops.
#include "cstr_rows.h"
#include "cstr_jit.h"
#include "keepout.h"
#include "solver_internal.h"

namespace {

struct RowsArgs {
  int K, x, u;
  long long units;
  const double *a, *h, *X_prev, *f, *fx, *fu, *X_ref;
  double *f_aug, *fx_aug, *fu_aug, *X_prev_aug, *X_ref_aug, *xu_aug;
  unsigned m_kx, m_xd, m_xd2, m_uxd;  // floor(2^32 / d) + 1 for d = K x, xd, xd xd, u xd: e / d == umulhi(e, m) for e d < 2^32 (d >= 2)
};

constexpr int RA_UNITS = 32, RA_THREADS = 256;
constexpr int RA_LD = (KEEPOUT_MAX_K * (KEEPOUT_MAX_DIM - KEEPOUT_MAX_K)) | 1;  // 49: K x is largest at K = 4, x = 12

__global__ void __launch_bounds__(RA_THREADS) k_rows_augment(RowsArgs a) {
  __shared__ double rows[RA_UNITS * RA_LD];  // [unit]: a_1 (x) | .. | a_K (x)
  const int t = threadIdx.x, x = a.x, u = a.u, K = a.K, xd = x + K, kx = K * x;
  const long long first = (long long)blockIdx.x * RA_UNITS;
  const int n = (int)((a.units - first) < RA_UNITS ? (a.units - first) : RA_UNITS);
  {
    const double *src = a.a + first * kx;
    for (unsigned e = t; e < (unsigned)(n * kx); e += RA_THREADS) {
      const unsigned un = kx == 1 ? e : __umulhi(e, a.m_kx);  // (the constant of d = 1 does not fit 32 bits)
      rows[un * RA_LD + (e - un * kx)] = src[e];
    }
  }
  __syncthreads();
  // a_k'col as an fma chain in entry order.  (Loading the whole column ahead of the chain, unrolled to x = 15 with the tail predicated
  // off, was measured and is slower: 488 against 437 us at M 4096, N 50, x 12 — the lane's load latency is not what the kernel waits for.)
  auto comb = [&](const double *rec, const double *col) {
    double v = rec[0] * col[0];
    for (int c = 1; c < x; c++) v = fma(rec[c], col[c], v);
    return v;
  };
  // ---- vectors: f~ = [f | a'f], X_prev~ = [X_prev | 0], X_ref~ = [X_ref | 0], x_u~[x ..] = h ----------------------------------------------
  {
    const double *f = a.f + first * x, *Xp = a.X_prev + first * x, *Xr = a.X_ref ? a.X_ref + first * x : nullptr, *h = a.h + first * K;
    double *fo = a.f_aug + first * xd, *Xpo = a.X_prev_aug + first * xd, *Xro = a.X_ref_aug + first * xd, *xuo = a.xu_aug + first * xd;
    for (unsigned e = t; e < (unsigned)(n * xd); e += RA_THREADS) {
      const unsigned un = __umulhi(e, a.m_xd), r = e - un * xd;
      const bool copy = r < (unsigned)x;
      const unsigned src = un * x + r;
      fo[e] = copy ? f[src] : comb(rows + un * RA_LD + (r - x) * x, f + un * x);
      Xpo[e] = copy ? Xp[src] : 0.0;
      if (Xr) Xro[e] = copy ? Xr[src] : 0.0;
      if (!copy) xuo[e] = h[un * K + (r - x)];  // the bound on the auxiliary state (the first x entries are the caller's)
    }
  }
  // ---- fx~ ---------------------------------------------------------------------------------------------------------------------------
  {
    const int xx = x * x, dd = xd * xd;
    const double *fx = a.fx + first * xx;
    double *out = a.fx_aug + first * dd;
    for (unsigned e = t; e < (unsigned)(n * dd); e += RA_THREADS) {
      const unsigned un = __umulhi(e, a.m_xd2), k2 = e - un * dd, c = __umulhi(k2, a.m_xd), r = k2 - c * xd;
      double v = 0.0;
      if (c < (unsigned)x) {
        const double *col = fx + un * xx + c * x;
        v = r < (unsigned)x ? col[r] : comb(rows + un * RA_LD + (r - x) * x, col);
      }
      out[e] = v;
    }
  }
  // ---- fu~ ---------------------------------------------------------------------------------------------------------------------------
  {
    const int ux = u * x, ud = u * xd;
    const double *fu = a.fu + first * ux;
    double *out = a.fu_aug + first * ud;
    for (unsigned e = t; e < (unsigned)(n * ud); e += RA_THREADS) {
      const unsigned un = __umulhi(e, a.m_uxd), k2 = e - un * ud, c = __umulhi(k2, a.m_xd), r = k2 - c * xd;
      const double *col = fu + un * ux + c * x;
      out[e] = r < (unsigned)x ? col[r] : comb(rows + un * RA_LD + (r - x) * x, col);
    }
  }
}

unsigned magic(unsigned d) { return (unsigned)((1ull << 32) / d) + 1u; }

bool sizes_ok(size_t N, size_t M) { return N != 0 && M != 0 && N <= (size_t)0x7fffffff && M <= (size_t)0x7fffffff; }

}  // namespace

void launch_rows_augment(int K, int x, int u, int N, int M, const double *a, const double *h, const double *X_prev, const double *f, const double *fx,
                         const double *fu, const double *X_ref, double *f_aug, double *fx_aug, double *fu_aug, double *X_prev_aug, double *X_ref_aug,
                         double *xu_aug, hipStream_t s) {
  RowsArgs r;
  const int xd = x + K;
  r.K = K; r.x = x; r.u = u; r.units = (long long)M * N;
  r.a = a; r.h = h; r.X_prev = X_prev; r.f = f; r.fx = fx; r.fu = fu; r.X_ref = X_ref;
  r.f_aug = f_aug; r.fx_aug = fx_aug; r.fu_aug = fu_aug; r.X_prev_aug = X_prev_aug; r.X_ref_aug = X_ref_aug; r.xu_aug = xu_aug;
  r.m_kx = magic((unsigned)(K * x)); r.m_xd = magic((unsigned)xd); r.m_xd2 = magic((unsigned)(xd * xd)); r.m_uxd = magic((unsigned)(u * xd));
  if (r.units <= 0) return;
  hipLaunchKernelGGL(k_rows_augment, dim3((unsigned)((r.units + RA_UNITS - 1) / RA_UNITS)), dim3(RA_THREADS), 0, s, r);
}

unsigned *cstr_bad_counter(pmpc_ctx *c) {
  if (c->ws.cstr_bad.ensure(sizeof(unsigned))) HIP_CHECK(hipMemsetAsync(c->ws.cstr_bad.p, 0, sizeof(unsigned), c->stream));
  return (unsigned *)c->ws.cstr_bad.p;
}

extern "C" {

int pmpc_custom_cstr_rows_device(pmpc_ctx *c, int id, size_t N, size_t M, const double *X_prev, const double *gparams, double *a, double *h, double *g) {
  if (!c || !custom_cstr_known(c, id) || !sizes_ok(N, M) || !X_prev || !gparams || !a || !h) return 2;
  try {
    HIP_CHECK(hipSetDevice(c->device));
    ProfScope ps(c, 6);
    custom_launch_cstr_rows(id, (int)N, (int)M, X_prev, gparams, a, h, g, cstr_bad_counter(c), c->stream);
    HIP_CHECK(hipGetLastError());
  } catch (const PmpcHipError &) {
    return 1;
  }
  return 0;
}

int pmpc_rows_augment_device(pmpc_ctx *c, int K, size_t xdim, size_t udim, size_t N, size_t M, const double *a, const double *h, const double *X_prev,
                             const double *f, const double *fx, const double *fu, const double *X_ref, double *f_aug, double *fx_aug, double *fu_aug,
                             double *X_prev_aug, double *X_ref_aug, double *xu_aug) {
  if (!c || !keepout_strip_dims_valid(xdim, K, udim) || !sizes_ok(N, M)) return 2;
  if (!a || !h || !X_prev || !f || !fx || !fu || !f_aug || !fx_aug || !fu_aug || !X_prev_aug || !xu_aug || (X_ref && !X_ref_aug)) return 2;
  try {
    HIP_CHECK(hipSetDevice(c->device));
    ProfScope ps(c, 6);
    launch_rows_augment(K, (int)xdim, (int)udim, (int)N, (int)M, a, h, X_prev, f, fx, fu, X_ref, f_aug, fx_aug, fu_aug, X_prev_aug, X_ref_aug, xu_aug,
                        c->stream);
    HIP_CHECK(hipGetLastError());
  } catch (const PmpcHipError &) {
    return 1;
  }
  return 0;
}

long long pmpc_cstr_bad_rows(pmpc_ctx *c, int reset) {
  if (!c || !c->ws.cstr_bad.p) return 0;
  unsigned n = 0;
  (void)hipSetDevice(c->device);
  HIP_WARN(hipStreamSynchronize(c->stream));
  HIP_WARN(hipMemcpy(&n, c->ws.cstr_bad.p, sizeof(n), hipMemcpyDeviceToHost));
  if (reset) HIP_WARN(hipMemset(c->ws.cstr_bad.p, 0, sizeof(n)));
  return (long long)n;
}

}  // extern "C"
