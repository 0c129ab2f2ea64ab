// keepout.hip — keep-out constraints of the SCP loop (built-in constraint kind 1, include/pmpc_abi.h pmpc_scp_cstr): every stage of every
// particle stays outside K balls in a position sub-space of the state.  About the previous iterate the constraint is the half-space
//
//     n'(p - c) >= r,   n = (pbar - c) / |pbar - c|,   pbar = X_prev[i, j, pos_idx]      (n = first position axis if |pbar - c| < 1e-12)
//
// i.e. the row  a_x'x <= h  with a_x[pos_idx] = -n, h = -r - n'c  on the state of stage j.  The solver holds it as an upper bound on an
// auxiliary state that the linearised dynamics produce (pmpc_amd/extra_cstrs.py aux_state_problem, form 0): the state grows to
// xd = x + K, component x + k of f~ is a_x'f, its row of fx~ / fu~ is a_x'fx / a_x'fu, its column of fx~ is zero.  numpy specification:
// pmpc_amd/extra_cstrs.py keepout_augment.
//
//   k_keepout_augment   (X_prev, f, fx, fu [, X_ref]) -> (f~, fx~, fu~, X_prev~ [, X_ref~], x_u~[x .. xd))  for M N (particle, stage) units
//   k_keepout_strip_residual   X~out -> Xo (the first x entries of every row) and the SCP residual of (Xo, Xp), (Uo, Up), below
//
// Layout (ABI: blocks column-major, a unit's block of fx is [column][row]):
//
//     fx  (x columns of x)          fx~  (xd columns of xd)               fu (u columns of x)     fu~ (u columns of xd)
//     c0: r0 .. r(x-1)              c0: r0 .. r(x-1) | a_1'fx[:,c0] .. a_K'fx[:,c0]
//     ...                           ...                                   the same, per control column
//     c(x-1): ...                   c(x-1): ...      | ...
//                                   cx .. c(xd-1): 0 .. 0
//
// A workgroup takes UNITS consecutive units, which are consecutive in every array: each thread slice of THREADS / UNITS lanes owns one
// unit for the directions only — its first K lanes compute n_k and h_k once, into LDS — and then ALL threads walk the workgroup's range
// of each OUTPUT array, consecutive lanes storing consecutive doubles (and loading nearly consecutive ones: the source skips nothing,
// the lanes of augmented rows gather pos_dim entries of the column their neighbours copy).  An output index is split into (unit, column,
// row) with multiply-high by constants of the launch: no integer division in the loops.
#include "keepout.h"
#include "solver_internal.h"

namespace {

struct KeepoutArgs {
  pmpc_scp_cstr c;
  int x, u, N;
  long long units;
  const double *X_prev, *f, *fx, *fu, *X_ref;
  double *f_aug, *fx_aug, *fu_aug, *X_prev_aug, *X_ref_aug, *xu_aug;
  unsigned m_xd, m_xd2, m_uxd;  // floor(2^32 / d) + 1 for d = xd, xd xd, u xd: e / d == umulhi(e, m) for e d < 2^32
};

constexpr int KO_UNITS = 32, KO_THREADS = 256;

__global__ void __launch_bounds__(KO_THREADS) k_keepout_augment(KeepoutArgs a) {
  constexpr int SLICE = KO_THREADS / KO_UNITS;
  static_assert(SLICE >= KEEPOUT_MAX_K, "the first K lanes of a unit's slice compute its directions");
  __shared__ double dir[KO_UNITS][KEEPOUT_MAX_K][4];  // [unit][k]: a_x[pos_idx[0..2]] = -n_k, [3] unused (32-byte records)
  const int t = threadIdx.x, x = a.x, u = a.u, K = a.c.K, pd = a.c.pos_dim, xd = x + K;
  const long long first = (long long)blockIdx.x * KO_UNITS;
  const int n = (int)((a.units - first) < KO_UNITS ? (a.units - first) : KO_UNITS);
  {
    const int sl = t / SLICE, k = t % SLICE;
    if (sl < n && k < K) {
      const long long unit = first + sl, i = unit / a.N, j = unit - i * a.N;
      const double *cen = a.c.centres + i * a.c.centre_stride_particle + j * a.c.centre_stride_stage + k * pd;
      const double *xp = a.X_prev + unit * x;
      double d[3], cc[3], r2 = 0.0;
#pragma unroll
      for (int q = 0; q < 3; q++) {  // (unrolled: every index of d, cc and pos_idx is a constant, nothing lives in scratch)
        cc[q] = q < pd ? cen[q] : 0.0;
        d[q] = q < pd ? xp[a.c.pos_idx[q]] - cc[q] : 0.0;
        r2 = fma(d[q], d[q], r2);
      }
      const double nrm = sqrt(r2);
      double nc = 0.0;
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const double nq = nrm < 1e-12 ? (q == 0 ? 1.0 : 0.0) : d[q] / nrm;
        nc = fma(nq, cc[q], nc);
        dir[sl][k][q] = -nq;
      }
      a.xu_aug[unit * xd + x + k] = -a.c.radius[k] - nc;  // h: the bound on the auxiliary state (the first x entries are the caller's)
    }
  }
  __syncthreads();
  const int p0 = a.c.pos_idx[0], p1 = a.c.pos_idx[1], p2 = pd == 3 ? a.c.pos_idx[2] : a.c.pos_idx[0];
  // a_k'src[pos_idx] as an fma chain (the record's third entry is 0 when pos_dim is 2)
  auto comb = [&](const double *rec, const double *col) {
    double v = rec[0] * col[p0];
    v = fma(rec[1], col[p1], v);
    if (pd == 3) v = fma(rec[2], col[p2], v);
    return v;
  };
  // ---- vectors: f~ = [f | a'f], X_prev~ = [X_prev | 0], X_ref~ = [X_ref | 0] ------------------------------------------------------
  {
    const double *f = a.f + first * x, *Xp = a.X_prev + first * x, *Xr = a.X_ref ? a.X_ref + first * x : nullptr;
    double *fo = a.f_aug + first * xd, *Xpo = a.X_prev_aug + first * xd, *Xro = a.X_ref_aug + first * xd;
    for (unsigned e = t; e < (unsigned)(n * xd); e += KO_THREADS) {
      const unsigned un = __umulhi(e, a.m_xd), r = e - un * xd;
      const bool copy = r < (unsigned)x;
      const unsigned src = un * x + r;
      fo[e] = copy ? f[src] : comb(dir[un][r - x], f + un * x);
      Xpo[e] = copy ? Xp[src] : 0.0;
      if (Xr) Xro[e] = copy ? Xr[src] : 0.0;
    }
  }
  // ---- fx~ ---------------------------------------------------------------------------------------------------------------------------
  {
    const int xx = x * x, dd = xd * xd;
    const double *fx = a.fx + first * xx;
    double *out = a.fx_aug + first * dd;
    for (unsigned e = t; e < (unsigned)(n * dd); e += KO_THREADS) {
      const unsigned un = __umulhi(e, a.m_xd2), k2 = e - un * dd, c = __umulhi(k2, a.m_xd), r = k2 - c * xd;
      double v = 0.0;
      if (c < (unsigned)x) {
        const double *col = fx + un * xx + c * x;
        v = r < (unsigned)x ? col[r] : comb(dir[un][r - x], col);
      }
      out[e] = v;
    }
  }
  // ---- fu~ ---------------------------------------------------------------------------------------------------------------------------
  {
    const int ux = u * x, ud = u * xd;
    const double *fu = a.fu + first * ux;
    double *out = a.fu_aug + first * ud;
    for (unsigned e = t; e < (unsigned)(n * ud); e += KO_THREADS) {
      const unsigned un = __umulhi(e, a.m_uxd), k2 = e - un * ud, c = __umulhi(k2, a.m_xd), r = k2 - c * xd;
      const double *col = fu + un * ux + c * x;
      out[e] = r < (unsigned)x ? col[r] : comb(dir[un][r - x], col);
    }
  }
}

unsigned magic(unsigned d) { return (unsigned)((1ull << 32) / d) + 1u; }

// ---- strip + residual ----------------------------------------------------------------------------------------------------------------
// The way back from a sub-problem at xd = x + K states: Xo <- the first x entries of every row of X~out, and the SCP residual
// max(max_rows |Xo - Xp|_2, max_rows |Uo - Up|_2) of the iteration into *out_bits, in ONE pass over X~out (k_scp_residual's result, bit
// for bit: the same sums in the same order, see row_sq_max).
//
// A wave takes floor(64 / d_in) whole rows at a time — d_in <= 16: at least four, 52 to 64 live lanes — so that lane l holds entry
// l of the wave's range: consecutive lanes load consecutive doubles of X~out (and of U), store nearly consecutive ones of Xo.  (row, entry)
// of a lane is one multiply-high before the loop; the loop adds a constant to the base.  The row sums go through lane shuffles, LDS
// holds only the block's 256 maxima.
struct StripResArgs {
  const double *X_aug, *Xp, *Uo, *Up;
  double *Xo;
  long long rows;
  int x, xd, u, rpw_x, rpw_u;  // rpw: rows per wave and trip
  unsigned m_xd, m_u;
  unsigned long long *out_bits;
};

// max over the wave's rows of |in[row, :d] - prev[row, :]|^2 (in: rows of d_in >= d doubles; prev, out: rows of d), on the row's first
// lane.  The sum of a row is residual_block's: four contiguous quarters of q = ceil(d / 4) entries, each an fma chain in entry order from
// 0, then (a0 + a1) + (a2 + a3) — here every lane of a quarter runs the quarter's chain on values fetched from its lanes.
template <bool STRIP>
__device__ __forceinline__ double row_sq_max(const double *in, double *out, const double *prev, long long rows, int d_in, int d, int rpw,
                                             unsigned m_din, long long gw, long long nw, int lane) {
  const int row_l = d_in == 1 ? lane : (int)__umulhi((unsigned)lane, m_din), r = lane - row_l * d_in;  // (the constant of d = 1 does not fit 32 bits)
  const int q = (d + 3) >> 2, head = row_l * d_in;
  const int sq = (r >= q) + (r >= 2 * q) + (r >= 3 * q);  // the quarter entry r is in
  const int qs = head + sq * q, qn = min(d, (sq + 1) * q) - sq * q;  // its first lane, its length (<= 0: none, r >= d)
  double m = 0.0;
  for (long long g = gw; g * rpw < rows; g += nw) {  // (the trip count is the wave's: the shuffles below are convergent)
    const long long row = g * rpw + row_l;
    const bool on = row_l < rpw && row < rows;
    double t = 0.0;
    if (on) {
      const double v = in[row * d_in + r];
      if (r < d) {
        if (STRIP) out[row * d + r] = v;
        t = v - prev[row * d + r];
      }
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {  // q <= 4 (d <= 16)
      const double ti = __shfl(t, qs + i, 64);
      if (i < qn) acc = fma(ti, ti, acc);
    }
    double a[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const double ak = __shfl(acc, head + k * q, 64);
      a[k] = k * q < d ? ak : 0.0;  // (an empty quarter: the lane asked belongs to the auxiliary entries or to the next row)
    }
    const double sum = (a[0] + a[1]) + (a[2] + a[3]);
    if (on && r == 0) m = (sum == sum) ? fmax(m, sum) : INFINITY;  // a NaN trajectory must not look converged
  }
  return m;
}

__global__ void __launch_bounds__(256) k_keepout_strip_residual(StripResArgs a) {
  __shared__ double sh[256];
  const int t = threadIdx.x, lane = t & 63;
  const long long gw = (long long)blockIdx.x * 4 + (t >> 6), nw = (long long)gridDim.x * 4;
  const double mx = row_sq_max<true>(a.X_aug, a.Xo, a.Xp, a.rows, a.xd, a.x, a.rpw_x, a.m_xd, gw, nw, lane);
  const double mu = row_sq_max<false>(a.Uo, nullptr, a.Up, a.rows, a.u, a.u, a.rpw_u, a.m_u, gw, nw, lane);
  sh[t] = sqrt(fmax(mx, mu));
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] = fmax(sh[t], sh[t + o]);
    __syncthreads();
  }
  if (t == 0) atomicMax(a.out_bits, (unsigned long long)__double_as_longlong(sh[0]));
}

}  // namespace

void launch_keepout_strip_residual(const double *X_aug, double *Xo, const double *Xp, const double *Uo, const double *Up, long long rows, int x,
                                   int K, int u, double *out, hipStream_t s, bool zero_out) {
  if (rows <= 0) return;
  if (zero_out) HIP_CHECK(hipMemsetAsync(out, 0, sizeof(double), s));  // (else: the caller vouches that *out is 0)
  StripResArgs a;
  a.X_aug = X_aug; a.Xo = Xo; a.Xp = Xp; a.Uo = Uo; a.Up = Up; a.rows = rows; a.x = x; a.xd = x + K; a.u = u;
  a.rpw_x = 64 / a.xd; a.rpw_u = 64 / u;
  a.m_xd = magic((unsigned)a.xd); a.m_u = magic((unsigned)u);
  a.out_bits = (unsigned long long *)out;
  // one wave per trip of the walk over X~out, four waves a block; capped like the residual kernel's grid (one atomic per block)
  const long long trips = (rows + a.rpw_x - 1) / a.rpw_x;
  long long nb = (trips + 3) / 4;
  const long long cap = rows >= 200000 ? 1024 : 256;
  if (nb > cap) nb = cap;
  hipLaunchKernelGGL(k_keepout_strip_residual, dim3((unsigned)nb), dim3(256), 0, s, a);
}

bool keepout_strip_dims_valid(size_t xdim, int K, size_t udim) {
  return xdim >= 1 && K >= 1 && K <= KEEPOUT_MAX_K && xdim + (size_t)K <= (size_t)KEEPOUT_MAX_DIM && udim >= 1 && udim <= (size_t)KEEPOUT_MAX_DIM;
}

bool keepout_cstr_valid(const pmpc_scp_cstr *c, int xdim) {
  if (!c || c->kind != 1 || c->K < 1 || c->K > KEEPOUT_MAX_K || c->pos_dim < 2 || c->pos_dim > 3 || xdim < 1 || xdim + c->K > KEEPOUT_MAX_DIM) return false;
  if (!c->centres || !c->radius || c->centre_stride_particle < 0 || c->centre_stride_stage < 0) return false;
  for (int d = 0; d < c->pos_dim; d++) {
    if (c->pos_idx[d] < 0 || c->pos_idx[d] >= xdim) return false;
    for (int e = 0; e < d; e++)
      if (c->pos_idx[e] == c->pos_idx[d]) return false;
  }
  return true;
}

void launch_keepout_augment(const pmpc_scp_cstr &cstr, int x, int u, int N, int M, const double *X_prev, const double *f, const double *fx,
                            const double *fu, const double *X_ref, double *f_aug, double *fx_aug, double *fu_aug, double *X_prev_aug,
                            double *X_ref_aug, double *xu_aug, hipStream_t s) {
  KeepoutArgs a;
  const int xd = x + cstr.K;
  a.c = cstr; a.x = x; a.u = u; a.N = N; a.units = (long long)M * N;
  a.X_prev = X_prev; a.f = f; a.fx = fx; a.fu = fu; a.X_ref = X_ref;
  a.f_aug = f_aug; a.fx_aug = fx_aug; a.fu_aug = fu_aug; a.X_prev_aug = X_prev_aug; a.X_ref_aug = X_ref_aug; a.xu_aug = xu_aug;
  a.m_xd = magic((unsigned)xd); a.m_xd2 = magic((unsigned)(xd * xd)); a.m_uxd = magic((unsigned)(u * xd));
  if (a.units <= 0) return;
  hipLaunchKernelGGL(k_keepout_augment, dim3((unsigned)((a.units + KO_UNITS - 1) / KO_UNITS)), dim3(KO_THREADS), 0, s, a);
}

extern "C" {

size_t pmpc_abi_scp_cstr_size(void) { return sizeof(pmpc_scp_cstr); }

int pmpc_keepout_augment_device(pmpc_ctx *c, const pmpc_scp_cstr *cstr, size_t xdim, size_t udim, size_t N, size_t M, const double *X_prev,
                                const double *f, const double *fx, const double *fu, const double *X_ref, double *f_aug, double *fx_aug,
                                double *fu_aug, double *X_prev_aug, double *X_ref_aug, double *xu_aug) {
  if (!c || xdim > (size_t)KEEPOUT_MAX_DIM || !keepout_cstr_valid(cstr, (int)xdim) || udim < 1 || udim > (size_t)KEEPOUT_MAX_DIM || N == 0 || M == 0) return 2;
  if (!X_prev || !f || !fx || !fu || !f_aug || !fx_aug || !fu_aug || !X_prev_aug || !xu_aug || (X_ref && !X_ref_aug)) return 2;
  if (N > (size_t)0x7fffffff || M > (size_t)0x7fffffff) return 2;
  try {
    HIP_CHECK(hipSetDevice(c->device));
    ProfScope ps(c, 6);
    launch_keepout_augment(*cstr, (int)xdim, (int)udim, (int)N, (int)M, X_prev, f, fx, fu, X_ref, f_aug, fx_aug, fu_aug, X_prev_aug, X_ref_aug,
                           xu_aug, c->stream);
    HIP_CHECK(hipGetLastError());
  } catch (const PmpcHipError &) {
    return 1;
  }
  return 0;
}

int pmpc_keepout_strip_residual_device(pmpc_ctx *c, size_t xdim, int K, size_t udim, size_t N, size_t M, const double *X_aug, double *X,
                                       const double *X_prev, const double *U, const double *U_prev, double *out) {
  if (!c || !keepout_strip_dims_valid(xdim, K, udim) || N == 0 || M == 0 || N > (size_t)0x7fffffff || M > (size_t)0x7fffffff) return 2;
  if (!X_aug || !X || !X_prev || !U || !U_prev || !out) return 2;
  try {
    HIP_CHECK(hipSetDevice(c->device));
    ProfScope ps(c, 7);
    launch_keepout_strip_residual(X_aug, X, X_prev, U, U_prev, (long long)M * (long long)N, (int)xdim, K, (int)udim, out, c->stream, true);
    HIP_CHECK(hipGetLastError());
  } catch (const PmpcHipError &) {
    return 1;
  }
  return 0;
}

}  // extern "C"
