// cone_smooth_math.h — the host mathematics of the smoothed cone objective's Newton iteration (SmoothSolve, solver_cone_smooth.hip): plain
// C++ over double* / std::vector<double>, no device call, no context.  Included by solver_cone_smooth.hip ONLY (same compiler, same flags:
// no fused multiply-add on the host side, so every loop here keeps the iteration order and expression shape its result depends on), and by
// the stand-alone program of tests/test_cone_smooth_math.py.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <utility>
#include <vector>

namespace pmpc_smooth {

// (beyond |w| = 40 the exponential is below the last bit of 1: no libm call.  At config D all but a few dozen of the 4096 rows are
//  saturated at every evaluation, and the exponentials of solve_t / Fval were more than half of a Newton step's wall time)
inline double sigm(double w) { return w > 40.0 ? 1.0 : (w < -40.0 ? std::exp(w) : (w >= 0.0 ? 1.0 / (1.0 + std::exp(-w)) : std::exp(w) / (1.0 + std::exp(w)))); }
inline double softplus(double w) { return w > 40.0 ? w : (w < -40.0 ? std::exp(w) : (w > 0.0 ? w + std::log1p(std::exp(-w)) : std::log1p(std::exp(w)))); }

// The epigraph rows J_i - t <= 0 under the entropic proximal term (exponential method of multipliers for multipliers boxed in [0, cap]):
// with l_i = logit(lam_i / cap)
//   m_i(v) = cap * sigmoid(l_i + v / rho),   psi(v; l_i) = rho cap [softplus(l_i + v / rho) - softplus(l_i)],   psi'' = m (cap - m) / (rho cap) > 0:
// every row carries a rank-one term, F is smooth (the quadratic proximal term's clipping makes its second derivative jump between 0
// and 1/rho — at config D the semismooth Newton iteration then flips a handful of rows in and out of the hinge for ever), and the
// update l_i += v_i / rho sends the multiplier of a row below the threshold to zero geometrically.
struct HingeRows {
  std::vector<double> lam;  // the logits l_i
  double rho = 1.0;         // proximal parameter = width of the smoothed hinge in cost units
  double cap = 1.0, K = 1.0;  // multipliers in [0, cap], summing to K
  double t_guess = std::numeric_limits<double>::quiet_NaN();  // solve_t: where the last one ended

  int M() const { return (int)lam.size(); }
  double mult(int i, const std::vector<double> &Jv, double t) const { return cap * sigm(lam[i] + (Jv[i] - t) / rho); }

  // sum_i m_i(J_i - t) = K  (smooth, strictly decreasing in t): safeguarded Newton
  double solve_t(const std::vector<double> &Jv) {
    double lo = 1e300, hi = -1e300;
    for (int i = 0; i < M(); i++) { const double c0 = Jv[i] + rho * lam[i]; lo = std::min(lo, c0); hi = std::max(hi, c0); }
    lo -= 50.0 * rho + 1.0; hi += 50.0 * rho + 1.0;
    double tt = (t_guess == t_guess && t_guess > lo && t_guess < hi) ? t_guess : 0.5 * (lo + hi);
    for (int it = 0; it < 200; it++) {
      double sm = 0.0, ds = 0.0;
      for (int i = 0; i < M(); i++) {
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
  }

  // F at costs Jv, threshold t and barrier value bval
  double Fval(const std::vector<double> &Jv, double t, double bval) const {
    double f = 0.0;
    for (int i = 0; i < M(); i++) f += softplus(lam[i] + (Jv[i] - t) / rho) - softplus(lam[i]);
    return K * t + bval + rho * cap * f;
  }

  // What a Newton step at (Jv, t) needs of every row: multiplier mu_i, curvature sig_i = psi'', cost weight of the sweeps (a particle of
  // multiplier zero keeps a strictly convex sub-problem).  Returns sum mu_i.
  double newton_weights(const std::vector<double> &Jv, double t, std::vector<double> &mu, std::vector<double> &sig, double *weight) const {
    double summu = 0.0;
    for (int i = 0; i < M(); i++) {
      mu[i] = mult(i, Jv, t);
      sig[i] = mu[i] * (cap - mu[i]) / (rho * cap);
      summu += mu[i];
      weight[i] = std::max(mu[i], 1e-8);
    }
    return summu;
  }

  // multiplier update of the proximal method at (Jv, t): l_i += (J_i - t) / rho.  Returns the largest change of a multiplier.
  double update(const std::vector<double> &Jv, double t) {
    double dl = 0.0;
    for (int i = 0; i < M(); i++) {
      const double m_old = cap * sigm(lam[i]), m_new = mult(i, Jv, t);
      dl = std::max(dl, std::fabs(m_new - m_old));
      lam[i] = std::min(700.0, std::max(-700.0, lam[i] + (Jv[i] - t) / rho));
    }
    return dl;
  }

  // largest complementarity violation of an epigraph row at the threshold t
  double complementarity(const std::vector<double> &Jv, double t) const {
    double comp = 0.0;
    for (int i = 0; i < M(); i++) {
      const double m_i = cap * sigm(lam[i]), v = Jv[i] - t;
      comp = std::max(comp, v > 0.0 ? v * (cap - m_i) : -v * m_i);
    }
    return comp;
  }

  // Remembered logits may belong to ANOTHER problem of this shape.  A multiplier saturated at the wrong end of [0, cap] takes
  // |l| rho / |J - t| updates to come back: where the costs at the start rank a particle clearly on the other side of the threshold
  // than its remembered multiplier says, the logit is pulled back to +-12 (inside an SCP loop the sides agree and nothing changes)
  void pull_back(const std::vector<double> &Jv) {
    std::vector<int> idx(M());
    for (int i = 0; i < M(); i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](int a_, int b_) { return Jv[a_] > Jv[b_]; });
    const int n_top = (int)(K / cap);  // about this many rows carry the full multiplier
    for (int r = 0; r < M(); r++) {
      const int i = idx[r];
      if (lam[i] > 12.0 && r >= n_top + 2) lam[i] = 12.0;
      if (lam[i] < -12.0 && r < n_top - 1) lam[i] = -12.0;
    }
  }
};

// The (nc + 1) Newton system of the shared controls and t.  Per particle: H_i (nc x nc, column-major, only the UPPER triangle is read),
// condensed gradients gb_i (of sum m_i J_i + barrier) and ga_i (of J_i), dots_i = {-kappa_i, pi_i, .} and the curvature sig_i of its row;
// Sherman-Morrison folds every row's rank-one term in.  solve(): false = zero pivot; else sol = [du_c | dt] and coef_i, the weight of
// the second solve's feed-forward in particle i's direction.
struct NewtonSystem {
  int M, nc, n1;
  std::vector<double> A, rhs, sol, sp, kap, pi_;
  NewtonSystem(int M_, int nc_) : M(M_), nc(nc_), n1(nc_ + 1), A((size_t)n1 * n1, 0.0), rhs(n1, 0.0), sol(n1, 0.0), sp(M_), kap(M_), pi_(M_) {}

  void assemble(const double *Hh, const double *gb, const double *ga, const double *dots, const double *sig, double k_minus_summu) {
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
    rhs[nc] -= k_minus_summu;
    A[nc + (size_t)n1 * nc] = cc > 0.0 ? cc : 1.0;  // (no row strictly inside: t stays — it is re-optimised exactly at the next point)
    if (!(cc > 0.0)) {
      rhs[nc] = 0.0;
      for (int r = 0; r < nc; r++) A[r + (size_t)n1 * nc] = A[nc + (size_t)n1 * r] = 0.0;
    }
  }

  // Gaussian elimination with partial pivoting (the matrix is positive definite; n1 = Nc u + 1): sol = A^-1 rhs.  false: zero pivot
  bool eliminate() {
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
      if (!(std::fabs(d) > 0.0)) return false;
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
    return true;
  }

  void coefficients(const double *ga, const double *sig, double *coef) const {
    const double dt = sol[nc];
    for (int i = 0; i < M; i++) {
      double e_ = pi_[i] - dt;
      for (int r = 0; r < nc; r++) e_ += ga[(size_t)i * nc + r] * sol[r];
      coef[i] = sig[i] * e_ / (1.0 + sig[i] * kap[i]);
    }
  }

  bool solve(const double *Hh, const double *gb, const double *ga, const double *dots, const double *sig, double k_minus_summu, double *coef) {
    assemble(Hh, gb, ga, dots, sig, k_minus_summu);
    if (!eliminate()) return false;
    coefficients(ga, sig, coef);
    return true;
  }
};

// The multiplier iteration is a fixed-point map that contracts LINEARLY at a fixed hinge width (rate ~ rho / (rho + curvature)): once
// the width sits on its floor and two successive updates of the rows INSIDE the hinge point the same way with a steady ratio r, the
// remaining geometric series is summed at once (Aitken):  l += r / (1 - r) * delta.  (Measured at config D: 50 updates at rate 0.74.)
// Rows at either end of [0, cap] drift to +-infinity at constant speed in the logits anyway and are left alone.
struct Aitken {
  std::vector<double> dlam_prev, dlam_cur;
  bool have_prev_delta = false;
  double r_prev = -1.0, rho_at_prev_delta = -1.0;
  int since_extrap = 2;
  explicit Aitken(int M) : dlam_prev(M, 0.0), dlam_cur(M, 0.0) {}

  struct Outcome {
    bool extrapolated;
    double r, gain;
    int nin;  // rows inside the hinge
  };
  // after the update lam_before -> lam at width rho: extrapolates lam where the rule applies, else remembers this update
  Outcome step(std::vector<double> &lam, const std::vector<double> &lam_before, double rho, double cap) {
    const int M = (int)lam.size();
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
      have_prev_delta = false;
      since_extrap = 0;
      r_prev = -1.0;
      return {true, r, gain, nin};
    }
    r_prev = (have_prev_delta && same_map) ? r : -1.0;
    dlam_prev.swap(dlam_cur);
    have_prev_delta = true;
    rho_at_prev_delta = rho;
    since_extrap++;
    return {false, r, 0.0, nin};
  }
};

// Full steps in the quadratic regime: after a step s the iterate is off by ~ quad_c s^2.  Once that is a tenth of the tolerance the
// step that would only confirm it (1e-9 .. 1e-14 in the traces of config D: a third of all Newton steps, two factor sweeps each) is
// not taken.  quad_c: contraction constant |step_{n+1}| ~ quad_c |step_n|^2, measured on this solve's own consecutive full steps (the
// largest ratio seen; 1e3 until there is one).
struct QuadRegime {
  double quad_c = 1e3;
  double s_prev = -1.0;  // the previous full Newton step of this inner solve (new_inner_solve, damped_step: none)
  void new_inner_solve() { s_prev = -1.0; }
  void damped_step() { s_prev = -1.0; }
  // a full step of size `step`: true = the inner problem counts as solved to step_tol without the confirming step
  bool full_step(double step, double step_tol) {
    if (s_prev > 0.0 && s_prev < 1e-2 && step < s_prev) quad_c = std::max(quad_c == 1e3 ? 1.0 : quad_c, std::min(1e6, step / (s_prev * s_prev)));
    if (step <= 1e-3 && 10.0 * quad_c * step * step <= step_tol) return true;
    s_prev = step;
    return false;
  }
};

// Proximal parameter rho = width of the smoothed hinge in cost units.  The method converges for ANY rho (the multipliers are exact at
// its fixed point); a narrow hinge makes one multiplier update nearly exact but its inner problem nearly non-smooth — with few rows
// strictly inside, every Newton step crosses kinks and the line search cuts it to nothing (measured at config D: steps of 1e-4 below
// rho ~ 1e-3 max|J|) —, a wide one gives inner problems that settle in a few full steps and more multiplier updates.  Adaptive: start
// wide, narrow by 3 after an inner solve that took full steps, widen by 3 after one that was damped throughout.
struct HingeWidth {
  double rho_min = 0.0, rho_max = 0.0, rho_floor = 0.0, dl_last = 1e300;

  // the range from the costs at the start; returns the first width (remembered: the width the last solve of the shape ended with, or <= 0)
  double start(const std::vector<double> &J, double remembered) {
    double jlo = 1e300, jhi = -1e300;
    for (size_t i = 0; i < J.size(); i++) { jlo = std::min(jlo, J[i]); jhi = std::max(jhi, J[i]); }
    rho_min = 1e-6 * std::max(1.0, std::max(std::fabs(jlo), std::fabs(jhi)));
    rho_max = 1e5 * rho_min;
    double rho = remembered > 0.0 ? 3.0 * remembered : 1e4 * rho_min;
    if (!(rho >= rho_min && rho <= rho_max)) rho = 1e4 * rho_min;
    return rho;
  }
  // the inner problem was not solved at rho: never below 3 rho again (until the floor decays), ten times wider now
  double widened(double rho) {
    rho_floor = std::max(rho_floor, 3.0 * rho);
    return std::min(rho_max, 10.0 * rho);
  }
  // After a solved inner problem with n_damped steps cut below 0.2 and a multiplier change dl.  A sharper hinge makes the multiplier
  // updates contract faster — wanted while they are far off or contracting slowly; never below a width whose inner problem this solve
  // has already failed to solve.  (The floor is what a failed inner solve from a FAR start taught; next to the fixed point a sharper
  // hinge is solvable again — Newton starts inside its basin — so the floor decays while the inner solves take full steps.)
  double adapted(double rho, int n_damped, double dl, double cap) {
    if (n_damped == 0) rho_floor *= 0.5;
    if (n_damped == 0 && (dl > 1e-2 * cap || dl > 0.3 * dl_last)) rho = std::max(std::max(rho_min, rho_floor), rho / 3.0);
    else if (n_damped >= 3) rho = std::min(rho_max, 3.0 * rho);
    dl_last = dl;
    return rho;
  }
};

// the inner problems are solved as sharply as the multipliers are known (looser — 1e-1 dl, cap 1e-3 — measured: no fewer Newton steps)
inline double step_tolerance(double dl_prev) { return std::max(1e-9, std::min(1e-5, 1e-3 * dl_prev)); }

}  // namespace pmpc_smooth
