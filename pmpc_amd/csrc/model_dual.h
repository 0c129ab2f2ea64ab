// model_dual.h — forward-mode dual numbers for the runtime-compiled dynamics models (model_jit.hip, model_kernels.h).
//
// Dual<ND> carries a value and ND directional derivatives.  A user's `template <class T> step(const T *x, const T *u, const double *p,
// T *xn)` is instantiated with T = double (rollout, plan shift) and with T = Dual<W> (linearisation: W derivative directions per pass);
// every function below has the name of its <cmath> counterpart, so one body serves both.  At a kink (fabs at 0, fmin / fmax at a tie)
// the derivative is that of the branch the VALUE takes (fabs: the branch of v >= 0; fmin / fmax: the first argument).  Comparisons go
// by value.  This very file is what the runtime compiler reads (the Makefile wraps it into model_dual.inc) and what the host test
// compiles with g++: host C++ and device code behind PMPC_HD.
#pragma once
#if defined(__HIPCC_RTC__)
#define PMPC_HD __device__ __forceinline__
#elif defined(__HIPCC__)
#include <cmath>
#define PMPC_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define PMPC_HD inline
#endif

namespace pmpc_dual {

template <int ND>
struct Dual {
  double v;
  double d[ND];
  PMPC_HD Dual() : v(0.0) {
    for (int k = 0; k < ND; k++) d[k] = 0.0;
  }
  PMPC_HD Dual(double value) : v(value) {  // a constant: no direction moves it
    for (int k = 0; k < ND; k++) d[k] = 0.0;
  }
  PMPC_HD Dual &operator+=(const Dual &b) { return *this = *this + b; }
  PMPC_HD Dual &operator-=(const Dual &b) { return *this = *this - b; }
  PMPC_HD Dual &operator*=(const Dual &b) { return *this = *this * b; }
  PMPC_HD Dual &operator/=(const Dual &b) { return *this = *this / b; }
  PMPC_HD Dual &operator+=(double b) { v += b; return *this; }
  PMPC_HD Dual &operator-=(double b) { v -= b; return *this; }
  PMPC_HD Dual &operator*=(double b) { return *this = *this * b; }
  PMPC_HD Dual &operator/=(double b) { return *this = *this / b; }
};

// r = (value, da * a' + db * b'): the chain rule of a function of one or two duals
template <int ND>
PMPC_HD Dual<ND> chain(double value, double da, const Dual<ND> &a) {
  Dual<ND> r;
  r.v = value;
  for (int k = 0; k < ND; k++) r.d[k] = da * a.d[k];
  return r;
}
template <int ND>
PMPC_HD Dual<ND> chain(double value, double da, const Dual<ND> &a, double db, const Dual<ND> &b) {
  Dual<ND> r;
  r.v = value;
  for (int k = 0; k < ND; k++) r.d[k] = da * a.d[k] + db * b.d[k];
  return r;
}

template <int ND> PMPC_HD Dual<ND> operator+(const Dual<ND> &a) { return a; }
template <int ND> PMPC_HD Dual<ND> operator-(const Dual<ND> &a) { return chain(-a.v, -1.0, a); }

template <int ND> PMPC_HD Dual<ND> operator+(const Dual<ND> &a, const Dual<ND> &b) { return chain(a.v + b.v, 1.0, a, 1.0, b); }
template <int ND> PMPC_HD Dual<ND> operator-(const Dual<ND> &a, const Dual<ND> &b) { return chain(a.v - b.v, 1.0, a, -1.0, b); }
template <int ND> PMPC_HD Dual<ND> operator*(const Dual<ND> &a, const Dual<ND> &b) { return chain(a.v * b.v, b.v, a, a.v, b); }
template <int ND> PMPC_HD Dual<ND> operator/(const Dual<ND> &a, const Dual<ND> &b) {
  const double ib = 1.0 / b.v, q = a.v * ib;
  return chain(q, ib, a, -q * ib, b);
}

template <int ND> PMPC_HD Dual<ND> operator+(const Dual<ND> &a, double b) { Dual<ND> r = a; r.v += b; return r; }
template <int ND> PMPC_HD Dual<ND> operator-(const Dual<ND> &a, double b) { Dual<ND> r = a; r.v -= b; return r; }
template <int ND> PMPC_HD Dual<ND> operator*(const Dual<ND> &a, double b) { return chain(a.v * b, b, a); }
template <int ND> PMPC_HD Dual<ND> operator/(const Dual<ND> &a, double b) { return chain(a.v / b, 1.0 / b, a); }

template <int ND> PMPC_HD Dual<ND> operator+(double a, const Dual<ND> &b) { Dual<ND> r = b; r.v += a; return r; }
template <int ND> PMPC_HD Dual<ND> operator-(double a, const Dual<ND> &b) { return chain(a - b.v, -1.0, b); }
template <int ND> PMPC_HD Dual<ND> operator*(double a, const Dual<ND> &b) { return chain(a * b.v, a, b); }
template <int ND> PMPC_HD Dual<ND> operator/(double a, const Dual<ND> &b) {
  const double q = a / b.v;
  return chain(q, -q / b.v, b);
}

#define PMPC_DUAL_CMP(op)                                                                             \
  template <int ND> PMPC_HD bool operator op(const Dual<ND> &a, const Dual<ND> &b) { return a.v op b.v; } \
  template <int ND> PMPC_HD bool operator op(const Dual<ND> &a, double b) { return a.v op b; }            \
  template <int ND> PMPC_HD bool operator op(double a, const Dual<ND> &b) { return a op b.v; }
PMPC_DUAL_CMP(<)
PMPC_DUAL_CMP(<=)
PMPC_DUAL_CMP(>)
PMPC_DUAL_CMP(>=)
PMPC_DUAL_CMP(==)
PMPC_DUAL_CMP(!=)
#undef PMPC_DUAL_CMP

template <int ND> PMPC_HD Dual<ND> sin(const Dual<ND> &a) { return chain(::sin(a.v), ::cos(a.v), a); }
template <int ND> PMPC_HD Dual<ND> cos(const Dual<ND> &a) { return chain(::cos(a.v), -::sin(a.v), a); }
template <int ND> PMPC_HD Dual<ND> tan(const Dual<ND> &a) {
  const double t = ::tan(a.v);
  return chain(t, 1.0 + t * t, a);
}
template <int ND> PMPC_HD Dual<ND> exp(const Dual<ND> &a) {
  const double e = ::exp(a.v);
  return chain(e, e, a);
}
template <int ND> PMPC_HD Dual<ND> log(const Dual<ND> &a) { return chain(::log(a.v), 1.0 / a.v, a); }
template <int ND> PMPC_HD Dual<ND> sqrt(const Dual<ND> &a) {
  const double s = ::sqrt(a.v);
  return chain(s, 0.5 / s, a);
}
template <int ND> PMPC_HD Dual<ND> tanh(const Dual<ND> &a) {
  const double t = ::tanh(a.v);
  return chain(t, 1.0 - t * t, a);
}
template <int ND> PMPC_HD Dual<ND> atan(const Dual<ND> &a) { return chain(::atan(a.v), 1.0 / (1.0 + a.v * a.v), a); }
// atan2(y, x): d = (x dy - y dx) / (x^2 + y^2)
template <int ND> PMPC_HD Dual<ND> atan2(const Dual<ND> &y, const Dual<ND> &x) {
  const double ir = 1.0 / (x.v * x.v + y.v * y.v);
  return chain(::atan2(y.v, x.v), x.v * ir, y, -y.v * ir, x);
}
template <int ND> PMPC_HD Dual<ND> atan2(const Dual<ND> &y, double x) { return chain(::atan2(y.v, x), x / (x * x + y.v * y.v), y); }
template <int ND> PMPC_HD Dual<ND> atan2(double y, const Dual<ND> &x) { return chain(::atan2(y, x.v), -y / (x.v * x.v + y * y), x); }
// pow with a constant exponent
template <int ND> PMPC_HD Dual<ND> pow(const Dual<ND> &a, double e) { return chain(::pow(a.v, e), e * ::pow(a.v, e - 1.0), a); }
template <int ND> PMPC_HD Dual<ND> fabs(const Dual<ND> &a) { return a.v >= 0.0 ? a : -a; }
template <int ND> PMPC_HD Dual<ND> fmin(const Dual<ND> &a, const Dual<ND> &b) { return a.v <= b.v ? a : b; }
template <int ND> PMPC_HD Dual<ND> fmax(const Dual<ND> &a, const Dual<ND> &b) { return a.v >= b.v ? a : b; }
template <int ND> PMPC_HD Dual<ND> fmin(const Dual<ND> &a, double b) { return a.v <= b ? a : Dual<ND>(b); }
template <int ND> PMPC_HD Dual<ND> fmax(const Dual<ND> &a, double b) { return a.v >= b ? a : Dual<ND>(b); }
template <int ND> PMPC_HD Dual<ND> fmin(double a, const Dual<ND> &b) { return a <= b.v ? Dual<ND>(a) : b; }
template <int ND> PMPC_HD Dual<ND> fmax(double a, const Dual<ND> &b) { return a >= b.v ? Dual<ND>(a) : b; }

}  // namespace pmpc_dual
