// The pair term of the scalar field sums (stream function, analytic vorticity) and the float64 logarithm it needs: device
// helpers only, no kernel inside, so any unit may include it -- field_kernels.hpp (pair_scalar_f64, flowfield.hip) and
// march_kernels.hpp (the wake energy of ludvm_march_set_integrals, march.hip) form their psi pairs with the same code.
#pragma once
#include "pair_kernels.hpp"

namespace ludvm {

enum ScalarKind { kScalarPsi = 0, kScalarOmega = 1 };      // (= LUDVM_FIELD_*, flowfield.hip asserts it)
constexpr double kInv4PiD = 0.07957747154594766788444;      // (kInvPiD: pair_kernels.hpp)

// ln(a) in float64 to < 1 ulp for a >= 0 (-inf at 0; +inf and NaN pass through), in about 40 instructions where OCML's log
// takes about 90 -- and the logarithm is most of a PSI pair.  The classical form (fdlibm's e_log.c, whose minimax coefficients
// Lg1 .. Lg7 these are): a = 2^k m with m in [sqrt(1/2), sqrt(2)), f = m - 1, s = f / (2 + f), and
//   ln m = f - f^2 / 2 + s (f^2 / 2 + R(s^2)),  R(z) = Lg1 z + ... + Lg7 z^7,   ln a = k ln2_hi + (ln m + k ln2_lo).
// The quotient is v_rcp_f64 refined by two Newton steps and one residual correction, not a division (its scale / fixup
// steps guard ranges f and 2 + f never leave).  v_frexp_* normalise subnormals themselves.
__device__ __forceinline__ double log_f64(double a) {
  double m = __builtin_amdgcn_frexp_mant(a);                // [1/2, 1)
  int k = __builtin_amdgcn_frexp_exp(a);
  const bool low = m < 0.70710678118654752440;
  m = low ? m + m : m;
  k = low ? k - 1 : k;
  const double f = m - 1.0, d = 2.0 + f;                    // f in [-0.293, 0.414], d in [1.707, 2.414]
  double y = __builtin_amdgcn_rcp(d);
  y = __builtin_fma(y, __builtin_fma(-d, y, 1.0), y);
  y = __builtin_fma(y, __builtin_fma(-d, y, 1.0), y);
  double s = f * y;
  s = __builtin_fma(__builtin_fma(-d, s, f), y, s);
  const double z = s * s, w = z * z;
  const double t1 = w * __builtin_fma(w, __builtin_fma(w, 1.531383769920937332e-01, 2.222219843214978396e-01), 3.999999999940941908e-01);
  const double t2 = z * __builtin_fma(w, __builtin_fma(w, __builtin_fma(w, 1.479819860511658591e-01, 1.818357216161805012e-01),
                                                       2.857142874366239149e-01), 6.666666666666735130e-01);
  const double hfsq = 0.5 * f * f, dk = (double)k;
  const double r = dk * 6.93147180369123816490e-01 -
                   ((hfsq - __builtin_fma(s, hfsq + (t2 + t1), dk * 1.90821492927058770002e-10)) - f);
  // (a = 0 leaves a finite r: the -inf is ADDED, so that the compiler keeps one straight line of code for every lane)
  return (a < __builtin_inf() ? r : a) + (a == 0.0 ? -__builtin_inf() : 0.0);
}

template <int KIND>
__device__ __forceinline__ double scalar_term(double dx, double dz, double vc4) {
  const double r2 = __builtin_fma(dz, dz, dx * dx);
  const double q = __builtin_fma(r2, r2, vc4);
  const double y = rsqrt_f64(q);
  if (KIND == kScalarOmega) return y * y * y;               // s^-3 (the factor -vc^4 / pi: once per target)
  const double s = q > 0.0 ? q * y : q;                     // sqrt(q); q = 0 (inviscid, coincident): 0, not 0 * inf
  return log_f64(0.5 * (r2 + s));
}

}  // namespace ludvm
