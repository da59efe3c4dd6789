// special_fn.hpp -- the one digamma of the global-step kernels (gmm_train.hip, gmm_wide.hip, lds_global.hip) and their
// NIW scale matrix, usable on the host as well: `__host__ __device__` under hipcc, plain `inline` for any C++ compiler
// (tests/test_special_fn_cpu.py compiles a stand-alone program from this header alone and compares it with a 50-digit
// digamma).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SVAE_HOST_DEVICE __host__ __device__
#else
#define SVAE_HOST_DEVICE
#endif

namespace svae {

// psi(x), x > 0: recurrence up to x >= 10, then the asymptotic series (error < 1e-16 there).  Anything else -- zero, a
// negative number, NaN -- returns NaN BEFORE the recurrence: the loop then runs at most 10 trips whatever the input (for
// x = -inf, or below about -9e15, x + 1 == x and an unguarded loop never ends; x is alpha or (nu - i)/2 straight from
// device-resident parameters nobody inspects).
SVAE_HOST_DEVICE inline double digamma_pos(double x) {
  if (!(x > 0.0)) return __builtin_nan("");
  double acc = 0.0;
  while (x < 10.0) { acc -= 1.0 / x; x += 1.0; }
  const double r = 1.0 / x, r2 = r * r;
  const double s = -1.0 / 12.0 + r2 * (1.0 / 120.0 + r2 * (-1.0 / 252.0 + r2 * (1.0 / 240.0 + r2 * (-1.0 / 132.0
                   + r2 * (691.0 / 32760.0 + r2 * (-1.0 / 12.0))))));
  return acc + log(x) - 0.5 * r + r2 * s;
}

// The NIW scale matrix S = A - b b'/kappa from the natural parameter, entry (i, j), without the digits the plain
// A_ij - b_i (b_j / kappa) loses for a mean far off the spread (|m|^2 kappa / |S|: the rounding of m_j = b_j / kappa is
// multiplied by b_i).  niw_mean_residual returns r_j = (b_j - m_j kappa) / kappa, the part of b_j / kappa that m_j
// dropped (exact remainder by fma); S_ij = (A_ij - b_i m_j) - b_i r_j with the first difference rounded once.
SVAE_HOST_DEVICE inline double niw_mean_residual(double b_j, double m_j, double kappa) {
  return __builtin_fma(-m_j, kappa, b_j) / kappa;
}

SVAE_HOST_DEVICE inline double niw_scale_entry(double A_ij, double b_i, double m_j, double r_j) {
  return __builtin_fma(-b_i, r_j, __builtin_fma(-b_i, m_j, A_ij));
}

}  // namespace svae
