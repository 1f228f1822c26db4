// react.h — the rate matrix K of dc/dt = -K c and the mobilities w of pfv_transport_advance_react: their check and the
// parameter block the kernels take.  Self-contained (no backend): the entry point calls react_check and react_make,
// the kernels of sweep.inc read ReactPar, and tools/react_host_check.cpp compiles the check for the host alone.
//
// Admissible K (k x k, row-major): K_aa >= 0, K_ab <= 0 off the diagonal, and no column sum below
// -k 2^-52 sum_a |K_ab| (no mass created, up to the rounding of a sum of k terms).  With acc > 0 and A_ii >= 0 every
// row block diag(acc_a + w_a A_ii) + rho K then is a strictly column-diagonally-dominant M-matrix: regular, eliminated
// without pivoting, and with a non-negative inverse.
#pragma once

#include <cmath>
#include <string>

namespace pfv {

constexpr int kReactMax = 8;  // the k x k block and the right-hand side of a row live in registers (sweep_row_react)

struct ReactPar {
  double w[kReactMax];              // mobility per component (1 where the caller passed none)
  double K[kReactMax * kReactMax];  // the caller's matrix, K[a * k + b]
};

// "" when (k, rate, mobility) are admissible; else the text of the error, naming the first offender
inline std::string react_check(int k, const double* rate, const double* mobility) {
  auto finite = [](double v) { return v == v && std::fabs(v) <= 1.79769313486231570e308; };
  if (k < 1 || k > kReactMax) return "k must lie in 1 .. 8 (k = " + std::to_string(k) + ")";
  if (!rate) return "rate is required";
  auto name = [](int a, int b) { return "rate[" + std::to_string(a) + "][" + std::to_string(b) + "]"; };
  for (int a = 0; a < k; ++a)
    for (int b = 0; b < k; ++b) {
      const double v = rate[a * k + b];
      if (!finite(v)) return name(a, b) + " is not finite";
      if (a == b && v < 0.0) return name(a, b) + " is negative (a diagonal entry must not be)";
      if (a != b && v > 0.0) return name(a, b) + " is positive (an off-diagonal entry must not be)";
    }
  for (int b = 0; b < k; ++b) {
    double sum = 0.0, mag = 0.0;
    for (int a = 0; a < k; ++a) {
      sum += rate[a * k + b];
      mag += std::fabs(rate[a * k + b]);
    }
    if (sum < -(double)k * 2.220446049250313e-16 * mag)
      return "column " + std::to_string(b) + " of rate has a negative sum (" + std::to_string(sum) +
             "): component " + std::to_string(b) + " would create mass";
  }
  if (mobility)
    for (int a = 0; a < k; ++a) {
      if (!finite(mobility[a])) return "mobility[" + std::to_string(a) + "] is not finite";
      if (mobility[a] < 0.0) return "mobility[" + std::to_string(a) + "] is negative";
    }
  return "";
}

// (after react_check)
inline ReactPar react_make(int k, const double* rate, const double* mobility) {
  ReactPar P;
  for (int a = 0; a < kReactMax; ++a) P.w[a] = a < k && mobility ? mobility[a] : 1.0;
  for (int m = 0; m < kReactMax * kReactMax; ++m) P.K[m] = m < k * k ? rate[m] : 0.0;
  return P;
}

}  // namespace pfv
