// isotherm.h — the sorption isotherm S(c) of the sorbing transport step (pfv_transport_advance_sorb): its two parameters,
// their check and its evaluation with the derivative.  Self-contained (no backend): the kernels of sweep.inc inline
// isotherm_eval, the entry point calls isotherm_check, and tools/isotherm_host_check.cpp compiles both for the host alone.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/porefv.h"

#ifndef PFV_FN
#define PFV_FN inline
#endif

namespace pfv {

// One component's isotherm as the kernels read it from a device array under the component index: 24 bytes, three
// doubles wide (the array lives in a buffer of doubles).
struct Isotherm {
  int32_t kind = PFV_ISOTHERM_LINEAR;
  int32_t pad = 0;
  double p0 = 0.0, p1 = 0.0;  // linear: Kd, -; Freundlich: Kf, n; Langmuir: q_max, b
};
static_assert(sizeof(Isotherm) == 3 * sizeof(double), "Isotherm is three doubles wide");

// "" when (kind, p0, p1) describe an isotherm; else the text of the error, naming the first offender
inline std::string isotherm_check(int kind, double p0, double p1) {
  auto finite = [](double v) { return v == v && std::fabs(v) <= 1.79769313486231570e308; };
  if (kind == PFV_ISOTHERM_LINEAR) {
    if (!finite(p0)) return "linear isotherm parameter Kd (index 0) is not finite";
    if (p0 < 0.0) return "linear isotherm parameter Kd (index 0) is negative";
    return "";
  }
  if (kind == PFV_ISOTHERM_FREUNDLICH) {
    if (!finite(p0)) return "Freundlich parameter Kf (index 0) is not finite";
    if (!finite(p1)) return "Freundlich parameter n (index 1) is not finite";
    if (p0 < 0.0) return "Freundlich parameter Kf (index 0) is negative";
    if (!(p1 > 0.0)) return "Freundlich parameter n (index 1) must be positive";
    return "";
  }
  if (kind == PFV_ISOTHERM_LANGMUIR) {
    if (!finite(p0)) return "Langmuir parameter q_max (index 0) is not finite";
    if (!finite(p1)) return "Langmuir parameter b (index 1) is not finite";
    if (p0 < 0.0) return "Langmuir parameter q_max (index 0) is negative";
    if (p1 < 0.0) return "Langmuir parameter b (index 1) is negative";
    return "";
  }
  return "unknown isotherm kind " + std::to_string(kind);
}

// (after isotherm_check; the second parameter of a linear isotherm is not kept)
inline Isotherm isotherm_make(int kind, double p0, double p1) {
  Isotherm I;
  I.kind = kind;
  I.p0 = p0;
  I.p1 = kind == PFV_ISOTHERM_LINEAR ? 0.0 : p1;
  return I;
}

// S(c) and S'(c) for c >= 0.  Freundlich takes the slope from the value, n S / c -- no second power --; at c = 0 it is
// the limit: +infinity for n < 1, Kf for n = 1, 0 for n > 1.  An infinite slope is a value the caller must expect.
PFV_FN double isotherm_eval(const Isotherm& I, double c, double* dS) {
  if (I.kind == PFV_ISOTHERM_FREUNDLICH) {
    const double S = I.p0 * pow(c, I.p1);
    if (c > 0.0) *dS = I.p1 * S / c;
    else *dS = I.p1 < 1.0 ? (I.p0 > 0.0 ? HUGE_VAL : 0.0) : (I.p1 == 1.0 ? I.p0 : 0.0);
    return S;
  }
  if (I.kind == PFV_ISOTHERM_LANGMUIR) {
    const double inv = 1.0 / (1.0 + I.p1 * c);
    const double qb = I.p0 * I.p1;
    *dS = qb * inv * inv;
    return qb * c * inv;
  }
  *dS = I.p0;
  return I.p0 * c;
}

}  // namespace pfv
