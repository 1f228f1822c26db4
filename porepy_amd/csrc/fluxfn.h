// fluxfn.h — the flux function f(s) of the saturation step (pfv_transport_advance_nl): its parameters, their check and
// its evaluation with the derivative.  Self-contained (no backend): the kernels of sweep.inc inline fluxfn_eval, the
// entry point calls fluxfn_check, and tools/fluxfn_host_check.cpp compiles both for the host alone.
#pragma once

#include <cmath>
#include <string>

#include "../../include/porefv.h"

#ifndef PFV_FN
#define PFV_FN inline
#endif

namespace pfv {

constexpr int kFluxTableMin = 2, kFluxTableMax = 1024;

struct FluxFn {
  int kind = PFV_FLUXFN_LINEAR;
  double s_wr = 0.0, inv_span = 1.0;  // Corey: s_e = (s - s_wr) * inv_span, inv_span = 1 / (1 - s_wr - s_nr)
  double n_w = 1.0, n_n = 1.0, inv_mu_w = 1.0, inv_mu_n = 1.0;
  const double* table = nullptr;      // table: m values on uniform knots over [0, 1] (device memory in the kernels)
  int m = 0;
};

// "" when (kind, params, n_params) describe a flux function; else the text of the error, naming the first offender
inline std::string fluxfn_check(int kind, const double* params, int n_params) {
  auto finite = [](double v) { return v == v && std::fabs(v) <= 1.79769313486231570e308; };
  if (kind == PFV_FLUXFN_LINEAR) {
    if (n_params != 0) return "PFV_FLUXFN_LINEAR takes no parameters (n_params = " + std::to_string(n_params) + ")";
    return "";
  }
  if (kind == PFV_FLUXFN_COREY) {
    if (n_params != 6 || !params)
      return "PFV_FLUXFN_COREY takes 6 parameters: s_wr, s_nr, n_w, n_n, mu_w, mu_n (n_params = " +
             std::to_string(n_params) + ")";
    static const char* name[6] = {"s_wr", "s_nr", "n_w", "n_n", "mu_w", "mu_n"};
    for (int k = 0; k < 6; ++k)
      if (!finite(params[k])) return std::string("Corey parameter ") + name[k] + " (index " + std::to_string(k) + ") is not finite";
    for (int k = 0; k < 2; ++k)
      if (params[k] < 0.0) return std::string("Corey parameter ") + name[k] + " (index " + std::to_string(k) + ") is negative";
    if (params[0] + params[1] >= 1.0) return "Corey parameters s_wr + s_nr (indices 0, 1) must stay below 1";
    for (int k = 2; k < 6; ++k)
      if (!(params[k] > 0.0)) return std::string("Corey parameter ") + name[k] + " (index " + std::to_string(k) + ") must be positive";
    return "";
  }
  if (kind == PFV_FLUXFN_TABLE) {
    if (n_params < kFluxTableMin || n_params > kFluxTableMax || !params)
      return "PFV_FLUXFN_TABLE takes 2 .. 1024 values (n_params = " + std::to_string(n_params) + ")";
    for (int k = 0; k < n_params; ++k) {
      if (!finite(params[k])) return "flux table value " + std::to_string(k) + " is not finite";
      if (k > 0 && params[k] < params[k - 1]) return "flux table decreases at value " + std::to_string(k);
    }
    return "";
  }
  return "unknown flux function kind " + std::to_string(kind);
}

// (after fluxfn_check; a table's values are referenced, not copied)
inline FluxFn fluxfn_make(int kind, const double* params, int n_params, const double* table) {
  FluxFn F;
  F.kind = kind;
  if (kind == PFV_FLUXFN_COREY) {
    F.s_wr = params[0];
    F.inv_span = 1.0 / (1.0 - params[0] - params[1]);
    F.n_w = params[2];
    F.n_n = params[3];
    F.inv_mu_w = 1.0 / params[4];
    F.inv_mu_n = 1.0 / params[5];
  } else if (kind == PFV_FLUXFN_TABLE) {
    F.table = table;
    F.m = n_params;
  }
  return F;
}

// f(s) and f'(s) (one-sided, 0 where the curve is flat: outside [0, 1], beyond the residual saturations)
PFV_FN double fluxfn_eval(const FluxFn& F, double s, double* df) {
  if (F.kind == PFV_FLUXFN_COREY) {
    double se = (s - F.s_wr) * F.inv_span;
    const bool inside = se > 0.0 && se < 1.0;
    se = se < 0.0 ? 0.0 : (se > 1.0 ? 1.0 : se);
    const double lw = pow(se, F.n_w) * F.inv_mu_w, ln = pow(1.0 - se, F.n_n) * F.inv_mu_n;
    const double tot = lw + ln;
    // d lw / d se = n_w lw / se, d ln / d se = -n_n ln / (1 - se): no second pair of powers
    *df = inside ? (F.n_w * lw / se * ln + lw * F.n_n * ln / (1.0 - se)) / (tot * tot) * F.inv_span : 0.0;
    return lw / tot;
  }
  if (F.kind == PFV_FLUXFN_TABLE) {
    const double sc = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    const double x = sc * (double)(F.m - 1);
    int k = (int)x;
    if (k > F.m - 2) k = F.m - 2;
    const double t0 = F.table[k], d = F.table[k + 1] - t0;
    *df = (s >= 0.0 && s <= 1.0) ? d * (double)(F.m - 1) : 0.0;
    return t0 + (x - (double)k) * d;
  }
  *df = 1.0;
  return s;
}

// The derivatives of f(s) with respect to the six Corey parameters, out[0 .. 6) in the order s_wr, s_nr, n_w, n_n, mu_w,
// mu_n (pfv_transport_adjoint_nl: grad_fluxfn).  With lw = se^n_w / mu_w, ln = (1 - se)^n_n / mu_n, tot = lw + ln:
// df/dlw = ln / tot^2, df/dln = -lw / tot^2; the exponents enter through lw log se and ln log(1 - se), the viscosities
// through -lw / mu_w and -ln / mu_n, the residual saturations through se with df/dse = f' / inv_span.  All six are 0
// where se lies outside (0, 1), as f' of fluxfn_eval is: the clamp holds f there, and no log 0 is evaluated.  Another
// kind has no such parameters: zeros.
PFV_FN void fluxfn_eval_params(const FluxFn& F, double s, double out[6]) {
  for (int k = 0; k < 6; ++k) out[k] = 0.0;
  if (F.kind != PFV_FLUXFN_COREY) return;
  const double se = (s - F.s_wr) * F.inv_span;
  if (!(se > 0.0 && se < 1.0)) return;
  const double lw = pow(se, F.n_w) * F.inv_mu_w, ln = pow(1.0 - se, F.n_n) * F.inv_mu_n;
  const double tot = lw + ln, inv2 = 1.0 / (tot * tot);
  const double f_lw = ln * inv2, f_ln = -lw * inv2;
  const double f_se = (F.n_w * lw / se * ln + lw * F.n_n * ln / (1.0 - se)) * inv2;
  out[0] = f_se * ((se - 1.0) * F.inv_span);
  out[1] = f_se * (se * F.inv_span);
  out[2] = f_lw * (lw * log(se));
  out[3] = f_ln * (ln * log(1.0 - se));
  out[4] = -f_lw * (lw * F.inv_mu_w);
  out[5] = -f_ln * (ln * F.inv_mu_n);
}

}  // namespace pfv
