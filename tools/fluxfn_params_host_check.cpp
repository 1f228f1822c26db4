// Stand-alone host program for csrc/fluxfn.h: the derivatives of the Corey curve with respect to its six parameters
// (fluxfn_eval_params, what grad_fluxfn of pfv_transport_adjoint_nl sums up) and the slope f' of fluxfn_eval, against
// central differences of fluxfn_eval over a grid of s and several parameter sets.  Build it with the address and
// undefined-behaviour sanitizers and run it:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/fluxfn_params_host_check.cpp -o check
// (tests/test_saturation_adjoint_emulation.py does).  Exit status 0 and the line "fluxfn params host check: ok" when
// everything holds; the line before it holds the largest deviation seen per derivative.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../porepy_amd/csrc/fluxfn.h"

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static double f_of(const std::vector<double>& p, double s) {
  double df;
  return pfv::fluxfn_eval(pfv::fluxfn_make(PFV_FLUXFN_COREY, p.data(), 6, nullptr), s, &df);
}

int main() {
  const std::vector<std::vector<double>> sets = {{0.1, 0.15, 2.0, 2.0, 1.0, 5.0}, {0.0, 0.0, 3.0, 1.5, 1.0, 1.0},
                                                 {0.2, 0.0, 0.5, 0.5, 2.0, 1.0},  {0.0, 0.3, 1.0, 4.0, 1.0, 10.0},
                                                 {0.05, 0.25, 2.5, 3.5, 0.4, 3.0}};
  const double h = 1e-6;
  double worst[7] = {0, 0, 0, 0, 0, 0, 0};  // the six parameters, then f'
  for (const std::vector<double>& p : sets) {
    CHECK(pfv::fluxfn_check(PFV_FLUXFN_COREY, p.data(), 6).empty());
    const pfv::FluxFn F = pfv::fluxfn_make(PFV_FLUXFN_COREY, p.data(), 6, nullptr);
    const double lo = p[0], hi = 1.0 - p[1];
    for (int k = -250; k <= 1250; ++k) {
      const double s = k / 1000.0;
      double out[6], df;
      pfv::fluxfn_eval_params(F, s, out);
      pfv::fluxfn_eval(F, s, &df);
      for (int m = 0; m < 6; ++m) CHECK(out[m] == out[m]);  // (no NaN anywhere: no log 0, no 0 / 0)
      if (!(s > lo && s < hi)) {  // on and beyond the residual saturations: the clamp of fluxfn_eval
        for (int m = 0; m < 6; ++m) CHECK(out[m] == 0.0);
        CHECK(df == 0.0);
        continue;
      }
      // signs: more residual water or a larger water exponent or viscosity lowers f, the other three raise it
      CHECK(out[0] <= 0.0 && out[1] >= 0.0 && out[2] <= 0.0 && out[3] >= 0.0 && out[4] <= 0.0 && out[5] >= 0.0);
      if (!(s > lo + 0.02 && s < hi - 0.02)) continue;  // (the differences stay away from the kinks)
      for (int m = 0; m < 6; ++m) {
        std::vector<double> a = p, b = p;
        a[m] += h;
        b[m] -= h;
        const double num = (f_of(a, s) - f_of(b, s)) / (2 * h);
        const double dev = std::fabs(num - out[m]) / (1.0 + std::fabs(out[m]));
        worst[m] = std::max(worst[m], dev);
        CHECK(dev <= 1e-6);
      }
      const double num = (f_of(p, s + h) - f_of(p, s - h)) / (2 * h);
      const double dev = std::fabs(num - df) / (1.0 + std::fabs(df));
      worst[6] = std::max(worst[6], dev);
      CHECK(dev <= 1e-6);
    }
  }
  // another kind has no such parameters
  double out[6] = {1, 1, 1, 1, 1, 1};
  pfv::fluxfn_eval_params(pfv::fluxfn_make(PFV_FLUXFN_LINEAR, nullptr, 0, nullptr), 0.3, out);
  for (int m = 0; m < 6; ++m) CHECK(out[m] == 0.0);
  std::printf("largest deviation from central differences (h = %g), relative to 1 + |derivative|: s_wr %.1e, s_nr %.1e, "
              "n_w %.1e, n_n %.1e, mu_w %.1e, mu_n %.1e, f' %.1e\n",
              h, worst[0], worst[1], worst[2], worst[3], worst[4], worst[5], worst[6]);
  if (failures) {
    std::printf("fluxfn params host check: %d failures\n", failures);
    return 1;
  }
  std::printf("fluxfn params host check: ok\n");
  return 0;
}
