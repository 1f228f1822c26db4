// Stand-alone host program for csrc/fluxfn.h: the parameter check of pfv_transport_advance_nl and the host-side
// evaluation of the flux functions.  Build it with the address and undefined-behaviour sanitizers and run it:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/fluxfn_host_check.cpp -o check
// (tests/test_saturation_emulation.py does).  Exit status 0 and the line "fluxfn host check: ok" when everything holds.
#include <cstdio>
#include <limits>
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

static bool refused(int kind, const std::vector<double>& p, const char* needle) {
  const std::string m = pfv::fluxfn_check(kind, p.empty() ? nullptr : p.data(), (int)p.size());
  return !m.empty() && m.find(needle) != std::string::npos;
}

// f nondecreasing on a fine grid that reaches beyond [0, 1]; df the slope of f inside (lo, hi), away from the kinks at
// the residual saturations (lo >= hi: not checked)
static void curve(const pfv::FluxFn& F, double lo, double hi) {
  double df, prev = pfv::fluxfn_eval(F, -0.25, &df);
  CHECK(df == 0.0);
  for (int k = -250; k <= 1250; ++k) {
    const double s = k / 1000.0, f = pfv::fluxfn_eval(F, s, &df);
    CHECK(f >= prev && df >= 0.0 && f == f);
    prev = f;
    if (s > lo + 0.02 && s < hi - 0.02) {
      const double h = 1e-6;
      double t;
      const double num = (pfv::fluxfn_eval(F, s + h, &t) - pfv::fluxfn_eval(F, s - h, &t)) / (2 * h);
      CHECK(std::fabs(num - df) <= 1e-4 * (1.0 + std::fabs(df)));
    }
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<double> corey = {0.1, 0.15, 2.0, 2.0, 1.0, 5.0};
  CHECK(pfv::fluxfn_check(PFV_FLUXFN_LINEAR, nullptr, 0).empty());
  CHECK(pfv::fluxfn_check(PFV_FLUXFN_COREY, corey.data(), 6).empty());
  CHECK(refused(PFV_FLUXFN_LINEAR, {1.0}, "n_params = 1"));
  CHECK(refused(7, {}, "unknown flux function kind 7"));
  CHECK(refused(-1, {}, "unknown flux function kind -1"));
  CHECK(refused(PFV_FLUXFN_COREY, {0.1, 0.15, 2.0, 2.0, 1.0}, "n_params = 5"));
  CHECK(refused(PFV_FLUXFN_COREY, {}, "n_params = 0"));
  CHECK(refused(PFV_FLUXFN_COREY, {-0.1, 0.15, 2, 2, 1, 5}, "s_wr (index 0)"));
  CHECK(refused(PFV_FLUXFN_COREY, {0.1, -0.15, 2, 2, 1, 5}, "s_nr (index 1)"));
  CHECK(refused(PFV_FLUXFN_COREY, {0.5, 0.5, 2, 2, 1, 5}, "s_wr + s_nr"));
  CHECK(refused(PFV_FLUXFN_COREY, {0.1, 0.15, 0, 2, 1, 5}, "n_w (index 2)"));
  CHECK(refused(PFV_FLUXFN_COREY, {0.1, 0.15, 2, -1, 1, 5}, "n_n (index 3)"));
  CHECK(refused(PFV_FLUXFN_COREY, {0.1, 0.15, 2, 2, 0, 5}, "mu_w (index 4)"));
  CHECK(refused(PFV_FLUXFN_COREY, {0.1, 0.15, 2, 2, 1, nan}, "mu_n (index 5)"));
  CHECK(refused(PFV_FLUXFN_COREY, {0.1, inf, 2, 2, 1, 5}, "s_nr (index 1)"));
  CHECK(refused(PFV_FLUXFN_TABLE, {0.5}, "n_params = 1)"));
  CHECK(refused(PFV_FLUXFN_TABLE, std::vector<double>(1025, 0.5), "n_params = 1025"));
  CHECK(refused(PFV_FLUXFN_TABLE, {0.0, 0.2, 0.5, 0.4, 1.0}, "decreases at value 3"));
  CHECK(refused(PFV_FLUXFN_TABLE, {0.0, 0.2, inf, 1.0}, "value 2 is not finite"));
  CHECK(refused(PFV_FLUXFN_TABLE, {nan, 0.2}, "value 0 is not finite"));
  CHECK(pfv::fluxfn_check(PFV_FLUXFN_TABLE, std::vector<double>(1024, 0.5).data(), 1024).empty());

  double df;
  const pfv::FluxFn lin = pfv::fluxfn_make(PFV_FLUXFN_LINEAR, nullptr, 0, nullptr);
  CHECK(pfv::fluxfn_eval(lin, 0.3, &df) == 0.3 && df == 1.0);

  const pfv::FluxFn C = pfv::fluxfn_make(PFV_FLUXFN_COREY, corey.data(), 6, nullptr);
  CHECK(pfv::fluxfn_eval(C, 0.0, &df) == 0.0 && df == 0.0);
  CHECK(pfv::fluxfn_eval(C, 0.1, &df) == 0.0);
  CHECK(pfv::fluxfn_eval(C, 0.85, &df) == 1.0);
  CHECK(pfv::fluxfn_eval(C, 1.0, &df) == 1.0 && df == 0.0);
  {  // s_e = 0.5: l_w = 0.25, l_n = 0.05
    const double f = pfv::fluxfn_eval(C, 0.1 + 0.5 * 0.75, &df);
    CHECK(std::fabs(f - 0.25 / 0.30) <= 1e-15);
  }
  curve(C, 0.1, 0.85);
  for (const std::vector<double>& p : {std::vector<double>{0, 0, 3.0, 1.5, 1, 1}, std::vector<double>{0.2, 0.0, 0.5, 0.5, 2, 1},
                                       std::vector<double>{0.0, 0.3, 1.0, 4.0, 1, 10}}) {
    CHECK(pfv::fluxfn_check(PFV_FLUXFN_COREY, p.data(), 6).empty());
    curve(pfv::fluxfn_make(PFV_FLUXFN_COREY, p.data(), 6, nullptr), p[0], 1.0 - p[1]);
  }

  // tables: the two shortest, the longest, and every knot and interval end of a 9-knot one (an index past the last
  // interval would read beyond the heap block)
  for (int m : {2, 3, 9, 1024}) {
    std::vector<double> v((size_t)m);
    for (int k = 0; k < m; ++k) v[(size_t)k] = (double)k * k / ((double)(m - 1) * (m - 1));
    CHECK(pfv::fluxfn_check(PFV_FLUXFN_TABLE, v.data(), m).empty());
    const pfv::FluxFn T = pfv::fluxfn_make(PFV_FLUXFN_TABLE, v.data(), m, v.data());
    curve(T, 0.0, 0.0);
    for (int k = 0; k < m; ++k) {
      const double f = pfv::fluxfn_eval(T, (double)k / (m - 1), &df);
      CHECK(std::fabs(f - v[(size_t)k]) <= 1e-15);
    }
    CHECK(pfv::fluxfn_eval(T, 1.0, &df) == 1.0);
    CHECK(pfv::fluxfn_eval(T, std::nextafter(1.0, 0.0), &df) <= 1.0);
    CHECK(pfv::fluxfn_eval(T, 2.0, &df) == 1.0 && df == 0.0);
    CHECK(pfv::fluxfn_eval(T, -1.0, &df) == 0.0 && df == 0.0);
  }
  if (failures) {
    std::printf("fluxfn host check: %d failures\n", failures);
    return 1;
  }
  std::printf("fluxfn host check: ok\n");
  return 0;
}
