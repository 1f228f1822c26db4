// Stand-alone host program for csrc/isotherm.h: the parameter check of pfv_transport_advance_sorb and the host-side
// evaluation of the isotherms, against closed forms at the edges.  Build it with the address and undefined-behaviour
// sanitizers and run it:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/isotherm_host_check.cpp -o check
// (tests/test_sorb_emulation.py does).  Exit status 0 and the line "isotherm host check: ok" when everything holds.
#include <cstdio>
#include <limits>

#include "../porepy_amd/csrc/isotherm.h"

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static bool refused(int kind, double p0, double p1, const char* needle) {
  const std::string m = pfv::isotherm_check(kind, p0, p1);
  return !m.empty() && m.find(needle) != std::string::npos;
}

static bool close(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fabs(b); }

// S(0) = 0, S nondecreasing with a slope >= 0 on a grid that spans twenty decades, and dS the slope of S
static void curve(const pfv::Isotherm& I) {
  double dS, prev = pfv::isotherm_eval(I, 0.0, &dS);
  CHECK(prev == 0.0 && dS >= 0.0);
  for (int k = -200; k <= 20; ++k) {
    const double c = std::pow(10.0, k / 10.0), S = pfv::isotherm_eval(I, c, &dS);
    CHECK(S >= prev && S == S && dS >= 0.0 && dS == dS);
    prev = S;
    double t;
    const double h = 1e-6 * c;
    const double num = (pfv::isotherm_eval(I, c + h, &t) - pfv::isotherm_eval(I, c - h, &t)) / (2 * h);
    CHECK(std::fabs(num - dS) <= 1e-6 * (std::fabs(dS) + 1e-300));
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double sub = std::numeric_limits<double>::denorm_min() * 1024;  // a subnormal c
  // ---- the check
  CHECK(pfv::isotherm_check(PFV_ISOTHERM_LINEAR, 0.0, nan).empty());  // (the second parameter is not read)
  CHECK(pfv::isotherm_check(PFV_ISOTHERM_LINEAR, 2.5, 0.0).empty());
  CHECK(pfv::isotherm_check(PFV_ISOTHERM_FREUNDLICH, 0.0, 0.5).empty());
  CHECK(pfv::isotherm_check(PFV_ISOTHERM_FREUNDLICH, 1.0, 1.0).empty());
  CHECK(pfv::isotherm_check(PFV_ISOTHERM_LANGMUIR, 0.0, 0.0).empty());
  CHECK(pfv::isotherm_check(PFV_ISOTHERM_LANGMUIR, 2.0, 3.0).empty());
  CHECK(refused(3, 1.0, 1.0, "unknown isotherm kind 3"));
  CHECK(refused(-1, 1.0, 1.0, "unknown isotherm kind -1"));
  CHECK(refused(PFV_ISOTHERM_LINEAR, -1.0, 0.0, "Kd (index 0) is negative"));
  CHECK(refused(PFV_ISOTHERM_LINEAR, nan, 0.0, "Kd (index 0) is not finite"));
  CHECK(refused(PFV_ISOTHERM_LINEAR, inf, 0.0, "Kd (index 0) is not finite"));
  CHECK(refused(PFV_ISOTHERM_FREUNDLICH, -1.0, 0.5, "Kf (index 0) is negative"));
  CHECK(refused(PFV_ISOTHERM_FREUNDLICH, 1.0, 0.0, "n (index 1) must be positive"));
  CHECK(refused(PFV_ISOTHERM_FREUNDLICH, 1.0, -0.5, "n (index 1) must be positive"));
  CHECK(refused(PFV_ISOTHERM_FREUNDLICH, inf, 0.5, "Kf (index 0) is not finite"));
  CHECK(refused(PFV_ISOTHERM_FREUNDLICH, 1.0, nan, "n (index 1) is not finite"));
  CHECK(refused(PFV_ISOTHERM_FREUNDLICH, nan, -1.0, "Kf (index 0) is not finite"));  // (the first offender)
  CHECK(refused(PFV_ISOTHERM_LANGMUIR, -2.0, 3.0, "q_max (index 0) is negative"));
  CHECK(refused(PFV_ISOTHERM_LANGMUIR, 2.0, -3.0, "b (index 1) is negative"));
  CHECK(refused(PFV_ISOTHERM_LANGMUIR, 2.0, inf, "b (index 1) is not finite"));
  CHECK(refused(PFV_ISOTHERM_LANGMUIR, nan, 3.0, "q_max (index 0) is not finite"));

  // ---- the evaluation at the edges
  double dS;
  const pfv::Isotherm lin = pfv::isotherm_make(PFV_ISOTHERM_LINEAR, 2.5, nan);
  CHECK(lin.p1 == 0.0);
  CHECK(pfv::isotherm_eval(lin, 0.0, &dS) == 0.0 && dS == 2.5);
  CHECK(pfv::isotherm_eval(lin, 0.3, &dS) == 2.5 * 0.3 && dS == 2.5);
  CHECK(pfv::isotherm_eval(lin, sub, &dS) == 2.5 * sub && dS == 2.5);

  const pfv::Isotherm half = pfv::isotherm_make(PFV_ISOTHERM_FREUNDLICH, 3.0, 0.5);  // n < 1
  CHECK(pfv::isotherm_eval(half, 0.0, &dS) == 0.0 && dS == inf);
  CHECK(close(pfv::isotherm_eval(half, 0.25, &dS), 1.5, 1e-15) && close(dS, 3.0, 1e-15));
  CHECK(close(pfv::isotherm_eval(half, sub, &dS), 3.0 * std::sqrt(sub), 1e-15) && dS > 0.0 && dS == dS);
  CHECK(close(dS, 1.5 / std::sqrt(sub), 1e-14));
  const pfv::Isotherm tiny = pfv::isotherm_make(PFV_ISOTHERM_FREUNDLICH, 1.0, 0.01);  // the slope overflows: +inf, no NaN
  CHECK(pfv::isotherm_eval(tiny, sub, &dS) > 0.0 && dS == inf);
  const pfv::Isotherm none = pfv::isotherm_make(PFV_ISOTHERM_FREUNDLICH, 0.0, 0.5);  // Kf = 0: no sorption at all
  CHECK(pfv::isotherm_eval(none, 0.0, &dS) == 0.0 && dS == 0.0);
  CHECK(pfv::isotherm_eval(none, 0.3, &dS) == 0.0 && dS == 0.0);

  const pfv::Isotherm one = pfv::isotherm_make(PFV_ISOTHERM_FREUNDLICH, 0.8, 1.0);  // n = 1: the linear curve
  CHECK(pfv::isotherm_eval(one, 0.0, &dS) == 0.0 && dS == 0.8);
  CHECK(close(pfv::isotherm_eval(one, 0.3, &dS), 0.8 * 0.3, 1e-15) && close(dS, 0.8, 1e-15));
  CHECK(close(pfv::isotherm_eval(one, sub, &dS), 0.8 * sub, 1e-3) && close(dS, 0.8, 1e-3));

  const pfv::Isotherm steep = pfv::isotherm_make(PFV_ISOTHERM_FREUNDLICH, 2.0, 1.5);  // n > 1
  CHECK(pfv::isotherm_eval(steep, 0.0, &dS) == 0.0 && dS == 0.0);
  CHECK(close(pfv::isotherm_eval(steep, 4.0, &dS), 16.0, 1e-15) && close(dS, 6.0, 1e-15));
  CHECK(pfv::isotherm_eval(steep, sub, &dS) == 0.0 && dS == 0.0);  // (sub^1.5 underflows)

  const pfv::Isotherm lang = pfv::isotherm_make(PFV_ISOTHERM_LANGMUIR, 2.0, 3.0);
  CHECK(pfv::isotherm_eval(lang, 0.0, &dS) == 0.0 && dS == 6.0);
  CHECK(close(pfv::isotherm_eval(lang, 1.0, &dS), 1.5, 1e-15) && close(dS, 6.0 / 16.0, 1e-15));
  CHECK(close(pfv::isotherm_eval(lang, sub, &dS), 6.0 * sub, 1e-3) && dS == 6.0);
  CHECK(close(pfv::isotherm_eval(lang, 1e300, &dS), 2.0, 1e-15) && dS >= 0.0);  // saturation
  const pfv::Isotherm flat = pfv::isotherm_make(PFV_ISOTHERM_LANGMUIR, 2.0, 0.0);  // b = 0: no sorption at all
  CHECK(pfv::isotherm_eval(flat, 0.0, &dS) == 0.0 && dS == 0.0);
  CHECK(pfv::isotherm_eval(flat, 0.7, &dS) == 0.0 && dS == 0.0);

  for (const pfv::Isotherm& I : {lin, half, one, steep, lang, pfv::isotherm_make(PFV_ISOTHERM_FREUNDLICH, 0.8, 0.7)}) curve(I);

  if (failures) {
    std::printf("isotherm host check: %d failures\n", failures);
    return 1;
  }
  std::printf("isotherm host check: ok\n");
  return 0;
}
