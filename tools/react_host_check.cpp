// Stand-alone host program for csrc/react.h: the check of the rate matrix and the mobilities of
// pfv_transport_advance_react.  Build it with the address and undefined-behaviour sanitizers and run it:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/react_host_check.cpp -o check
// (tests/test_react_emulation.py does).  Exit status 0 and the line "react host check: ok" when everything holds.
#include <cstdio>
#include <limits>
#include <vector>

#include "../porepy_amd/csrc/react.h"

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

// the arrays are heap blocks of exactly k * k and k values: a read past them is the sanitizer's to find
static std::string check(int k, const std::vector<double>& K, const std::vector<double>& w) {
  return pfv::react_check(k, K.empty() ? nullptr : K.data(), w.empty() ? nullptr : w.data());
}

static bool refused(int k, const std::vector<double>& K, const std::vector<double>& w, const char* needle) {
  const std::string m = check(k, K, w);
  if (m.empty() || m.find(needle) == std::string::npos) std::printf("  got: \"%s\"\n", m.c_str());
  return !m.empty() && m.find(needle) != std::string::npos;
}

// the chain 0 -> 1 -> ... -> k - 1, the last member stable
static std::vector<double> chain(int k) {
  std::vector<double> K((size_t)k * k, 0.0);
  for (int a = 0; a + 1 < k; ++a) {
    K[(size_t)a * k + a] = 0.5 + 0.1 * a;
    K[(size_t)(a + 1) * k + a] = -(0.5 + 0.1 * a);
  }
  return K;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (int k = 1; k <= pfv::kReactMax; ++k) {
    const std::vector<double> K = chain(k);
    CHECK(check(k, K, {}).empty());
    CHECK(check(k, K, std::vector<double>((size_t)k, 0.0)).empty());
    CHECK(check(k, std::vector<double>((size_t)k * k, 0.0), std::vector<double>((size_t)k, 2.0)).empty());
    const pfv::ReactPar P = pfv::react_make(k, K.data(), nullptr);
    for (int a = 0; a < pfv::kReactMax; ++a) CHECK(P.w[a] == 1.0);
    for (int m = 0; m < pfv::kReactMax * pfv::kReactMax; ++m) CHECK(P.K[m] == (m < k * k ? K[(size_t)m] : 0.0));
    std::vector<double> w((size_t)k, 0.25);
    w[(size_t)k - 1] = 0.0;
    const pfv::ReactPar Q = pfv::react_make(k, K.data(), w.data());
    for (int a = 0; a < pfv::kReactMax; ++a) CHECK(Q.w[a] == (a < k - 1 ? 0.25 : (a == k - 1 ? 0.0 : 1.0)));
  }
  CHECK(refused(0, {}, {}, "k = 0"));
  CHECK(refused(9, std::vector<double>(81, 0.0), {}, "k = 9"));
  CHECK(refused(-3, {}, {}, "k = -3"));
  CHECK(refused(2, {}, {}, "rate is required"));
  CHECK(refused(2, {-1.0, 0.0, 0.0, 1.0}, {}, "rate[0][0] is negative"));
  CHECK(refused(2, {1.0, 0.0, 0.0, -1e-300}, {}, "rate[1][1] is negative"));
  CHECK(refused(2, {1.0, 0.5, 0.0, 1.0}, {}, "rate[0][1] is positive"));
  CHECK(refused(3, {1, 0, 0, 0, 1, 0, 0, nan, 1}, {}, "rate[2][1] is not finite"));
  CHECK(refused(3, {1, 0, 0, 0, inf, 0, 0, nan, 1}, {}, "rate[1][1] is not finite"));
  CHECK(refused(3, {1, 0, -inf, 0, -1, 0, 0, 0, 1}, {}, "rate[0][2] is not finite"));  // (the first offender, row-major)
  CHECK(refused(2, {1.0, 0.0, -1.5, 1.0}, {}, "column 0 of rate has a negative sum"));
  CHECK(refused(2, {1.0, -1.0 - 1e-12, -1.0, 1.0}, {}, "column 1 of rate has a negative sum"));
  // zero column sums up to rounding are accepted: 0.1 + 0.2 against -0.1 and -0.2 sums to 5.6e-17, and its mirror
  // image -(0.1 + 0.2) + 0.1 + 0.2 to -5.6e-17 when the sum runs the other way
  CHECK(check(3, {0.1 + 0.2, 0, 0, -0.1, 0, 0, -0.2, 0, 0}, {}).empty());
  {
    const double d = 0.1 + 0.7, below = std::nextafter(d, 0.0);
    CHECK(check(3, {below, 0, 0, -0.1, 0, 0, -0.7, 0, 0}, {}).empty());  // (one ulp short: within k 2^-52 sum |K|)
    CHECK(refused(3, {d - 1e-14, 0, 0, -0.1, 0, 0, -0.7, 0, 0}, {}, "column 0"));
  }
  CHECK(refused(2, {1, 0, 0, 1}, {1.0, -0.5}, "mobility[1] is negative"));
  CHECK(refused(2, {1, 0, 0, 1}, {nan, -0.5}, "mobility[0] is not finite"));
  CHECK(refused(2, {1, 0, 0, 1}, {1.0, inf}, "mobility[1] is not finite"));
  CHECK(refused(2, {-1, 0, 0, 1}, {1.0, -1.0}, "rate[0][0]"));  // (the matrix before the mobilities)
  if (failures) {
    std::printf("react host check: %d failures\n", failures);
    return 1;
  }
  std::printf("react host check: ok\n");
  return 0;
}
