// regularise_driver.cpp -- TEST INFRASTRUCTURE: the device-free arithmetic of the regularised resampling
// (include/mcl_regularise.h) under AddressSanitizer + UBSan with plain g++: regularise_factor_impl and
// regularise_bandwidth_impl of mcl_host_pure.h, the functions mcl_regularise_factor / mcl_regularise_bandwidth forward to
// (and, the factor, the function the device runs), driven with random, degenerate and hostile inputs.
// Exit code 0 and no sanitizer report = pass.  tests/test_regularise_host.py builds and runs it.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../smarc_navigation_amd/csrc/mcl_host_pure.h"

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

static int pk(int r, int c) { return r * (r + 1) / 2 + c; }

int main() {
  std::mt19937_64 rng(20261019);
  std::normal_distribution<double> N(0.0, 1.0);
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (int dims : {3, 6}) {
    const int np = dims * (dims + 1) / 2;
    for (int trial = 0; trial < 400; ++trial) {
      // C = A A' of a random A with rank `rank` (full, or deficient: dead columns), heap arrays of the exact size
      const int rank = trial % 4 == 0 ? 1 + trial % dims : dims + 6;   // (dims + 6 columns: far from singular)
      std::vector<double> A((size_t)dims * rank), C((size_t)np), L((size_t)np, -7.0);
      for (double& v : A) v = N(rng);
      if (trial % 7 == 3)
        for (int k = 0; k < rank; ++k) A[(size_t)(dims - 1) * rank + k] = 0.0;   // a constant dimension
      for (int r = 0; r < dims; ++r)
        for (int c = 0; c <= r; ++c) {
          double s = 0.0;
          for (int k = 0; k < rank; ++k) s += A[(size_t)r * rank + k] * A[(size_t)c * rank + k];
          C[(size_t)pk(r, c)] = s;
        }
      int32_t dead = -1;
      CHECK(regularise_factor_impl(C.data(), dims, L.data(), &dead) == MCL_OK);
      CHECK(dead >= 0 && dead < (1 << dims));
      if (rank > dims && trial % 7 != 3) CHECK(dead == 0);
      if (trial % 7 == 3) {
        CHECK(dead & (1 << (dims - 1)));
        for (int c = 0; c < dims; ++c) CHECK(L[(size_t)pk(dims - 1, c)] == 0.0);
      }
      double worst = 0.0, big = 0.0;
      for (int r = 0; r < dims; ++r)
        for (int c = 0; c <= r; ++c) {
          if (dead & (1 << c)) CHECK(L[(size_t)pk(r, c)] == 0.0);
          double s = 0.0;
          for (int k = 0; k <= c; ++k) s += L[(size_t)pk(r, k)] * L[(size_t)pk(c, k)];
          worst = std::fmax(worst, std::fabs(s - C[(size_t)pk(r, c)]));
          big = std::fmax(big, std::fabs(C[(size_t)pk(r, c)]));
        }
      // (a dead column leaves out less than 2^-26 of its variance, hence less than 2^-13 of a covariance with it)
      CHECK(worst <= 2e-4 * big);
      // in place
      std::vector<double> M(C);
      int32_t dead2 = -1;
      CHECK(regularise_factor_impl(M.data(), dims, M.data(), &dead2) == MCL_OK && dead2 == dead);
      for (int k = 0; k < np; ++k) CHECK(M[(size_t)k] == L[(size_t)k]);
    }
    // hostile values: every column is dead or finite garbage, nothing is read or written out of bounds
    for (double bad : {nan, inf, -inf, -1.0, 0.0, 1e308, 5e-324}) {
      std::vector<double> C((size_t)np, bad), L((size_t)np, -7.0);
      int32_t dead = -1;
      CHECK(regularise_factor_impl(C.data(), dims, L.data(), &dead) == MCL_OK);
      if (std::isnan(bad) || bad <= 0.0) CHECK(dead == (1 << dims) - 1);
    }
    int32_t dead = 0;
    double c1[21] = {0}, l1[21];
    CHECK(regularise_factor_impl(nullptr, dims, l1, &dead) == MCL_ERR_INVALID);
    CHECK(regularise_factor_impl(c1, dims, nullptr, &dead) == MCL_ERR_INVALID);
    CHECK(regularise_factor_impl(c1, dims, l1, nullptr) == MCL_ERR_INVALID);
    // bandwidth
    for (long long n : {1ll, 2ll, 63ll, 1000ll, 1ll << 20, (1ll << 31) - 1, 1ll << 62})
      for (double scale : {1e-3, 0.5, 1.0, 7.0, 1e6})
        for (int shrink : {0, 1}) {
          double h = -1.0, a = -1.0;
          CHECK(regularise_bandwidth_impl(n, dims, scale, shrink, &h, &a) == MCL_OK);
          CHECK(h > 0.0 && std::isfinite(h) && a >= 0.0 && a <= 1.0);
          if (shrink) CHECK(h <= 1.0 && std::fabs(a * a + h * h - 1.0) < 1e-12);
          else CHECK(a == 1.0);
        }
    double h, a;
    for (double bad : {nan, inf, -inf, -1.0, 0.0}) CHECK(regularise_bandwidth_impl(100, dims, bad, 1, &h, &a) == MCL_ERR_INVALID);
    CHECK(regularise_bandwidth_impl(0, dims, 1.0, 1, &h, &a) == MCL_ERR_INVALID);
    CHECK(regularise_bandwidth_impl(100, dims, 1.0, 1, nullptr, &a) == MCL_ERR_INVALID);
    CHECK(regularise_bandwidth_impl(100, dims, 1.0, 1, &h, nullptr) == MCL_ERR_INVALID);
  }
  for (int dims : {-1, 0, 1, 2, 4, 5, 7, 1 << 30}) {
    double c[21] = {0}, l[21], h, a;
    int32_t dead;
    CHECK(regularise_factor_impl(c, dims, l, &dead) == MCL_ERR_INVALID);
    CHECK(regularise_bandwidth_impl(100, dims, 1.0, 1, &h, &a) == MCL_ERR_INVALID);
    mcl_regularise_config cfg = {1.0, 1, dims};
    const char* why = nullptr;
    CHECK(regularise_config_check_impl(&cfg, &why) == MCL_ERR_INVALID && why);
  }
  CHECK(regularise_config_check_impl(nullptr, nullptr) == MCL_ERR_INVALID);
  std::printf("regularise_driver: ok\n");
  return 0;
}
