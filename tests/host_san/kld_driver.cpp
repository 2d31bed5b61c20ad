// kld_driver.cpp -- TEST INFRASTRUCTURE: the device-free arithmetic of KLD-sampling (include/mcl_kld.h) under
// AddressSanitizer + UBSan with plain g++: kld_bound_impl, kld_grid_check_impl, kld_transfer_u53 and kld_bitmap_words of
// csrc/mcl_kld_pure.h, the functions the device-free entry points forward to, driven with the issue's anchors, random,
// degenerate and hostile inputs.  Exit code 0 and no sanitizer report = pass.  tests/test_kld_host.py builds and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "../../smarc_navigation_amd/csrc/mcl_kld_pure.h"

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

static mcl_mode_grid grid(double cell, int nx, int ny, int n_yaw) {
  mcl_mode_grid g;
  std::memset(&g, 0, sizeof g);
  g.x0 = -3.0;
  g.y0 = 7.0;
  g.cell = cell;
  g.nx = nx;
  g.ny = ny;
  g.n_yaw = n_yaw;
  return g;
}

int main() {
  const double Z = 2.3263478740408408, inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  const int64_t TOP = (int64_t)1 << 31;
  int64_t n = -7;
  // ---- the anchors of include/mcl_kld.h's definition
  const int64_t ks[8] = {2, 3, 10, 30, 100, 1000, 10000, 100000};
  const int64_t a05[8] = {66, 93, 217, 497, 1347, 11060, 103310, 1010424};
  const int64_t a01[8] = {330, 462, 1085, 2481, 6733, 55297, 516546, 5052116};
  for (int i = 0; i < 8; ++i) {
    CHECK(kld_bound_impl(ks[i], 0.05, Z, 1, TOP, &n) == MCL_OK && n == a05[i]);
    CHECK(kld_bound_impl(ks[i], 0.01, Z, 1, TOP, &n) == MCL_OK && n == a01[i]);
  }
  // ---- k <= 1, the clamps, a v that is not finite
  CHECK(kld_bound_impl(0, 0.05, Z, 5, 9, &n) == MCL_OK && n == 5);
  CHECK(kld_bound_impl(1, 0.05, Z, 5, 9, &n) == MCL_OK && n == 5);
  CHECK(kld_bound_impl(2, 0.05, Z, 100, 200, &n) == MCL_OK && n == 100);
  CHECK(kld_bound_impl(1000, 0.05, Z, 1, 200, &n) == MCL_OK && n == 200);
  CHECK(kld_bound_impl(std::numeric_limits<int64_t>::max(), 1e-300, 1e300, 1, TOP, &n) == MCL_OK && n == TOP);
  CHECK(kld_bound_impl(2, 5e-324, Z, 1, 77, &n) == MCL_OK && n == 77);
  CHECK(kld_bound_impl(2, 0.05, 0.0, 1, TOP, &n) == MCL_OK && n >= 1);
  // ---- every refused argument
  n = -7;
  CHECK(kld_bound_impl(2, 0.05, Z, 1, TOP, nullptr) == MCL_ERR_INVALID);
  CHECK(kld_bound_impl(-1, 0.05, Z, 1, TOP, &n) == MCL_ERR_INVALID);
  for (double e : {0.0, -0.05, inf, -inf, nan}) CHECK(kld_bound_impl(2, e, Z, 1, TOP, &n) == MCL_ERR_INVALID);
  for (double z : {-1e-300, -1.0, inf, -inf, nan}) CHECK(kld_bound_impl(2, 0.05, z, 1, TOP, &n) == MCL_ERR_INVALID);
  CHECK(kld_bound_impl(2, 0.05, Z, 0, TOP, &n) == MCL_ERR_INVALID);
  CHECK(kld_bound_impl(2, 0.05, Z, 9, 8, &n) == MCL_ERR_INVALID);
  CHECK(kld_bound_impl(2, 0.05, Z, 1, TOP + 1, &n) == MCL_ERR_INVALID);
  CHECK(kld_bound_impl(2, 0.05, Z, std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max(), &n) == MCL_ERR_INVALID);
  CHECK(n == -7);
  // ---- random sweep: inside the clamps, monotone in k
  std::mt19937_64 rng(12345);
  for (int it = 0; it < 20000; ++it) {
    const int64_t k = (int64_t)(rng() >> (1 + rng() % 63));
    const double eps = std::ldexp(1.0, -(int)(rng() % 40));
    const int64_t lo = 1 + (int64_t)(rng() % 1000), hi = lo + (int64_t)(rng() % (uint64_t)(TOP - lo + 1));
    int64_t a = 0, b = 0;
    CHECK(kld_bound_impl(k, eps, Z, lo, hi, &a) == MCL_OK && a >= lo && a <= hi);
    if (k < std::numeric_limits<int64_t>::max()) {
      CHECK(kld_bound_impl(k + 1, eps, Z, lo, hi, &b) == MCL_OK && b >= a);
    }
  }
  // ---- the lattice check at its limits
  int64_t cells = -1;
  const char* why = nullptr;
  mcl_mode_grid g = grid(0.5, 1 << 12, 1 << 12, 8);
  CHECK(kld_grid_check_impl(&g, &cells, &why) == MCL_OK && cells == ((int64_t)1 << 27) && why == nullptr);
  CHECK(kld_grid_check_impl(&g, nullptr, nullptr) == MCL_OK);
  g = grid(0.5, (1 << 12) + 1, 1 << 12, 8);
  CHECK(kld_grid_check_impl(&g, &cells, &why) == MCL_ERR_INVALID && why != nullptr);
  g = grid(0.5, (1 << 27) + 1, 1, 1);
  CHECK(kld_grid_check_impl(&g, &cells, &why) == MCL_ERR_INVALID);
  g = grid(0.5, 1 << 27, 1, 1);
  CHECK(kld_grid_check_impl(&g, &cells, &why) == MCL_OK && cells == ((int64_t)1 << 27));
  g = grid(0.5, 0x7fffffff, 0x7fffffff, 1024);   // (no product overflows)
  CHECK(kld_grid_check_impl(&g, &cells, &why) == MCL_ERR_INVALID);
  g = grid(0.5, 4, 4, 1024);
  CHECK(kld_grid_check_impl(&g, &cells, &why) == MCL_OK && cells == 16 * 1024);
  g = grid(0.5, 4, 4, 1025);
  CHECK(kld_grid_check_impl(&g, &cells, &why) == MCL_ERR_INVALID);
  for (double c : {0.0, -1.0, inf, nan}) {
    g = grid(c, 4, 4, 4);
    CHECK(kld_grid_check_impl(&g, &cells, &why) == MCL_ERR_INVALID);
  }
  g = grid(0.5, 4, 4, 4);
  g.x0 = nan;
  CHECK(kld_grid_check_impl(&g, &cells, &why) == MCL_ERR_INVALID);
  g = grid(0.5, 4, 4, 4);
  g.y0 = inf;
  CHECK(kld_grid_check_impl(&g, &cells, &why) == MCL_ERR_INVALID);
  for (int bad = 0; bad < 3; ++bad) {
    g = grid(0.5, bad == 0 ? 0 : 4, bad == 1 ? -1 : 4, bad == 2 ? 0 : 4);
    CHECK(kld_grid_check_impl(&g, &cells, &why) == MCL_ERR_INVALID);
  }
  CHECK(kld_grid_check_impl(nullptr, &cells, &why) == MCL_ERR_INVALID && why != nullptr);
  // ---- the bitmap's size: a whole number of 16-byte vectors that covers every cell
  for (int64_t c : {(int64_t)1, (int64_t)31, (int64_t)32, (int64_t)33, (int64_t)127, (int64_t)128, (int64_t)129, (int64_t)1 << 27}) {
    const int64_t w = kld_bitmap_words(c);
    CHECK(w % 4 == 0 && w * 32 >= c && (w - 4) * 32 < c);
  }
  // ---- the uniform
  uint64_t u = 1;
  double x = 0.0;
  CHECK(kld_transfer_u53(&x, 1, 0, &u) && u == 0);
  x = 1.0 - std::ldexp(1.0, -53);
  CHECK(kld_transfer_u53(&x, 1, 0, &u) && u == ((uint64_t)1 << 53) - 1);
  for (double bad : {1.0, -1e-300, 2.0, inf, -inf, nan}) {
    u = 99;
    CHECK(!kld_transfer_u53(&bad, 1, 0, &u) && u == 99);
  }
  uint64_t a = 0, b = 0, c = 0;
  CHECK(kld_transfer_u53(nullptr, 42, 0, &a) && kld_transfer_u53(nullptr, 42, 1, &b) && kld_transfer_u53(nullptr, 43, 0, &c));
  CHECK(a < ((uint64_t)1 << 53) && b < ((uint64_t)1 << 53) && a != b && a != c);
  CHECK(native_u53_purpose(42, 0, 3) == native_u53(42, 0) && native_u53_purpose(42, 0, KLD_TRANSFER_PURPOSE) == a && a != native_u53(42, 0));
  std::printf("kld_driver: ok\n");
  return 0;
}
