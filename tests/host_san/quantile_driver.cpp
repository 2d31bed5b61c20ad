// quantile_driver.cpp -- TEST INFRASTRUCTURE: the device-free arithmetic of the exact order statistics
// (include/mcl_quantile.h) under AddressSanitizer + UBSan with plain g++: quantile_key_impl / quantile_value_impl /
// quantile_threshold_impl / quantile_reached_impl of mcl_host_pure.h, the functions the four device-free entry points
// forward to, and quant_start / quant_pick_bin, the rules the shard search (and, quant_start, the plan kernel) runs, driven
// with random, degenerate and hostile inputs.
// Exit code 0 and no sanitizer report = pass.  tests/test_quantile_host.py builds and runs it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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

static double from_bits(uint64_t b) {
  double v;
  std::memcpy(&v, &b, sizeof v);
  return v;
}

int main() {
  std::mt19937_64 rng(20261019);
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // keys: the order of the doubles, -0 and +0 one key, every value comes back
  std::vector<double> vals = {0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, 1e300, -1e300, inf, -inf,
                              std::numeric_limits<double>::max(), std::numeric_limits<double>::lowest(),
                              std::numeric_limits<double>::min(), -std::numeric_limits<double>::min()};
  for (int k = 0; k < 4000; ++k) {
    const double v = from_bits(rng());
    if (!std::isnan(v)) vals.push_back(v);
  }
  std::sort(vals.begin(), vals.end());
  uint64_t prev = 0;
  for (size_t i = 0; i < vals.size(); ++i) {
    uint64_t k = 0;
    double back = nan;
    CHECK(quantile_key_impl(vals[i], &k) == MCL_OK);
    CHECK(quantile_value_impl(k, &back) == MCL_OK);
    CHECK(back == vals[i] && !(vals[i] == 0.0 && std::signbit(back)));
    if (i > 0) CHECK(vals[i] == vals[i - 1] ? k == prev : k > prev);
    prev = k;
  }
  uint64_t k0 = 1, k1 = 2;
  CHECK(quantile_key_impl(0.0, &k0) == MCL_OK && quantile_key_impl(-0.0, &k1) == MCL_OK && k0 == k1);
  CHECK(quantile_key_impl(nan, &k0) == MCL_ERR_INVALID && quantile_key_impl(1.0, nullptr) == MCL_ERR_INVALID);
  double d = 0.0;
  CHECK(quantile_value_impl(1, nullptr) == MCL_ERR_INVALID);
  for (uint64_t k : {(uint64_t)0, (uint64_t)1, ~(uint64_t)0}) CHECK(quantile_value_impl(k, &d) == MCL_OK && std::isnan(d));
  // thresholds
  uint64_t P = 0;
  CHECK(quantile_threshold_impl(1.0 / 4294967296.0, &P) == MCL_OK && P == 1);
  CHECK(quantile_threshold_impl(0.5, &P) == MCL_OK && P == (1ull << 31));
  CHECK(quantile_threshold_impl(1.0, &P) == MCL_OK && P == (1ull << 32));
  for (double bad : {nan, inf, -inf, 0.0, -1.0, std::nextafter(1.0 / 4294967296.0, 0.0), std::nextafter(1.0, 2.0), 1e300})
    CHECK(quantile_threshold_impl(bad, &P) == MCL_ERR_INVALID);
  CHECK(quantile_threshold_impl(0.5, nullptr) == MCL_ERR_INVALID);
  for (int k = 0; k < 2000; ++k) {
    const double p = std::ldexp((double)(rng() >> 11), -53);
    if (p < 1.0 / 4294967296.0) continue;
    CHECK(quantile_threshold_impl(p, &P) == MCL_OK && P >= 1 && P <= (1ull << 32) && (double)P <= p * 4294967296.0 &&
          (double)(P + 1) > p * 4294967296.0);
  }
  // the predicate against a 128-bit restatement that divides instead of shifting, extremes included
  typedef unsigned __int128 u128;
  int32_t r = -1;
  CHECK(quantile_reached_impl(1, 1, 1, nullptr) == MCL_ERR_INVALID);
  const uint64_t top = ~(uint64_t)0;
  CHECK(quantile_reached_impl(top, top, top, &r) == MCL_OK && r == 0);
  CHECK(quantile_reached_impl(top, top, 1ull << 32, &r) == MCL_OK && r == 1);
  CHECK(quantile_reached_impl(top, top, (1ull << 32) + 1, &r) == MCL_OK && r == 0);
  CHECK(quantile_reached_impl(0, 0, top, &r) == MCL_OK && r == 1);
  for (int k = 0; k < 20000; ++k) {
    const uint64_t mass = rng() >> (rng() % 64), total = rng() >> (rng() % 64), Pk = rng() >> (rng() % 64);
    const u128 rhs = (u128)Pk * total;
    const u128 need = (rhs >> 32) + ((rhs & 0xffffffffull) ? 1 : 0);   // ceil(P total / 2^32)
    CHECK(quantile_reached_impl(mass, total, Pk, &r) == MCL_OK && r == ((u128)mass >= need ? 1 : 0));
  }
  // where the select starts: the shared leading bytes, never past the last round
  for (int k = 0; k < 20000; ++k) {
    uint64_t a = rng(), b = rng();
    const int share = (int)(rng() % 9);   // leading bytes forced equal
    if (share == 8) b = a;
    else if (share > 0) b = (a & ~(~(uint64_t)0 >> (8 * share))) | (b >> (8 * share));
    const uint64_t lo = std::min(a, b), hi = std::max(a, b);
    const QuantStart s = quant_start(lo, hi);
    CHECK(s.start >= 0 && s.start <= QUANT_ROUNDS - 1 && s.start >= std::min(share, QUANT_ROUNDS - 1));
    if (s.start > 0) CHECK(s.prefix == lo >> (64 - 8 * s.start) && s.prefix == hi >> (64 - 8 * s.start));
    else CHECK(s.prefix == 0);
    if (s.start < QUANT_ROUNDS - 1) CHECK((lo >> (56 - 8 * s.start)) != (hi >> (56 - 8 * s.start)));
  }
  const QuantStart none = quant_start(~(uint64_t)0, 0);
  CHECK(none.start == QUANT_ROUNDS - 1 && none.prefix == 0);
  // the bin of a round: heap histograms of the exact size, the first bin that reaches
  for (int k = 0; k < 2000; ++k) {
    std::vector<uint64_t> hist(256, 0);
    const int filled = 1 + (int)(rng() % 256);
    uint64_t in_row = 0;
    for (int f = 0; f < filled; ++f) {
      const uint64_t q = rng() >> (16 + rng() % 48);   // (256 of them stay below 2^56)
      hist[rng() % 256] += q;
      in_row += q;
    }
    const uint64_t below = rng() >> 9, above = rng() >> 9, total = below + in_row + above;
    const uint64_t Pk = 1 + rng() % (1ull << 32);
    uint64_t cum = 0;
    const int dbin = quant_pick_bin(hist.data(), below, total, Pk, &cum);
    uint64_t c = below;
    int want = -1;
    for (int b = 0; b < 256 && want < 0; ++b) {
      c += hist[b];
      if (((u128)c << 32) >= (u128)Pk * total) want = b;
    }
    CHECK(dbin == want && (dbin < 0 || cum == c));
  }
  std::vector<uint64_t> zero(256, 0);
  uint64_t cum = 7;
  CHECK(quant_pick_bin(zero.data(), 0, 0, 1, &cum) == -1);
  // queries
  mcl_quantile_query q = {MCL_Q_RADIUS2, 1, {1.0, 2.0, 3.0}};
  CHECK(quantile_query_why(&q) == nullptr && quantile_query_why(nullptr) != nullptr);
  for (int bad : {-1, 5, 1 << 30}) {
    q.quantity = bad;
    CHECK(quantile_query_why(&q) != nullptr);
  }
  q.quantity = MCL_Q_X;
  for (double bad : {nan, inf, -inf})
    for (int c = 0; c < 3; ++c) {
      mcl_quantile_query b = q;
      b.centre[c] = bad;
      CHECK(quantile_query_why(&b) != nullptr);
    }
  std::printf("quantile_driver: ok\n");
  return 0;
}
