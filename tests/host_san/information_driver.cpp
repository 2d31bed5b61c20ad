// information_driver.cpp -- TEST INFRASTRUCTURE: the device-free arithmetic of the ping information
// (include/mcl_information.h) under AddressSanitizer + UBSan with plain g++: information_merge_impl /
// information_matrix_impl of mcl_host_pure.h, the functions the two device-free entry points forward to, and
// info_difference / info_jump_q / info_steps_why / info_legal, the rules the kernel and its launcher run, driven with
// random, degenerate and hostile inputs.
// Exit code 0 and no sanitizer report = pass.  tests/test_information_host.py builds and runs it.
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

struct Triple {
  long long x, y, w;
};

static mcl_information_sums record_of(const std::vector<Triple>& d, long long n_miss, long long n_jump) {
  mcl_information_sums r = {(int64_t)d.size() + n_miss + n_jump, n_miss, n_jump, 0, 0, 0, 0, 0, 0};
  for (const Triple& t : d) {
    r.sxx += (uint64_t)(t.x * t.x);
    r.syy += (uint64_t)(t.y * t.y);
    r.sww += (uint64_t)(t.w * t.w);
    r.sxy += t.x * t.y;
    r.sxw += t.x * t.w;
    r.syw += t.y * t.w;
  }
  return r;
}

int main() {
  std::mt19937_64 rng(20261020);
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double pi = 3.14159265358979323846;
  const long long D_MAX = 1ll << 23;   // the largest |d| of a contributing pair
  // ---- the quantised difference: exact on the grid, ties to even, the whole range without a clamp
  CHECK(info_difference(10.f, 10.f) == 0 && info_difference(10.25f, 10.f) == 1024 && info_difference(10.f, 10.25f) == -1024);
  CHECK(info_difference(4096.f, 0.f) == (1ll << 24) && info_difference(0.f, 4096.f) == -(1ll << 24));
  CHECK(info_difference(1.f + 1.f / 8192.f, 1.f) == 0 && info_difference(1.f + 3.f / 8192.f, 1.f) == 2);
  CHECK(info_jump_q(1.0) == 4096 && info_jump_q(2048.0) == D_MAX && info_jump_q(0.0003) == 1);
  // ---- the steps
  {
    mcl_information_steps s = {0.5, 0.01, 80.0};
    CHECK(info_steps_why(&s, 80.0) == nullptr && info_steps_why(nullptr, 80.0) != nullptr);
    CHECK(info_steps_why(&s, 79.0) != nullptr && info_steps_why(&s, 4096.5) != nullptr && info_steps_why(&s, 0.0) != nullptr);
    CHECK(info_steps_why(&s, nan) != nullptr);
    for (double bad : {0.0, -1.0, nan, inf}) {
      mcl_information_steps t = s;
      t.delta_xy = bad;
      CHECK(info_steps_why(&t, 80.0) != nullptr);
      t = s;
      t.delta_yaw = bad;
      CHECK(info_steps_why(&t, 80.0) != nullptr);
      t = s;
      t.jump_max = bad;
      CHECK(info_steps_why(&t, 80.0) != nullptr);
    }
    s.jump_max = 2048.0;
    CHECK(info_steps_why(&s, 4096.0) == nullptr);
    s.jump_max = 2048.5;
    CHECK(info_steps_why(&s, 4096.0) != nullptr);
  }
  const double sigma = 0.2, dxy = 0.5, dyaw = 0.01;
  mcl_information_result o;
  // ---- the edges of the matrix
  {
    const mcl_information_sums none = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(information_matrix_impl(&none, 1, 0, sigma, dxy, dyaw, &o) == MCL_OK);
    CHECK(o.rank_pos == 0 && o.crlb_strong == inf && o.crlb_weak == inf && o.hit_share == 0.0 && o.lambda_max == 0.0 && o.weak_axis == 0.0);
    // a ridge across x: only d_x, no yaw information: J_ww == 0, rank 1, the weak axis is y
    const mcl_information_sums ridge = record_of(std::vector<Triple>(100, Triple{4096, 0, 0}), 3, 2);
    CHECK(information_matrix_impl(&ridge, 1, 0, sigma, dxy, dyaw, &o) == MCL_OK);
    CHECK(o.rank_pos == 1 && o.crlb_weak == inf && o.weak_axis == pi / 2 && o.J[0] == 1.0 / (sigma * sigma) && o.J[5] == 0.0);
    CHECK(o.crlb_strong == 1.0 / std::sqrt(o.J[0]) && o.hit_share == 100.0 / 105.0);
    CHECK(information_matrix_impl(&ridge, 1, 1, sigma, dxy, dyaw, &o) == MCL_OK && o.J[0] == 100.0 / (sigma * sigma) && o.rank_pos == 1);
    // a ridge across y: the weak axis is x
    const mcl_information_sums ridge_y = record_of(std::vector<Triple>(10, Triple{0, -4096, 0}), 0, 0);
    CHECK(information_matrix_impl(&ridge_y, 1, 1, sigma, dxy, dyaw, &o) == MCL_OK && o.rank_pos == 1 && o.weak_axis == 0.0);
    // yaw explains everything: d_x = 2 d_w in every pair -- the Schur complement is rounding, the rank 0
    std::vector<Triple> tied;
    for (int k = 1; k <= 50; ++k) tied.push_back(Triple{2 * k * 37, 0, k * 37});
    const mcl_information_sums t = record_of(tied, 0, 0);
    CHECK(information_matrix_impl(&t, 1, 1, sigma, dxy, dyaw, &o) == MCL_OK && o.rank_pos == 0 && o.crlb_strong == inf && o.J[0] > 0.0);
    // full rank
    std::vector<Triple> full;
    for (int k = 0; k < 64; ++k) full.push_back(Triple{1000 + 13 * k, (k % 7) * 300 - 900, (k % 5) * 20 - 40});
    const mcl_information_sums f = record_of(full, 1, 0);
    CHECK(information_matrix_impl(&f, 1, 1, sigma, dxy, dyaw, &o) == MCL_OK && o.rank_pos == 2);
    CHECK(o.lambda_max >= o.lambda_min && o.lambda_min > 0.0 && o.crlb_weak >= o.crlb_strong && o.weak_axis >= 0.0 && o.weak_axis < pi);
    // beams with m == 0 are skipped: the result of (none, f, all-miss) is the result of f, but for the hit share
    const mcl_information_sums miss = {7, 7, 0, 0, 0, 0, 0, 0, 0};
    const mcl_information_sums three[3] = {none, f, miss};
    mcl_information_result o3;
    CHECK(information_matrix_impl(&f, 1, 0, sigma, dxy, dyaw, &o) == MCL_OK && information_matrix_impl(three, 3, 0, sigma, dxy, dyaw, &o3) == MCL_OK);
    CHECK(std::memcmp(o.J, o3.J, sizeof o.J) == 0 && o3.hit_share == 64.0 / 72.0 && o3.rank_pos == 2);
  }
  // ---- the largest legal sums: 2^15 pairs of +-2^23
  {
    std::vector<Triple> top(INFO_MAX_N, Triple{D_MAX, -D_MAX, D_MAX});
    const mcl_information_sums r = record_of(top, 0, 0);
    CHECK(r.sxx == (1ull << 61) && r.sxy == -(1ll << 61) && info_legal(r));
    CHECK(information_matrix_impl(&r, 1, 0, sigma, dxy, dyaw, &o) == MCL_OK && std::isfinite(o.J[0]) && o.rank_pos == 0);
    const mcl_information_sums one = record_of(std::vector<Triple>(1, Triple{1, 1, 1}), 0, 0);
    const mcl_information_sums two[2] = {r, one};
    mcl_information_sums out;
    CHECK(information_merge_impl(two, 2, 1, &out) == MCL_ERR_INVALID);   // one more pair cannot be added
  }
  // ---- records that are no sums are refused, by the matrix and by the merge
  {
    const mcl_information_sums bad[] = {{-1, 0, 0, 0, 0, 0, 0, 0, 0},         {INFO_MAX_N + 1, 0, 0, 0, 0, 0, 0, 0, 0},
                                        {10, 11, 0, 0, 0, 0, 0, 0, 0},        {10, 6, 5, 0, 0, 0, 0, 0, 0},
                                        {10, -1, 0, 0, 0, 0, 0, 0, 0},        {10, 0, -1, 0, 0, 0, 0, 0, 0},
                                        {10, 0, 0, (10ull << 46) + 1, 0, 0, 0, 0, 0}, {10, 5, 5, 1, 0, 0, 0, 0, 0},
                                        {10, 0, 0, 100, 100, 0, 101, 0, 0},   {10, 0, 0, 100, 0, 100, 0, -101, 0},
                                        {10, 0, 0, 0, 100, 100, 0, 0, 101},   {10, 0, 0, 0, 0, 0, 1, 0, 0},
                                        {10, 0, 0, 1, 1, 1, INT64_MIN, 0, 0}, {10, 0, 0, ~0ull, ~0ull, ~0ull, INT64_MAX, 0, 0}};
    for (const mcl_information_sums& r : bad) {
      mcl_information_sums out;
      CHECK(!info_legal(r) && information_matrix_impl(&r, 1, 0, sigma, dxy, dyaw, &o) == MCL_ERR_INVALID);
      CHECK(information_matrix_impl(&r, 1, 1, sigma, dxy, dyaw, &o) == MCL_ERR_INVALID && information_merge_impl(&r, 1, 1, &out) == MCL_ERR_INVALID);
    }
    const mcl_information_sums ok = {10, 0, 0, 100, 100, 100, 100, -100, 100};
    CHECK(info_legal(ok));
    for (double s : {0.0, -1.0, nan, inf}) {
      CHECK(information_matrix_impl(&ok, 1, 0, s, dxy, dyaw, &o) == MCL_ERR_INVALID);
      CHECK(information_matrix_impl(&ok, 1, 0, sigma, s, dyaw, &o) == MCL_ERR_INVALID);
      CHECK(information_matrix_impl(&ok, 1, 0, sigma, dxy, s, &o) == MCL_ERR_INVALID);
    }
    CHECK(information_matrix_impl(nullptr, 1, 0, sigma, dxy, dyaw, &o) == MCL_ERR_INVALID);
    CHECK(information_matrix_impl(&ok, 1, 0, sigma, dxy, dyaw, nullptr) == MCL_ERR_INVALID);
    CHECK(information_matrix_impl(&ok, 0, 0, sigma, dxy, dyaw, &o) == MCL_ERR_INVALID);
  }
  // ---- random records: J against a long-double restatement from the triples themselves, the eigenvalues against the
  // characteristic polynomial, the merge of any split against the whole; heap arrays of the exact size
  for (int k = 0; k < 300; ++k) {
    const int B = 1 + (int)(rng() % 9);
    std::vector<mcl_information_sums> recs(B), parts(2 * (size_t)B);
    long double Jxx = 0, Jxy = 0;
    for (int b = 0; b < B; ++b) {
      const int n = (int)(rng() % 500);
      const long long scale = 1ll << (rng() % 24);
      std::vector<Triple> d(n);
      for (Triple& t : d) {
        t.x = (long long)(rng() % (uint64_t)(2 * scale + 1)) - scale;
        t.y = (long long)(rng() % (uint64_t)(2 * scale + 1)) - scale;
        t.w = (long long)(rng() % (uint64_t)(2 * scale + 1)) - scale;
      }
      recs[b] = record_of(d, (long long)(rng() % 3), (long long)(rng() % 3));
      CHECK(info_legal(recs[b]));
      if (n > 0) {
        Jxx += (long double)recs[b].sxx / ((long double)n * 16777216.0L * 4.0L * dxy * dxy);
        Jxy += (long double)recs[b].sxy / ((long double)n * 16777216.0L * 4.0L * dxy * dxy);
      }
      const int cut = (int)(rng() % (uint64_t)(n + 1));
      parts[b] = record_of(std::vector<Triple>(d.begin(), d.begin() + cut), recs[b].n_miss, 0);
      parts[B + b] = record_of(std::vector<Triple>(d.begin() + cut, d.end()), 0, recs[b].n_jump);
    }
    CHECK(information_matrix_impl(recs.data(), B, 0, sigma, dxy, dyaw, &o) == MCL_OK);
    CHECK(std::fabs((long double)o.J[0] - Jxx / (sigma * sigma)) <= 1e-12L * (Jxx / (sigma * sigma)) + 1e-300L);
    CHECK(std::fabs((long double)o.J[1] - Jxy / (sigma * sigma)) <= 1e-12L * (std::fabs(Jxy) / (sigma * sigma)) + 1e-9L * (long double)o.J[0]);
    CHECK(o.lambda_max >= o.lambda_min && o.lambda_min >= 0.0 && o.weak_axis >= 0.0 && o.weak_axis < pi && o.hit_share >= 0.0 && o.hit_share <= 1.0);
    CHECK(o.rank_pos >= 0 && o.rank_pos <= 2 && (o.rank_pos == 2) == std::isfinite(o.crlb_weak) && (o.rank_pos > 0) == std::isfinite(o.crlb_strong));
    std::vector<mcl_information_result> per(B);
    CHECK(information_matrix_impl(recs.data(), B, 1, sigma, dxy, dyaw, per.data()) == MCL_OK);
    std::vector<mcl_information_sums> whole(B);
    CHECK(information_merge_impl(parts.data(), 2, B, whole.data()) == MCL_OK);
    CHECK(std::memcmp(whole.data(), recs.data(), sizeof(mcl_information_sums) * B) == 0);
  }
  {
    mcl_information_sums a = {1, 0, 0, 1, 1, 1, 1, 1, 1}, out;
    CHECK(information_merge_impl(nullptr, 1, 1, &out) == MCL_ERR_INVALID && information_merge_impl(&a, 1, 1, nullptr) == MCL_ERR_INVALID);
    CHECK(information_merge_impl(&a, 0, 1, &out) == MCL_ERR_INVALID && information_merge_impl(&a, 1, 0, &out) == MCL_ERR_INVALID);
  }
  std::printf("information_driver: ok\n");
  return 0;
}
