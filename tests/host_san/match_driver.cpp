// match_driver.cpp -- TEST INFRASTRUCTURE: the device-free arithmetic of the ping matching (include/mcl_match.h) under
// AddressSanitizer + UBSan with plain g++: match_config_check_impl / match_solve_impl / match_better_impl /
// match_derived_impl of mcl_host_pure.h, the functions the device-free entry points forward to, and match_solve_core /
// match_better, the rules the kernel runs itself, driven with random, degenerate and hostile inputs.
// Exit code 0 and no sanitizer report = pass.  tests/test_match_host.py builds and runs it.
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

struct Pair {
  long long d[4], rho;
};

static mcl_match_sums record_of(const std::vector<Pair>& p, int D, long long n_miss, long long n_jump) {
  mcl_match_sums r;
  std::memset(&r, 0, sizeof r);
  r.n = (int64_t)p.size() + n_miss + n_jump;
  r.n_miss = n_miss;
  r.n_jump = n_jump;
  for (const Pair& t : p) {
    for (int j = 0; j < D; ++j) {
      for (int k = 0; k <= j; ++k) r.S[j * (j + 1) / 2 + k] += t.d[j] * t.d[k];
      r.C[j] += t.d[j] * t.rho;
    }
    r.s_rho += t.rho;
    r.s_rho2 += t.rho * t.rho;
  }
  return r;
}

static mcl_match_config config(int dims) {
  mcl_match_config c;
  std::memset(&c, 0, sizeof c);
  c.dims = dims;
  c.max_iter = 12;
  c.min_beams = 8;
  c.grad_floor_q = 2;
  c.step_max_xy = 2.0;
  c.step_max_yaw = 0.1;
  c.tol_xy = 1e-3;
  c.tol_yaw = 1e-4;
  c.steps.delta_xy = 0.5;
  c.steps.delta_yaw = 0.01;
  c.steps.jump_max = 80.0;
  return c;
}

int main() {
  std::mt19937_64 rng(20261020);
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const long long D_MAX = 1ll << 23, RHO_MAX = 1ll << 24;
  const char* why = nullptr;
  // ---- the config
  {
    mcl_match_config c = config(3);
    CHECK(match_config_check_impl(&c, 80.0, &why) == MCL_OK && why == nullptr);
    CHECK(match_config_check_impl(&c, 80.0, nullptr) == MCL_OK);
    CHECK(match_config_check_impl(nullptr, 80.0, &why) == MCL_ERR_INVALID && why != nullptr);
    CHECK(match_config_check_impl(&c, 79.0, &why) == MCL_ERR_INVALID && match_config_check_impl(&c, 4097.0, &why) == MCL_ERR_INVALID);
    for (int bad : {2, 5, 0, -3}) {
      mcl_match_config t = c;
      t.dims = bad;
      CHECK(match_config_check_impl(&t, 80.0, &why) == MCL_ERR_INVALID);
    }
    for (int bad : {0, 33, -1}) {
      mcl_match_config t = c;
      t.max_iter = bad;
      CHECK(match_config_check_impl(&t, 80.0, &why) == MCL_ERR_INVALID);
    }
    for (double bad : {0.0, -1.0, nan, inf}) {
      mcl_match_config t = c;
      t.step_max_xy = bad;
      CHECK(match_config_check_impl(&t, 80.0, &why) == MCL_ERR_INVALID);
      t = c;
      t.step_max_yaw = bad;
      CHECK(match_config_check_impl(&t, 80.0, &why) == MCL_ERR_INVALID);
      t = c;
      t.steps.delta_xy = bad;
      CHECK(match_config_check_impl(&t, 80.0, &why) == MCL_ERR_INVALID);
      t = c;
      t.steps.delta_yaw = bad;
      CHECK(match_config_check_impl(&t, 80.0, &why) == MCL_ERR_INVALID);
    }
    for (double bad : {-1e-9, nan, inf}) {
      mcl_match_config t = c;
      t.tol_xy = bad;
      CHECK(match_config_check_impl(&t, 80.0, &why) == MCL_ERR_INVALID);
      t = c;
      t.tol_yaw = bad;
      CHECK(match_config_check_impl(&t, 80.0, &why) == MCL_ERR_INVALID);
    }
    mcl_match_config t = c;
    t.min_beams = 0;
    CHECK(match_config_check_impl(&t, 80.0, &why) == MCL_ERR_INVALID);
    t = c;
    t.grad_floor_q = 4097;
    CHECK(match_config_check_impl(&t, 80.0, &why) == MCL_ERR_INVALID);
    t.grad_floor_q = 4096;
    t.max_iter = 32;
    t.tol_xy = 0.0;
    CHECK(match_config_check_impl(&t, 80.0, &why) == MCL_OK);
  }
  double delta[4];
  int32_t dead = 0, better = 0;
  mcl_match_derived_t dv;
  // ---- the edges of the solve
  for (int D = 3; D <= 4; ++D) {
    const mcl_match_config c = config(D);
    const int beyond = D == 3 ? 8 : 0;
    mcl_match_sums none;
    std::memset(&none, 0, sizeof none);
    CHECK(match_solve_impl(&none, &c, MCL_MATCH_J0, delta, &dead) == MCL_OK && dead == 15);
    CHECK(delta[0] == 0.0 && delta[1] == 0.0 && delta[2] == 0.0 && delta[3] == 0.0 && !std::signbit(delta[0]));
    CHECK(match_derived_impl(&none, &c, 0.2, &dv) == MCL_OK && dv.rms == 0.0 && dv.m == 0 && dv.dead == 15 && dv.cov[0] == inf);
    // a unit gradient in x alone and a residual of 100 quanta: the step is 100 / 4096 m but for the damping
    std::vector<Pair> px(10, Pair{{4096, 0, 0, 0}, 100});
    const mcl_match_sums rx = record_of(px, D, 2, 1);
    CHECK(match_solve_impl(&rx, &c, MCL_MATCH_J_MIN, delta, &dead) == MCL_OK && dead == (2 | 4 | 8));
    CHECK(std::fabs(delta[0] - 100.0 / 4096.0) < 1e-7 && delta[1] == 0.0 && delta[2] == 0.0 && delta[3] == 0.0);
    CHECK(match_derived_impl(&rx, &c, 0.2, &dv) == MCL_OK && dv.m == 10 && dv.rms == 100.0 / 4096.0 && dv.mean == dv.rms);
    CHECK(dv.J[0] == 10.0 / (0.2 * 0.2) && std::fabs(dv.cov[0] - 0.2 * 0.2 / 10.0) < 1e-15 && dv.cov[2] == inf && dv.dead == (2 | 4 | 8));
    // the damping shortens the step, monotonically
    double last = 1.0;
    for (int j = MCL_MATCH_J_MIN; j <= MCL_MATCH_J_MAX + 2; ++j) {
      CHECK(match_solve_impl(&rx, &c, j, delta, &dead) == MCL_OK && delta[0] > 0.0 && delta[0] < last);
      last = delta[0];
    }
    CHECK(match_solve_impl(&rx, &c, MCL_MATCH_J_MIN - 1, delta, &dead) == MCL_ERR_INVALID);
    CHECK(match_solve_impl(&rx, &c, MCL_MATCH_J_MAX + 3, delta, &dead) == MCL_ERR_INVALID);
    // a residual so large that the step is clamped, in the horizontal, in yaw and in z
    std::vector<Pair> big;
    for (int k = 0; k < 64; ++k) big.push_back(Pair{{4096 + 7 * k, (k % 7) * 300 - 900, (k % 5) * 20 - 40, (k % 3) * 2000 - 1000}, RHO_MAX});
    const mcl_match_sums rb = record_of(big, D, 0, 0);
    CHECK(match_solve_impl(&rb, &c, MCL_MATCH_J0, delta, &dead) == MCL_OK && dead == beyond);
    CHECK(std::sqrt(delta[0] * delta[0] + delta[1] * delta[1]) <= c.step_max_xy * (1 + 1e-15));
    CHECK(std::fabs(delta[2]) <= c.step_max_yaw * (1 + 1e-15) && std::fabs(delta[3]) <= c.step_max_xy * (1 + 1e-15));
    // the largest legal sums
    std::vector<Pair> top(MCL_MATCH_MAX_BEAMS, Pair{{D_MAX, -D_MAX, D_MAX, -D_MAX}, RHO_MAX});
    const mcl_match_sums rt = record_of(top, D, 0, 0);
    CHECK(rt.S[0] == (1ll << 57) && rt.C[0] == (1ll << 58) && rt.s_rho2 == (1ll << 59) && match_legal(rt));
    CHECK(match_solve_impl(&rt, &c, MCL_MATCH_J_MAX, delta, &dead) == MCL_OK && std::isfinite(delta[0]));
    CHECK(match_derived_impl(&rt, &c, 0.2, &dv) == MCL_OK && std::isfinite(dv.J[0]) && dv.rms == 4096.0);
    std::vector<Pair> less = top;
    less.back().rho = RHO_MAX - 1;
    const mcl_match_sums rl = record_of(less, D, 0, 0);
    CHECK(match_better_impl(&rl, &rt, 8, &better) == MCL_OK && better == 1);
    CHECK(match_better_impl(&rt, &rl, 8, &better) == MCL_OK && better == 0);
    CHECK(match_better_impl(&rt, &rt, 8, &better) == MCL_OK && better == 0);
    CHECK(match_better_impl(&rl, &rt, 2049, &better) == MCL_OK && better == 0);
    CHECK(match_better_impl(&rl, &rt, 0, &better) == MCL_ERR_INVALID);
  }
  // ---- records that are no sums, null pointers
  {
    const mcl_match_config c = config(4);
    const mcl_match_sums ok = record_of(std::vector<Pair>(10, Pair{{100, 50, 3, -8}, 7}), 4, 0, 0);
    CHECK(match_legal(ok));
    std::vector<mcl_match_sums> bad(9, ok);
    bad[0].n = -1;
    bad[1].n = MCL_MATCH_MAX_BEAMS + 1;
    bad[2].n_miss = 11;
    bad[3].n_jump = -1;
    bad[4].S[0] = -1;
    bad[5].S[1] = INT64_MIN;
    bad[6].C[3] = INT64_MAX;
    bad[7].s_rho2 = -1;
    bad[8].s_rho = INT64_MIN;
    for (const mcl_match_sums& r : bad) {
      CHECK(!match_legal(r) && match_solve_impl(&r, &c, 0, delta, &dead) == MCL_ERR_INVALID);
      CHECK(match_derived_impl(&r, &c, 0.2, &dv) == MCL_ERR_INVALID && match_better_impl(&r, &ok, 1, &better) == MCL_ERR_INVALID);
      CHECK(match_better_impl(&ok, &r, 1, &better) == MCL_ERR_INVALID);
    }
    CHECK(match_solve_impl(nullptr, &c, 0, delta, &dead) == MCL_ERR_INVALID && match_solve_impl(&ok, nullptr, 0, delta, &dead) == MCL_ERR_INVALID);
    CHECK(match_solve_impl(&ok, &c, 0, nullptr, &dead) == MCL_ERR_INVALID && match_solve_impl(&ok, &c, 0, delta, nullptr) == MCL_ERR_INVALID);
    CHECK(match_better_impl(nullptr, &ok, 1, &better) == MCL_ERR_INVALID && match_better_impl(&ok, &ok, 1, nullptr) == MCL_ERR_INVALID);
    CHECK(match_derived_impl(&ok, &c, 0.2, nullptr) == MCL_ERR_INVALID && match_derived_impl(nullptr, &c, 0.2, &dv) == MCL_ERR_INVALID);
    for (double s : {0.0, -1.0, nan, inf}) CHECK(match_derived_impl(&ok, &c, s, &dv) == MCL_ERR_INVALID);
  }
  // ---- random records: the step against a long-double Gaussian elimination of the damped system, the covariance against
  // the information (cov J = the identity over the live dimensions); heap arrays of the exact size
  for (int trial = 0; trial < 400; ++trial) {
    const int D = 3 + (trial & 1);
    mcl_match_config c = config(D);
    c.step_max_xy = c.step_max_yaw = 1e12;
    const int n = 1 + (int)(rng() % 300);
    const long long scale = 1ll << (4 + rng() % 18), rs = 1ll << (rng() % 20);
    std::vector<Pair> p((size_t)n);
    for (Pair& t : p) {
      for (int k = 0; k < 4; ++k) t.d[k] = (long long)(rng() % (uint64_t)(2 * scale + 1)) - scale;
      t.rho = (long long)(rng() % (uint64_t)(2 * rs + 1)) - rs;
    }
    const mcl_match_sums r = record_of(p, D, (long long)(rng() % 3), (long long)(rng() % 3));
    CHECK(match_legal(r));
    const int j = MCL_MATCH_J_MIN + (int)(rng() % 43);
    CHECK(match_solve_impl(&r, &c, j, delta, &dead) == MCL_OK);
    std::vector<int> live;
    for (int k = 0; k < D; ++k)
      if (!((dead >> k) & 1)) live.push_back(k);
    const int nl = (int)live.size();
    const double dl[4] = {c.steps.delta_xy, c.steps.delta_xy, c.steps.delta_yaw, c.steps.delta_xy};
    std::vector<long double> A((size_t)nl * nl), b((size_t)nl);
    for (int i = 0; i < nl; ++i) {
      for (int k = 0; k < nl; ++k) {
        const int hi = std::max(live[i], live[k]), lo = std::min(live[i], live[k]);
        A[(size_t)i * nl + k] = (long double)r.S[hi * (hi + 1) / 2 + lo] / (4.0L * dl[live[i]] * dl[live[k]] * 16777216.0L);
      }
      A[(size_t)i * nl + i] *= 1.0L + std::ldexp(1.0L, j);
      b[(size_t)i] = (long double)r.C[live[i]] / (2.0L * dl[live[i]] * 16777216.0L);
    }
    long double res = 0, mag = 0;
    for (int i = 0; i < nl; ++i) {
      long double s = -b[(size_t)i];
      for (int k = 0; k < nl; ++k) s += A[(size_t)i * nl + k] * (long double)delta[live[k]];
      res = std::max(res, std::fabs(s));
      mag = std::max(mag, std::fabs(b[(size_t)i]));
      for (int k = 0; k < nl; ++k) mag = std::max(mag, std::fabs(A[(size_t)i * nl + k] * (long double)delta[live[k]]));
    }
    CHECK(res <= 1e-6L * mag + 1e-300L);   // (a factor with pivots down to 2^-26 of the diagonal loses digits, not the answer)
    CHECK(match_derived_impl(&r, &c, 0.3, &dv) == MCL_OK && dv.m == n && dv.rms >= std::fabs(dv.mean));
    for (int k = 0; k < D; ++k) CHECK(((dv.dead >> k) & 1) ? dv.cov[k * (k + 1) / 2 + k] == inf : dv.cov[k * (k + 1) / 2 + k] > 0.0);
    const mcl_match_sums q = record_of(std::vector<Pair>(p.begin(), p.begin() + n / 2 + 1), D, 0, 0);
    CHECK(match_better_impl(&q, &r, 1, &better) == MCL_OK);
    typedef unsigned __int128 u128;
    CHECK((better == 1) == ((u128)q.s_rho2 * (u128)match_m(r) < (u128)r.s_rho2 * (u128)match_m(q)));
  }
  std::printf("match_driver: ok\n");
  return 0;
}
