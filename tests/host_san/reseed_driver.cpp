// reseed_driver.cpp -- TEST INFRASTRUCTURE: the device-free arithmetic of the sensor resetting (include/mcl_reseed.h) under
// AddressSanitizer + UBSan with plain g++: reseed_select_impl, reseed_select_check_impl, reseed_components_check_impl and
// reseed_rank of mcl_host_pure.h, the functions the device-free entry points forward to (and the kernel's rank), driven
// with random, degenerate and hostile inputs.  Exit code 0 and no sanitizer report = pass.  tests/test_reseed_host.py
// builds and runs it.
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

static mcl_reseed_select_config select_config(int max_components) {
  mcl_reseed_select_config c;
  std::memset(&c, 0, sizeof c);
  c.max_components = max_components;
  c.min_beams = 16;
  c.max_rms = 0.5;
  c.sep_xy = 1.0;
  c.sep_yaw = 0.1;
  c.cov_scale = 1.0;
  c.add_std_xy = 0.25;
  c.add_std_yaw = 0.02;
  c.dead_std_xy = 4.0;
  c.dead_std_yaw = 0.2;
  return c;
}

// a record of n contributing beams whose differences are random (a well-conditioned S) or, per bit of `flat`, zero
static mcl_match_sums record(std::mt19937_64& gen, long long n, int D, int flat, long long rho) {
  mcl_match_sums r;
  std::memset(&r, 0, sizeof r);
  r.n = n;
  std::uniform_int_distribution<long long> U(-3000, 3000);
  for (long long b = 0; b < n; ++b) {
    long long d[4] = {0, 0, 0, 0};
    for (int k = 0; k < D; ++k) d[k] = ((flat >> k) & 1) ? 0 : U(gen);
    for (int j = 0; j < D; ++j) {
      for (int k = 0; k <= j; ++k) r.S[j * (j + 1) / 2 + k] += d[j] * d[k];
      r.C[j] += d[j] * rho;
    }
    r.s_rho += rho;
    r.s_rho2 += rho * rho;
  }
  return r;
}

int main() {
  const double pi = 3.14159265358979323846, inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::mt19937_64 gen(11);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  const char* why = nullptr;
  // ---- the selection config: every rule
  {
    mcl_reseed_select_config c = select_config(16);
    CHECK(reseed_select_check_impl(&c, &why) == MCL_OK && why == nullptr);
    CHECK(reseed_select_check_impl(&c, nullptr) == MCL_OK);
    CHECK(reseed_select_check_impl(nullptr, &why) == MCL_ERR_INVALID && why);
    for (int m : {0, -1, 257}) {
      c = select_config(m);
      CHECK(reseed_select_check_impl(&c, &why) == MCL_ERR_INVALID && why);
    }
    for (int f = 0; f < 8; ++f)
      for (double bad : {-1.0, nan, inf, 0.0}) {
        c = select_config(4);
        double* field[8] = {&c.max_rms, &c.sep_xy, &c.sep_yaw, &c.cov_scale, &c.add_std_xy, &c.add_std_yaw, &c.dead_std_xy, &c.dead_std_yaw};
        *field[f] = bad;
        const bool zero_ok = f != 3 && f < 6;   // cov_scale and the dead stds must be > 0
        CHECK((reseed_select_check_impl(&c, &why) == MCL_OK) == (bad == 0.0 && zero_ok));
      }
    c = select_config(4);
    c.min_beams = 0;
    CHECK(reseed_select_check_impl(&c, &why) == MCL_ERR_INVALID);
  }
  // ---- the component table: every rule, both ends of W
  {
    std::vector<mcl_reseed_component> t(MCL_RESEED_MAX_COMPONENTS + 1);
    std::memset(t.data(), 0, t.size() * sizeof t[0]);
    uint64_t W = 0;
    CHECK(reseed_components_why(t.data(), 1, &W) != nullptr);           // W = 0
    t[0].mass = 1;
    CHECK(reseed_components_why(t.data(), 1, &W) == nullptr && W == 1);
    CHECK(reseed_components_why(t.data(), MCL_RESEED_MAX_COMPONENTS, &W) == nullptr && W == 1);
    CHECK(reseed_components_why(t.data(), MCL_RESEED_MAX_COMPONENTS + 1, &W) != nullptr);
    CHECK(reseed_components_why(t.data(), 0, &W) != nullptr && reseed_components_why(nullptr, 1, &W) != nullptr);
    t[0].mass = 1u << 31;
    CHECK(reseed_components_why(t.data(), 2, &W) == nullptr && W == (1ull << 31));
    t[1].mass = 1;
    CHECK(reseed_components_why(t.data(), 2, &W) != nullptr);           // 2^31 + 1
    t[0].mass = t[1].mass = 0xffffffffu;                                 // (no 32-bit wrap of the sum)
    CHECK(reseed_components_why(t.data(), 2, nullptr) != nullptr);
    t[0].mass = 1, t[1].mass = 0;
    for (int k = 0; k < 9; ++k)
      for (double bad : {nan, inf, -inf}) {
        mcl_reseed_component c = t[0];
        (k < 3 ? c.mean[k] : c.chol[k - 3]) = bad;
        CHECK(reseed_components_check_impl(&c, 1, &why) == MCL_ERR_INVALID && why);
      }
    for (int k : {0, 2, 5}) {
      mcl_reseed_component c = t[0];
      c.chol[k] = -1e-300;
      CHECK(reseed_components_check_impl(&c, 1, &why) == MCL_ERR_INVALID);
      c.chol[k] = -0.0;
      CHECK(reseed_components_check_impl(&c, 1, &why) == MCL_OK);
    }
    mcl_reseed_component c = t[0];
    c.chol[1] = c.chol[3] = c.chol[4] = -5.0;   // the off-diagonal may be negative
    CHECK(reseed_components_check_impl(&c, 1, nullptr) == MCL_OK);
  }
  // ---- the rank: both ends of t and of W against 128-bit arithmetic
  {
    const uint64_t tmax = (1ull << 53) - 1;
    for (uint64_t W : {1ull, 2ull, 3ull, 255ull, 65537ull, (1ull << 31) - 1, 1ull << 31}) {
      CHECK(reseed_rank(0, W) == 0);
      CHECK(reseed_rank(tmax, W) == W - 1);
      for (int it = 0; it < 2000; ++it) {
        const uint64_t t = gen() >> 11;
        CHECK(reseed_rank(t, W) == (uint32_t)(((unsigned __int128)t * W) >> 53));
      }
    }
  }
  // ---- the selection: random result sets in both dimensions, dead masks 0 ... 7, hostile records and statuses
  for (int D = 3; D <= 4; ++D) {
    const mcl_match_config mc = config(D);
    for (int round = 0; round < 40; ++round) {
      const int M = 1 + (int)(gen() % 60);
      std::vector<mcl_match_result> res((size_t)M);
      std::memset(res.data(), 0, res.size() * sizeof res[0]);
      for (int i = 0; i < M; ++i) {
        res[i].x = 50.0 * U(gen);
        res[i].y = 50.0 * U(gen);
        res[i].yaw = pi * U(gen);
        res[i].status = (int)(gen() % 5 == 0 ? gen() % 4 : 0);
        res[i].final = record(gen, 8 + (long long)(gen() % 120), D, (int)(gen() % 8 == 0 ? gen() % 8 : 0), (long long)(gen() % 3000));
        if (i > 0 && gen() % 4 == 0) {   // a twin of the fix before it: one hypothesis
          res[i].x = res[i - 1].x + 0.1;
          res[i].y = res[i - 1].y;
          res[i].yaw = res[i - 1].yaw;
        }
      }
      for (int maxc : {1, 3, 256}) {
        mcl_reseed_select_config sc = select_config(maxc);
        std::vector<mcl_reseed_component> comps((size_t)maxc);
        std::vector<int64_t> idx((size_t)maxc);
        int32_t n = -1;
        CHECK(reseed_select_impl(res.data(), M, &mc, 0.2, &sc, comps.data(), idx.data(), &n) == MCL_OK);
        CHECK(n >= 0 && n <= maxc && n <= M);
        for (int c = 0; c < n; ++c) {
          CHECK(idx[c] >= 0 && idx[c] < M && res[idx[c]].status == MCL_MATCH_CONVERGED && comps[c].mass == 1);
          CHECK(reseed_components_check_impl(&comps[c], 1, nullptr) == MCL_OK);
          CHECK(comps[c].chol[0] > 0.0 && comps[c].chol[2] > 0.0 && comps[c].chol[5] > 0.0);   // add_std > 0: every dimension spreads
        }
        if (n > 0) CHECK(reseed_components_check_impl(comps.data(), n, nullptr) == MCL_OK);
      }
    }
    // no candidate: every status but CONVERGED
    {
      std::vector<mcl_match_result> res(3);
      std::memset(res.data(), 0, res.size() * sizeof res[0]);
      for (int i = 0; i < 3; ++i) {
        res[i].status = i + 1;
        res[i].final = record(gen, 64, D, 0, 10);
      }
      mcl_reseed_select_config sc = select_config(4);
      mcl_reseed_component comps[4];
      int64_t idx[4];
      int32_t n = -1;
      CHECK(reseed_select_impl(res.data(), 3, &mc, 0.2, &sc, comps, idx, &n) == MCL_OK && n == 0);
      // what is refused: nulls, M, sigma, a config either check refuses, a CONVERGED record that cannot be a sum, a pose that is not finite
      CHECK(reseed_select_impl(nullptr, 3, &mc, 0.2, &sc, comps, idx, &n) == MCL_ERR_INVALID);
      CHECK(reseed_select_impl(res.data(), 3, nullptr, 0.2, &sc, comps, idx, &n) == MCL_ERR_INVALID);
      CHECK(reseed_select_impl(res.data(), 3, &mc, 0.2, nullptr, comps, idx, &n) == MCL_ERR_INVALID);
      CHECK(reseed_select_impl(res.data(), 3, &mc, 0.2, &sc, nullptr, idx, &n) == MCL_ERR_INVALID);
      CHECK(reseed_select_impl(res.data(), 3, &mc, 0.2, &sc, comps, nullptr, &n) == MCL_ERR_INVALID);
      CHECK(reseed_select_impl(res.data(), 3, &mc, 0.2, &sc, comps, idx, nullptr) == MCL_ERR_INVALID);
      CHECK(reseed_select_impl(res.data(), 0, &mc, 0.2, &sc, comps, idx, &n) == MCL_ERR_INVALID);
      CHECK(reseed_select_impl(res.data(), MCL_MATCH_MAX_POSES + 1, &mc, 0.2, &sc, comps, idx, &n) == MCL_ERR_INVALID);
      for (double s : {0.0, -1.0, nan, inf}) CHECK(reseed_select_impl(res.data(), 3, &mc, s, &sc, comps, idx, &n) == MCL_ERR_INVALID);
      res[0].status = MCL_MATCH_CONVERGED;
      res[0].final.n_miss = res[0].final.n + 1;
      CHECK(reseed_select_impl(res.data(), 3, &mc, 0.2, &sc, comps, idx, &n) == MCL_ERR_INVALID);
      res[0].final = record(gen, 64, D, 0, 10);
      res[0].yaw = nan;
      CHECK(reseed_select_impl(res.data(), 3, &mc, 0.2, &sc, comps, idx, &n) == MCL_ERR_INVALID);
      res[0].yaw = 0.0;
      CHECK(reseed_select_impl(res.data(), 3, &mc, 0.2, &sc, comps, idx, &n) == MCL_OK && n == 1 && idx[0] == 0);
      // the largest legal swath record, flat in every dimension: all dead, the dead stds and the added ones make the factor
      res[0].final = record(gen, 0, D, 7, 0);
      res[0].final.n = MCL_SWATH_MAX_BEAMS;
      CHECK(reseed_select_impl(res.data(), 3, &mc, 0.2, &sc, comps, idx, &n) == MCL_OK && n == 1);
      CHECK(comps[0].chol[1] == 0.0 && comps[0].chol[3] == 0.0 && comps[0].chol[4] == 0.0);
      CHECK(std::fabs(comps[0].chol[0] - std::sqrt(16.0 + 0.0625)) < 1e-12 && std::fabs(comps[0].chol[5] - std::sqrt(0.04 + 0.0004)) < 1e-12);
    }
  }
  std::printf("reseed_driver: ok\n");
  return 0;
}
