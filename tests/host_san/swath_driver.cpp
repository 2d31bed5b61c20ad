// swath_driver.cpp -- TEST INFRASTRUCTURE: the device-free arithmetic of the swath matching (include/mcl_swath.h) under
// AddressSanitizer + UBSan with plain g++: swath_offsets_impl / swath_check_impl of mcl_host_pure.h and the ping matching's
// solve, compare and derived quantities at a swath's bounds (n up to 16384, the largest legal sums), the functions the
// device-free entry points forward to, driven with random, degenerate and hostile inputs.
// Exit code 0 and no sanitizer report = pass.  tests/test_swath_host.py builds and runs it.
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

// n contributing beams with the same differences d and residual rho
static mcl_match_sums uniform_record(long long n, int D, long long d, long long rho) {
  mcl_match_sums r;
  std::memset(&r, 0, sizeof r);
  r.n = n;
  for (int j = 0; j < D; ++j) {
    for (int k = 0; k <= j; ++k) r.S[j * (j + 1) / 2 + k] = n * d * d * (((j + k) & 1) ? -1 : 1);
    r.C[j] = n * d * rho * ((j & 1) ? -1 : 1);
  }
  r.s_rho = n * rho;
  r.s_rho2 = n * rho * rho;
  return r;
}

int main() {
  const double pi = 3.14159265358979323846, inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::mt19937_64 gen(7);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  // ---- offsets: every K, every anchor; the anchor's row exact zeros; composing gives the poses back
  for (int K = 1; K <= MCL_SWATH_MAX_PINGS; ++K) {
    std::vector<double> p(6 * (size_t)K);
    for (int k = 0; k < K; ++k) {
      p[k] = 300.0 * U(gen), p[K + k] = 300.0 * U(gen), p[2 * K + k] = 20.0 * U(gen);
      p[3 * K + k] = 0.2 * U(gen), p[4 * K + k] = 0.2 * U(gen), p[5 * K + k] = pi * U(gen);
    }
    std::vector<mcl_swath_offset> off((size_t)K);
    for (int a = -1; a < K; ++a) {
      CHECK(swath_offsets_impl(p.data(), K, a, off.data()) == MCL_OK);
      const int an = a < 0 ? K - 1 : a;
      const mcl_swath_offset& o = off[(size_t)an];
      CHECK(o.dx == 0.0 && o.dy == 0.0 && o.dz == 0.0 && o.dyaw == 0.0 && !std::signbit(o.dx) && !std::signbit(o.dy));
      CHECK(o.roll == p[3 * K + an] && o.pitch == p[4 * K + an]);
      const double s = std::sin(p[5 * K + an]), c = std::cos(p[5 * K + an]);
      for (int k = 0; k < K; ++k) {
        const mcl_swath_offset& q = off[(size_t)k];
        CHECK(std::fabs(p[an] + (c * q.dx - s * q.dy) - p[k]) < 1e-12 * 300.0 && std::fabs(p[K + an] + (s * q.dx + c * q.dy) - p[K + k]) < 1e-12 * 300.0);
        CHECK(p[2 * K + an] + q.dz == p[2 * K + k] || std::fabs(p[2 * K + an] + q.dz - p[2 * K + k]) < 1e-14);
        CHECK(q.dyaw >= -pi && q.dyaw < pi);
        CHECK(std::fabs(std::remainder(p[5 * K + an] + q.dyaw - p[5 * K + k], 2.0 * pi)) < 1e-12);
      }
      const char* why = "x";
      CHECK(swath_check_impl(K, 256, off.data(), &why) == MCL_OK && swath_check_impl(K, 257, off.data(), &why) == (K * 257 <= MCL_SWATH_MAX_BEAMS ? MCL_OK : MCL_ERR_INVALID));
    }
    CHECK(swath_offsets_impl(p.data(), K, K, off.data()) == MCL_ERR_INVALID && swath_offsets_impl(p.data(), K, -2, off.data()) == MCL_ERR_INVALID);
    p[(size_t)(gen() % (6 * (size_t)K))] = (K & 1) ? inf : nan;
    CHECK(swath_offsets_impl(p.data(), K, -1, off.data()) == MCL_ERR_INVALID);
  }
  {
    double p[6] = {0, 0, 0, 0, 0, 0};
    mcl_swath_offset o;
    CHECK(swath_offsets_impl(nullptr, 1, 0, &o) == MCL_ERR_INVALID && swath_offsets_impl(p, 1, 0, nullptr) == MCL_ERR_INVALID);
    CHECK(swath_offsets_impl(p, 0, 0, &o) == MCL_ERR_INVALID && swath_offsets_impl(p, 65, 0, &o) == MCL_ERR_INVALID);
    // a yaw pair across +-pi
    double q[12] = {0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 3.1, -3.1};
    mcl_swath_offset two[2];
    CHECK(swath_offsets_impl(q, 2, 1, two) == MCL_OK);
    CHECK(std::fabs(two[0].dyaw - (6.2 - 2.0 * pi)) < 1e-14 && two[1].dyaw == 0.0);
    CHECK(swath_offsets_impl(q, 2, 0, two) == MCL_OK);
    CHECK(std::fabs(two[1].dyaw - (2.0 * pi - 6.2)) < 1e-14);
  }
  // ---- the check
  {
    std::vector<mcl_swath_offset> off(MCL_SWATH_MAX_PINGS);
    std::memset(off.data(), 0, sizeof(mcl_swath_offset) * off.size());
    const char* why = nullptr;
    CHECK(swath_check_impl(64, 256, off.data(), &why) == MCL_OK && why == nullptr);
    CHECK(swath_check_impl(8, 2048, off.data(), nullptr) == MCL_OK && swath_check_impl(1, 1, off.data(), &why) == MCL_OK);
    CHECK(swath_check_impl(0, 8, off.data(), &why) == MCL_ERR_INVALID && why && swath_check_impl(65, 8, off.data(), &why) == MCL_ERR_INVALID);
    CHECK(swath_check_impl(8, 0, off.data(), &why) == MCL_ERR_INVALID && swath_check_impl(1, 2049, off.data(), &why) == MCL_ERR_INVALID);
    CHECK(swath_check_impl(64, 257, off.data(), &why) == MCL_ERR_INVALID && swath_check_impl(9, 2048, off.data(), nullptr) == MCL_ERR_INVALID);
    CHECK(swath_check_impl(4, 8, nullptr, &why) == MCL_ERR_INVALID);
    const double bad[3] = {inf, -inf, nan};
    for (int f = 0; f < 6; ++f)
      for (int b = 0; b < 3; ++b) {
        std::vector<mcl_swath_offset> o2 = off;
        reinterpret_cast<double*>(&o2[3])[f] = bad[b];
        CHECK(swath_check_impl(4, 8, o2.data(), &why) == MCL_ERR_INVALID && swath_check_impl(3, 8, o2.data(), &why) == MCL_OK);
      }
  }
  // ---- solve, compare and derived at a swath's bounds
  {
    const long long N = MCL_SWATH_MAX_BEAMS, DM = 1ll << 23, RM = 1ll << 24;
    for (int D = 3; D <= 4; ++D) {
      const mcl_match_config c = config(D);
      const mcl_match_sums top = uniform_record(N, D, DM, RM);
      CHECK(top.S[0] == 1ll << 60 && top.C[0] == 1ll << 61 && top.s_rho2 == 1ll << 62);
      double delta[4];
      int32_t dead = -1, better = -1;
      mcl_match_derived_t dv;
      for (int j = MCL_MATCH_J_MIN; j <= MCL_MATCH_J_MAX + 2; ++j) {
        CHECK(match_solve_impl(&top, &c, j, delta, &dead, MCL_SWATH_MAX_BEAMS) == MCL_OK);
        for (int k = 0; k < 4; ++k) CHECK(std::isfinite(delta[k]));
      }
      CHECK(match_solve_impl(&top, &c, 0, delta, &dead) == MCL_ERR_INVALID);   // the ping's entry point keeps its bound
      CHECK(match_derived_impl(&top, &c, 0.2, &dv, MCL_SWATH_MAX_BEAMS) == MCL_OK && dv.m == N && dv.rms == 4096.0);
      CHECK(match_derived_impl(&top, &c, 0.2, &dv) == MCL_ERR_INVALID);
      mcl_match_sums less = top;
      less.s_rho2 -= 1;
      CHECK(match_better_impl(&less, &top, 8, &better, MCL_SWATH_MAX_BEAMS) == MCL_OK && better == 1);
      CHECK(match_better_impl(&top, &less, 8, &better, MCL_SWATH_MAX_BEAMS) == MCL_OK && better == 0);
      CHECK(match_better_impl(&top, &top, 8, &better, MCL_SWATH_MAX_BEAMS) == MCL_OK && better == 0);
      CHECK(match_better_impl(&less, &top, 8, &better) == MCL_ERR_INVALID);
      mcl_match_sums over = top;
      over.n += 1;
      CHECK(match_solve_impl(&over, &c, 0, delta, &dead, MCL_SWATH_MAX_BEAMS) == MCL_ERR_INVALID);
      over = top;
      over.s_rho2 += 1;
      CHECK(match_derived_impl(&over, &c, 0.2, &dv, MCL_SWATH_MAX_BEAMS) == MCL_ERR_INVALID);
      over = top;
      over.S[0] += 1;
      CHECK(match_better_impl(&over, &top, 8, &better, MCL_SWATH_MAX_BEAMS) == MCL_ERR_INVALID);
      // random records of many beams
      std::uniform_int_distribution<long long> Dd(-DM, DM), Dr(-RM, RM), Dn(1, N);
      for (int trial = 0; trial < 400; ++trial) {
        const long long n = Dn(gen);
        mcl_match_sums r = uniform_record(n, D, Dd(gen) >> (trial % 20), Dr(gen) >> (trial % 23));
        r.n += trial % 3;
        r.n_miss = trial % 3;
        CHECK(r.n > N || match_solve_impl(&r, &c, MCL_MATCH_J_MIN + trial % 43, delta, &dead, MCL_SWATH_MAX_BEAMS) == MCL_OK);
        CHECK(r.n > N || match_derived_impl(&r, &c, 0.05, &dv, MCL_SWATH_MAX_BEAMS) == MCL_OK);
        CHECK(r.n > N || match_better_impl(&r, &top, 1, &better, MCL_SWATH_MAX_BEAMS) == MCL_OK);
      }
    }
  }
  std::printf("swath_driver: ok\n");
  return 0;
}
