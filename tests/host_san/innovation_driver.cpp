// innovation_driver.cpp -- TEST INFRASTRUCTURE: the device-free arithmetic of the ping innovation statistics
// (include/mcl_innovation.h) under AddressSanitizer + UBSan with plain g++: innovation_sample_impl / innovation_dirs_impl /
// innovation_merge_impl / innovation_gate_impl of mcl_host_pure.h, the functions the four device-free entry points forward
// to, and innov_quantise / innov_q_support / innov_shard_sample / innov_u128_to_double, the rules the kernel and its launcher
// run, driven with random, degenerate and hostile inputs.
// Exit code 0 and no sanitizer report = pass.  tests/test_innovation_host.py builds and runs it.
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

typedef unsigned __int128 u128;

static mcl_innovation_beam record_of(const std::vector<long long>& q, long long n_within) {
  mcl_innovation_beam r = {(int64_t)q.size(), 0, n_within, 0, 0};
  for (long long v : q) {
    r.s1 += v;
    r.s2 += (uint64_t)(v * v);
  }
  return r;
}

int main() {
  std::mt19937_64 rng(20261020);
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const float fnan = std::numeric_limits<float>::quiet_NaN(), fmax = std::numeric_limits<float>::max();
  // ---- the quantised residual: exact on the grid, clamped whatever the range is
  CHECK(innov_quantise(10.f, 10.f) == 0 && innov_quantise(10.25f, 10.f) == 1024 && innov_quantise(10.f, 10.25f) == -1024);
  CHECK(innov_quantise(fmax, 0.f) == INNOV_Q_MAX && innov_quantise(-fmax, 0.f) == -INNOV_Q_MAX);
  CHECK(innov_quantise(4096.f, 0.f) == INNOV_Q_MAX && innov_quantise(0.f, 4096.f) == -INNOV_Q_MAX);
  CHECK(innov_quantise(std::numeric_limits<float>::infinity(), 1.f) == INNOV_Q_MAX);
  CHECK(innov_quantise(1.f + 1.f / 8192.f, 1.f) == 0 && innov_quantise(1.f + 3.f / 8192.f, 1.f) == 2);   // ties to even
  CHECK(innov_q_support(3.0, 0.2) == 2457 && innov_q_support(0.0, 0.2) == 0 && innov_q_support(1e300, 1.0) == INNOV_Q_MAX);
  // ---- the sample
  int64_t stride = 0, count = 0;
  CHECK(innovation_sample_impl(4096, 1000, &stride, &count) == MCL_OK && stride == 5 && count == 820);
  CHECK(innovation_sample_impl(10, 4096, &stride, &count) == MCL_OK && stride == 1 && count == 10);
  CHECK(innovation_sample_impl(0xffffffffll, 32768, &stride, &count) == MCL_OK && count <= 32768);
  CHECK(innovation_sample_impl(0, 1, &stride, &count) == MCL_ERR_INVALID && innovation_sample_impl(5, 0, &stride, &count) == MCL_ERR_INVALID);
  CHECK(innovation_sample_impl(5, 32769, &stride, &count) == MCL_ERR_INVALID && innovation_sample_impl(5, 5, nullptr, &count) == MCL_ERR_INVALID);
  CHECK(innovation_sample_impl(5, 5, &stride, nullptr) == MCL_ERR_INVALID);
  for (int k = 0; k < 20000; ++k) {
    const int64_t ng = 1 + (int64_t)(rng() % (1ull << (1 + rng() % 32)));
    const int32_t ms = 1 + (int32_t)(rng() % 32768);
    CHECK(innovation_sample_impl(ng, ms, &stride, &count) == MCL_OK);
    CHECK(stride >= 1 && count >= 1 && count <= ms && (count - 1) * stride < ng && count * stride >= ng);
    // any split into two shards samples what the whole samples
    const int64_t cut = (int64_t)(rng() % (uint64_t)(ng + 1));
    long long f0 = -1, f1 = -1;
    const long long c0 = innov_shard_sample(0, cut, stride, &f0), c1 = innov_shard_sample(cut, ng - cut, stride, &f1);
    CHECK(c0 + c1 == count && f0 == 0 && f1 >= 0 && f1 < stride && (c1 == 0 || (cut + f1) % stride == 0));
    CHECK(c1 == 0 || f1 + (c1 - 1) * stride < ng - cut);
  }
  // ---- directions: unit, x = 0, refusals; heap buffers of the exact size
  {
    const int B = 513;
    std::vector<float> a(B), d(3 * B);
    for (int b = 0; b < B; ++b) a[b] = -1.5f + 3.0f * (float)b / (float)(B - 1);
    CHECK(innovation_dirs_impl(a.data(), B, d.data()) == MCL_OK);
    for (int b = 0; b < B; ++b) {
      const double n2 = (double)d[3 * b + 1] * d[3 * b + 1] + (double)d[3 * b + 2] * d[3 * b + 2];
      CHECK(d[3 * b] == 0.f && std::fabs(n2 - 1.0) < 1e-6 && d[3 * b + 2] < 0.f);
    }
    a[7] = fnan;
    CHECK(innovation_dirs_impl(a.data(), B, d.data()) == MCL_ERR_INVALID);
    a[7] = std::numeric_limits<float>::infinity();
    CHECK(innovation_dirs_impl(a.data(), B, d.data()) == MCL_ERR_INVALID);
    CHECK(innovation_dirs_impl(nullptr, 1, d.data()) == MCL_ERR_INVALID && innovation_dirs_impl(a.data(), 1, nullptr) == MCL_ERR_INVALID);
    CHECK(innovation_dirs_impl(a.data(), 0, d.data()) == MCL_ERR_INVALID && innovation_dirs_impl(a.data(), MCL_INNOVATION_MAX_BEAMS + 1, d.data()) == MCL_ERR_INVALID);
  }
  // ---- 128-bit integers to the nearest double, ties to even
  CHECK(innov_u128_to_double(0) == 0.0 && innov_u128_to_double(((u128)1 << 64)) == 18446744073709551616.0);
  CHECK(innov_u128_to_double(~(u128)0) == std::ldexp(1.0, 128));
  CHECK(innov_u128_to_double(((u128)1 << 78) + ((u128)1 << 25)) == std::ldexp(1.0, 78));                        // a tie: down to even
  CHECK(innov_u128_to_double(((u128)1 << 78) + ((u128)1 << 25) + 1) == std::ldexp(1.0, 78) + std::ldexp(1.0, 26));  // above the tie
  CHECK(innov_u128_to_double(((u128)1 << 78) + ((u128)3 << 25)) == std::ldexp(1.0, 78) + std::ldexp(1.0, 27));  // a tie: up to even
  for (int k = 0; k < 20000; ++k) {
    const u128 v = (((u128)rng() << 64) | rng()) >> (rng() % 128);
    const double got = innov_u128_to_double(v);
    const long double want = (long double)(uint64_t)(v >> 64) * 18446744073709551616.0L + (long double)(uint64_t)v;   // (64-bit mantissa: one rounding that
    CHECK(std::fabs((long double)got - want) <= std::ldexp((long double)got, -52));                                    //  bounds ours from outside; the ties are above)
  }
  // ---- the gate at its edges
  const double sigma = 0.2;
  const long long q20 = 16384;   // 20 sigma
  const mcl_innovation_beam cand = record_of(std::vector<long long>(100, -q20), 0), clean = record_of(std::vector<long long>(100, 0), 100);
  const mcl_innovation_beam none = {0, 0, 0, 0, 0};
  mcl_innovation_verdict v;
  {
    std::vector<mcl_innovation_beam> beams(64, clean);
    std::vector<mcl_innovation_derived> per(64);
    for (int b = 0; b < 16; ++b) beams[b] = cand;
    CHECK(innovation_gate_impl(beams.data(), 64, sigma, nullptr, per.data(), &v) == MCL_OK);
    CHECK(v.n_valid == 64 && v.n_candidates == 16 && v.n_gated == 16 && v.inconsistent == 0);
    for (int b = 0; b < 64; ++b) CHECK(per[b].gated == (b < 16 ? 1 : 0) && per[b].valid == 1);
    CHECK(per[0].nu == -4.0 && per[0].var == 0.0 && per[0].nis == 16.0 / (sigma * sigma) && per[0].support == 0.0);
    beams[16] = cand;
    CHECK(innovation_gate_impl(beams.data(), 64, sigma, nullptr, per.data(), &v) == MCL_OK);
    CHECK(v.n_candidates == 17 && v.n_gated == 0 && v.inconsistent == 1);
    for (int b = 0; b < 64; ++b) CHECK(per[b].gated == 0);
    CHECK(innovation_gate_impl(beams.data(), 64, sigma, nullptr, nullptr, &v) == MCL_OK && v.inconsistent == 1);   // no per-beam array
    beams.assign(64, none);
    CHECK(innovation_gate_impl(beams.data(), 64, sigma, nullptr, per.data(), &v) == MCL_OK);
    CHECK(v.n_valid == 0 && v.n_gated == 0 && v.inconsistent == 0 && v.mean_nu == 0.0 && v.nis_sum == 0.0 && per[63].valid == 0);
  }
  {
    // the largest legal sums: 2^15 residuals of +-2^24
    std::vector<long long> q(INNOV_MAX_N, INNOV_Q_MAX);
    mcl_innovation_beam top = record_of(q, 0);
    mcl_innovation_derived d;
    CHECK(top.s2 == (1ull << 63) && top.s1 == (1ll << 39) && innov_legal(top));
    CHECK(innovation_gate_impl(&top, 1, sigma, nullptr, &d, &v) == MCL_OK && d.var == 0.0 && d.nu == 4096.0);
    for (size_t k = 0; k < q.size(); k += 2) q[k] = -INNOV_Q_MAX;
    top = record_of(q, 0);
    CHECK(top.s2 == (1ull << 63) && top.s1 == 0 && innov_legal(top));
    CHECK(innovation_gate_impl(&top, 1, sigma, nullptr, &d, &v) == MCL_OK && d.var == 16777216.0 && d.nu == 0.0 && d.nis == 0.0);
    // one more sample cannot be added
    const mcl_innovation_beam one = record_of(std::vector<long long>(1, 1), 1);
    const mcl_innovation_beam two[2] = {top, one};
    mcl_innovation_beam out;
    CHECK(innovation_merge_impl(two, 2, 1, &out) == MCL_ERR_INVALID);
  }
  // ---- records that are no sums are refused, by the gate and by the merge
  {
    const mcl_innovation_beam bad[] = {{-1, 0, 0, 0, 0}, {INNOV_MAX_N + 1, 0, 0, 0, 0}, {10, 11, 0, 0, 0}, {10, 0, 11, 0, 0},
                                       {10, 0, 0, 10 * INNOV_Q_MAX + 1, 10ull << 48}, {10, 0, 0, 0, (10ull << 48) + 1},
                                       {10, 0, 0, 100, 999}, {0, 0, 0, 1, 1}, {10, -1, 0, 0, 0}, {1, 0, 0, INT64_MIN, 1ull << 48},
                                       {1, 0, 0, INT64_MAX, ~0ull}};
    for (const mcl_innovation_beam& r : bad) {
      mcl_innovation_beam out;
      CHECK(!innov_legal(r) && innovation_gate_impl(&r, 1, sigma, nullptr, nullptr, &v) == MCL_ERR_INVALID);
      CHECK(innovation_merge_impl(&r, 1, 1, &out) == MCL_ERR_INVALID);
    }
    for (double s : {0.0, -1.0, nan, inf}) CHECK(innovation_gate_impl(&clean, 1, s, nullptr, nullptr, &v) == MCL_ERR_INVALID);
    for (mcl_innovation_gate_config c : {mcl_innovation_gate_config{-1.0, 0.01, 0.25}, mcl_innovation_gate_config{nan, 0.01, 0.25},
                                         mcl_innovation_gate_config{10.0, 1.5, 0.25}, mcl_innovation_gate_config{10.0, 0.01, nan}})
      CHECK(innovation_gate_impl(&clean, 1, sigma, &c, nullptr, &v) == MCL_ERR_INVALID);
    CHECK(innovation_gate_impl(nullptr, 1, sigma, nullptr, nullptr, &v) == MCL_ERR_INVALID);
    CHECK(innovation_gate_impl(&clean, 1, sigma, nullptr, nullptr, nullptr) == MCL_ERR_INVALID);
    CHECK(innovation_gate_impl(&clean, 0, sigma, nullptr, nullptr, &v) == MCL_ERR_INVALID);
  }
  // ---- random records: the variance's numerator against a restatement from the residuals themselves, the merge of any
  // split against the whole
  for (int k = 0; k < 300; ++k) {
    const int n = 1 + (int)(rng() % 2000);
    const long long scale = 1ll << (rng() % 25);
    std::vector<long long> q(n);
    for (long long& x : q) x = (long long)(rng() % (uint64_t)(2 * scale + 1)) - scale;
    const mcl_innovation_beam r = record_of(q, 0);
    mcl_innovation_derived d;
    CHECK(innov_legal(r) && innovation_gate_impl(&r, 1, sigma, nullptr, &d, &v) == MCL_OK);
    long double mean = 0, var = 0;
    for (long long x : q) mean += (long double)x;
    mean /= n;
    for (long long x : q) var += ((long double)x - mean) * ((long double)x - mean);
    var = var / n / 16777216.0L;
    CHECK(d.var >= 0.0 && std::fabs((long double)d.var - var) <= 1e-9L * (var + 1e-12L) + 1e-18L);
    CHECK(std::fabs((long double)d.nu - mean / 4096.0L) <= 1e-12L * (std::fabs(mean) + 1.0L));
    const int cut = (int)(rng() % (uint64_t)(n + 1));
    const mcl_innovation_beam parts[2] = {record_of(std::vector<long long>(q.begin(), q.begin() + cut), 0),
                                          record_of(std::vector<long long>(q.begin() + cut, q.end()), 0)};
    mcl_innovation_beam whole;
    CHECK(innovation_merge_impl(parts, 2, 1, &whole) == MCL_OK && std::memcmp(&whole, &r, sizeof r) == 0);
  }
  {
    // B beams x parts, heap arrays of the exact size
    const int B = 7, P = 3;
    std::vector<mcl_innovation_beam> parts((size_t)B * P, clean), out(B);
    CHECK(innovation_merge_impl(parts.data(), P, B, out.data()) == MCL_OK && out[B - 1].n == 300 && out[0].n_within == 300);
    CHECK(innovation_merge_impl(nullptr, P, B, out.data()) == MCL_ERR_INVALID && innovation_merge_impl(parts.data(), P, B, nullptr) == MCL_ERR_INVALID);
    CHECK(innovation_merge_impl(parts.data(), 0, B, out.data()) == MCL_ERR_INVALID && innovation_merge_impl(parts.data(), P, 0, out.data()) == MCL_ERR_INVALID);
  }
  std::printf("innovation_driver: ok\n");
  return 0;
}
