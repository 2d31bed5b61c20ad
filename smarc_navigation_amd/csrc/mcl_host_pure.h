// mcl_host_pure.h -- the host arithmetic of libmcl_hip.so that touches no device: tf.transformations' Euler /
// quaternion formulas, Philox on the host, the resample exchange's transfer plan, matrix_from_tf, the merge of shards'
// weight statistics, and the safety bounds kernels rely on unchecked (steepest patch gradient of a height grid, landmark
// gate radius, the box of the uniform draws, the range update's beam table, which measured ranges count (beam_valid),
// the lattice of mcl_pose_modes, the bytes of mcl_history_enable and mcl_drift_enable, the stds of mcl_drift_config, the pose arguments of the acoustic updates and
// mcl_history_bracket), and the lattice, predicate
// and round plan of mcl_temper (also run by its pick kernel: MCL_HD), and the rules, bandwidth and factor of
// mcl_regularise (the factor also run by its kernel), and the keys, threshold, predicate,
// start and bin choice of mcl_cloud_quantiles (include/mcl_quantile.h; the kernels run the same functions), and the
// quantised residual, sample, merge and gate of mcl_ping_innovation (include/mcl_innovation.h), and the quantised
// difference, steps, merge and matrix of mcl_ping_information (include/mcl_information.h), and the compare, solve, checks
// and derived quantities of mcl_match_ping (include/mcl_match.h; its kernel runs the first two), and the checks, the rank
// and the selection of mcl_reseed.h (its kernel runs the rank).  No HIP header: the
// translation unit mcl_api.hip includes it through mcl_host.h, and `make host-asan` compiles it -- with mcl_dr_impl.h and
// the node's core -- under AddressSanitizer / UBSan / ThreadSanitizer with plain g++ (the reference is racy
// by construction, auv_pf.py:126,202-211,264-285; GPU sanitizers are not available on this pool).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mcl.h"
#include "../../include/mcl_recovery.h"
#include "../../include/mcl_modes.h"
#include "../../include/mcl_history.h"
#include "../../include/mcl_acoustic.h"
#include "../../include/mcl_temper.h"
#include "../../include/mcl_drift.h"
#include "../../include/mcl_regularise.h"
#include "../../include/mcl_quantile.h"
#include "../../include/mcl_innovation.h"
#include "../../include/mcl_information.h"
#include "../../include/mcl_match.h"
#include "../../include/mcl_swath.h"
#include "../../include/mcl_reseed.h"

namespace {

typedef unsigned int u32_host;

// euler_from_quaternion(q,'sxyz') -- tf.transformations' published algorithm (auv_particle.py:50)
void euler_from_quat(const double qin[4], double rpy[3]) {
  double nq = qin[0] * qin[0] + qin[1] * qin[1] + qin[2] * qin[2] + qin[3] * qin[3];
  double M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (nq >= 2.220446049250313e-16 * 4.0) {
    double s = std::sqrt(2.0 / nq);
    double q[4] = {qin[0] * s, qin[1] * s, qin[2] * s, qin[3] * s};
    double o[4][4];
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b) o[a][b] = q[a] * q[b];
    M[0] = 1.0 - o[1][1] - o[2][2];
    M[1] = o[0][1] - o[2][3];
    M[2] = o[0][2] + o[1][3];
    M[3] = o[0][1] + o[2][3];
    M[4] = 1.0 - o[0][0] - o[2][2];
    M[5] = o[1][2] - o[0][3];
    M[6] = o[0][2] - o[1][3];
    M[7] = o[1][2] + o[0][3];
    M[8] = 1.0 - o[0][0] - o[1][1];
  }
  double cy = std::sqrt(M[0] * M[0] + M[3] * M[3]);
  if (cy > 2.220446049250313e-16 * 4.0) {
    rpy[0] = std::atan2(M[7], M[8]);
    rpy[1] = std::atan2(-M[6], cy);
    rpy[2] = std::atan2(M[3], M[0]);
  } else {
    rpy[0] = std::atan2(-M[5], M[4]);
    rpy[1] = std::atan2(-M[6], cy);
    rpy[2] = 0.0;
  }
}

void philox_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t o[4]) {
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0;
  o[1] = c1;
  o[2] = c2;
  o[3] = c3;
}
uint64_t native_u53(uint64_t seed, uint32_t step) {
  uint32_t o[4];
  philox_host(0xFFFFFFFFu, 0u, step, 3u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
  return ((uint64_t)(o[0] >> 5) << 26) | (uint64_t)(o[1] >> 6);
}

int ceil_log2(long long n) {
  int l = 0;
  while ((1ll << l) < n) ++l;
  return l;
}


// the range of global dupes positions that shard `from` holds and shard `to` needs: [lo, hi).  Lpre / Spre: exclusive
// prefix sums of the shards' lost-slot and surplus-copy counts (world + 1 entries).  Pure host arithmetic: also what
// mcl_exchange_plan exposes, so the plan is property-tested without a GPU (tests/test_exchange_plan.py).
void plan_range(const u32_host* Lpre, const u32_host* Spre, int from, int to, u32_host& lo, u32_host& hi) {
  lo = std::max(Spre[from], Lpre[to]);
  hi = std::min(Spre[from + 1], Lpre[to + 1]);
  if (hi < lo) hi = lo;
}

// mcl_exchange_plan (include/mcl.h): what `rank` sends to / receives from each peer
int exchange_plan_impl(int32_t world, const uint32_t* lost, const uint32_t* surplus, int32_t rank, uint32_t* send_off,
                       uint32_t* send_cnt, uint32_t* recv_off, uint32_t* recv_cnt) {
  if (world < 1 || !lost || !surplus || rank < 0 || rank >= world || !send_off || !send_cnt || !recv_off || !recv_cnt)
    return MCL_ERR_INVALID;
  std::vector<u32_host> Lpre((size_t)world + 1, 0u), Spre((size_t)world + 1, 0u);
  unsigned long long tl = 0, ts = 0;
  for (int r = 0; r < world; ++r) {
    tl += lost[r];
    ts += surplus[r];
    if (tl > 0xffffffffull || ts > 0xffffffffull) return MCL_ERR_INVALID;
    Lpre[r + 1] = (u32_host)tl;
    Spre[r + 1] = (u32_host)ts;
  }
  if (tl != ts) return MCL_ERR_INVALID;   // every lost slot takes exactly one surplus copy
  for (int r = 0; r < world; ++r) {
    u32_host lo, hi;
    plan_range(Lpre.data(), Spre.data(), rank, r, lo, hi);   // what `rank` holds and r needs
    send_off[r] = lo - Spre[rank];
    send_cnt[r] = hi - lo;
    plan_range(Lpre.data(), Spre.data(), r, rank, lo, hi);   // what r holds and `rank` needs
    recv_off[r] = lo - Lpre[rank];
    recv_cnt[r] = hi - lo;
  }
  return MCL_OK;
}

// n_eff and log_mean_lik of mcl_wstats from its sums: the ONE place that forms them (mcl_weight_stats and the merge)
void wstats_finish(mcl_wstats* s) {
  const bool any = s->argmax_gid >= 0 && s->sum_w2 > 0.0;
  s->n_eff = any ? (s->sum_w * s->sum_w) / s->sum_w2 : 0.0;
  s->log_mean_lik = any && s->n > 0 ? s->max_lw + std::log(s->sum_w / (double)s->n) : -INFINITY;
}

// mcl_weight_stats_merge (include/mcl_recovery.h): statistics of the union of the parts, in the order given
int weight_stats_merge_impl(const mcl_wstats* parts, int32_t n_parts, mcl_wstats* out) {
  if (!parts || !out || n_parts < 1) return MCL_ERR_INVALID;
  int win = -1;   // the part that holds the maximum: the largest max_lw, the lowest id among equal ones
  for (int p = 0; p < n_parts; ++p) {
    if (parts[p].n < 0 || parts[p].n_live < 0 || parts[p].n_live > parts[p].n) return MCL_ERR_INVALID;
    if (parts[p].argmax_gid < 0) continue;   // nothing finite in this part
    if (win < 0 || parts[p].max_lw > parts[win].max_lw ||
        (parts[p].max_lw == parts[win].max_lw && parts[p].argmax_gid < parts[win].argmax_gid))
      win = p;
  }
  mcl_wstats r;
  r.n = r.n_live = 0;
  r.argmax_gid = -1;
  r.max_lw = -INFINITY;
  r.sum_w = r.sum_w2 = 0.0;
  for (int c = 0; c < 6; ++c) r.map_pose[c] = 0.0;
  if (win >= 0) {
    r.argmax_gid = parts[win].argmax_gid;
    r.max_lw = parts[win].max_lw;
    for (int c = 0; c < 6; ++c) r.map_pose[c] = parts[win].map_pose[c];
  }
  for (int p = 0; p < n_parts; ++p) {
    r.n += parts[p].n;
    r.n_live += parts[p].n_live;
    if (parts[p].argmax_gid < 0) continue;
    const double f = std::exp(parts[p].max_lw - r.max_lw);   // (exactly 1 for the winning part)
    r.sum_w += parts[p].sum_w * f;
    r.sum_w2 += parts[p].sum_w2 * (f * f);
  }
  wstats_finish(&r);
  *out = r;
  return MCL_OK;
}

// Particle.matrix_from_tf (auv_particle.py:110-125): 4 x 4 from translation + quaternion (quaternion_matrix of
// tf.transformations: scale by sqrt(2 / |q|^2), outer product)
int matrix_from_tf_impl(const double translation[3], const double quaternion[4], double m16[16]) {
  if (!translation || !quaternion || !m16) return MCL_ERR_INVALID;
  const double* qi = quaternion;
  const double nq = qi[0] * qi[0] + qi[1] * qi[1] + qi[2] * qi[2] + qi[3] * qi[3];
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (nq >= 2.220446049250313e-16 * 4.0) {
    const double s = std::sqrt(2.0 / nq);
    const double q[4] = {qi[0] * s, qi[1] * s, qi[2] * s, qi[3] * s};
    double o[4][4];
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b) o[a][b] = q[a] * q[b];
    R[0] = 1.0 - o[1][1] - o[2][2];
    R[1] = o[0][1] - o[2][3];
    R[2] = o[0][2] + o[1][3];
    R[3] = o[0][1] + o[2][3];
    R[4] = 1.0 - o[0][0] - o[2][2];
    R[5] = o[1][2] - o[0][3];
    R[6] = o[0][2] - o[1][3];
    R[7] = o[1][2] + o[0][3];
    R[8] = 1.0 - o[0][0] - o[1][1];
  }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) m16[r * 4 + c] = R[r * 3 + c];
    m16[r * 4 + 3] = translation[r];
  }
  m16[12] = m16[13] = m16[14] = 0.0;
  m16[15] = 1.0;
  return MCL_OK;
}

// ---- safety bounds: each of them says how far something can reach, and a kernel relies on it unchecked

// steepest gradient of the bilinear patches of a height grid (z[ix * ny + iy], node spacing res): the fan sweep's tilt
// bound.  A patch's x slope lies between those of the cell's two x edges, its y slope between those of the two y edges.
double grid_slope_max(const float* z, int nx, int ny, double res) {
  double g2 = 0.0;
  for (int ix = 0; ix + 1 < nx; ++ix)
    for (int iy = 0; iy + 1 < ny; ++iy) {
      const size_t k = (size_t)ix * ny + iy;
      const double h00 = z[k], h01 = z[k + 1], h10 = z[k + ny], h11 = z[k + ny + 1];
      const double ax = std::max(std::fabs(h10 - h00), std::fabs(h11 - h01));
      const double ay = std::max(std::fabs(h01 - h00), std::fabs(h11 - h10));
      g2 = std::max(g2, ax * ax + ay * ay);
    }
  return std::sqrt(g2) / res;
}

// largest eigenvalue bound of a symmetric 3x3 (xx xy xz yy yz zz): Gershgorin
double sym3_lam_bound(const double* s) {
  const double r0 = s[0] + std::fabs(s[1]) + std::fabs(s[2]), r1 = s[3] + std::fabs(s[1]) + std::fabs(s[4]),
               r2 = s[5] + std::fabs(s[2]) + std::fabs(s[4]);
  return std::max(r0, std::max(r1, r2));
}
double sym3_det(const double* s) {
  return s[0] * (s[3] * s[5] - s[4] * s[4]) - s[1] * (s[1] * s[5] - s[4] * s[2]) + s[2] * (s[1] * s[4] - s[3] * s[2]);
}
// measurement covariance of a landmark update: the Q of mcl_set_landmark_noise (q_set; nullptr: none given), else sigma^2 I
void landmark_q(const double* q_set, double sigma, double Q[6]) {
  for (int k = 0; k < 6; ++k) Q[k] = q_set ? q_set[k] : 0.0;
  if (!q_set) Q[0] = Q[3] = Q[5] = sigma * sigma;
}
// every landmark inside the gate lies within this distance of the detection: d^2 >= |nu|^2 / lambda_max(S), with
// lambda_max(S) <= lam_cov_max + lambda_max(Q) in Mahalanobis mode (maha) and S = sigma^2 I otherwise.  The landmark cell
// grid is built for this radius: a smaller one would let the kernels miss a gated landmark.
double landmark_gate_radius(bool maha, double lam_cov_max, const double Q[6], double sigma, double gate) {
  if (!maha) return sigma * std::sqrt(gate);
  return std::sqrt(gate * (lam_cov_max + sym3_lam_bound(Q)));
}

// the box of mcl_init_particles_uniform / mcl_inject_uniform against its own rules and, in the map frame, against the
// map -> odom transform m2o (rows of a 3 x 4): MCL_OK, or the status with *reason saying which rule
int check_box(const mcl_box* box, const double m2o[12], const char** reason) {
  const double b[6] = {box->x_min, box->x_max, box->y_min, box->y_max, box->yaw_min, box->yaw_max};
  *reason = nullptr;
  for (int c = 0; c < 3 && !*reason; ++c) {
    if (!std::isfinite(b[2 * c]) || !std::isfinite(b[2 * c + 1])) *reason = "a bound of the box is not finite";
    else if (b[2 * c + 1] < b[2 * c]) *reason = "a maximum of the box lies below its minimum";
  }
  if (!*reason && box->yaw_max - box->yaw_min > 2.0 * 3.14159265358979323846) *reason = "the yaw interval is longer than 2 pi";
  if (!*reason && box->frame != MCL_FRAME_ODOM && box->frame != MCL_FRAME_MAP) *reason = "unknown frame";
  if (*reason) return MCL_ERR_INVALID;
  if (box->frame == MCL_FRAME_MAP &&
      (std::fabs(m2o[2]) > 1e-12 || std::fabs(m2o[6]) > 1e-12 || std::fabs(m2o[8]) > 1e-12 || std::fabs(m2o[9]) > 1e-12 ||
       std::fabs(m2o[10] - 1.0) > 1e-12)) {
    *reason = "a box in the map frame needs an m2o that turns about z alone";
    return MCL_ERR_UNSUPPORTED;
  }
  return MCL_OK;
}

// the lattice of mcl_pose_modes against its rules (include/mcl_modes.h): MCL_OK and *n_cells = nx ny n_yaw, or
// MCL_ERR_INVALID with *reason saying which rule.  The histogram kernels index u32 arrays of n_cells words with the cell
// ids this admits, unchecked.
int mode_grid_check_impl(const mcl_mode_grid* g, int64_t* n_cells, const char** reason) {
  const char* why = nullptr;
  if (!g) why = "null grid";
  else if (!std::isfinite(g->cell) || !(g->cell > 0.0)) why = "cell must be finite and > 0";
  else if (!std::isfinite(g->x0) || !std::isfinite(g->y0)) why = "x0 or y0 is not finite";
  else if (g->nx < 1 || g->ny < 1 || g->n_yaw < 1) why = "nx, ny and n_yaw must be >= 1";
  else if (g->n_yaw > MCL_MODES_MAX_YAW) why = "n_yaw > 64";
  else if ((int64_t)g->nx * (int64_t)g->ny > MCL_MODES_MAX_CELLS ||   // (each factor < 2^31: neither product overflows)
           (int64_t)g->nx * (int64_t)g->ny * (int64_t)g->n_yaw > MCL_MODES_MAX_CELLS)
    why = "more than 2^24 cells";
  if (reason) *reason = why;
  if (why) return MCL_ERR_INVALID;
  if (n_cells) *n_cells = (int64_t)g->nx * (int64_t)g->ny * (int64_t)g->n_yaw;
  return MCL_OK;
}

// the device bytes mcl_history_enable allocates (include/mcl_history.h): depth frames of n x (u32 parent + 3 doubles), two
// link and two count buffers of n x u32, HISTORY_RES_WORDS result doubles per frame, HISTORY_PART_WORDS reduction records
// (mcl_host_history.h checks both constants against the kernels').  n <= 2^31 - 1 and depth <= 1024 cannot overflow 64 bits.
constexpr int64_t HISTORY_RES_WORDS = 10, HISTORY_PART_WORDS = 8 * 2048;
int history_bytes_impl(int64_t n, int32_t depth, int64_t* bytes) {
  if (!bytes || n < 1 || n > 0x7fffffffll || depth < 1 || depth > MCL_HISTORY_MAX_DEPTH) return MCL_ERR_INVALID;
  *bytes = 28 * n * (int64_t)depth + 16 * n + 8 * HISTORY_RES_WORDS * (int64_t)depth + 8 * HISTORY_PART_WORDS;
  return MCL_OK;
}

// the device bytes mcl_drift_enable allocates (include/mcl_drift.h): three doubles per particle, DRIFT_PART_WORDS reduction
// records and DRIFT_RESULT_WORDS result words (mcl_host_drift.h checks both constants against the kernels')
constexpr int64_t DRIFT_RESULT_WORDS = 12, DRIFT_PART_WORDS = 9 * 2048;
int drift_bytes_impl(int64_t n, int64_t* bytes) {
  if (!bytes || n < 1 || n > 0x7fffffffll) return MCL_ERR_INVALID;
  *bytes = 24 * n + 8 * DRIFT_PART_WORDS + 8 * DRIFT_RESULT_WORDS;
  return MCL_OK;
}
// the stds of a drift configuration: every one finite and >= 0; *reason names the first that is not
int drift_config_check_impl(const mcl_drift_config* cfg, const char** reason) {
  static const char* const bad[6] = {"init_std[0] (cx) must be finite and >= 0", "init_std[1] (cy) must be finite and >= 0",
                                     "init_std[2] (bw) must be finite and >= 0", "walk_std[0] (cx) must be finite and >= 0",
                                     "walk_std[1] (cy) must be finite and >= 0", "walk_std[2] (bw) must be finite and >= 0"};
  const char* why = nullptr;
  if (!cfg) why = "null config";
  for (int c = 0; c < 6 && !why; ++c) {
    const double s = c < 3 ? cfg->init_std[c] : cfg->walk_std[c - 3];
    if (!std::isfinite(s) || !(s >= 0.0)) why = bad[c];
  }
  if (reason) *reason = why;
  return why ? MCL_ERR_INVALID : MCL_OK;
}

// the pose arguments the acoustic updates share (include/mcl_acoustic.h), as far as they need no handle: nullptr, or the
// rule that is broken
const char* acoustic_pose_check(const double offset[3], const double zrp[3], int lag, double frac) {
  if (lag < -1) return "lag below -1";
  if (!(frac >= 0.0 && frac < 1.0)) return "frac outside [0, 1)";
  if (lag < 0 && frac > 0.0) return "frac > 0 needs a lag";
  if (lag >= 0 && !zrp) return "a lagged update needs zrp (frames hold x, y, yaw only)";
  for (int k = 0; k < 3; ++k) {
    if (offset && !std::isfinite(offset[k])) return "offset is not finite";
    if (zrp && !std::isfinite(zrp[k])) return "zrp is not finite";
  }
  return nullptr;
}

// mcl_history_bracket (include/mcl_acoustic.h): where `stamp` falls among the frames' stamps, newest first
int history_bracket_impl(const double* s, int32_t held, double stamp, int32_t* lag, double* frac, int32_t* where) {
  if (!s || !lag || !frac || !where || held < 1 || !std::isfinite(stamp)) return MCL_ERR_INVALID;
  for (int32_t k = 0; k < held; ++k)
    if (!std::isfinite(s[k]) || (k > 0 && !(s[k - 1] > s[k]))) return MCL_ERR_INVALID;
  *frac = 0.0;
  if (stamp >= s[0]) {
    *lag = 0;
    *where = 1;
    return MCL_OK;
  }
  if (stamp <= s[held - 1]) {
    *lag = held - 1;
    *where = -1;
    return MCL_OK;
  }
  int32_t k = 0;
  while (!(stamp > s[k + 1])) ++k;   // (s[held - 1] < stamp < s[0]: k + 1 <= held - 1)
  const double f = (s[k] - stamp) / (s[k] - s[k + 1]);
  *lag = k;
  *frac = f < 1.0 ? f : std::nextafter(1.0, 0.0);   // (both differences may round to the same number)
  *where = 0;
  return MCL_OK;
}

// (functions the kernels run too -- one statement of each rule -- are MCL_HD)
#if defined(__HIPCC__)
#define MCL_HD __host__ __device__
#else
#define MCL_HD
#endif
// A measured range counts in a likelihood when it is positive; zero, negative and NaN mark a beam without a return.  The
// one statement of the rule: the cast, slice and range kernels, and the host's beam table of the fan sweep.
MCL_HD inline bool beam_valid(float range) { return range > 0.f; }

// beam table of a range update: B directions normalised in fp64, then rounded; out[4 b ...] = unit x, y, z and the
// measured range (0 without ranges).  A zero or non-finite direction is refused.
int normalise_beams(const float* dirs, const float* ranges, int B, float* out) {
  for (int b = 0; b < B; ++b) {
    const double x = dirs[3 * b], y = dirs[3 * b + 1], z = dirs[3 * b + 2];
    const double nrm = std::sqrt(x * x + y * y + z * z);
    if (!(nrm > 0.0) || !std::isfinite(nrm)) return MCL_ERR_INVALID;
    out[4 * b] = (float)(x / nrm);
    out[4 * b + 1] = (float)(y / nrm);
    out[4 * b + 2] = (float)(z / nrm);
    out[4 * b + 3] = ranges ? ranges[b] : 0.f;
  }
  return MCL_OK;
}

// ---- ESS-targeted tempering (include/mcl_temper.h): the exponent lattice, the pass predicate and the round plan.  The
// pick kernel (csrc/mcl_temper.h) runs these very functions on the device: one statement of each rule.
// beta_j = T[j mod 64] 2^-(j div 64), T[i] = the correctly rounded double of 2^(-i / 64), written with the 17 digits
// that name one double (no hexadecimal literals: `make host-asan` compiles this file as C++14); 0 <= j <= 2048 (unchecked)
MCL_HD inline double temper_beta(int j) {
  constexpr double T[64] = {
      1, 0.98922801319397546, 0.97857206208770009, 0.96803089674614717,
      0.9576032806985737, 0.9472879907934828, 0.93708381705514998, 0.92698956254169274,
      0.91700404320467122, 0.90712608775019943, 0.89735453750155358, 0.88768824626326059,
      0.87812608018664973, 0.86866691763685311, 0.85930964906123897, 0.85005317685926174,
      0.8408964152537145, 0.83183829016336819, 0.82287773907698247, 0.81401371092867392,
      0.80524516597462714, 0.7965710756711335, 0.78799042255394325, 0.77950220011891846,
      0.77110541270397037, 0.76279907537226921, 0.75458221379671142, 0.74645386414563242,
      0.73841307296974967, 0.73045889709032352, 0.72259040348852333, 0.71480666919598501,
      0.70710678118654757, 0.69948983626915562, 0.69195494098191601, 0.68450121148729526,
      0.67712777346844633, 0.66983376202665146, 0.66261832157987066, 0.65548060576238221,
      0.64841977732550482, 0.64143500803938913, 0.63452547859586661, 0.62769037851234555,
      0.620928906036742, 0.61424026805343501, 0.60762367999023448, 0.60107836572635154,
      0.59460355750136051, 0.58819849582514061, 0.58186242938878874, 0.57559461497649134,
      0.56939431737834578, 0.56326080930412092, 0.55719337129794622, 0.55119129165392045,
      0.54525386633262884, 0.53938039887855993, 0.53357020033841185, 0.52782258918027858,
      0.52213689121370688, 0.51651243951061421, 0.51094857432705831, 0.50544464302585024};
  // (T[i] in (1/2, 1] and j div 64 <= 32: the product with a power of two >= 2^-32 is exact)
  return T[j & 63] * (1.0 / (double)(1ull << (j >> 6)));
}
// s1^2 >= n_t s2 2^32 in 128 bits, for every s1, s2 and n_t >= 1: a right side of 2^128 or more cannot pass
MCL_HD inline bool temper_pass(unsigned long long s1, unsigned long long s2, unsigned long long n_t) {
  typedef unsigned __int128 u128;
  const u128 lhs = (u128)s1 * s1;
  const u128 p = (u128)n_t * s2;
  if ((unsigned long long)(p >> 96) != 0ull) return false;
  return lhs >= (p << 32);
}
// the candidates of a round (include/mcl_temper.h) are base + step k, k < count; count -1: bad argument
struct TemperPlan {
  int base, step, count;
};
MCL_HD inline TemperPlan temper_plan(int round, int j_prev) {
  const TemperPlan bad = {0, 0, -1}, none = {0, 0, 0};
  if (round == 1) return TemperPlan{0, 128, 17};
  if (j_prev < 0 || j_prev > MCL_TEMPER_LEVELS) return bad;
  if (round == 2) return j_prev % 128 != 0 ? bad : (j_prev == 0 ? none : TemperPlan{j_prev - 120, 8, 15});
  if (round == 3) return j_prev % 8 != 0 ? bad : (j_prev == 0 ? none : TemperPlan{j_prev - 7, 1, 7});
  return bad;
}
// what a round's outcome means: first = the level of its first passing candidate (-1: none passed)
struct TemperStep {
  int j, done, floor_hit;
};
MCL_HD inline TemperStep temper_next(int round, int j_prev, int first) {
  TemperStep r;
  r.floor_hit = 0;
  if (round == 1) {
    r.j = first < 0 ? MCL_TEMPER_LEVELS : first;
    r.floor_hit = first < 0 ? 1 : 0;
    r.done = (first < 0 || r.j == 0) ? 1 : 0;
  } else {
    r.j = first < 0 ? j_prev : first;
    r.done = round == 3 ? 1 : 0;
  }
  return r;
}
int temper_beta_impl(int32_t j, double* beta) {
  if (!beta || j < 0 || j > MCL_TEMPER_LEVELS) return MCL_ERR_INVALID;
  *beta = temper_beta(j);
  return MCL_OK;
}
int temper_pass_impl(uint64_t s1, uint64_t s2, int64_t n_target, int32_t* pass) {
  if (!pass || n_target < 1) return MCL_ERR_INVALID;
  *pass = temper_pass(s1, s2, (unsigned long long)n_target) ? 1 : 0;
  return MCL_OK;
}
int temper_candidates_impl(int32_t round, int32_t j_prev, int32_t* cand, int32_t* n_cand) {
  if (!cand || !n_cand) return MCL_ERR_INVALID;
  const TemperPlan p = temper_plan(round, j_prev);
  if (p.count < 0) return MCL_ERR_INVALID;
  for (int k = 0; k < p.count; ++k) cand[k] = p.base + p.step * k;
  *n_cand = p.count;
  return MCL_OK;
}
// the search over sums somebody else forms (mcl_group_temper): sums(cand, nc, s1, s2) fills the CLOUD's sums at the
// candidates; the rounds, the first pass and temper_next exactly as the pick kernel runs them
template <class Sums>
int temper_search(long long n_target, Sums&& sums, int* j_out, int* floor_hit, int* levels) {
  int j = 0;
  *levels = 0;
  *floor_hit = 0;
  for (int round = 1; round <= 3; ++round) {
    const TemperPlan p = temper_plan(round, j);
    int32_t cand[MCL_TEMPER_MAX_CAND];
    uint64_t s1[MCL_TEMPER_MAX_CAND], s2[MCL_TEMPER_MAX_CAND];
    for (int k = 0; k < p.count; ++k) cand[k] = p.base + p.step * k;
    if (p.count > 0) {
      const int rc = sums(cand, p.count, s1, s2);
      if (rc != MCL_OK) return rc;
    }
    int first = -1;
    for (int k = p.count - 1; k >= 0; --k)
      if (temper_pass(s1[k], s2[k], (unsigned long long)n_target)) first = cand[k];
    const TemperStep st = temper_next(round, j, first);
    j = st.j;
    *levels += p.count;
    *floor_hit |= st.floor_hit;
    if (st.done) break;
  }
  *j_out = j;
  return MCL_OK;
}

// ---- regularised resampling (include/mcl_regularise.h): the configuration's rules, the bandwidth, and the factor of the
// cloud's covariance.  The factor kernel (csrc/mcl_regularise.h) runs reg_factor itself: one statement of the rule.
constexpr int REG_MAX_DIMS = 6, REG_MAX_PACKED = 21;
MCL_HD inline int reg_packed(int r, int c) { return r * (r + 1) / 2 + c; }   // (r >= c)
MCL_HD inline bool reg_dims_ok(int dims) { return dims == 3 || dims == 6; }
// C, L packed lower-triangular, D (D + 1) / 2 words; returns the dead mask.  Every product, sum, quotient and root is an
// operation of its own (no contraction), k increasing: a restatement in any language gives the same bits.
MCL_HD inline int reg_factor(const double* C, int D, double* L) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int dead = 0;
  for (int j = 0; j < D; ++j) {
    const double cjj = C[reg_packed(j, j)];
    double p = cjj;
    for (int k = 0; k < j; ++k) {
      const double l = L[reg_packed(j, k)];
      const double q = l * l;
      p = p - q;
    }
    const double floor_ = cjj * (1.0 / 67108864.0);   // 2^-26, exact
    if (p > floor_) {                                 // (false for NaN and for C_jj <= 0)
      const double d = sqrt(p);
      L[reg_packed(j, j)] = d;
      for (int i = j + 1; i < D; ++i) {
        double t = C[reg_packed(i, j)];
        for (int k = 0; k < j; ++k) {
          const double q = L[reg_packed(i, k)] * L[reg_packed(j, k)];
          t = t - q;
        }
        L[reg_packed(i, j)] = t / d;
      }
    } else {
      dead |= 1 << j;
      for (int i = j; i < D; ++i) L[reg_packed(i, j)] = 0.0;
    }
  }
  return dead;
}
int regularise_factor_impl(const double* cov, int32_t dims, double* chol, int32_t* dead) {
  if (!cov || !chol || !dead || !reg_dims_ok(dims)) return MCL_ERR_INVALID;
  double c[REG_MAX_PACKED], l[REG_MAX_PACKED];   // (cov and chol may be the same array)
  const int np = dims * (dims + 1) / 2;
  for (int k = 0; k < np; ++k) c[k] = cov[k];
  *dead = reg_factor(c, dims, l);
  for (int k = 0; k < np; ++k) chol[k] = l[k];
  return MCL_OK;
}
const char* regularise_config_why(const mcl_regularise_config* cfg) {
  if (!cfg) return "null config";
  if (!std::isfinite(cfg->scale) || !(cfg->scale > 0.0)) return "scale must be finite and > 0";
  if (!reg_dims_ok(cfg->dims)) return "dims must be 3 (x, y, yaw) or 6 (x, y, yaw, cx, cy, bw)";
  return nullptr;
}
int regularise_config_check_impl(const mcl_regularise_config* cfg, const char** reason) {
  const char* why = regularise_config_why(cfg);
  if (reason) *reason = why;
  return why ? MCL_ERR_INVALID : MCL_OK;
}
// h0 = scale (4 / ((D + 2) n))^(1 / (D + 4)); shrink: h = min(h0, 1), a = sqrt(1 - h h)
int regularise_bandwidth_impl(int64_t n, int32_t dims, double scale, int32_t shrink, double* h, double* a) {
  if (!h || !a || n < 1 || !reg_dims_ok(dims) || !std::isfinite(scale) || !(scale > 0.0)) return MCL_ERR_INVALID;
  const double D = (double)dims;
  const double h0 = scale * std::pow(4.0 / ((D + 2.0) * (double)n), 1.0 / (D + 4.0));
  if (shrink) {
    *h = h0 < 1.0 ? h0 : 1.0;
    *a = std::sqrt(1.0 - *h * *h);
  } else {
    *h = h0;
    *a = 1.0;
  }
  return MCL_OK;
}

// ---- exact order statistics (include/mcl_quantile.h): the key of a value, the threshold of a probability, the 128-bit
// predicate, where the radix select starts and which bin a round picks.  The kernels (csrc/mcl_quantile.h) run quant_key,
// quant_reached and quant_start themselves; the host-driven shard search runs quant_pick_bin, whose rule -- the first bin
// whose cumulative mass reaches the threshold -- the pick kernel states once more across a wave.
constexpr int QUANT_ROUNDS = 8;   // bytes of a key
// key(v + 0.0): order-preserving, -0 and +0 one key (NaN: the callers exclude it)
MCL_HD inline unsigned long long quant_key(double v) {
  const double w = v + 0.0;
  unsigned long long b;
  __builtin_memcpy(&b, &w, sizeof b);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
MCL_HD inline double quant_value(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  __builtin_memcpy(&v, &b, sizeof v);
  return v;
}
// 2^32 mass >= P total in 128 bits: the left side is below 2^96, the right side below 2^128
MCL_HD inline bool quant_reached(unsigned long long mass, unsigned long long total, unsigned long long P) {
  typedef unsigned __int128 u128;
  return ((u128)mass << 32) >= (u128)P * (u128)total;
}
// the first round that has to run and the bytes above it, from the smallest and largest key of the used particles: the
// leading bytes both share are skipped, the last round always runs (it also finds S); no used particle (kmin > kmax): the
// last round alone, over nothing
struct QuantStart {
  int start;                   // 0 ... 7
  unsigned long long prefix;   // the key's leading `start` bytes
};
MCL_HD inline QuantStart quant_start(unsigned long long kmin, unsigned long long kmax) {
  QuantStart r = {QUANT_ROUNDS - 1, 0ull};
  if (kmin > kmax) return r;
  int s = 0;
  while (s < QUANT_ROUNDS - 1 && (kmin >> (56 - 8 * s)) == (kmax >> (56 - 8 * s))) ++s;
  r.start = s;
  r.prefix = s == 0 ? 0ull : kmin >> (64 - 8 * s);
  return r;
}
// the bin a round picks: the first d with reached(below + hist[0] + ... + hist[d]); -1: none (total = 0).  *cum = the
// cumulative mass up to and including the bin.
inline int quant_pick_bin(const uint64_t hist[256], uint64_t below, uint64_t total, uint64_t P, uint64_t* cum) {
  if (total == 0) return -1;
  uint64_t c = below;
  for (int d = 0; d < 256; ++d) {
    c += hist[d];
    if (quant_reached(c, total, P)) {
      *cum = c;
      return d;
    }
  }
  return -1;
}
int quantile_key_impl(double v, uint64_t* key) {
  if (!key || std::isnan(v)) return MCL_ERR_INVALID;
  *key = quant_key(v);
  return MCL_OK;
}
int quantile_value_impl(uint64_t key, double* v) {
  if (!v) return MCL_ERR_INVALID;
  *v = quant_value(key);
  return MCL_OK;
}
int quantile_threshold_impl(double p, uint64_t* P) {
  if (!P || !(p >= 1.0 / 4294967296.0 && p <= 1.0)) return MCL_ERR_INVALID;
  *P = (uint64_t)std::floor(p * 4294967296.0);   // (the scaling by 2^32 is exact; 1 <= P <= 2^32)
  return MCL_OK;
}
int quantile_reached_impl(uint64_t mass, uint64_t total, uint64_t P, int32_t* reached) {
  if (!reached) return MCL_ERR_INVALID;
  *reached = quant_reached(mass, total, P) ? 1 : 0;
  return MCL_OK;
}
// what every query has to satisfy before a handle is looked at: nullptr, or the rule that is broken
const char* quantile_query_why(const mcl_quantile_query* q) {
  if (!q) return "null query";
  if (q->quantity < MCL_Q_X || q->quantity > MCL_Q_RADIUS2) return "unknown quantity";
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(q->centre[k])) return "the centre is not finite";
  return nullptr;
}

// ---- ping innovation statistics (include/mcl_innovation.h): the quantised residual (the kernel, csrc/mcl_innovation.h,
// runs innov_quantise itself), the sample, the direction table, the legality of a record, its derived quantities, the
// merge and the gate.
constexpr long long INNOV_Q_MAX = 1ll << 24;
constexpr long long INNOV_MAX_N = MCL_INNOVATION_MAX_SAMPLES;
// q = rint((r - e) 2^12) clamped to +-2^24 (the bounds are integers: clamping first gives the same number, and keeps the
// conversion inside the integer's range whatever the measured range is)
MCL_HD inline long long innov_quantise(float r, float e) {
  double x = ((double)r - (double)e) * 4096.0;
  x = x < -16777216.0 ? -16777216.0 : (x > 16777216.0 ? 16777216.0 : x);
  return (long long)rint(x);
}
// |q| <= this counts in n_within
inline long long innov_q_support(double support_k, double sigma) {
  const double s = std::floor(support_k * sigma * 4096.0);
  return s >= 16777216.0 ? INNOV_Q_MAX : (long long)s;   // (the callers refuse NaN and negatives)
}
int innovation_sample_impl(int64_t n_global, int32_t max_samples, int64_t* stride, int64_t* count) {
  if (!stride || !count || n_global < 1 || max_samples < 1 || max_samples > MCL_INNOVATION_MAX_SAMPLES) return MCL_ERR_INVALID;
  const int64_t s = (n_global - 1) / max_samples + 1;
  *stride = s;
  *count = (n_global - 1) / s + 1;
  return MCL_OK;
}
// the slots of a shard [goff, goff + n) whose global id is a multiple of stride: first, first + stride, ...; returns how many
inline long long innov_shard_sample(long long goff, long long n, long long stride, long long* first) {
  const long long f = (stride - goff % stride) % stride;
  *first = f;
  return f < n ? (n - f - 1) / stride + 1 : 0;
}
int innovation_dirs_impl(const float* angles, int32_t B, float* dirs_out) {
  if (!angles || !dirs_out || B < 1 || B > MCL_INNOVATION_MAX_BEAMS) return MCL_ERR_INVALID;
  for (int b = 0; b < B; ++b) {
    if (!std::isfinite(angles[b])) return MCL_ERR_INVALID;
    const float raw[3] = {0.f, (float)std::sin((double)angles[b]), (float)-std::cos((double)angles[b])};
    float unit[4];
    if (normalise_beams(raw, nullptr, 1, unit) != MCL_OK) return MCL_ERR_INVALID;
    for (int c = 0; c < 3; ++c) dirs_out[3 * b + c] = unit[c];
  }
  return MCL_OK;
}
// can the record be a sum of the definition?
inline bool innov_legal(const mcl_innovation_beam& r) {
  typedef unsigned __int128 u128;
  if (r.n < 0 || r.n > INNOV_MAX_N || r.n_miss < 0 || r.n_miss > r.n || r.n_within < 0 || r.n_within > r.n) return false;
  if (r.s1 == INT64_MIN) return false;   // (has no absolute value)
  const long long a1 = r.s1 < 0 ? -r.s1 : r.s1;
  if (a1 > r.n * INNOV_Q_MAX) return false;
  if ((u128)r.s2 > (u128)r.n << 48) return false;
  return (u128)a1 * (u128)a1 <= (u128)r.n * (u128)r.s2;   // Cauchy-Schwarz
}
// the nearest double of a 128-bit integer, ties to even: the leading 64 bits with the rest folded into the last one (a
// sticky bit, eleven places below the double's last), converted by the hardware, scaled exactly
inline double innov_u128_to_double(unsigned __int128 v) {
  const uint64_t hi = (uint64_t)(v >> 64);
  if (hi == 0) return (double)(uint64_t)v;
  int sh = 0;
  while (sh < 64 && (hi >> sh) != 0) ++sh;   // 1 ... 64: bits above the low word
  const uint64_t top = (uint64_t)(v >> sh);
  const bool sticky = (v & (((unsigned __int128)1 << sh) - 1)) != 0;
  return std::ldexp((double)(top | (sticky ? 1ull : 0ull)), sh);
}
inline mcl_innovation_derived innov_derive(const mcl_innovation_beam& r, double sigma) {
  typedef unsigned __int128 u128;
  mcl_innovation_derived d = {0.0, 0.0, 0.0, 0.0, 0, 0};
  if (r.n <= 0) return d;
  const double n = (double)r.n;
  const unsigned long long a1 = (unsigned long long)(r.s1 < 0 ? -r.s1 : r.s1);
  const u128 num = (u128)r.n * (u128)r.s2 - (u128)a1 * (u128)a1;
  d.nu = (double)r.s1 / (n * 4096.0);
  d.var = innov_u128_to_double(num) / (n * n) * (1.0 / 16777216.0);
  const double nu2 = d.nu * d.nu, s2 = sigma * sigma, den = d.var + s2;
  d.nis = nu2 / den;
  d.support = (double)r.n_within / n;
  d.valid = 1;
  return d;
}
int innovation_merge_impl(const mcl_innovation_beam* parts, int32_t n_parts, int32_t B, mcl_innovation_beam* out) {
  if (!parts || !out || n_parts < 1 || B < 1) return MCL_ERR_INVALID;
  for (int b = 0; b < B; ++b) {
    mcl_innovation_beam acc = {0, 0, 0, 0, 0};
    for (int p = 0; p < n_parts; ++p) {
      const mcl_innovation_beam& r = parts[(size_t)p * B + b];
      if (!innov_legal(r) || acc.n + r.n > INNOV_MAX_N) return MCL_ERR_INVALID;   // (n within 2^15 keeps every other sum in range)
      acc.n += r.n;
      acc.n_miss += r.n_miss;
      acc.n_within += r.n_within;
      acc.s1 += r.s1;
      acc.s2 += r.s2;
    }
    out[b] = acc;
  }
  return MCL_OK;
}
inline mcl_innovation_gate_config innov_default_gate() { return mcl_innovation_gate_config{10.83, 0.01, 0.25}; }
int innovation_gate_impl(const mcl_innovation_beam* beams, int32_t B, double sigma, const mcl_innovation_gate_config* cfg,
                         mcl_innovation_derived* per_beam, mcl_innovation_verdict* verdict) {
  if (!beams || !verdict || B < 1 || !(sigma > 0.0) || !std::isfinite(sigma)) return MCL_ERR_INVALID;
  const mcl_innovation_gate_config c = cfg ? *cfg : innov_default_gate();
  if (!(c.nis_gate >= 0.0) || !(c.min_support >= 0.0 && c.min_support <= 1.0) ||
      !(c.max_gated_fraction >= 0.0 && c.max_gated_fraction <= 1.0))
    return MCL_ERR_INVALID;
  for (int b = 0; b < B; ++b)
    if (!innov_legal(beams[b])) return MCL_ERR_INVALID;
  mcl_innovation_verdict v = {0, 0, 0, 0, 0.0, 0.0};
  double nu_sum = 0.0;
  for (int b = 0; b < B; ++b) {
    const mcl_innovation_derived d = innov_derive(beams[b], sigma);
    if (!d.valid) continue;
    ++v.n_valid;
    v.nis_sum += d.nis;
    nu_sum += d.nu;
    if (d.nis > c.nis_gate && d.support < c.min_support) ++v.n_candidates;
  }
  v.mean_nu = v.n_valid > 0 ? nu_sum / (double)v.n_valid : 0.0;
  v.inconsistent = (double)v.n_candidates > c.max_gated_fraction * (double)v.n_valid ? 1 : 0;
  v.n_gated = v.inconsistent ? 0 : v.n_candidates;
  if (per_beam)
    for (int b = 0; b < B; ++b) {
      mcl_innovation_derived d = innov_derive(beams[b], sigma);
      d.gated = d.valid && !v.inconsistent && d.nis > c.nis_gate && d.support < c.min_support ? 1 : 0;
      per_beam[b] = d;
    }
  *verdict = v;
  return MCL_OK;
}

// ---- ping information (include/mcl_information.h): the quantised central difference (the kernel, csrc/mcl_information.h,
// runs info_difference itself), the legality of the steps and of a record, the merge and the derived quantities.
constexpr long long INFO_MAX_N = MCL_INFORMATION_MAX_SAMPLES;
// d = rint((e+ - e-) 2^12): both ranges lie in [0, r_max], r_max <= 4096 m, so |d| <= 2^24 without a clamp
MCL_HD inline long long info_difference(float e_plus, float e_minus) {
  return (long long)rint(((double)e_plus - (double)e_minus) * 4096.0);
}
// |d| above this is a jump (the callers have refused what info_steps_why refuses: the product is below 2^23 + 1)
inline long long info_jump_q(double jump_max) { return (long long)std::floor(jump_max * 4096.0); }
// nullptr when the steps are legal for this r_max, else the sentence that says what is wrong
const char* info_steps_why(const mcl_information_steps* s, double r_max) {
  if (!s) return "null steps";
  if (!(r_max > 0.0) || !(r_max <= MCL_INFORMATION_MAX_RANGE)) return "r_max outside (0, 4096] m (the quantised difference's range)";
  if (!(s->delta_xy > 0.0) || !std::isfinite(s->delta_xy)) return "delta_xy must be positive and finite";
  if (!(s->delta_yaw > 0.0) || !std::isfinite(s->delta_yaw)) return "delta_yaw must be positive and finite";
  if (!(s->jump_max > 0.0) || !(s->jump_max <= r_max)) return "jump_max outside (0, r_max]";
  if (!(s->jump_max <= MCL_INFORMATION_MAX_JUMP)) return "jump_max above 2048 m (the products' range)";
  return nullptr;
}
// can the record be a sum of the definition?
inline bool info_legal(const mcl_information_sums& r) {
  typedef unsigned __int128 u128;
  if (r.n < 0 || r.n > INFO_MAX_N || r.n_miss < 0 || r.n_jump < 0 || r.n_miss > r.n || r.n_jump > r.n - r.n_miss) return false;
  const u128 cap = (u128)(r.n - r.n_miss - r.n_jump) << 46;
  if ((u128)r.sxx > cap || (u128)r.syy > cap || (u128)r.sww > cap) return false;
  if (r.sxy == INT64_MIN || r.sxw == INT64_MIN || r.syw == INT64_MIN) return false;   // (have no absolute value)
  const u128 axy = (u128)(r.sxy < 0 ? -r.sxy : r.sxy), axw = (u128)(r.sxw < 0 ? -r.sxw : r.sxw), ayw = (u128)(r.syw < 0 ? -r.syw : r.syw);
  return axy * axy <= (u128)r.sxx * (u128)r.syy && axw * axw <= (u128)r.sxx * (u128)r.sww &&
         ayw * ayw <= (u128)r.syy * (u128)r.sww;   // Cauchy-Schwarz
}
int information_merge_impl(const mcl_information_sums* parts, int32_t n_parts, int32_t B, mcl_information_sums* out) {
  if (!parts || !out || n_parts < 1 || B < 1) return MCL_ERR_INVALID;
  for (int b = 0; b < B; ++b) {
    mcl_information_sums acc = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int p = 0; p < n_parts; ++p) {
      const mcl_information_sums& r = parts[(size_t)p * B + b];
      if (!info_legal(r) || acc.n + r.n > INFO_MAX_N) return MCL_ERR_INVALID;   // (n within 2^15 keeps every other sum in range)
      acc.n += r.n;
      acc.n_miss += r.n_miss;
      acc.n_jump += r.n_jump;
      acc.sxx += r.sxx;
      acc.syy += r.syy;
      acc.sww += r.sww;
      acc.sxy += r.sxy;
      acc.sxw += r.sxw;
      acc.syw += r.syw;
    }
    out[b] = acc;
  }
  return MCL_OK;
}
// the six sums of a record in the packed order xx, xy, xw, yy, yw, ww, each as the nearest double
inline void info_sums6(const mcl_information_sums& r, double s[6]) {
  s[0] = (double)r.sxx;
  s[1] = (double)r.sxy;
  s[2] = (double)r.sxw;
  s[3] = (double)r.syy;
  s[4] = (double)r.syw;
  s[5] = (double)r.sww;
}
// everything behind J: the Schur complement, its eigenvalues in closed form, the weak axis, the bounds, the rank
inline void info_eigen(mcl_information_result& o) {
  const double inf = std::numeric_limits<double>::infinity();
  const double* J = o.J;
  double a = J[0], b = J[1], c = J[3];
  if (J[5] != 0.0) {
    a = J[0] - (J[2] * J[2]) / J[5];
    b = J[1] - (J[2] * J[4]) / J[5];
    c = J[3] - (J[4] * J[4]) / J[5];
    // what is left of a position information that yaw explains altogether is rounding, not information
    if (a + c <= (J[0] + J[3]) * (1.0 / 1099511627776.0)) a = b = c = 0.0;
  }
  const double h = 0.5 * (a + c), g = 0.5 * (a - c);
  const double lmax = h + std::sqrt(g * g + b * b);
  if (!(lmax > 0.0)) {
    o.lambda_max = o.lambda_min = 0.0;
    o.weak_axis = 0.0;
    o.crlb_strong = o.crlb_weak = inf;
    o.rank_pos = 0;
    return;
  }
  const double det = a * c - b * b;
  const double lmin = det > 0.0 ? det / lmax : 0.0;
  const double pi = 3.14159265358979323846;
  double w = 0.5 * std::atan2(2.0 * b, a - c) + pi / 2;
  if (w >= pi) w -= pi;
  if (w < 0.0) w = 0.0;
  o.lambda_max = lmax;
  o.lambda_min = lmin;
  o.weak_axis = w;
  o.crlb_strong = 1.0 / std::sqrt(lmax);
  const bool weak = lmin <= lmax * (1.0 / 1099511627776.0);
  o.crlb_weak = weak ? inf : 1.0 / std::sqrt(lmin);
  o.rank_pos = weak ? 1 : 2;
}
int information_matrix_impl(const mcl_information_sums* recs, int32_t count, int32_t per_pose, double sigma, double delta_xy,
                            double delta_yaw, mcl_information_result* out) {
  if (!recs || !out || count < 1) return MCL_ERR_INVALID;
  if (!(sigma > 0.0) || !std::isfinite(sigma) || !(delta_xy > 0.0) || !std::isfinite(delta_xy) || !(delta_yaw > 0.0) ||
      !std::isfinite(delta_yaw))
    return MCL_ERR_INVALID;
  for (int k = 0; k < count; ++k)
    if (!info_legal(recs[k])) return MCL_ERR_INVALID;
  const double dl[3] = {delta_xy, delta_xy, delta_yaw};
  const int ja[6] = {0, 0, 0, 1, 1, 2}, ka[6] = {0, 1, 2, 1, 2, 2};
  double q[6];
  for (int e = 0; e < 6; ++e) q[e] = (4.0 * dl[ja[e]]) * dl[ka[e]];
  const double s2 = sigma * sigma;
  if (per_pose) {
    for (int k = 0; k < count; ++k) {
      mcl_information_result o;
      memset(&o, 0, sizeof o);
      double s[6];
      info_sums6(recs[k], s);
      for (int e = 0; e < 6; ++e) o.J[e] = s[e] / ((16777216.0 * q[e]) * s2);
      const long long m = recs[k].n - recs[k].n_miss - recs[k].n_jump;
      o.hit_share = recs[k].n > 0 ? (double)m / (double)recs[k].n : 0.0;
      info_eigen(o);
      out[k] = o;
    }
    return MCL_OK;
  }
  mcl_information_result o;
  memset(&o, 0, sizeof o);
  long long sum_m = 0, sum_n = 0;
  for (int k = 0; k < count; ++k) {
    const long long m = recs[k].n - recs[k].n_miss - recs[k].n_jump;
    sum_n += recs[k].n;
    if (m <= 0) continue;
    sum_m += m;
    double s[6];
    info_sums6(recs[k], s);
    const double mm = (double)m * 16777216.0;
    for (int e = 0; e < 6; ++e) o.J[e] += s[e] / (mm * q[e]);
  }
  for (int e = 0; e < 6; ++e) o.J[e] = o.J[e] / s2;
  o.hit_share = sum_n > 0 ? (double)sum_m / (double)sum_n : 0.0;
  info_eigen(o);
  *out = o;
  return MCL_OK;
}

// ---- ping matching (include/mcl_match.h): which record is better, the damped normal equations and their solution, the
// legality of a config and of a record, the derived quantities.  The kernel (csrc/mcl_match.h) runs match_better and
// match_solve_core itself, from one lane: one statement of each rule.  The functions index their arrays in loops, so
// the kernel hands them a workspace in LDS (MATCH_WS doubles), not in registers.
constexpr int MATCH_WS = 32;   // A[10], L[10], y[4], t[4], delta[4]
MCL_HD inline long long match_m(const mcl_match_sums& r) { return r.n - r.n_miss - r.n_jump; }
// m_q >= min_beams and s_rho2_q m_p < s_rho2_p m_q, in 128 bits (the products are below 2^70; a swath's, mcl_swath.h, 2^76)
MCL_HD inline bool match_better(const mcl_match_sums& q, const mcl_match_sums& p, int min_beams) {
  typedef unsigned __int128 u128;
  const long long mq = match_m(q), mp = match_m(p);
  if (mq < (long long)min_beams) return false;
  return (u128)(unsigned long long)q.s_rho2 * (u128)(unsigned long long)mp < (u128)(unsigned long long)p.s_rho2 * (u128)(unsigned long long)mq;
}
MCL_HD inline double match_pow2(int j) {   // 2^j, -1022 <= j <= 1023
  const unsigned long long b = (unsigned long long)(1023 + j) << 52;
  double v;
  __builtin_memcpy(&v, &b, sizeof v);
  return v;
}
// the dimensions without a gradient: S_kk <= m floor^2 (m <= 2^11, a swath's 2^14, floor <= 2^12: the product is below 2^38), and those >= D
MCL_HD inline int match_dead_gradient(const mcl_match_sums& r, int D, int grad_floor_q) {
  const long long lim = match_m(r) * (long long)grad_floor_q * (long long)grad_floor_q;
  int dead = 0;
  for (int k = 0; k < 4; ++k)
    if (k >= D || r.S[reg_packed(k, k)] <= lim) dead |= 1 << k;
  return dead;
}
MCL_HD inline int match_count_live(int dead) {
  int c = 0;
  for (int k = 0; k < 4; ++k) c += ((dead >> k) & 1) ? 0 : 1;
  return c;
}
MCL_HD inline int match_nth_live(int dead, int i) {   // the i-th dimension that is not dead
  for (int k = 0; k < 4; ++k)
    if (!((dead >> k) & 1)) {
      if (i == 0) return k;
      --i;
    }
  return 3;
}
// A (packed, compacted to the live dimensions) and b (into y) of the normal equations, without damping
MCL_HD inline void match_normal(const mcl_match_sums& r, int dead, double delta_xy, double delta_yaw, double* A, double* y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int nl = match_count_live(dead);
  for (int i = 0; i < nl; ++i) {
    const int ki = match_nth_live(dead, i);
    const double di = ki == 2 ? delta_yaw : delta_xy;
    for (int k = 0; k <= i; ++k) {
      const int kk = match_nth_live(dead, k);
      const double dk = kk == 2 ? delta_yaw : delta_xy;
      const double q = ((4.0 * di) * dk) * 16777216.0;
      A[reg_packed(i, k)] = (double)r.S[reg_packed(ki, kk)] / q;
    }
    y[i] = (double)r.C[ki] / ((2.0 * di) * 16777216.0);
  }
}
// L t = y, then L^T t' = t, without the columns `kill` (reg_factor's mask): y holds b on entry
MCL_HD inline void match_substitute(const double* L, int nl, int kill, double* y, double* t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int i = 0; i < nl; ++i) {
    if ((kill >> i) & 1) {
      y[i] = 0.0;
      continue;
    }
    double s = y[i];
    for (int k = 0; k < i; ++k) {
      const double q = L[reg_packed(i, k)] * y[k];
      s = s - q;
    }
    y[i] = s / L[reg_packed(i, i)];
  }
  for (int i = nl - 1; i >= 0; --i) {
    if ((kill >> i) & 1) {
      t[i] = 0.0;
      continue;
    }
    double s = y[i];
    for (int k = i + 1; k < nl; ++k) {
      const double q = L[reg_packed(k, i)] * t[k];
      s = s - q;
    }
    t[i] = s / L[reg_packed(i, i)];
  }
}
// the mask of reg_factor over the compacted dimensions, as a mask over x, y, yaw, z
MCL_HD inline int match_expand_mask(int dead, int kill) {
  int out = 0;
  const int nl = match_count_live(dead);
  for (int i = 0; i < nl; ++i)
    if ((kill >> i) & 1) out |= 1 << match_nth_live(dead, i);
  return out;
}
// SOLVE of include/mcl_match.h: the step into ws[28 ... 31], the dead mask returned.  The caller has checked the config.
MCL_HD inline int match_solve_core(const mcl_match_sums& r, const mcl_match_config& c, int j, double* ws) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double *A = ws, *L = ws + 10, *y = ws + 20, *t = ws + 24, *delta = ws + 28;
  const int dead0 = match_dead_gradient(r, c.dims, c.grad_floor_q);
  const int nl = match_count_live(dead0);
  for (int k = 0; k < 4; ++k) delta[k] = 0.0;
  if (nl == 0) return dead0;
  match_normal(r, dead0, c.steps.delta_xy, c.steps.delta_yaw, A, y);
  const double lam = match_pow2(j);
  for (int i = 0; i < nl; ++i) {
    const double q = lam * A[reg_packed(i, i)];
    A[reg_packed(i, i)] = A[reg_packed(i, i)] + q;
  }
  const int kill = reg_factor(A, nl, L);
  match_substitute(L, nl, kill, y, t);
  for (int i = 0; i < nl; ++i)
    if (!((kill >> i) & 1)) delta[match_nth_live(dead0, i)] = t[i];
  const double tx = delta[0], ty = delta[1];
  const double xx = tx * tx, yy = ty * ty;
  const double h = sqrt(xx + yy);
  double s = 1.0;
  if (h > c.step_max_xy) s = c.step_max_xy / h;
  const double az = fabs(delta[3]), aw = fabs(delta[2]);
  if (az * s > c.step_max_xy) s = c.step_max_xy / az;
  if (aw * s > c.step_max_yaw) s = c.step_max_yaw / aw;
  if (s < 1.0)
    for (int k = 0; k < 4; ++k) delta[k] = delta[k] * s;
  return dead0 | match_expand_mask(dead0, kill);
}
// nullptr, or the rule of the config that is broken (the steps against r_max: match_config_check_impl)
inline const char* match_config_why(const mcl_match_config* c) {
  if (!c) return "null config";
  if (c->dims != 3 && c->dims != 4) return "dims must be 3 (x, y, yaw) or 4 (x, y, yaw, z)";
  if (c->max_iter < 1 || c->max_iter > MCL_MATCH_MAX_ITER) return "max_iter outside 1 ... 32";
  if (c->min_beams < 1) return "min_beams must be >= 1";
  if (c->grad_floor_q < 0 || c->grad_floor_q > MCL_MATCH_MAX_GRAD_FLOOR) return "grad_floor_q outside 0 ... 4096";
  if (!(c->step_max_xy > 0.0) || !std::isfinite(c->step_max_xy)) return "step_max_xy must be positive and finite";
  if (!(c->step_max_yaw > 0.0) || !std::isfinite(c->step_max_yaw)) return "step_max_yaw must be positive and finite";
  if (!(c->tol_xy >= 0.0) || !std::isfinite(c->tol_xy)) return "tol_xy must be >= 0 and finite";
  if (!(c->tol_yaw >= 0.0) || !std::isfinite(c->tol_yaw)) return "tol_yaw must be >= 0 and finite";
  if (!(c->steps.delta_xy > 0.0) || !std::isfinite(c->steps.delta_xy)) return "delta_xy must be positive and finite";
  if (!(c->steps.delta_yaw > 0.0) || !std::isfinite(c->steps.delta_yaw)) return "delta_yaw must be positive and finite";
  return nullptr;
}
int match_config_check_impl(const mcl_match_config* cfg, double r_max, const char** reason) {
  const char* why = match_config_why(cfg);
  if (!why) why = info_steps_why(&cfg->steps, r_max);
  if (reason) *reason = why;
  return why ? MCL_ERR_INVALID : MCL_OK;
}
// can the record be a sum of the definition?  n_max: MCL_MATCH_MAX_BEAMS, or a swath's MCL_SWATH_MAX_BEAMS (m <= 2^14: 4 cap <= 2^62)
inline bool match_legal(const mcl_match_sums& r, long long n_max = MCL_MATCH_MAX_BEAMS) {
  if (r.n < 0 || r.n > n_max || r.n_miss < 0 || r.n_jump < 0 || r.n_miss > r.n || r.n_jump > r.n - r.n_miss) return false;
  const long long m = match_m(r), cap = m << 46;
  for (int j = 0; j < 4; ++j)
    for (int k = 0; k <= j; ++k) {
      const long long v = r.S[reg_packed(j, k)];
      if (v > cap || v < (j == k ? 0 : -cap)) return false;
    }
  for (int k = 0; k < 4; ++k)
    if (r.C[k] > 2 * cap || r.C[k] < -2 * cap) return false;
  if (r.s_rho2 < 0 || r.s_rho2 > 4 * cap) return false;
  return r.s_rho <= (m << 24) && r.s_rho >= -(m << 24);
}
int match_solve_impl(const mcl_match_sums* rec, const mcl_match_config* cfg, int32_t j, double* delta_out, int32_t* dead_out,
                     long long n_max = MCL_MATCH_MAX_BEAMS) {
  if (!rec || !delta_out || !dead_out || match_config_why(cfg) || j < MCL_MATCH_J_MIN || j > MCL_MATCH_J_MAX + 2 || !match_legal(*rec, n_max))
    return MCL_ERR_INVALID;
  double ws[MATCH_WS];
  *dead_out = match_solve_core(*rec, *cfg, j, ws);
  for (int k = 0; k < 4; ++k) delta_out[k] = ws[28 + k];
  return MCL_OK;
}
int match_better_impl(const mcl_match_sums* q, const mcl_match_sums* p, int32_t min_beams, int32_t* better,
                      long long n_max = MCL_MATCH_MAX_BEAMS) {
  if (!q || !p || !better || min_beams < 1 || !match_legal(*q, n_max) || !match_legal(*p, n_max)) return MCL_ERR_INVALID;
  *better = match_better(*q, *p, min_beams) ? 1 : 0;
  return MCL_OK;
}
int match_derived_impl(const mcl_match_sums* rec, const mcl_match_config* cfg, double sigma, mcl_match_derived_t* out,
                       long long n_max = MCL_MATCH_MAX_BEAMS) {
  if (!rec || !out || match_config_why(cfg) || !(sigma > 0.0) || !std::isfinite(sigma) || !match_legal(*rec, n_max)) return MCL_ERR_INVALID;
  mcl_match_derived_t o;
  memset(&o, 0, sizeof o);
  const long long m = match_m(*rec);
  o.m = (int32_t)m;
  if (m > 0) {
    o.rms = std::sqrt((double)rec->s_rho2 / (double)m) / 4096.0;
    o.mean = ((double)rec->s_rho / (double)m) / 4096.0;
  }
  const double z = o.rms / sigma, s2 = sigma * sigma;
  o.chi2 = z * z;
  double ws[MATCH_WS];
  double *A = ws, *L = ws + 10, *y = ws + 20, *t = ws + 24;
  const int dead0 = match_dead_gradient(*rec, cfg->dims, cfg->grad_floor_q);
  const int nl = match_count_live(dead0);
  match_normal(*rec, dead0, cfg->steps.delta_xy, cfg->steps.delta_yaw, A, y);
  for (int i = 0; i < nl; ++i)
    for (int k = 0; k <= i; ++k) o.J[reg_packed(match_nth_live(dead0, i), match_nth_live(dead0, k))] = A[reg_packed(i, k)] / s2;
  const int kill = nl > 0 ? reg_factor(A, nl, L) : 0;
  o.dead = dead0 | match_expand_mask(dead0, kill);
  for (int c = 0; c < nl; ++c) {
    if ((kill >> c) & 1) continue;
    for (int i = 0; i < nl; ++i) y[i] = i == c ? 1.0 : 0.0;
    match_substitute(L, nl, kill, y, t);
    for (int i = c; i < nl; ++i)
      if (!((kill >> i) & 1)) o.cov[reg_packed(match_nth_live(dead0, i), match_nth_live(dead0, c))] = t[i] * s2;
  }
  for (int k = 0; k < cfg->dims; ++k)
    if ((o.dead >> k) & 1) o.cov[reg_packed(k, k)] = std::numeric_limits<double>::infinity();
  *out = o;
  return MCL_OK;
}

// ---- swath matching (include/mcl_swath.h): the offsets of K dead-reckoned poses relative to one of them and the check of
// a swath.  Solve, compare and derived quantities are the ping matching's above with n_max = MCL_SWATH_MAX_BEAMS.
inline const char* swath_why(int K, int B, const mcl_swath_offset* off) {
  if (K < 1 || K > MCL_SWATH_MAX_PINGS) return "K outside 1 ... 64";
  if (B < 1 || B > MCL_MATCH_MAX_BEAMS) return "B outside 1 ... 2048";
  if ((long long)K * B > MCL_SWATH_MAX_BEAMS) return "K B above 16384";
  if (!off) return "null offsets";
  for (int k = 0; k < K; ++k) {
    const mcl_swath_offset& o = off[k];
    if (!std::isfinite(o.dx) || !std::isfinite(o.dy) || !std::isfinite(o.dz) || !std::isfinite(o.roll) || !std::isfinite(o.pitch) ||
        !std::isfinite(o.dyaw))
      return "an offset is not finite";
  }
  return nullptr;
}
int swath_check_impl(int K, int B, const mcl_swath_offset* off, const char** reason) {
  const char* why = swath_why(K, B, off);
  if (reason) *reason = why;
  return why ? MCL_ERR_INVALID : MCL_OK;
}
// the library's rule for a yaw that moved: kept when -pi <= t < pi, else ((t + pi) mod 2 pi) - pi with the floored modulo
inline double swath_wrap(double t) {
  const double pi = 3.14159265358979323846, b = 2.0 * pi;
  if (t >= -pi && t < pi) return t;
  double m = std::fmod(t + pi, b);
  if (m < 0.0) m = m + b;
  return m - pi;
}
int swath_offsets_impl(const double* p, int K, int anchor, mcl_swath_offset* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!p || !out || K < 1 || K > MCL_SWATH_MAX_PINGS || anchor < -1 || anchor >= K) return MCL_ERR_INVALID;
  for (int k = 0; k < 6 * K; ++k)
    if (!std::isfinite(p[k])) return MCL_ERR_INVALID;
  const int a = anchor < 0 ? K - 1 : anchor;
  const double *x = p, *y = p + K, *z = p + 2 * K, *roll = p + 3 * K, *pitch = p + 4 * K, *yaw = p + 5 * K;
  const double s = std::sin(yaw[a]), c = std::cos(yaw[a]);
  for (int k = 0; k < K; ++k) {
    mcl_swath_offset o;
    const double u = x[k] - x[a], w = y[k] - y[a];
    const double cu = c * u, sw = s * w, cw = c * w, su = s * u;
    o.dx = cu + sw;
    o.dy = cw - su;
    o.dz = z[k] - z[a];
    o.roll = roll[k];
    o.pitch = pitch[k];
    const double t = yaw[k] - yaw[a];
    o.dyaw = swath_wrap(t);
    if (k == a) o.dx = o.dy = o.dz = o.dyaw = 0.0;   // (the differences are +0.0 already; c * 0 + s * 0 may be -0.0)
    out[k] = o;
  }
  return MCL_OK;
}

// ---- sensor resetting (include/mcl_reseed.h): the rules of a component table and of the selection config, the component
// a 53-bit draw picks, and the selection of a mixture from match results.
inline const char* reseed_select_why(const mcl_reseed_select_config* c) {
  if (!c) return "null config";
  if (c->max_components < 1 || c->max_components > MCL_RESEED_MAX_COMPONENTS) return "max_components outside 1 ... 256";
  if (c->min_beams < 1) return "min_beams must be >= 1";
  if (!std::isfinite(c->max_rms) || c->max_rms < 0.0) return "max_rms must be finite and >= 0";
  if (!std::isfinite(c->sep_xy) || c->sep_xy < 0.0 || !std::isfinite(c->sep_yaw) || c->sep_yaw < 0.0) return "sep_xy and sep_yaw must be finite and >= 0";
  if (!std::isfinite(c->cov_scale) || !(c->cov_scale > 0.0)) return "cov_scale must be finite and > 0";
  if (!std::isfinite(c->add_std_xy) || c->add_std_xy < 0.0 || !std::isfinite(c->add_std_yaw) || c->add_std_yaw < 0.0)
    return "add_std_xy and add_std_yaw must be finite and >= 0";
  if (!std::isfinite(c->dead_std_xy) || !(c->dead_std_xy > 0.0) || !std::isfinite(c->dead_std_yaw) || !(c->dead_std_yaw > 0.0))
    return "dead_std_xy and dead_std_yaw must be finite and > 0";
  return nullptr;
}
int reseed_select_check_impl(const mcl_reseed_select_config* cfg, const char** reason) {
  const char* why = reseed_select_why(cfg);
  if (reason) *reason = why;
  return why ? MCL_ERR_INVALID : MCL_OK;
}
// the table of mcl_inject_gaussian; total (or nullptr): W, the sum of the masses
inline const char* reseed_components_why(const mcl_reseed_component* comps, int n_comp, uint64_t* total) {
  if (!comps) return "null components";
  if (n_comp < 1 || n_comp > MCL_RESEED_MAX_COMPONENTS) return "n_comp outside 1 ... 256";
  uint64_t W = 0;
  for (int c = 0; c < n_comp; ++c) {
    const mcl_reseed_component& k = comps[c];
    for (int r = 0; r < 3; ++r)
      if (!std::isfinite(k.mean[r])) return "a mean is not finite";
    for (int r = 0; r < 6; ++r)
      if (!std::isfinite(k.chol[r])) return "a factor entry is not finite";
    if (k.chol[0] < 0.0 || k.chol[2] < 0.0 || k.chol[5] < 0.0) return "a diagonal of the factor is negative";
    W += k.mass;
  }
  if (W == 0) return "the masses add up to 0";
  if (W > (1ull << 31)) return "the masses add up to more than 2^31";
  if (total) *total = W;
  return nullptr;
}
int reseed_components_check_impl(const mcl_reseed_component* comps, int n_comp, const char** reason) {
  const char* why = reseed_components_why(comps, n_comp, nullptr);
  if (reason) *reason = why;
  return why ? MCL_ERR_INVALID : MCL_OK;
}
// r = (t W) >> 53 of the 128-bit product (t < 2^53, W <= 2^31: r < W); the kernel runs the same function
MCL_HD inline uint32_t reseed_rank(uint64_t t, uint64_t W) {
  const uint64_t t_hi = t >> 32, t_lo = t & 0xffffffffull;   // W < 2^32: two 64-bit products, no carry lost
  const uint64_t lo = t_lo * W, hi = t_hi * W + (lo >> 32);  // t W = hi 2^32 + (lo mod 2^32)
  return (uint32_t)(hi >> 21);
}
int reseed_select_impl(const mcl_match_result* res, int64_t M, const mcl_match_config* mcfg, double sigma,
                       const mcl_reseed_select_config* cfg, mcl_reseed_component* comps_out, int64_t* index_out, int32_t* n_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!res || !comps_out || !index_out || !n_out || M < 1 || M > MCL_MATCH_MAX_POSES || reseed_select_why(cfg) || match_config_why(mcfg) ||
      !(sigma > 0.0) || !std::isfinite(sigma))
    return MCL_ERR_INVALID;
  struct Cand {
    double rms;
    int64_t i;
    mcl_match_derived_t d;
  };
  std::vector<Cand> cand;
  for (int64_t i = 0; i < M; ++i) {
    if (res[i].status != MCL_MATCH_CONVERGED) continue;
    Cand c;
    if (match_derived_impl(&res[i].final, mcfg, sigma, &c.d, MCL_SWATH_MAX_BEAMS) != MCL_OK) return MCL_ERR_INVALID;
    if (!std::isfinite(res[i].x) || !std::isfinite(res[i].y) || !std::isfinite(res[i].yaw)) return MCL_ERR_INVALID;
    if (c.d.m < cfg->min_beams || !(c.d.rms <= cfg->max_rms)) continue;
    c.rms = c.d.rms;
    c.i = i;
    cand.push_back(c);
  }
  std::stable_sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) { return a.rms < b.rms; });   // (by index within equal rms)
  int n = 0;
  for (const Cand& c : cand) {
    if (n == cfg->max_components) break;
    const mcl_match_result& r = res[c.i];
    bool near = false;
    for (int k = 0; k < n && !near; ++k) {
      const double dx = r.x - comps_out[k].mean[0], dy = r.y - comps_out[k].mean[1];
      const double xx = dx * dx, yy = dy * dy;
      const double dist = std::sqrt(xx + yy);
      const double t = r.yaw - comps_out[k].mean[2];
      near = dist <= cfg->sep_xy && std::fabs(swath_wrap(t)) <= cfg->sep_yaw;
    }
    if (near) continue;
    double cov[6];
    for (int k = 0; k < 6; ++k) cov[k] = cfg->cov_scale * c.d.cov[k];
    for (int k = 0; k < 3; ++k) {
      if (!((c.d.dead >> k) & 1)) continue;
      for (int j = 0; j < 3; ++j) cov[j >= k ? reg_packed(j, k) : reg_packed(k, j)] = 0.0;
      const double s = k == 2 ? cfg->dead_std_yaw : cfg->dead_std_xy;
      cov[reg_packed(k, k)] = s * s;
    }
    for (int k = 0; k < 3; ++k) {
      const double s = k == 2 ? cfg->add_std_yaw : cfg->add_std_xy;
      const double q = s * s;
      cov[reg_packed(k, k)] = cov[reg_packed(k, k)] + q;
    }
    mcl_reseed_component o;
    memset(&o, 0, sizeof o);
    o.mean[0] = r.x;
    o.mean[1] = r.y;
    o.mean[2] = r.yaw;
    int32_t dead;
    if (regularise_factor_impl(cov, 3, o.chol, &dead) != MCL_OK) return MCL_ERR_INVALID;
    o.mass = 1;
    comps_out[n] = o;
    index_out[n] = c.i;
    ++n;
  }
  *n_out = n;
  return MCL_OK;
}

}  // namespace
