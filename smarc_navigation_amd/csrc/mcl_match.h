// mcl_match.h -- kernel of the ping matching (include/mcl_match.h; gfx950, wave64): per start pose the whole
// Levenberg-Marquardt loop -- evaluate, compare, solve, step -- without a host round trip.
//
//   k_ping_match<MAP, D> : MAP as cast_map_ray's (map_dispatch), D = 3 (x, y, yaw) or 4 (x, y, yaw, z).  One workgroup per
//                       pose (blockIdx.x = the pose), its lanes the beam lanes of csrc/mcl_innovation.h: lane t casts the
//                       beams t, t + blockDim.x, ... in rounds of blockDim.x <= BEAM_CHUNK.
//     evaluation      : every lane reads the pose to evaluate out of LDS; in every wave the lanes 0 ... 2 D build its
//                       1 + 2 D sensor frames (variant v = lane: one fp64 addition on the stored number, then lane_frame --
//                       one round of sincos) and the other lanes read them with lane_frame_of.  A lane casts its beam from
//                       each frame with cast_from_frame<MAP> -- one loop, one copy of the cast: match_beam, the per-beam
//                       body k_swath_match (csrc/mcl_swath.h) runs too -- and keeps the nineteen
//                       integers of a record in registers over its rounds; then they go through wave_sum into one LDS row
//                       per wave.
//     decision        : after a barrier thread 0 (match_decide, fp contract off, the functions the host exports:
//                       match_better and match_solve_core of mcl_host_pure.h) adds the rows, decides whether the pose
//                       evaluated is better, solves for the next step and writes the next pose and the control word
//                       MatchBlock::go to LDS.  After a second barrier every lane reads them.  Every branch around a barrier
//                       depends on that LDS word or on kernel arguments alone: it is uniform over the workgroup.
//     no global atomics, no dependence on the launch geometry: a record is a sum of integers.
//     dump / trace    : ranges_out != nullptr: range v of beam b at evaluation t goes to ranges_out[((i T + t) NV + v) B + b],
//                       T = max_iter + 1, NV = 1 + 2 D; trace != nullptr: thread 0 writes row trace[i T + t].
//
// LDS: MATCH_WAVES rows of MATCH_WORDS 64-bit words and one MatchBlock -- MATCH_LDS_BYTES; tests/test_match_isa.py holds
// the compiled kernels to it.
//
// Bounds: b < n_beams guards the beam table, the ping and the dump's column; the pose index blockIdx.x < count = M by the
// launch (grid = M), and the six pose arrays have M doubles each; the evaluation index t <= max_iter < T since thread 0
// stops at trials == max_iter, so trace has M T rows and ranges_out M T NV B floats, the extents the host reserves;
// results has M records; rows[wave] with wave < blockDim.x / 64 <= MATCH_WAVES.
#pragma once
#include "mcl_information.h"

#define MATCH_WORDS 19                    // the 64-bit words of a mcl_match_sums
#define MATCH_WAVES (BEAM_CHUNK / 64)
#define MATCH_BLOCK_BYTES 600             // sizeof(MatchBlock)
#define MATCH_LDS_BYTES (MATCH_WAVES * MATCH_WORDS * 8 + MATCH_BLOCK_BYTES)

struct MatchArgs {
  MbesArgs m;               // frames, the map and r_max (fill_frames_and_map); st: the uploaded poses, n: M
  const float4* beam;       // B records: x, y, z the unit direction in the sensor frame, w the measured range
  mcl_match_result* results;   // M
  mcl_match_trace* trace;   // M x (max_iter + 1), zeroed by the host, or nullptr
  float* ranges_out;        // M x (max_iter + 1) x (1 + 2 D) x B, or nullptr
  mcl_match_config cfg;
  long long jump_q;         // floor(jump_max 2^12)
  int n_beams;
};

// the control block of a workgroup (LDS): written by thread 0 between the two barriers, read by everybody after the second
struct MatchBlock {
  mcl_match_sums cur, trial;   // the records of the current pose and of the pose just evaluated
  double ws[MATCH_WS];         // match_solve_core's workspace; ws[28 ... 31]: the step
  double pose[4];              // the pose to evaluate: x, y, yaw, z
  int go;                      // 1: evaluate `pose`; 0: stop
  int pad;
};
static_assert(sizeof(MatchBlock) == MATCH_BLOCK_BYTES, "MATCH_LDS_BYTES");
static_assert(sizeof(mcl_match_sums) == 8 * MATCH_WORDS && offsetof(mcl_match_sums, S) == 24 && offsetof(mcl_match_sums, C) == 104 &&
                  offsetof(mcl_match_sums, s_rho) == 136 && offsetof(mcl_match_sums, s_rho2) == 144,
              "k_ping_match's words");

// what thread 0 carries from one evaluation to the next
struct MatchLane0 {
  double x, y, yaw, z;      // the current pose
  int j, trials, accepted, dead;
};

// the library's rule for a yaw that moved (mcl_regularise.h, mcl_drift.h)
__device__ __forceinline__ double match_wrap(double t) { return (t >= -MCL_PI && t < MCL_PI) ? t : wrap_pi(t); }

// Thread 0, between the barriers: the record of evaluation t out of the waves' rows, THE LOOP of include/mcl_match.h up to
// the next pose to evaluate.  Returns nothing: blk.go and blk.pose say how it goes on.
__device__ __forceinline__ void match_decide(const MatchArgs& a, MatchBlock& blk, const long long (*rows)[MATCH_WORDS], int n_waves,
                                             MatchLane0& st, long long i, int t) {
#pragma clang fp contract(off)
  long long* tr = reinterpret_cast<long long*>(&blk.trial);
  for (int f = 0; f < MATCH_WORDS; ++f) {
    long long s = 0;
    for (int w = 0; w < n_waves; ++w) s += rows[w][f];
    tr[f] = s;
  }
  const int T = a.cfg.max_iter + 1;
  const double qx = blk.pose[0], qy = blk.pose[1], qw = blk.pose[2], qz = blk.pose[3];
  mcl_match_result* res = a.results + i;
  int status = -1, accept, j_used;
  if (t == 0) {
    st.x = qx, st.y = qy, st.yaw = qw, st.z = qz;
    st.j = j_used = MCL_MATCH_J0;
    st.trials = st.accepted = st.dead = 0;
    blk.cur = blk.trial;
    res->start = blk.trial;
    accept = match_m(blk.trial) >= (long long)a.cfg.min_beams ? 1 : 0;
    if (!accept) status = MCL_MATCH_NO_OVERLAP;
  } else {
    j_used = st.j;
    accept = match_better(blk.trial, blk.cur, a.cfg.min_beams) ? 1 : 0;
    if (accept) {
      blk.cur = blk.trial;
      st.x = qx, st.y = qy, st.yaw = qw, st.z = qz;
      ++st.accepted;
      st.j = st.j - 2 < MCL_MATCH_J_MIN ? MCL_MATCH_J_MIN : st.j - 2;
      const double dx = blk.ws[28], dy = blk.ws[29], dw = blk.ws[30], dz = blk.ws[31];
      const double xx = dx * dx, yy = dy * dy;
      if (sqrt(xx + yy) < a.cfg.tol_xy && fabs(dz) < a.cfg.tol_xy && fabs(dw) < a.cfg.tol_yaw) status = MCL_MATCH_CONVERGED;
    } else {
      st.j += 2;
      if (st.j > MCL_MATCH_J_MAX) status = MCL_MATCH_STALLED;
    }
  }
  if (a.trace) {
    mcl_match_trace* row = a.trace + (i * T + t);
    row->x = qx, row->y = qy, row->yaw = qw, row->z = qz;
    row->sums = blk.trial;
    row->j = j_used;
    row->accepted = accept;
  }
  if (status < 0) {
    if (blk.cur.s_rho2 == 0) {
      status = MCL_MATCH_CONVERGED;
    } else {
      st.dead = match_solve_core(blk.cur, a.cfg, st.j, blk.ws);
      const double dx = blk.ws[28], dy = blk.ws[29], dw = blk.ws[30], dz = blk.ws[31];
      if (dx == 0.0 && dy == 0.0 && dw == 0.0 && dz == 0.0) {
        status = MCL_MATCH_CONVERGED;
      } else if (st.trials == a.cfg.max_iter) {
        status = MCL_MATCH_MAX_ITER_HIT;
      } else {
        blk.pose[0] = dx != 0.0 ? st.x + dx : st.x;
        blk.pose[1] = dy != 0.0 ? st.y + dy : st.y;
        blk.pose[2] = dw != 0.0 ? match_wrap(st.yaw + dw) : st.yaw;
        blk.pose[3] = dz != 0.0 ? st.z + dz : st.z;
        ++st.trials;
      }
    }
  }
  if (status >= 0) {
    res->x = st.x, res->y = st.y, res->yaw = st.yaw, res->z = st.z;
    res->status = status;
    res->evaluations = 1 + st.trials;
    res->accepted = st.accepted;
    res->j = st.j;
    res->dead = st.dead;
    res->reserved = 0;
    res->final = blk.cur;
  }
  blk.go = status < 0 ? 1 : 0;
}

// One beam of one evaluation, shared by k_ping_match and k_swath_match (csrc/mcl_swath.h): the beam record bt cast from the
// 1 + 2 D frames the wave's lanes 0 ... 2 D hold in F, and what it adds to the lane's nineteen words.  Every lane of the wave
// calls it (lane_frame_of reads across the wave); cast: this lane has a counting beam.  dump: nullptr, or where the
// lane's range of variant 0 goes, variant v at dump[v B].
template <int MAP, int D>
__device__ __forceinline__ void match_beam(const MbesArgs& m, const LaneFrame& F, const float4& bt, bool cast, long long jump_q,
                                           float* dump, size_t B, long long (&acc)[MATCH_WORDS]) {
  constexpr int NV = 1 + 2 * D;
  double v[3];
  beam_in_vehicle(m, bt, v);
  float e0 = 0.f, ep = 0.f;
  long long d0 = 0, d1 = 0, d2 = 0, d3 = 0;
  bool miss = false;
#pragma unroll 1
  for (int var = 0; var < NV; ++var) {
    const LaneFrame U = lane_frame_of(F, var);
    float e = 0.f;
    if (cast) {
      e = cast_from_frame<MAP>(m, U, v);
      miss = miss || e == m.r_max;
      if (dump) dump[(size_t)var * B] = e;
    }
    if (var == 0) {
      e0 = e;
    } else if (var & 1) {
      ep = e;
    } else {
      const long long d = info_difference(ep, e);
      if (var == 2)
        d0 = d;
      else if (var == 4)
        d1 = d;
      else if (var == 6)
        d2 = d;
      else
        d3 = d;
    }
  }
  const long long a0 = d0 < 0 ? -d0 : d0, a1 = d1 < 0 ? -d1 : d1, a2 = d2 < 0 ? -d2 : d2, a3 = d3 < 0 ? -d3 : d3;
  const bool jump = cast && !miss && (a0 > jump_q || a1 > jump_q || a2 > jump_q || a3 > jump_q);
  acc[0] += cast ? 1 : 0;
  acc[1] += cast && miss ? 1 : 0;
  acc[2] += jump ? 1 : 0;
  if (cast && !miss && !jump) {
    const long long rho = innov_quantise(bt.w, e0);
    acc[3] += d0 * d0;
    acc[4] += d1 * d0;
    acc[5] += d1 * d1;
    acc[6] += d2 * d0;
    acc[7] += d2 * d1;
    acc[8] += d2 * d2;
    if constexpr (D == 4) {
      acc[9] += d3 * d0;
      acc[10] += d3 * d1;
      acc[11] += d3 * d2;
      acc[12] += d3 * d3;
      acc[16] += d3 * rho;
    }
    acc[13] += d0 * rho;
    acc[14] += d1 * rho;
    acc[15] += d2 * rho;
    acc[17] += rho;
    acc[18] += rho * rho;
  }
}

template <int MAP, int D>
__global__ void __launch_bounds__(BEAM_CHUNK) k_ping_match(MatchArgs a) {
  static_assert(D == 3 || D == 4, "x, y, yaw and perhaps z");
  constexpr int NV = 1 + 2 * D;
  __shared__ long long rows[MATCH_WAVES][MATCH_WORDS];
  __shared__ MatchBlock blk;
  const MbesArgs& m = a.m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i = blockIdx.x;
  const int T = a.cfg.max_iter + 1;
  const size_t B = (size_t)a.n_beams;
  const double roll = m.st[3][i], pitch = m.st[4][i];
  const double dxy = a.cfg.steps.delta_xy, dyaw = a.cfg.steps.delta_yaw;
  MatchLane0 st = {0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0};
  if (tid == 0) {
    blk.pose[0] = m.st[0][i];
    blk.pose[1] = m.st[1][i];
    blk.pose[2] = m.st[5][i];
    blk.pose[3] = m.st[2][i];
    blk.go = 1;
  }
  __syncthreads();
  for (int t = 0;; ++t) {
    // ---- lane v <= 2 D: the sensor frame of the pose in its v-th variant
    LaneFrame F = lane_frame_none();
    if (lane < NV) {
      double x = blk.pose[0], y = blk.pose[1], yaw = blk.pose[2], z = blk.pose[3];
      x = lane == 1 ? x + dxy : (lane == 2 ? x - dxy : x);
      y = lane == 3 ? y + dxy : (lane == 4 ? y - dxy : y);
      yaw = lane == 5 ? yaw + dyaw : (lane == 6 ? yaw - dyaw : yaw);
      z = lane == 7 ? z + dxy : (lane == 8 ? z - dxy : z);
      F = lane_frame(m, x, y, z, roll, pitch, yaw);
    }
    long long acc[MATCH_WORDS];
#pragma unroll
    for (int f = 0; f < MATCH_WORDS; ++f) acc[f] = 0;
    float* dump = a.ranges_out ? a.ranges_out + ((size_t)i * (size_t)T + (size_t)t) * NV * B : nullptr;
    for (int b0 = 0; b0 < a.n_beams; b0 += (int)blockDim.x) {
      const int b = b0 + tid;
      const bool have = b < a.n_beams;
      const float4 bt = have ? a.beam[b] : make_float4(0.f, 0.f, -1.f, 0.f);
      const bool cast = have && beam_valid(bt.w);
      if (__ballot(cast) == 0ull) continue;   // (a wave without a counting beam this round; no barrier inside the rounds)
      match_beam<MAP, D>(m, F, bt, cast, a.jump_q, dump ? dump + b : nullptr, B, acc);
    }
    // ---- the wave's record into its LDS row (all 64 lanes are here: the workgroup is whole waves)
#pragma unroll
    for (int f = 0; f < MATCH_WORDS; ++f) {
      const bool z_word = (f >= 9 && f <= 12) || f == 16;
      const long long w = (D == 3 && z_word) ? 0ll : (long long)wave_sum((u64)acc[f]);
      if (lane == 0) rows[wave][f] = w;
    }
    __syncthreads();
    if (tid == 0) match_decide(a, blk, rows, (int)(blockDim.x >> 6), st, i, t);
    __syncthreads();
    if (blk.go == 0) break;
  }
}
