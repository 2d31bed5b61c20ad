// mcl_swath.h -- kernel of the swath matching (include/mcl_swath.h; gfx950, wave64): k_ping_match's loop (csrc/mcl_match.h)
// over K pings that hang rigidly on one anchor pose.
//
//   k_swath_match<MAP, D> : one workgroup per start pose of the anchor, its lanes beam lanes as in k_ping_match.
//     evaluation      : every lane reads the anchor pose out of LDS; in every wave the lanes 0 ... 2 D take their variant of
//                       the ANCHOR (one fp64 addition on the stored number) and its yaw's sincos, once per evaluation.  Then
//                       the pings, an outer loop that is uniform over the workgroup: the offset of ping k is read from
//                       global memory by the loop's index (wave-uniform: scalar loads), the lanes 0 ... 2 D compose their
//                       variant's pose of ping k (swath_compose, fp contract off) and build its frame with lane_frame -- one
//                       more round of sincos per ping --, and the lanes cast that ping's beams in rounds of blockDim.x through
//                       match_beam, the per-beam body k_ping_match runs.  The nineteen words stay in registers across pings
//                       and rounds; after the pings one wave_sum per word and one LDS row per wave.
//     decision        : k_ping_match's: a barrier, match_decide (itself, not a copy) on thread 0, a barrier.  Every branch
//                       around a barrier depends on MatchBlock::go or on kernel arguments alone.
//     no global atomics, no scratch, no host round trip; LDS: MATCH_LDS_BYTES (tests/test_swath_isa.py).
//     dump            : range v of beam b of ping k at evaluation t goes to ranges_out[(((i T + t) K + k) NV + v) B + b].
//
// Bounds: k < n_pings = K guards the offsets (K records) and, with b < n_beams = B, the beam records (K B float4, ping k's
// at [k B + b]) and the dump's column; the rest as in csrc/mcl_match.h: blockIdx.x < M, t <= max_iter < T, so trace has
// M T rows and ranges_out M T K NV B floats, the extents the host reserves.
#pragma once
#include "../../include/mcl_swath.h"
#include "mcl_match.h"

struct SwathArgs {
  MatchArgs a;                   // k_ping_match's; beam: K x B records, n_beams: B
  const mcl_swath_offset* off;   // K
  int n_pings;                   // K
};

// the pose of a ping from a variant of the anchor (x, y, z, yaw; (s, c) its yaw's sincos) and the ping's offset: the
// definition's four lines, an exactly zero offset leaving the variant's bits
__device__ __forceinline__ void swath_compose(const mcl_swath_offset& o, double s, double c, double& x, double& y, double& z, double& yaw) {
#pragma clang fp contract(off)
  if (o.dx != 0.0 || o.dy != 0.0) {
    const double cx = c * o.dx, sy = s * o.dy, sx = s * o.dx, cy = c * o.dy;
    const double u = cx - sy, w = sx + cy;
    x = x + u;
    y = y + w;
  }
  if (o.dz != 0.0) z = z + o.dz;
  if (o.dyaw != 0.0) yaw = yaw + o.dyaw;
}

template <int MAP, int D>
__global__ void __launch_bounds__(BEAM_CHUNK) k_swath_match(SwathArgs sa) {
  static_assert(D == 3 || D == 4, "x, y, yaw and perhaps z");
  constexpr int NV = 1 + 2 * D;
  __shared__ long long rows[MATCH_WAVES][MATCH_WORDS];
  __shared__ MatchBlock blk;
  const MatchArgs& a = sa.a;
  const MbesArgs& m = a.m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i = blockIdx.x;
  const int T = a.cfg.max_iter + 1, K = sa.n_pings;
  const size_t B = (size_t)a.n_beams;
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
    // ---- lane v <= 2 D: the anchor in its v-th variant, and its yaw's sincos for the pings' lever arms
    double xv = 0.0, yv = 0.0, wv = 0.0, zv = 0.0, sv = 0.0, cv = 1.0;
    if (lane < NV) {
      xv = blk.pose[0], yv = blk.pose[1], wv = blk.pose[2], zv = blk.pose[3];
      xv = lane == 1 ? xv + dxy : (lane == 2 ? xv - dxy : xv);
      yv = lane == 3 ? yv + dxy : (lane == 4 ? yv - dxy : yv);
      wv = lane == 5 ? wv + dyaw : (lane == 6 ? wv - dyaw : wv);
      zv = lane == 7 ? zv + dxy : (lane == 8 ? zv - dxy : zv);
      sincos(wv, &sv, &cv);
    }
    long long acc[MATCH_WORDS];
#pragma unroll
    for (int f = 0; f < MATCH_WORDS; ++f) acc[f] = 0;
    for (int k = 0; k < K; ++k) {
      const mcl_swath_offset o = sa.off[k];
      LaneFrame F = lane_frame_none();
      if (lane < NV) {
        double x = xv, y = yv, z = zv, yaw = wv;
        swath_compose(o, sv, cv, x, y, z, yaw);
        F = lane_frame(m, x, y, z, o.roll, o.pitch, yaw);
      }
      const float4* beam = a.beam + (size_t)k * B;
      float* dump = a.ranges_out ? a.ranges_out + (((size_t)i * (size_t)T + (size_t)t) * (size_t)K + (size_t)k) * NV * B : nullptr;
      for (int b0 = 0; b0 < a.n_beams; b0 += (int)blockDim.x) {
        const int b = b0 + tid;
        const bool have = b < a.n_beams;
        const float4 bt = have ? beam[b] : make_float4(0.f, 0.f, -1.f, 0.f);
        const bool cast = have && beam_valid(bt.w);
        if (__ballot(cast) == 0ull) continue;   // (a wave without a counting beam this round; no barrier inside the rounds)
        match_beam<MAP, D>(m, F, bt, cast, a.jump_q, dump ? dump + b : nullptr, B, acc);
      }
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
