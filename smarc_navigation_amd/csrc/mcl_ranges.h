// mcl_ranges.h -- DVL / altimeter range update: a few rays in ANY direction per particle against the bathymetric map
// (terrain-aided navigation with the bottom ranges of a DVL: the altitude and the four Janus beams; no reference symbol --
// the reference reads the DVL's altitude, tf_convenience_topics/src/odom_listener.cpp:17).  Definition (the convention of
// oracle/mcl_oracle.c:orc_mbes_update, with the beam direction given instead of (0, sin a, -cos a)):
//   Rs = Rm R(roll, pitch, yaw) Ro,   o = m2o [x y z 1] + (Rm Rp) t_off,   d_b = Rs dir_b,
//   e_ib = range of the first hit of o + t d_b with the map (r_max without one),
//   lw_i (+)= -1/2 sum_b ((r_b - e_ib) / sigma)^2 - n_valid log(sigma sqrt(2 pi))   over the beams with r_b > 0.
//
//   k_ranges_update : one LANE per (particle, beam): B beams are padded to Bp = 1, 2, 4, 8 or 16 lanes, so a wave holds
//                     64 / Bp particles and every lane casts one ray (a DVL's beams are of similar length: the wave's
//                     lanes finish together).  Each lane builds its particle's sensor pose in fp64 from the SoA state
//                     (all three columns of R_map_sensor -- not the fan's pose records, which hold two) and casts its ray
//                     in fp32 with the map walks of the MBES traversal (mcl_mbes.h): cast_clear<SURF, true> on the
//                     NaN-ringed heights of a lattice map (height grid, triangulated regular grid), cast_ray on the
//                     triangle records of any other mesh.  Neither assumes wave-uniform rays (cast_clear's ballot only
//                     skips the grazing test when no lane needs it).
//
// Determinism (mcl_mbes.h header): a particle's log-likelihood depends on its own state, the beam table and the map only --
// the ray runs in coordinates relative to the particle's own cell (integer cell + fraction in [0, 1)), its lanes' squared
// residuals are added by the first lane in beam order, and nothing depends on the launch geometry or on neighbours.
// Sharded or permuted clouds therefore give the same bits.  The beam table (at most 16 x (direction, range)) travels in
// the kernel's argument block: no copy, no staging buffer, no stream synchronisation.
#pragma once
#include "mcl_mbes.h"

#define RANGES_MAX_BEAMS 16
#define RANGES_THREADS 256

struct RangesArgs {
  MbesArgs m;               // state (st, n), frames (m2o, off_t, off_R), the map (mcl_host_update.h: fill_frames_and_map) and r_max
  float4 beam[RANGES_MAX_BEAMS];  // x, y, z: unit direction in the sensor frame; w: measured range (<= 0 or NaN: invalid)
  long long i0, i1;         // the particles [i0, i1) this launch covers
  int n_beams, lg_bp;       // B, log2 of the lanes per particle (Bp >= B)
  int accumulate;           // 1: lw[i] += value, 0: lw[i] = value
  double sigma, lognorm;
  double* lw;
  float* exp_out;           // EXPECT_ONLY: [(i - i0) * B + b]
};

template <int MAP, bool EXPECT_ONLY>
__global__ void __launch_bounds__(RANGES_THREADS) k_ranges_update(RangesArgs a) {
  const int lg = a.lg_bp, bp = 1 << lg;
  const int lane = threadIdx.x & 63;
  const int b = lane & (bp - 1);
  const int lead = lane & ~(bp - 1);   // the particle's first lane
  const long long per_block = RANGES_THREADS >> lg;
  const MbesArgs& m = a.m;
  const float r_max = m.r_max;
  // (whole waves run every iteration: the shuffles below need all lanes)
  for (long long first = a.i0 + (long long)blockIdx.x * per_block; first < a.i1; first += (long long)gridDim.x * per_block) {
    const long long i = first + (threadIdx.x >> lg);
    const bool live = i < a.i1;
    const bool cast = live && b < a.n_beams;
    const float4 bt = a.beam[b];
    float e = r_max;
    if (cast) {
      // ---- the sensor pose of particle i and the direction of beam b in the map, fp64 (make_pose's frame, all three columns)
      double sr, cr, sp, cp, sy, cy;
      sincos(m.st[3][i], &sr, &cr);
      sincos(m.st[4][i], &sp, &cp);
      sincos(m.st[5][i], &sy, &cy);
      const PoseFrame F = pose_frame(m.m2o, m.off_t, m.st[0][i], m.st[1][i], m.st[2][i], sr, cr, sp, cp, sy, cy);
      double v[3], d[3];
      beam_in_vehicle(m, bt, v);
#pragma unroll
      for (int r = 0; r < 3; ++r) d[r] = F.Rmp[r * 3 + 0] * v[0] + F.Rmp[r * 3 + 1] * v[1] + F.Rmp[r * 3 + 2] * v[2];
      const float dx = (float)d[0], dy = (float)d[1], dz = (float)d[2];
      const float oz = (float)F.o[2];
      // ---- its own cell and the fraction inside it, then the map walk of the MBES traversal
      const OwnCell C = own_cell((F.o[0] - m.ox) * m.inv_res, (F.o[1] - m.oy) * m.inv_res);
      e = cast_map_ray<MAP>(m, C.sane, C.I0, C.J0, C.ul, C.vl, oz, dx, dy, dz);
    }
    if (EXPECT_ONLY) {
      if (cast) a.exp_out[(size_t)(i - a.i0) * a.n_beams + b] = e;
    } else {
      const bool valid = cast && beam_valid(bt.w);
      double term = 0.0;
      if (valid) {
        const double dr = ((double)bt.w - (double)e) / a.sigma;
        term = dr * dr;
      }
      // the particle's first lane adds its lanes' terms in beam order (a skipped beam adds +0.0: the sum is unchanged)
      double acc = __shfl(term, lead);
      for (int k = 1; k < bp; ++k) acc += __shfl(term, lead + k);
      const unsigned long long vmask = __ballot(valid);
      const int nv = __popcll((vmask >> lead) & ((2ull << (bp - 1)) - 1ull));
      if (live && b == 0) {
        const double val = -0.5 * acc - (double)nv * a.lognorm;
        a.lw[i] = a.accumulate ? a.lw[i] + val : val;
      }
    }
  }
}
