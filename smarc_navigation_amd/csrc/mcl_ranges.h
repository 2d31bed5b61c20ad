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
  const float inv_res = (float)m.inv_res;
  const float r_max = m.r_max;
  // (whole waves run every iteration: the shuffles below need all lanes)
  for (long long first = a.i0 + (long long)blockIdx.x * per_block; first < a.i1; first += (long long)gridDim.x * per_block) {
    const long long i = first + (threadIdx.x >> lg);
    const bool live = i < a.i1;
    const bool cast = live && b < a.n_beams;
    const float4 bt = a.beam[b];
    float e = r_max;
    if (cast) {
      // ---- the sensor pose of particle i and the direction of beam b in the map, fp64 (make_pose, all three columns)
      double sr, cr, sp, cp, sy, cy;
      sincos(m.st[3][i], &sr, &cr);
      sincos(m.st[4][i], &sp, &cp);
      sincos(m.st[5][i], &sy, &cy);
      const double x = m.st[0][i], y = m.st[1][i], z = m.st[2][i];
      const double Rp[9] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                            sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                            -sp,     cp * sr,                cp * cr};
      double Rmp[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          Rmp[r * 3 + c] = m.m2o[r * 4 + 0] * Rp[c] + m.m2o[r * 4 + 1] * Rp[3 + c] + m.m2o[r * 4 + 2] * Rp[6 + c];
      double o[3], v[3], d[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        o[r] = (m.m2o[r * 4 + 0] * x + m.m2o[r * 4 + 1] * y + m.m2o[r * 4 + 2] * z + m.m2o[r * 4 + 3]) +
               (Rmp[r * 3 + 0] * m.off_t[0] + Rmp[r * 3 + 1] * m.off_t[1] + Rmp[r * 3 + 2] * m.off_t[2]);
        v[r] = m.off_R[r * 3 + 0] * (double)bt.x + m.off_R[r * 3 + 1] * (double)bt.y + m.off_R[r * 3 + 2] * (double)bt.z;
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) d[r] = Rmp[r * 3 + 0] * v[0] + Rmp[r * 3 + 1] * v[1] + Rmp[r * 3 + 2] * v[2];
      const float dx = (float)d[0], dy = (float)d[1], dz = (float)d[2];
      const double um = (o[0] - m.ox) * m.inv_res, vm = (o[1] - m.oy) * m.inv_res;
      const float oz = (float)o[2];
      // ---- its own cell and the fraction inside it (own_fan without the fan's footprint)
      const bool sane = fabs(um) < 1e9 && fabs(vm) < 1e9;  // (NaN: false)
      const double fu = sane ? floor(um) : 0.0, fv = sane ? floor(vm) : 0.0;
      const int I0 = (int)fu, J0 = (int)fv;
      const float ul = sane ? (float)(um - fu) : 0.f, vl = sane ? (float)(vm - fv) : 0.f;
      if (!sane) {
        e = r_max;  // (NaN / absurd position: the ray misses)
      } else if (MAP != 1) {
        // lattice maps (k_mbes_cast): where the ray is over the map's rectangle, cells relative to the particle's own
        const float cu_lo = (float)(-I0), cu_hi = (float)(m.nx - 2 - I0), cv_lo = (float)(-J0), cv_hi = (float)(m.ny - 2 - J0);
        const float du = dx * inv_res, dv = dy * inv_res;
        float t0 = 0.f, t1 = r_max;
        bool miss = false;
        if (du == 0.f) {
          miss = ul < cu_lo || ul > cu_hi + 1.f;
        } else {
          const float r = fast_rcp(du), ta = (cu_lo - ul) * r, tb = (cu_hi + 1.f - ul) * r;
          t0 = fmaxf(t0, fminf(ta, tb));
          t1 = fminf(t1, fmaxf(ta, tb));
        }
        if (dv == 0.f) {
          miss = miss || vl < cv_lo || vl > cv_hi + 1.f;
        } else {
          const float r = fast_rcp(dv), ta = (cv_lo - vl) * r, tb = (cv_hi + 1.f - vl) * r;
          t0 = fmaxf(t0, fminf(ta, tb));
          t1 = fminf(t1, fmaxf(ta, tb));
        }
        if (miss || !(t0 <= t1)) {
          e = r_max;
        } else {
          const float* gpp = m.grid_pad + ((long long)(I0 + 1) * m.nyp + (J0 + 1));   // node (I0, J0) inside the ring (dereferenced at map cells only)
          if (MAP == 0)
            e = cast_clear<0, true>(gpp, m.nyp, m, ul, vl, oz, du, dv, dz, m.zmax_map, r_max, t0, t1, cu_lo, cu_hi, cv_lo, cv_hi);
          else if (m.diag_mode == 1)
            e = cast_clear<2, true>(gpp, m.nyp, m, ul, vl, oz, du, dv, dz, m.zmax_map, r_max, t0, t1, cu_lo, cu_hi, cv_lo, cv_hi);
          else if (m.diag_mode == 2)
            e = cast_clear<3, true>(gpp, m.nyp, m, ul, vl, oz, du, dv, dz, m.zmax_map, r_max, t0, t1, cu_lo, cu_hi, cv_lo, cv_hi);
          else
            e = cast_clear<1, true>(gpp, m.nyp, m, ul, vl, oz, du, dv, dz, m.zmax_map, r_max, t0, t1, cu_lo, cu_hi, cv_lo, cv_hi);
        }
      } else {
        // triangle records: the clipped general march over the whole cell grid, water column skipped
        RayStats rs = {0, 0, 0, 0};
        float t_lo = 0.f;
        if (dz < 0.f && oz > m.zmax_map) t_lo = fmaxf((m.zmax_map - oz) * fast_rcp(dz) - 1e-3f, 0.f);
        e = cast_ray(m.mesh.cell_info, m.mesh.gy, m, I0, J0, m.mesh.gx, m.mesh.gy, ul, vl, oz, dx * inv_res, dy * inv_res, dx,
                     dy, dz, t_lo, r_max, rs);
      }
    }
    if (EXPECT_ONLY) {
      if (cast) a.exp_out[(size_t)(i - a.i0) * a.n_beams + b] = e;
    } else {
      const bool valid = cast && bt.w > 0.f;   // (NaN fails the test)
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
