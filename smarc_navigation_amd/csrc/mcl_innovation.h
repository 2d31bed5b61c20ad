// mcl_innovation.h -- kernel of the ping innovation statistics (include/mcl_innovation.h; gfx950, wave64): per beam, over a
// strided sample of the cloud, the integer sums of the quantised residual q = rint((r_b - e_ib) 2^12).
//
//   k_innovation<MAP> : MAP 0 the height grid, 2 the node heights of a triangulated regular grid, 1 triangle records --
//                       ranges_launch's dispatch (mcl_host_ranges.h).  A LANE is a beam; a workgroup of up to 256 lanes owns
//                       a chunk of up to INNOV_CHUNK beams and a group of G <= 64 sampled particles, and loops over the
//                       particles: in an iteration every lane of a wave casts its own beam from the SAME particle, so
//                       adjacent lanes walk adjacent rays of one fan through the map.
//     pose            : built once per wave and particle, not once per ray: before the loop lane k of every wave builds
//                       the sensor frame of the group's k-th particle (three fp64 sincos, pose_frame, own_cell: the
//                       arithmetic of k_ranges_update) and iteration k reads it out of that lane (v_readlane, the loop
//                       counter is wave-uniform).  A wave pays one round of sincos for its G particles; no LDS, no barrier.
//     ray             : the lane's direction in the vehicle frame (off_R dir_b, fp64) is loop-invariant; per particle nine
//                       fp64 products turn it into the map frame, then the shared map-ray entry of mcl_mbes.h
//                       (cast_lattice_ray / cast_records_ray) casts in fp32 relative to the particle's own cell.
//     accumulation    : five integer accumulators per lane in registers across the G particles, then one 64-bit integer
//                       atomic add per field and beam into the zeroed 5 x B table (field-major).  Integer adds commute:
//                       the table holds the same bits for every G, grid and order of arrival (include/mcl_innovation.h).
//     dump            : exp_out != nullptr: e_ib also goes to exp_out[k B + b], k the sample's index in this shard.
//
// Bounds: b < n_beams guards the beam table, the accumulator table and exp_out's column; the slots first + k stride,
// k < count, lie below a.m.n by innov_shard_sample (mcl_host_pure.h); exp_out has count rows.
#pragma once
#include "mcl_mbes.h"

#define INNOV_CHUNK 256        // beams of a workgroup
#define INNOV_MAX_GROUP 64     // particles of a workgroup: one per lane of a wave
#define INNOV_FIELDS 5         // n, n_miss, n_within, s1, s2

struct InnovArgs {
  MbesArgs m;               // state, frames, the map and r_max (mcl_host_update.h: fill_frames_and_map)
  const float4* beam;       // B records: x, y, z the unit direction in the sensor frame, w the measured range
  u64* table;               // INNOV_FIELDS x B accumulators, [field * B + b], zeroed by the host
  float* exp_out;           // or nullptr
  long long first, stride, count;   // the sampled slots first + k stride, k < count
  long long q_support;
  int n_beams, group;       // B, G (1 ... INNOV_MAX_GROUP)
};

__device__ __forceinline__ double innov_readlane(double x, int j) {
  const long long b = __double_as_longlong(x);
  const unsigned lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), j);
  const unsigned hi = __builtin_amdgcn_readlane((int)(b >> 32), j);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ float innov_readlane(float x, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
}

template <int MAP>
__global__ void __launch_bounds__(INNOV_CHUNK) k_innovation(InnovArgs a) {
  const MbesArgs& m = a.m;
  const int lane = threadIdx.x & 63;
  const int chunks = (a.n_beams + INNOV_CHUNK - 1) / INNOV_CHUNK;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  const long long k0 = (long long)(blockIdx.x / (unsigned)chunks) * a.group;   // the group's first sample
  const int b = chunk * INNOV_CHUNK + (int)threadIdx.x;
  const bool have = b < a.n_beams;
  const float4 bt = have ? a.beam[b] : make_float4(0.f, 0.f, -1.f, 0.f);
  const bool cast = have && beam_valid(bt.w);
  if (__ballot(cast) == 0ull) return;   // (a wave without a valid beam; nothing below synchronises the workgroup)
  const long long left = a.count - k0;
  const int g_here = (int)(left < (long long)a.group ? left : (long long)a.group);
  // ---- the lane's direction in the vehicle frame
  double v[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    v[r] = m.off_R[r * 3 + 0] * (double)bt.x + m.off_R[r * 3 + 1] * (double)bt.y + m.off_R[r * 3 + 2] * (double)bt.z;
  // ---- lane k: the sensor frame of the group's k-th particle
  PoseFrame F;
#pragma unroll
  for (int r = 0; r < 9; ++r) F.Rmp[r] = 0.0;
  OwnCell C = {0, 0, 0.f, 0.f, false};
  float oz = 0.f;
  if (lane < g_here) {
    const long long i = a.first + (k0 + lane) * a.stride;
    double sr, cr, sp, cp, sy, cy;
    sincos(m.st[3][i], &sr, &cr);
    sincos(m.st[4][i], &sp, &cp);
    sincos(m.st[5][i], &sy, &cy);
    F = pose_frame(m.m2o, m.off_t, m.st[0][i], m.st[1][i], m.st[2][i], sr, cr, sp, cp, sy, cy);
    C = own_cell((F.o[0] - m.ox) * m.inv_res, (F.o[1] - m.oy) * m.inv_res);
    oz = (float)F.o[2];
  }
  const int sane_i = C.sane ? 1 : 0;
  const float r_max = m.r_max;
  int n = 0, n_miss = 0, n_within = 0;
  long long s1 = 0;
  u64 s2 = 0;
  for (int j = 0; j < g_here; ++j) {
    double R[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) R[r] = innov_readlane(F.Rmp[r], j);
    const int I0 = __builtin_amdgcn_readlane(C.I0, j), J0 = __builtin_amdgcn_readlane(C.J0, j);
    const float ul = innov_readlane(C.ul, j), vl = innov_readlane(C.vl, j), ozj = innov_readlane(oz, j);
    const bool sane = __builtin_amdgcn_readlane(sane_i, j) != 0;
    if (cast) {
      const float dx = (float)(R[0] * v[0] + R[1] * v[1] + R[2] * v[2]);
      const float dy = (float)(R[3] * v[0] + R[4] * v[1] + R[5] * v[2]);
      const float dz = (float)(R[6] * v[0] + R[7] * v[1] + R[8] * v[2]);
      float e;
      if (!sane) {
        e = r_max;  // (NaN / absurd position: the ray misses)
      } else if (MAP != 1) {
        e = cast_lattice_ray<MAP>(m, I0, J0, ul, vl, ozj, dx, dy, dz);
      } else {
        RayStats rs = {0, 0, 0, 0};
        e = cast_records_ray(m, I0, J0, ul, vl, ozj, dx, dy, dz, rs);
      }
      const long long q = innov_quantise(bt.w, e);
      const long long aq = q < 0 ? -q : q;
      ++n;
      n_miss += e == r_max ? 1 : 0;
      n_within += aq <= a.q_support ? 1 : 0;
      s1 += q;
      s2 += (u64)(aq * aq);
      if (a.exp_out) a.exp_out[(size_t)(k0 + j) * (size_t)a.n_beams + (size_t)b] = e;
    }
  }
  if (cast) {
    const size_t B = (size_t)a.n_beams;
    atomicAdd(&a.table[0 * B + b], (u64)n);
    atomicAdd(&a.table[1 * B + b], (u64)n_miss);
    atomicAdd(&a.table[2 * B + b], (u64)n_within);
    atomicAdd(&a.table[3 * B + b], (u64)s1);   // (two's complement: the signed sum)
    atomicAdd(&a.table[4 * B + b], s2);
  }
}
