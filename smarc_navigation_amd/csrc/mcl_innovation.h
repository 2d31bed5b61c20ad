// mcl_innovation.h -- kernel of the ping innovation statistics (include/mcl_innovation.h; gfx950, wave64): per beam, over a
// strided sample of the cloud, the integer sums of the quantised residual q = rint((r_b - e_ib) 2^12) -- and the
// arrangement it shares with the ping information (mcl_information.h): beam lanes that cast from sampled poses.
//
//   beam lanes        : a LANE is a beam; a workgroup of up to 256 lanes owns a chunk of up to BEAM_CHUNK beams and a group
//                       of G poses, and loops over the poses: in an iteration every lane of a wave casts its own beam from
//                       the SAME pose, so adjacent lanes walk adjacent rays of one fan through the map (beam_lane: which
//                       chunk, which group, how many of its poses exist).
//     pose            : built once per wave and pose, not once per ray: before the loop a lane of every wave builds the
//                       sensor frame of one of the group's poses (lane_frame: three fp64 sincos, pose_frame, own_cell -- the
//                       arithmetic of k_ranges_update) and the iteration that casts from it reads it out of that lane
//                       (lane_frame_of: v_readlane, the source lane is wave-uniform).  A wave pays one round of sincos for
//                       all the frames its lanes hold; no LDS, no barrier.
//     ray             : the lane's direction in the vehicle frame (beam_in_vehicle, fp64) is loop-invariant; per pose nine
//                       fp64 products turn it into the map frame, then the map-ray entry of mcl_mbes.h (cast_map_ray) casts
//                       in fp32 relative to the pose's own cell (cast_from_frame).
//     accumulation    : integer accumulators per lane in registers across the group's poses, then 64-bit integer atomic
//                       adds into a zeroed field-major table.  Integer adds commute: the table holds the same bits for
//                       every G, grid and order of arrival (include/mcl_innovation.h).
//
//   k_innovation<MAP> : MAP as cast_map_ray's -- map_dispatch (mcl_host_innovation.h).  G <= 64 sampled particles, lane k
//                       builds the frame of the group's k-th particle and iteration k casts from it; five accumulators
//                       and one atomic add per field and beam into the 5 x B table.
//     dump            : exp_out != nullptr: e_ib also goes to exp_out[k B + b], k the sample's index in this shard.
//
// Bounds: b < n_beams guards the beam table, the accumulator table and exp_out's column; the slots first + k stride,
// k < count, lie below a.m.n by innov_shard_sample (mcl_host_pure.h); exp_out has count rows.
#pragma once
#include "mcl_mbes.h"

#define BEAM_CHUNK 256         // beams of a workgroup
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

// ---- the workgroup's place: blockIdx.x = group * chunks + chunk
struct BeamLane {
  long long k0;             // the group's first pose (index into the sample)
  int b;                    // the lane's beam (>= n_beams: none)
  int g_here;               // poses of this group that exist: min(group, count - k0)
};
__device__ __forceinline__ BeamLane beam_lane(int n_beams, long long count, int group) {
  const int chunks = (n_beams + BEAM_CHUNK - 1) / BEAM_CHUNK;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  BeamLane L;
  L.k0 = (long long)(blockIdx.x / (unsigned)chunks) * group;
  L.b = chunk * BEAM_CHUNK + (int)threadIdx.x;
  const long long left = count - L.k0;
  L.g_here = (int)(left < (long long)group ? left : (long long)group);
  return L;
}

// ---- the sensor frame of one pose as a lane holds it and as the wave reads it
struct LaneFrame {
  double R[9];              // PoseFrame::Rmp
  int I0, J0;               // OwnCell
  float ul, vl;
  float oz;                 // (float)PoseFrame::o[2]
  int sane;                 // OwnCell::sane
};
__device__ __forceinline__ LaneFrame lane_frame_none() { return LaneFrame{}; }   // (all zero: what a lane without a pose holds)
__device__ __forceinline__ LaneFrame lane_frame(const MbesArgs& m, double x, double y, double z, double roll, double pitch, double yaw) {
  double sr, cr, sp, cp, sy, cy;
  sincos(roll, &sr, &cr);
  sincos(pitch, &sp, &cp);
  sincos(yaw, &sy, &cy);
  const PoseFrame P = pose_frame(m.m2o, m.off_t, x, y, z, sr, cr, sp, cp, sy, cy);
  const OwnCell C = own_cell((P.o[0] - m.ox) * m.inv_res, (P.o[1] - m.oy) * m.inv_res);
  LaneFrame F;
#pragma unroll
  for (int r = 0; r < 9; ++r) F.R[r] = P.Rmp[r];
  F.I0 = C.I0;
  F.J0 = C.J0;
  F.ul = C.ul;
  F.vl = C.vl;
  F.oz = (float)P.o[2];
  F.sane = C.sane ? 1 : 0;
  return F;
}
// the frame lane `src` built, in every lane (src wave-uniform)
__device__ __forceinline__ LaneFrame lane_frame_of(const LaneFrame& F, int src) {
  LaneFrame U;
#pragma unroll
  for (int r = 0; r < 9; ++r) U.R[r] = read_lane(F.R[r], src);
  U.I0 = read_lane(F.I0, src);
  U.J0 = read_lane(F.J0, src);
  U.ul = read_lane(F.ul, src);
  U.vl = read_lane(F.vl, src);
  U.oz = read_lane(F.oz, src);
  U.sane = read_lane(F.sane, src);
  return U;
}
// the expected range of the ray with direction v (vehicle frame) from the frame U
template <int MAP>
__device__ __forceinline__ float cast_from_frame(const MbesArgs& m, const LaneFrame& U, const double (&v)[3]) {
  const float dx = (float)(U.R[0] * v[0] + U.R[1] * v[1] + U.R[2] * v[2]);
  const float dy = (float)(U.R[3] * v[0] + U.R[4] * v[1] + U.R[5] * v[2]);
  const float dz = (float)(U.R[6] * v[0] + U.R[7] * v[1] + U.R[8] * v[2]);
  return cast_map_ray<MAP>(m, U.sane != 0, U.I0, U.J0, U.ul, U.vl, U.oz, dx, dy, dz);
}

template <int MAP>
__global__ void __launch_bounds__(BEAM_CHUNK) k_innovation(InnovArgs a) {
  const MbesArgs& m = a.m;
  const int lane = threadIdx.x & 63;
  const BeamLane L = beam_lane(a.n_beams, a.count, a.group);
  const int b = L.b;
  const bool have = b < a.n_beams;
  const float4 bt = have ? a.beam[b] : make_float4(0.f, 0.f, -1.f, 0.f);
  const bool cast = have && beam_valid(bt.w);
  if (__ballot(cast) == 0ull) return;   // (a wave without a valid beam; nothing below synchronises the workgroup)
  double v[3];
  beam_in_vehicle(m, bt, v);
  // ---- lane k: the sensor frame of the group's k-th particle
  LaneFrame F = lane_frame_none();
  if (lane < L.g_here) {
    const long long i = a.first + (L.k0 + lane) * a.stride;
    F = lane_frame(m, m.st[0][i], m.st[1][i], m.st[2][i], m.st[3][i], m.st[4][i], m.st[5][i]);
  }
  int n = 0, n_miss = 0, n_within = 0;
  long long s1 = 0;
  u64 s2 = 0;
  for (int j = 0; j < L.g_here; ++j) {
    const LaneFrame U = lane_frame_of(F, j);
    if (cast) {
      const float e = cast_from_frame<MAP>(m, U, v);
      const long long q = innov_quantise(bt.w, e);
      const long long aq = q < 0 ? -q : q;
      ++n;
      n_miss += e == m.r_max ? 1 : 0;
      n_within += aq <= a.q_support ? 1 : 0;
      s1 += q;
      s2 += (u64)(aq * aq);
      if (a.exp_out) a.exp_out[(size_t)(L.k0 + j) * (size_t)a.n_beams + (size_t)b] = e;
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
