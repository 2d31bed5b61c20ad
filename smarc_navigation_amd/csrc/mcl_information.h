// mcl_information.h -- kernel of the ping information (include/mcl_information.h; gfx950, wave64): for every pair (pose,
// beam) six casts from the pose perturbed by +-delta in x, y and yaw, the three quantised central differences d_x, d_y,
// d_w, and the integer sums of their six products -- per beam over a strided sample of the cloud, or per pose over the
// beams.
//
//   k_information<MAP, PER_POSE> : MAP 0 the height grid, 2 the node heights of a triangulated regular grid, 1 triangle
//                       records -- innovation_launch's dispatch.  A LANE is a beam; a workgroup of up to 256 lanes owns a
//                       chunk of up to INFO_CHUNK beams and a group of G <= INFO_MAX_GROUP poses, and loops over the poses
//                       and their six variants: in an iteration every lane of a wave casts its own beam from the SAME
//                       perturbed pose, so adjacent lanes walk adjacent rays of one fan through the map (k_innovation's
//                       arrangement, csrc/mcl_innovation.h).
//     pose            : before the loop lane 6 s + v of every wave builds the sensor frame of the group's s-th pose in its
//                       v-th variant (x+, x-, y+, y-, yaw+, yaw-: one fp64 addition on the stored number, then three fp64
//                       sincos, pose_frame, own_cell -- the arithmetic of k_innovation); the loop reads it out of that lane
//                       (v_readlane, the index is wave-uniform).  One round of sincos serves up to ten poses.
//     accumulation    : nine integers per lane in registers.
//                       PER_POSE = false: summed over the group's poses, then one 64-bit integer atomic add per field and
//                       beam into the zeroed 9 x B table (field-major).
//                       PER_POSE = true: after each pose the three counts come from wave ballots, the six sums from an
//                       integer butterfly over the lanes, and lane 0 adds them with one atomic per field and wave into
//                       table[field * M + pose].
//                       Integer adds commute: the table holds the same bits for every G, grid and order of arrival.
//     dump            : ranges_out != nullptr: the six ranges also go to ranges_out[(k * 6 + v) * B + b], k the pose's index.
//
// Bounds: b < n_beams guards the beam table, the accumulator table's column and ranges_out's column; the slots
// first + k stride, k < count, lie below the length of m.st's arrays (innov_shard_sample for the cloud, first = 0 and
// stride = 1 over the M uploaded poses); the table has INFO_FIELDS x (PER_POSE ? count : n_beams) words and k0 + j < count;
// ranges_out has count x 6 rows.  No LDS, no barrier.
#pragma once
#include "mcl_innovation.h"

#define INFO_CHUNK 256         // beams of a workgroup
#define INFO_MAX_GROUP 10      // poses of a workgroup: six lanes of a wave each
#define INFO_FIELDS 9          // n, n_miss, n_jump, sxx, syy, sww, sxy, sxw, syw

struct InfoArgs {
  MbesArgs m;               // frames, the map and r_max (mcl_host_update.h: fill_frames_and_map); st: the cloud, or the uploaded poses
  const float4* beam;       // B records: x, y, z the unit direction in the sensor frame
  u64* table;               // INFO_FIELDS accumulators per beam [field * B + b] or per pose [field * count + k], zeroed by the host
  float* ranges_out;        // or nullptr
  long long first, stride, count;   // the poses are the slots first + k stride, k < count
  long long jump_q;         // floor(jump_max 2^12)
  double delta_xy, delta_yaw;
  int n_beams, group;       // B, G (1 ... INFO_MAX_GROUP)
};

// the sum of x over the 64 lanes, in every lane (integers: the order does not matter)
__device__ __forceinline__ u64 info_wave_sum(u64 x) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(x & 0xffffffffull), d, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), d, 64);
    x += ((u64)hi << 32) | lo;
  }
  return x;
}

template <int MAP, bool PER_POSE>
__global__ void __launch_bounds__(INFO_CHUNK) k_information(InfoArgs a) {
  const MbesArgs& m = a.m;
  const int lane = threadIdx.x & 63;
  const int chunks = (a.n_beams + INFO_CHUNK - 1) / INFO_CHUNK;
  const int chunk = (int)(blockIdx.x % (unsigned)chunks);
  const long long k0 = (long long)(blockIdx.x / (unsigned)chunks) * a.group;   // the group's first pose
  const int b = chunk * INFO_CHUNK + (int)threadIdx.x;
  const bool cast = b < a.n_beams;
  if (__ballot(cast) == 0ull) return;   // (a wave without a beam; nothing below synchronises the workgroup)
  const float4 bt = cast ? a.beam[b] : make_float4(0.f, 0.f, -1.f, 0.f);
  const long long left = a.count - k0;
  const int g_here = (int)(left < (long long)a.group ? left : (long long)a.group);
  // ---- the lane's direction in the vehicle frame
  double v[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    v[r] = m.off_R[r * 3 + 0] * (double)bt.x + m.off_R[r * 3 + 1] * (double)bt.y + m.off_R[r * 3 + 2] * (double)bt.z;
  // ---- lane 6 s + v: the sensor frame of the group's s-th pose in its v-th variant
  PoseFrame F;
#pragma unroll
  for (int r = 0; r < 9; ++r) F.Rmp[r] = 0.0;
  OwnCell C = {0, 0, 0.f, 0.f, false};
  float oz = 0.f;
  if (lane < 6 * g_here) {
    const int s = lane / 6, var = lane - 6 * s;
    const long long i = a.first + (k0 + s) * a.stride;
    double x = m.st[0][i], y = m.st[1][i], yaw = m.st[5][i];
    x = var == 0 ? x + a.delta_xy : (var == 1 ? x - a.delta_xy : x);
    y = var == 2 ? y + a.delta_xy : (var == 3 ? y - a.delta_xy : y);
    yaw = var == 4 ? yaw + a.delta_yaw : (var == 5 ? yaw - a.delta_yaw : yaw);
    double sr, cr, sp, cp, sy, cy;
    sincos(m.st[3][i], &sr, &cr);
    sincos(m.st[4][i], &sp, &cp);
    sincos(yaw, &sy, &cy);
    F = pose_frame(m.m2o, m.off_t, x, y, m.st[2][i], sr, cr, sp, cp, sy, cy);
    C = own_cell((F.o[0] - m.ox) * m.inv_res, (F.o[1] - m.oy) * m.inv_res);
    oz = (float)F.o[2];
  }
  const int sane_i = C.sane ? 1 : 0;
  const float r_max = m.r_max;
  const size_t B = (size_t)a.n_beams;
  int n = 0, n_miss = 0, n_jump = 0;
  u64 sxx = 0, syy = 0, sww = 0;
  long long sxy = 0, sxw = 0, syw = 0;
  for (int j = 0; j < g_here; ++j) {
    long long dx = 0, dy = 0, dw = 0;
    bool miss = false;
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
      float ep = 0.f, em = 0.f;
#pragma unroll 1
      for (int sgn = 0; sgn < 2; ++sgn) {
        const int src = 6 * j + 2 * k + sgn;
        double R[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) R[r] = innov_readlane(F.Rmp[r], src);
        const int I0 = __builtin_amdgcn_readlane(C.I0, src), J0 = __builtin_amdgcn_readlane(C.J0, src);
        const float ul = innov_readlane(C.ul, src), vl = innov_readlane(C.vl, src), ozj = innov_readlane(oz, src);
        const bool sane = __builtin_amdgcn_readlane(sane_i, src) != 0;
        if (cast) {
          const float rx = (float)(R[0] * v[0] + R[1] * v[1] + R[2] * v[2]);
          const float ry = (float)(R[3] * v[0] + R[4] * v[1] + R[5] * v[2]);
          const float rz = (float)(R[6] * v[0] + R[7] * v[1] + R[8] * v[2]);
          float e;
          if (!sane) {
            e = r_max;  // (NaN / absurd position: the ray misses)
          } else if (MAP != 1) {
            e = cast_lattice_ray<MAP>(m, I0, J0, ul, vl, ozj, rx, ry, rz);
          } else {
            RayStats rs = {0, 0, 0, 0};
            e = cast_records_ray(m, I0, J0, ul, vl, ozj, rx, ry, rz, rs);
          }
          miss = miss || e == r_max;
          if (sgn == 0)
            ep = e;
          else
            em = e;
          if (a.ranges_out) a.ranges_out[((size_t)(k0 + j) * 6 + (size_t)(2 * k + sgn)) * B + (size_t)b] = e;
        }
      }
      const long long d = info_difference(ep, em);
      if (k == 0)
        dx = d;
      else if (k == 1)
        dy = d;
      else
        dw = d;
    }
    const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, aw = dw < 0 ? -dw : dw;
    const bool jump = cast && !miss && (ax > a.jump_q || ay > a.jump_q || aw > a.jump_q);
    const bool use = cast && !miss && !jump;
    if (!PER_POSE) {
      n += cast ? 1 : 0;
      n_miss += cast && miss ? 1 : 0;
      n_jump += jump ? 1 : 0;
      if (use) {
        sxx += (u64)(dx * dx);
        syy += (u64)(dy * dy);
        sww += (u64)(dw * dw);
        sxy += dx * dy;
        sxw += dx * dw;
        syw += dy * dw;
      }
    } else {
      const u64 w_n = (u64)__popcll(__ballot(cast)), w_miss = (u64)__popcll(__ballot(cast && miss)), w_jump = (u64)__popcll(__ballot(jump));
      const u64 w_xx = info_wave_sum(use ? (u64)(dx * dx) : 0ull), w_yy = info_wave_sum(use ? (u64)(dy * dy) : 0ull);
      const u64 w_ww = info_wave_sum(use ? (u64)(dw * dw) : 0ull), w_xy = info_wave_sum(use ? (u64)(dx * dy) : 0ull);
      const u64 w_xw = info_wave_sum(use ? (u64)(dx * dw) : 0ull), w_yw = info_wave_sum(use ? (u64)(dy * dw) : 0ull);
      if (lane == 0) {
        const size_t M = (size_t)a.count, k = (size_t)(k0 + j);
        atomicAdd(&a.table[0 * M + k], w_n);
        atomicAdd(&a.table[1 * M + k], w_miss);
        atomicAdd(&a.table[2 * M + k], w_jump);
        atomicAdd(&a.table[3 * M + k], w_xx);
        atomicAdd(&a.table[4 * M + k], w_yy);
        atomicAdd(&a.table[5 * M + k], w_ww);
        atomicAdd(&a.table[6 * M + k], w_xy);   // (two's complement: the signed sums)
        atomicAdd(&a.table[7 * M + k], w_xw);
        atomicAdd(&a.table[8 * M + k], w_yw);
      }
    }
  }
  if (!PER_POSE && cast) {
    atomicAdd(&a.table[0 * B + b], (u64)n);
    atomicAdd(&a.table[1 * B + b], (u64)n_miss);
    atomicAdd(&a.table[2 * B + b], (u64)n_jump);
    atomicAdd(&a.table[3 * B + b], sxx);
    atomicAdd(&a.table[4 * B + b], syy);
    atomicAdd(&a.table[5 * B + b], sww);
    atomicAdd(&a.table[6 * B + b], (u64)sxy);   // (two's complement: the signed sums)
    atomicAdd(&a.table[7 * B + b], (u64)sxw);
    atomicAdd(&a.table[8 * B + b], (u64)syw);
  }
}
