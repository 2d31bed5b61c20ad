// mcl_information.h -- kernel of the ping information (include/mcl_information.h; gfx950, wave64): for every pair (pose,
// beam) six casts from the pose perturbed by +-delta in x, y and yaw, the three quantised central differences d_x, d_y,
// d_w, and the integer sums of their six products -- per beam over a strided sample of the cloud, or per pose over the
// beams.
//
//   k_information<MAP, PER_POSE> : the beam lanes of csrc/mcl_innovation.h (its header: the chunk and the group, the frame
//                       a lane builds and the wave reads, the ray, why the table's bits do not depend on G), with
//                       G <= INFO_MAX_GROUP poses and six variants of each: in an iteration every lane of a wave casts its
//                       own beam from the SAME perturbed pose.
//     pose            : lane 6 s + v of every wave builds the sensor frame of the group's s-th pose in its v-th variant
//                       (x+, x-, y+, y-, yaw+, yaw-: one fp64 addition on the stored number, then lane_frame).  One round
//                       of sincos serves up to ten poses.
//     accumulation    : nine integers per lane in registers.
//                       PER_POSE = false: summed over the group's poses, then one 64-bit integer atomic add per field and
//                       beam into the zeroed 9 x B table (field-major).
//                       PER_POSE = true: after each pose the three counts come from wave ballots, the six sums from the
//                       wave's integer sum (mcl_device.h: wave_sum), and lane 0 adds them with one atomic per field and
//                       wave into table[field * M + pose].
//     dump            : ranges_out != nullptr: the six ranges also go to ranges_out[(k * 6 + v) * B + b], k the pose's index.
//
// Bounds: b < n_beams guards the beam table, the accumulator table's column and ranges_out's column; the slots
// first + k stride, k < count, lie below the length of m.st's arrays (innov_shard_sample for the cloud, first = 0 and
// stride = 1 over the M uploaded poses); the table has INFO_FIELDS x (PER_POSE ? count : n_beams) words and k0 + j < count;
// ranges_out has count x 6 rows.  No LDS, no barrier.
#pragma once
#include "mcl_innovation.h"

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

template <int MAP, bool PER_POSE>
__global__ void __launch_bounds__(BEAM_CHUNK) k_information(InfoArgs a) {
  const MbesArgs& m = a.m;
  const int lane = threadIdx.x & 63;
  const BeamLane L = beam_lane(a.n_beams, a.count, a.group);
  const int b = L.b;
  const bool cast = b < a.n_beams;
  if (__ballot(cast) == 0ull) return;   // (a wave without a beam; nothing below synchronises the workgroup)
  const float4 bt = cast ? a.beam[b] : make_float4(0.f, 0.f, -1.f, 0.f);
  double v[3];
  beam_in_vehicle(m, bt, v);
  // ---- lane 6 s + v: the sensor frame of the group's s-th pose in its v-th variant
  LaneFrame F = lane_frame_none();
  if (lane < 6 * L.g_here) {
    const int s = lane / 6, var = lane - 6 * s;
    const long long i = a.first + (L.k0 + s) * a.stride;
    double x = m.st[0][i], y = m.st[1][i], yaw = m.st[5][i];
    x = var == 0 ? x + a.delta_xy : (var == 1 ? x - a.delta_xy : x);
    y = var == 2 ? y + a.delta_xy : (var == 3 ? y - a.delta_xy : y);
    yaw = var == 4 ? yaw + a.delta_yaw : (var == 5 ? yaw - a.delta_yaw : yaw);
    F = lane_frame(m, x, y, m.st[2][i], m.st[3][i], m.st[4][i], yaw);
  }
  const float r_max = m.r_max;
  const size_t B = (size_t)a.n_beams;
  int n = 0, n_miss = 0, n_jump = 0;
  u64 sxx = 0, syy = 0, sww = 0;
  long long sxy = 0, sxw = 0, syw = 0;
  for (int j = 0; j < L.g_here; ++j) {
    long long dx = 0, dy = 0, dw = 0;
    bool miss = false;
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
      float ep = 0.f, em = 0.f;
#pragma unroll 1
      for (int sgn = 0; sgn < 2; ++sgn) {
        const LaneFrame U = lane_frame_of(F, 6 * j + 2 * k + sgn);
        if (cast) {
          const float e = cast_from_frame<MAP>(m, U, v);
          miss = miss || e == r_max;
          if (sgn == 0)
            ep = e;
          else
            em = e;
          if (a.ranges_out) a.ranges_out[((size_t)(L.k0 + j) * 6 + (size_t)(2 * k + sgn)) * B + (size_t)b] = e;
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
      // (all 64 lanes are here: the workgroup's size is a multiple of 64 and only whole waves returned above)
      const u64 w_n = (u64)__popcll(__ballot(cast)), w_miss = (u64)__popcll(__ballot(cast && miss)), w_jump = (u64)__popcll(__ballot(jump));
      const u64 w_xx = wave_sum(use ? (u64)(dx * dx) : 0ull), w_yy = wave_sum(use ? (u64)(dy * dy) : 0ull);
      const u64 w_ww = wave_sum(use ? (u64)(dw * dw) : 0ull), w_xy = wave_sum(use ? (u64)(dx * dy) : 0ull);
      const u64 w_xw = wave_sum(use ? (u64)(dx * dw) : 0ull), w_yw = wave_sum(use ? (u64)(dy * dw) : 0ull);
      if (lane == 0) {
        const size_t M = (size_t)a.count, k = (size_t)(L.k0 + j);
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
