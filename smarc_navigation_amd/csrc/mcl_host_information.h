// mcl_host_information.h -- host side of the ping information (include/mcl_information.h; kernel: csrc/mcl_information.h;
// steps, merge and matrix: mcl_host_pure.h; the checks, beam table, sample, scratch block, launch geometry, fetch and group
// run it shares with the innovation statistics: mcl_host_innovation.h).  mcl_api.hip forwards to information_run /
// group_information_run / pose_information_run.  Nothing here writes a member of the handle but the shared scratch block
// (beamstat_dev), info_pose (the uploaded poses of mcl_pose_information) and the expected-range buffer every *_expected
// call shares (the dump).
#pragma once
#include "mcl_host_innovation.h"
#include "mcl_information.h"

namespace {

// a record is the table's column: INFO_FIELDS words in the table's field order
static_assert(sizeof(mcl_information_sums) == 8 * INFO_FIELDS && offsetof(mcl_information_sums, n) == 0 &&
                  offsetof(mcl_information_sums, n_miss) == 8 && offsetof(mcl_information_sums, n_jump) == 16 &&
                  offsetof(mcl_information_sums, sxx) == 24 && offsetof(mcl_information_sums, syy) == 32 &&
                  offsetof(mcl_information_sums, sww) == 40 && offsetof(mcl_information_sums, sxy) == 48 &&
                  offsetof(mcl_information_sums, sxw) == 56 && offsetof(mcl_information_sums, syw) == 64,
              "k_information's fields");

struct InfoPing {
  const float* angles;
  int B;
  double r_max;
  const double* sensor_offset;
  const mcl_information_steps* steps;
};

// what both accumulations ask of a ping geometry and of the handle (particles: the cloud's accumulation only)
int information_check(mcl_handle* h, const char* who, const InfoPing& p, bool particles) {
  if (!p.angles) return fail(h, MCL_ERR_INVALID, std::string(who) + ": null argument");
  RET_IF(ping_check_beams(h, who, p.B));
  if (const char* why = info_steps_why(p.steps, p.r_max)) return fail(h, MCL_ERR_INVALID, std::string(who) + ": " + why);
  return ping_check_state(h, who, particles);
}
int information_check_cloud(mcl_handle* h, const char* who, const InfoPing& p, int max_samples) {
  RET_IF(ping_check_samples(h, who, max_samples));
  return information_check(h, who, p, true);
}

// poses of a workgroup: a workgroup casts six rays per lane and pose, one after the other, so a small launch wants many
// short workgroups -- about sixteen per compute unit --, with at least two poses per round of sincos and at most the ten a
// wave's lanes hold (DESIGN 5m has the measurement); MCL_INFORMATION_GROUP=n (A/B) forces it.  The result does not depend
// on it.
int information_group(const mcl_handle* h, long long count, int chunks) {
  if (h->env_info_group > 0) return std::min(h->env_info_group, INFO_MAX_GROUP);
  const long long g = (count * chunks + 4095) / 4096;
  return (int)std::min<long long>(std::max<long long>(g, 2), INFO_MAX_GROUP);
}

// queue the upload of the beam table, the memset of the accumulators and the kernel over `count` poses -- the slots
// first + k stride of `st` (6 arrays of `pitch` doubles).  per_pose: one record per pose, else one per beam.  dump (per beam
// only): the six ranges go to h->exp_dev (count x 6 x B).
int information_launch(mcl_handle* h, const InfoPing& p, const double* st, long long pitch, long long first, long long stride,
                       long long count, bool per_pose, bool dump) {
  const int B = p.B;
  std::vector<float> beam;
  RET_IF(ping_beam_table(h, "ping_information", p.angles, nullptr, B, beam));
  InfoArgs ia;
  memset(&ia, 0, sizeof ia);
  RET_IF(beamstat_prepare(h, beam, B, INFO_FIELDS, per_pose ? (size_t)count : (size_t)B, count, &ia.table));
  if (count == 0) return MCL_OK;
  if (dump) RESERVE(h, h->exp_dev, (size_t)count * 6 * (size_t)B);
  fill_frames_and_map(h, p.sensor_offset, p.r_max, ia.m);
  for (int c = 0; c < 6; ++c) ia.m.st[c] = st + (size_t)c * (size_t)pitch;
  ia.m.n = pitch;
  ia.beam = reinterpret_cast<const float4*>(h->beamstat_dev.p);
  ia.ranges_out = dump ? h->exp_dev.p : nullptr;
  ia.first = first;
  ia.stride = stride;
  ia.count = count;
  ia.jump_q = info_jump_q(p.steps->jump_max);
  ia.delta_xy = p.steps->delta_xy;
  ia.delta_yaw = p.steps->delta_yaw;
  ia.n_beams = B;
  const BeamGeometry g = beam_geometry(B);
  ia.group = information_group(h, count, g.chunks);
  const unsigned grid = g.grid(count, ia.group);
  map_dispatch(h, [&](auto map) {
    constexpr int MAP = decltype(map)::value;
    if (per_pose)
      k_information<MAP, true><<<grid, g.threads, 0, h->stream>>>(ia);
    else
      k_information<MAP, false><<<grid, g.threads, 0, h->stream>>>(ia);
  });
  HIPCHK(h, hipGetLastError());
  return MCL_OK;
}
// this shard's sampled slots of the cloud, queued; *count = how many those are
int information_launch_cloud(mcl_handle* h, const InfoPing& p, int max_samples, bool dump, long long* count) {
  RET_IF(set_device(h));
  long long first = 0, stride = 0;
  RET_IF(cloud_sample(h, max_samples, "ping_information", &first, &stride, count));
  if (*count > 0) RET_IF(materialise_uniform(h));
  return information_launch(h, p, h->state[h->cur], h->n, first, stride, *count, false, dump);
}

// mcl_ping_information
int information_run(mcl_handle* h, const InfoPing& p, int max_samples, mcl_information_sums* out, float* ranges_out,
                    int64_t* n_sampled) {
  RET_IF(information_check_cloud(h, "ping_information", p, max_samples));
  long long count = 0;
  RET_IF(information_launch_cloud(h, p, max_samples, ranges_out != nullptr, &count));
  RET_IF(stats_fetch(h, p.B, INFO_FIELDS, (size_t)p.B, out, ranges_out, (size_t)count * 6 * (size_t)p.B));
  *n_sampled = count;
  return MCL_OK;
}

// mcl_group_ping_information
int group_information_run(mcl_handle** sh, int ns, const InfoPing& p, int max_samples, mcl_information_sums* out,
                          int64_t* n_sampled) {
  return group_stats_run(
      sh, ns, p.B, out, n_sampled, [&](mcl_handle* h) { return information_check_cloud(h, "group_ping_information", p, max_samples); },
      [&](mcl_handle* h, long long* count) { return information_launch_cloud(h, p, max_samples, false, count); }, information_merge_impl,
      "group_ping_information: the shards' records do not add up to one sample (do the handles hold one cloud?)");
}

// mcl_pose_information: the poses go to the handle's scratch buffer, MbesArgs::st points there; the cloud is not touched
int pose_information_run(mcl_handle* h, const InfoPing& p, const double* poses, long long M, mcl_information_sums* out) {
  if (!poses) return fail(h, MCL_ERR_INVALID, "pose_information: null argument");
  if (M < 1 || M > MCL_INFORMATION_MAX_POSES) return fail(h, MCL_ERR_INVALID, "pose_information: M outside 1 ... 2^20");
  RET_IF(information_check(h, "pose_information", p, false));
  for (long long k = 0; k < 6 * M; ++k)
    if (!std::isfinite(poses[k])) return fail(h, MCL_ERR_INVALID, "pose_information: a pose is not finite");
  RET_IF(set_device(h));
  RESERVE(h, h->info_pose, 6 * (size_t)M);
  RET_IF(upload(h, h->info_pose, poses, sizeof(double) * 6 * (size_t)M));
  RET_IF(information_launch(h, p, h->info_pose, M, 0, 1, M, true, false));
  return stats_fetch(h, p.B, INFO_FIELDS, (size_t)M, out, nullptr, 0);
}

}  // namespace
