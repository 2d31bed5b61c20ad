// mcl_host_information.h -- host side of the ping information (include/mcl_information.h; kernel: csrc/mcl_information.h;
// steps, merge and matrix: mcl_host_pure.h).  mcl_api.hip forwards to information_run / group_information_run /
// pose_information_run.  Nothing here writes a member of the handle but its two lazily reserved blocks (info_dev, the beam
// table and the accumulators; info_pose, the uploaded poses of mcl_pose_information) and the expected-range buffer every
// *_expected call shares (the dump).  It starts where the range update starts: fill_frames_and_map.
#pragma once
#include "mcl_host.h"
#include "mcl_information.h"

namespace {

struct InfoPing {
  const float* angles;
  int B;
  double r_max;
  const double* sensor_offset;
  const mcl_information_steps* steps;
};

// what both accumulations ask of a ping geometry and of the handle (particles: the caller's business)
int information_check(mcl_handle* h, const char* who, const InfoPing& p) {
  if (!p.angles) return fail(h, MCL_ERR_INVALID, std::string(who) + ": null argument");
  if (p.B < 1 || p.B > MCL_INFORMATION_MAX_BEAMS) return fail(h, MCL_ERR_INVALID, std::string(who) + ": B outside 1 ... 2048");
  if (const char* why = info_steps_why(p.steps, p.r_max)) return fail(h, MCL_ERR_INVALID, std::string(who) + ": " + why);
  return need_map(h, who);
}
int information_check_cloud(mcl_handle* h, const char* who, const InfoPing& p, int max_samples) {
  if (max_samples < 1 || max_samples > MCL_INFORMATION_MAX_SAMPLES)
    return fail(h, MCL_ERR_INVALID, std::string(who) + ": max_samples outside 1 ... 32768");
  RET_IF(information_check(h, who, p));
  if (!h->have_state)
    return fail(h, MCL_ERR_STATE, std::string(who) + ": no particles (call mcl_init_particles / mcl_set_particles first)");
  return MCL_OK;
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

template <int MAP, bool PER_POSE>
void launch_information(mcl_handle* h, unsigned grid, unsigned threads, const InfoArgs& ia) {
  k_information<MAP, PER_POSE><<<grid, threads, 0, h->stream>>>(ia);
}

// queue the upload of the beam table, the memset of the accumulators and the kernel over `count` poses -- the slots
// first + k stride of `st` (6 arrays of `pitch` doubles).  per_pose: one record per pose, else one per beam.  dump (per beam
// only): the six ranges go to h->exp_dev (count x 6 x B).
int information_launch(mcl_handle* h, const InfoPing& p, const double* st, long long pitch, long long first, long long stride,
                       long long count, bool per_pose, bool dump) {
  const int B = p.B;
  std::vector<float> dirs(3 * (size_t)B), beam(4 * (size_t)B);
  if (innovation_dirs_impl(p.angles, B, dirs.data()) != MCL_OK || normalise_beams(dirs.data(), nullptr, B, beam.data()) != MCL_OK)
    return fail(h, MCL_ERR_INVALID, "ping_information: a beam angle is not finite");
  // the block: B beam records (16 bytes each) in front, the accumulators behind them
  const size_t rows = per_pose ? (size_t)count : (size_t)B;
  RESERVE(h, h->info_dev, 2 * (size_t)B + INFO_FIELDS * rows);
  u64* table = h->info_dev + 2 * (size_t)B;
  HIPCHK(h, hipMemsetAsync(table, 0, sizeof(u64) * INFO_FIELDS * rows, h->stream));
  if (count == 0) return MCL_OK;
  RET_IF(upload(h, h->info_dev, beam.data(), sizeof(float) * 4 * (size_t)B));
  if (dump) RESERVE(h, h->exp_dev, (size_t)count * 6 * (size_t)B);
  InfoArgs ia;
  memset(&ia, 0, sizeof ia);
  fill_frames_and_map(h, p.sensor_offset, p.r_max, ia.m);
  for (int c = 0; c < 6; ++c) ia.m.st[c] = st + (size_t)c * (size_t)pitch;
  ia.m.n = pitch;
  ia.beam = reinterpret_cast<const float4*>(h->info_dev.p);
  ia.table = table;
  ia.ranges_out = dump ? h->exp_dev.p : nullptr;
  ia.first = first;
  ia.stride = stride;
  ia.count = count;
  ia.jump_q = info_jump_q(p.steps->jump_max);
  ia.delta_xy = p.steps->delta_xy;
  ia.delta_yaw = p.steps->delta_yaw;
  ia.n_beams = B;
  const int chunks = (B + INFO_CHUNK - 1) / INFO_CHUNK;
  ia.group = information_group(h, count, chunks);
  const unsigned threads = B >= INFO_CHUNK ? INFO_CHUNK : (unsigned)((B + 63) / 64 * 64);
  const unsigned grid = (unsigned)(((count + ia.group - 1) / ia.group) * chunks);   // (<= 2^20 x 8)
  // the map walk: 0 the height grid, 2 the node heights of a triangulated regular grid, 1 triangle records
  const int map = h->map_kind == 0 ? 0 : (structured_mesh(h) ? 2 : 1);
  if (per_pose) {
    if (map == 0)
      launch_information<0, true>(h, grid, threads, ia);
    else if (map == 2)
      launch_information<2, true>(h, grid, threads, ia);
    else
      launch_information<1, true>(h, grid, threads, ia);
  } else {
    if (map == 0)
      launch_information<0, false>(h, grid, threads, ia);
    else if (map == 2)
      launch_information<2, false>(h, grid, threads, ia);
    else
      launch_information<1, false>(h, grid, threads, ia);
  }
  HIPCHK(h, hipGetLastError());
  return MCL_OK;
}
// this shard's sampled slots of the cloud, queued; *count = how many those are
int information_launch_cloud(mcl_handle* h, const InfoPing& p, int max_samples, bool dump, long long* count) {
  RET_IF(set_device(h));
  int64_t stride = 0, total = 0;
  if (innovation_sample_impl(h->ng, max_samples, &stride, &total) != MCL_OK)
    return fail(h, MCL_ERR_INVALID, "ping_information: bad sample");
  long long first = 0;
  *count = innov_shard_sample(h->goff, h->n, stride, &first);
  if (*count > 0) RET_IF(materialise_uniform(h));
  return information_launch(h, p, h->state[h->cur], h->n, first, stride, *count, false, dump);
}
// the accumulators of a queued launch (and its dump), one synchronisation; rows: B per beam, M per pose
int information_fetch(mcl_handle* h, int B, size_t rows, long long dumped, mcl_information_sums* out, float* ranges_out) {
  RET_IF(set_device(h));
  std::vector<u64> w((size_t)INFO_FIELDS * rows);
  HIPCHK(h, hipMemcpyAsync(w.data(), h->info_dev + 2 * (size_t)B, sizeof(u64) * w.size(), hipMemcpyDeviceToHost, h->stream));
  if (ranges_out && dumped > 0)
    HIPCHK(h, hipMemcpyAsync(ranges_out, h->exp_dev, sizeof(float) * (size_t)dumped * 6 * (size_t)B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t k = 0; k < rows; ++k) {
    out[k].n = (int64_t)w[0 * rows + k];
    out[k].n_miss = (int64_t)w[1 * rows + k];
    out[k].n_jump = (int64_t)w[2 * rows + k];
    out[k].sxx = w[3 * rows + k];
    out[k].syy = w[4 * rows + k];
    out[k].sww = w[5 * rows + k];
    out[k].sxy = (int64_t)w[6 * rows + k];
    out[k].sxw = (int64_t)w[7 * rows + k];
    out[k].syw = (int64_t)w[8 * rows + k];
  }
  return MCL_OK;
}

// mcl_ping_information
int information_run(mcl_handle* h, const InfoPing& p, int max_samples, mcl_information_sums* out, float* ranges_out,
                    int64_t* n_sampled) {
  RET_IF(information_check_cloud(h, "ping_information", p, max_samples));
  long long count = 0;
  RET_IF(information_launch_cloud(h, p, max_samples, ranges_out != nullptr, &count));
  RET_IF(information_fetch(h, p.B, (size_t)p.B, count, out, ranges_out));
  *n_sampled = count;
  return MCL_OK;
}

// mcl_group_ping_information: every shard's launch queued, then the fetches, then the merge
int group_information_run(mcl_handle** sh, int ns, const InfoPing& p, int max_samples, mcl_information_sums* out,
                          int64_t* n_sampled) {
  for (int s = 0; s < ns; ++s) RET_IF(information_check_cloud(sh[s], "group_ping_information", p, max_samples));
  std::vector<long long> count((size_t)ns, 0);
  for (int s = 0; s < ns; ++s) RET_IF(information_launch_cloud(sh[s], p, max_samples, false, &count[s]));
  std::vector<mcl_information_sums> parts((size_t)ns * p.B);
  long long total = 0;
  for (int s = 0; s < ns; ++s) {
    RET_IF(information_fetch(sh[s], p.B, (size_t)p.B, 0, parts.data() + (size_t)s * p.B, nullptr));
    total += count[s];
  }
  if (information_merge_impl(parts.data(), ns, p.B, out) != MCL_OK)
    return fail(sh[0], MCL_ERR_INVALID, "group_ping_information: the shards' records do not add up to one sample (do the handles hold one cloud?)");
  *n_sampled = total;
  return MCL_OK;
}

// mcl_pose_information: the poses go to the handle's scratch buffer, MbesArgs::st points there; the cloud is not touched
int pose_information_run(mcl_handle* h, const InfoPing& p, const double* poses, long long M, mcl_information_sums* out) {
  if (!poses) return fail(h, MCL_ERR_INVALID, "pose_information: null argument");
  if (M < 1 || M > MCL_INFORMATION_MAX_POSES) return fail(h, MCL_ERR_INVALID, "pose_information: M outside 1 ... 2^20");
  RET_IF(information_check(h, "pose_information", p));
  for (long long k = 0; k < 6 * M; ++k)
    if (!std::isfinite(poses[k])) return fail(h, MCL_ERR_INVALID, "pose_information: a pose is not finite");
  RET_IF(set_device(h));
  RESERVE(h, h->info_pose, 6 * (size_t)M);
  RET_IF(upload(h, h->info_pose, poses, sizeof(double) * 6 * (size_t)M));
  RET_IF(information_launch(h, p, h->info_pose, M, 0, 1, M, true, false));
  return information_fetch(h, p.B, (size_t)M, 0, out, nullptr);
}

}  // namespace
