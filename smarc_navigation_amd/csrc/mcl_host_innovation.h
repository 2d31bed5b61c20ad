// mcl_host_innovation.h -- host side of the ping innovation statistics (include/mcl_innovation.h; kernel:
// csrc/mcl_innovation.h; sample, direction table, merge and gate: mcl_host_pure.h) and, in front of it, the pipeline it
// shares with the ping information (mcl_host_information.h), whose kernels are beam lanes too: the checks, the beam table,
// the sample, the scratch block, the launch geometry, the fetch and the group run.  mcl_api.hip forwards to innovation_run /
// group_innovation_run.  Nothing here writes a member of the handle but the lazily reserved scratch block (beamstat_dev)
// and the expected-range buffer every *_expected call shares.  It starts where the range update starts:
// fill_frames_and_map; the kernel's MAP is map_dispatch's (mcl_host_update.h).
#pragma once
#include <cstddef>

#include "mcl_host.h"
#include "mcl_innovation.h"

namespace {

// ------------------------------------------------------------------ what the two statistics share
static_assert(MCL_INNOVATION_MAX_BEAMS == 2048 && MCL_INFORMATION_MAX_BEAMS == 2048, "the text of ping_check_beams");
static_assert(MCL_INNOVATION_MAX_SAMPLES == 32768 && MCL_INFORMATION_MAX_SAMPLES == 32768, "the text of ping_check_samples");
// The checks both ask, in pieces: each feature puts its own (sigma, support_k, r_max; the steps) between them in the order
// its errors have always been reported in.
int ping_check_beams(mcl_handle* h, const char* who, int B) {
  if (B < 1 || B > MCL_INNOVATION_MAX_BEAMS) return fail(h, MCL_ERR_INVALID, std::string(who) + ": B outside 1 ... 2048");
  return MCL_OK;
}
int ping_check_samples(mcl_handle* h, const char* who, int max_samples) {
  if (max_samples < 1 || max_samples > MCL_INNOVATION_MAX_SAMPLES)
    return fail(h, MCL_ERR_INVALID, std::string(who) + ": max_samples outside 1 ... 32768");
  return MCL_OK;
}
// a map, and (particles) a cloud to sample
int ping_check_state(mcl_handle* h, const char* who, bool particles) {
  RET_IF(need_map(h, who));
  if (particles && !h->have_state)
    return fail(h, MCL_ERR_STATE, std::string(who) + ": no particles (call mcl_init_particles / mcl_set_particles first)");
  return MCL_OK;
}

// angles -> directions -> the B normalised beam records (x, y, z, w = the range, 0 without ranges)
int ping_beam_table(mcl_handle* h, const char* who, const float* angles, const float* ranges, int B, std::vector<float>& beam) {
  std::vector<float> dirs(3 * (size_t)B);
  beam.resize(4 * (size_t)B);
  if (innovation_dirs_impl(angles, B, dirs.data()) != MCL_OK || normalise_beams(dirs.data(), ranges, B, beam.data()) != MCL_OK)
    return fail(h, MCL_ERR_INVALID, std::string(who) + ": a beam angle is not finite");
  return MCL_OK;
}
// the strided sample of the cloud and this shard's part of it: the slots first + k stride, k < count
int cloud_sample(mcl_handle* h, int max_samples, const char* who, long long* first, long long* stride, long long* count) {
  int64_t s = 0, total = 0;
  if (innovation_sample_impl(h->ng, max_samples, &s, &total) != MCL_OK) return fail(h, MCL_ERR_INVALID, std::string(who) + ": bad sample");
  *stride = s;
  *count = innov_shard_sample(h->goff, h->n, s, first);
  return MCL_OK;
}
// The scratch block: B beam records (16 bytes each) in front, fields x rows accumulators (field-major) behind them.
// Queues the memset of the accumulators and, when there is something to cast (count > 0), the upload of the records;
// *table = the accumulators.  The block's contents are dead once stats_fetch has read them.
int beamstat_prepare(mcl_handle* h, const std::vector<float>& beam, int B, int fields, size_t rows, long long count, u64** table) {
  RESERVE(h, h->beamstat_dev, 2 * (size_t)B + (size_t)fields * rows);
  *table = h->beamstat_dev + 2 * (size_t)B;
  HIPCHK(h, hipMemsetAsync(*table, 0, sizeof(u64) * (size_t)fields * rows, h->stream));
  if (count == 0) return MCL_OK;
  return upload(h, h->beamstat_dev, beam.data(), sizeof(float) * 4 * (size_t)B);
}
// the launch of beam lanes (csrc/mcl_innovation.h: beam_lane): whole waves, one workgroup per chunk and group
struct BeamGeometry {
  int chunks;
  unsigned threads;
  unsigned grid(long long count, int group) const { return (unsigned)(((count + group - 1) / group) * chunks); }   // (<= 2^20 x 8)
};
BeamGeometry beam_geometry(int B) {
  return {(B + BEAM_CHUNK - 1) / BEAM_CHUNK, B >= BEAM_CHUNK ? (unsigned)BEAM_CHUNK : (unsigned)((B + 63) / 64 * 64)};
}
// the accumulators of a queued launch as `rows` records of `fields` 64-bit words each, and dump_floats floats of its dump
// out of exp_dev (dump_out: or nullptr); one synchronisation
int stats_fetch(mcl_handle* h, int B, int fields, size_t rows, void* records_out, float* dump_out, size_t dump_floats) {
  RET_IF(set_device(h));
  std::vector<u64> w((size_t)fields * rows), rec((size_t)fields);
  HIPCHK(h, hipMemcpyAsync(w.data(), h->beamstat_dev + 2 * (size_t)B, sizeof(u64) * w.size(), hipMemcpyDeviceToHost, h->stream));
  if (dump_out && dump_floats > 0)
    HIPCHK(h, hipMemcpyAsync(dump_out, h->exp_dev, sizeof(float) * dump_floats, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t k = 0; k < rows; ++k) {
    for (int f = 0; f < fields; ++f) rec[(size_t)f] = w[(size_t)f * rows + k];
    memcpy(static_cast<char*>(records_out) + sizeof(u64) * (size_t)fields * k, rec.data(), sizeof(u64) * (size_t)fields);
  }
  return MCL_OK;
}
// A statistic over the shards of one cloud: every shard checked, then every launch queued (launch(h, &count)), then the
// fetches of the B records of each, then the merge; merge_failed: the sentence of a merge that does not add up.
template <class Rec, class Check, class Launch, class Merge>
int group_stats_run(mcl_handle** sh, int ns, int B, Rec* out, int64_t* n_sampled, Check check, Launch launch, Merge merge,
                    const char* merge_failed) {
  for (int s = 0; s < ns; ++s) RET_IF(check(sh[s]));
  std::vector<long long> count((size_t)ns, 0);
  for (int s = 0; s < ns; ++s) RET_IF(launch(sh[s], &count[s]));
  std::vector<Rec> parts((size_t)ns * B);
  long long total = 0;
  for (int s = 0; s < ns; ++s) {
    RET_IF(stats_fetch(sh[s], B, (int)(sizeof(Rec) / sizeof(u64)), (size_t)B, parts.data() + (size_t)s * B, nullptr, 0));
    total += count[s];
  }
  if (merge(parts.data(), ns, B, out) != MCL_OK) return fail(sh[0], MCL_ERR_INVALID, merge_failed);
  *n_sampled = total;
  return MCL_OK;
}

// ------------------------------------------------------------------ the innovation statistics
// a record is the table's column: INNOV_FIELDS words in the table's field order
static_assert(sizeof(mcl_innovation_beam) == 8 * INNOV_FIELDS && offsetof(mcl_innovation_beam, n) == 0 &&
                  offsetof(mcl_innovation_beam, n_miss) == 8 && offsetof(mcl_innovation_beam, n_within) == 16 &&
                  offsetof(mcl_innovation_beam, s1) == 24 && offsetof(mcl_innovation_beam, s2) == 32,
              "k_innovation's fields");

struct InnovPing {
  const float* ranges;
  const float* angles;
  int B;
  double sigma, support_k, r_max;
  const double* sensor_offset;
  int max_samples;
};

int innovation_check(mcl_handle* h, const char* who, const InnovPing& p) {
  if (!p.ranges || !p.angles) return fail(h, MCL_ERR_INVALID, std::string(who) + ": null argument");
  RET_IF(ping_check_beams(h, who, p.B));
  if (!(p.sigma > 0.0) || !std::isfinite(p.sigma)) return fail(h, MCL_ERR_INVALID, std::string(who) + ": sigma must be positive and finite");
  if (!(p.support_k >= 0.0) || !std::isfinite(p.support_k)) return fail(h, MCL_ERR_INVALID, std::string(who) + ": support_k must be >= 0 and finite");
  if (!(p.r_max > 0.0) || !(p.r_max <= MCL_INNOVATION_MAX_RANGE))
    return fail(h, MCL_ERR_INVALID, std::string(who) + ": r_max outside (0, 4096] m (the quantised residual's range)");
  RET_IF(ping_check_samples(h, who, p.max_samples));
  return ping_check_state(h, who, true);
}

// particles of a workgroup: enough groups to give every compute unit about four workgroups, at least four particles per
// round of sincos (DESIGN 5l has the measurement); MCL_INNOVATION_GROUP=n (A/B) forces it.  The result does not depend on it.
int innovation_group(const mcl_handle* h, long long count, int chunks) {
  if (h->env_innov_group > 0) return std::min(h->env_innov_group, INNOV_MAX_GROUP);
  const long long g = (count * chunks + 1023) / 1024;
  return (int)std::min<long long>(std::max<long long>(g, 4), INNOV_MAX_GROUP);
}

// queue the upload of the beam table, the memset of the accumulators and the kernel over this shard's sampled slots;
// *count = how many those are.  dump: the expected ranges go to h->exp_dev (count x B).
int innovation_launch(mcl_handle* h, const InnovPing& p, bool dump, long long* count) {
  RET_IF(set_device(h));
  const int B = p.B;
  std::vector<float> beam;
  RET_IF(ping_beam_table(h, "ping_innovation", p.angles, p.ranges, B, beam));
  InnovArgs ia;
  memset(&ia, 0, sizeof ia);
  RET_IF(cloud_sample(h, p.max_samples, "ping_innovation", &ia.first, &ia.stride, count));
  if (*count > 0) RET_IF(materialise_uniform(h));
  RET_IF(beamstat_prepare(h, beam, B, INNOV_FIELDS, (size_t)B, *count, &ia.table));
  if (*count == 0) return MCL_OK;
  if (dump) RESERVE(h, h->exp_dev, (size_t)*count * (size_t)B);
  fill_frames_and_map(h, p.sensor_offset, p.r_max, ia.m);
  ia.beam = reinterpret_cast<const float4*>(h->beamstat_dev.p);
  ia.exp_out = dump ? h->exp_dev.p : nullptr;
  ia.count = *count;
  ia.q_support = innov_q_support(p.support_k, p.sigma);
  ia.n_beams = B;
  const BeamGeometry g = beam_geometry(B);
  ia.group = innovation_group(h, *count, g.chunks);
  map_dispatch(h, [&](auto map) { k_innovation<decltype(map)::value><<<g.grid(*count, ia.group), g.threads, 0, h->stream>>>(ia); });
  HIPCHK(h, hipGetLastError());
  return MCL_OK;
}

// mcl_ping_innovation
int innovation_run(mcl_handle* h, const InnovPing& p, mcl_innovation_beam* out, float* exp_out, int64_t* n_sampled) {
  RET_IF(innovation_check(h, "ping_innovation", p));
  long long count = 0;
  RET_IF(innovation_launch(h, p, exp_out != nullptr, &count));
  RET_IF(stats_fetch(h, p.B, INNOV_FIELDS, (size_t)p.B, out, exp_out, (size_t)count * (size_t)p.B));
  *n_sampled = count;
  return MCL_OK;
}

// mcl_group_ping_innovation
int group_innovation_run(mcl_handle** sh, int ns, const InnovPing& p, mcl_innovation_beam* out, int64_t* n_sampled) {
  return group_stats_run(
      sh, ns, p.B, out, n_sampled, [&](mcl_handle* h) { return innovation_check(h, "group_ping_innovation", p); },
      [&](mcl_handle* h, long long* count) { return innovation_launch(h, p, false, count); }, innovation_merge_impl,
      "group_ping_innovation: the shards' records do not add up to one sample (do the handles hold one cloud?)");
}

}  // namespace
