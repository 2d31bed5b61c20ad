// mcl_host_innovation.h -- host side of the ping innovation statistics (include/mcl_innovation.h; kernel:
// csrc/mcl_innovation.h; sample, direction table, merge and gate: mcl_host_pure.h).  mcl_api.hip forwards to innovation_run /
// group_innovation_run.  Nothing here writes a member of the handle but its lazily reserved block (innov_dev) and the
// expected-range buffer every *_expected call shares.  It starts where the range update starts: fill_frames_and_map.
#pragma once
#include "mcl_host.h"
#include "mcl_innovation.h"

namespace {

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
  if (p.B < 1 || p.B > MCL_INNOVATION_MAX_BEAMS) return fail(h, MCL_ERR_INVALID, std::string(who) + ": B outside 1 ... 2048");
  if (!(p.sigma > 0.0) || !std::isfinite(p.sigma)) return fail(h, MCL_ERR_INVALID, std::string(who) + ": sigma must be positive and finite");
  if (!(p.support_k >= 0.0) || !std::isfinite(p.support_k)) return fail(h, MCL_ERR_INVALID, std::string(who) + ": support_k must be >= 0 and finite");
  if (!(p.r_max > 0.0) || !(p.r_max <= MCL_INNOVATION_MAX_RANGE))
    return fail(h, MCL_ERR_INVALID, std::string(who) + ": r_max outside (0, 4096] m (the quantised residual's range)");
  if (p.max_samples < 1 || p.max_samples > MCL_INNOVATION_MAX_SAMPLES)
    return fail(h, MCL_ERR_INVALID, std::string(who) + ": max_samples outside 1 ... 32768");
  RET_IF(need_map(h, who));
  if (!h->have_state)
    return fail(h, MCL_ERR_STATE, std::string(who) + ": no particles (call mcl_init_particles / mcl_set_particles first)");
  return MCL_OK;
}

// particles of a workgroup: enough groups to give every compute unit about four workgroups, at least four particles per
// round of sincos (DESIGN 5l has the measurement); MCL_INNOVATION_GROUP=n (A/B) forces it.  The result does not depend on it.
int innovation_group(const mcl_handle* h, long long count, int chunks) {
  if (h->env_innov_group > 0) return std::min(h->env_innov_group, INNOV_MAX_GROUP);
  const long long g = (count * chunks + 1023) / 1024;
  return (int)std::min<long long>(std::max<long long>(g, 4), INNOV_MAX_GROUP);
}

template <int MAP>
void launch_innovation(mcl_handle* h, unsigned grid, unsigned threads, const InnovArgs& ia) {
  k_innovation<MAP><<<grid, threads, 0, h->stream>>>(ia);
}

// queue the upload of the beam table, the memset of the accumulators and the kernel over this shard's sampled slots;
// *count = how many those are.  dump: the expected ranges go to h->exp_dev (count x B).
int innovation_launch(mcl_handle* h, const InnovPing& p, bool dump, long long* count) {
  RET_IF(set_device(h));
  const int B = p.B;
  std::vector<float> dirs(3 * (size_t)B), beam(4 * (size_t)B);
  if (innovation_dirs_impl(p.angles, B, dirs.data()) != MCL_OK || normalise_beams(dirs.data(), p.ranges, B, beam.data()) != MCL_OK)
    return fail(h, MCL_ERR_INVALID, "ping_innovation: a beam angle is not finite");
  int64_t stride = 0, total = 0;
  if (innovation_sample_impl(h->ng, p.max_samples, &stride, &total) != MCL_OK)
    return fail(h, MCL_ERR_INVALID, "ping_innovation: bad sample");
  long long first = 0;
  *count = innov_shard_sample(h->goff, h->n, stride, &first);
  // the block: B beam records (16 bytes each) in front, the 5 x B accumulators behind them
  RESERVE(h, h->innov_dev, (size_t)(2 + INNOV_FIELDS) * (size_t)B);
  u64* table = h->innov_dev + 2 * (size_t)B;
  HIPCHK(h, hipMemsetAsync(table, 0, sizeof(u64) * INNOV_FIELDS * (size_t)B, h->stream));
  if (*count == 0) return MCL_OK;
  RET_IF(materialise_uniform(h));
  RET_IF(upload(h, h->innov_dev, beam.data(), sizeof(float) * 4 * (size_t)B));
  if (dump) RESERVE(h, h->exp_dev, (size_t)*count * (size_t)B);
  InnovArgs ia;
  memset(&ia, 0, sizeof ia);
  fill_frames_and_map(h, p.sensor_offset, p.r_max, ia.m);
  ia.beam = reinterpret_cast<const float4*>(h->innov_dev.p);
  ia.table = table;
  ia.exp_out = dump ? h->exp_dev.p : nullptr;
  ia.first = first;
  ia.stride = stride;
  ia.count = *count;
  ia.q_support = innov_q_support(p.support_k, p.sigma);
  ia.n_beams = B;
  const int chunks = (B + INNOV_CHUNK - 1) / INNOV_CHUNK;
  ia.group = innovation_group(h, *count, chunks);
  const unsigned threads = B >= INNOV_CHUNK ? INNOV_CHUNK : (unsigned)((B + 63) / 64 * 64);
  const unsigned grid = (unsigned)(((*count + ia.group - 1) / ia.group) * chunks);   // (<= 32768 x 8)
  // the map walk: 0 the height grid, 2 the node heights of a triangulated regular grid, 1 triangle records
  if (h->map_kind == 0)
    launch_innovation<0>(h, grid, threads, ia);
  else if (structured_mesh(h))
    launch_innovation<2>(h, grid, threads, ia);
  else
    launch_innovation<1>(h, grid, threads, ia);
  HIPCHK(h, hipGetLastError());
  return MCL_OK;
}
// the accumulators of a queued launch (and its dump), one synchronisation
int innovation_fetch(mcl_handle* h, int B, long long count, mcl_innovation_beam* out, float* exp_out) {
  RET_IF(set_device(h));
  std::vector<u64> w((size_t)INNOV_FIELDS * B);
  HIPCHK(h, hipMemcpyAsync(w.data(), h->innov_dev + 2 * (size_t)B, sizeof(u64) * w.size(), hipMemcpyDeviceToHost, h->stream));
  if (exp_out && count > 0)
    HIPCHK(h, hipMemcpyAsync(exp_out, h->exp_dev, sizeof(float) * (size_t)count * (size_t)B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int b = 0; b < B; ++b) {
    out[b].n = (int64_t)w[0 * (size_t)B + b];
    out[b].n_miss = (int64_t)w[1 * (size_t)B + b];
    out[b].n_within = (int64_t)w[2 * (size_t)B + b];
    out[b].s1 = (int64_t)w[3 * (size_t)B + b];
    out[b].s2 = w[4 * (size_t)B + b];
  }
  return MCL_OK;
}

// mcl_ping_innovation
int innovation_run(mcl_handle* h, const InnovPing& p, mcl_innovation_beam* out, float* exp_out, int64_t* n_sampled) {
  RET_IF(innovation_check(h, "ping_innovation", p));
  long long count = 0;
  RET_IF(innovation_launch(h, p, exp_out != nullptr, &count));
  RET_IF(innovation_fetch(h, p.B, count, out, exp_out));
  *n_sampled = count;
  return MCL_OK;
}

// mcl_group_ping_innovation: every shard's launch queued, then the fetches, then the merge
int group_innovation_run(mcl_handle** sh, int ns, const InnovPing& p, mcl_innovation_beam* out, int64_t* n_sampled) {
  for (int s = 0; s < ns; ++s) RET_IF(innovation_check(sh[s], "group_ping_innovation", p));
  std::vector<long long> count((size_t)ns, 0);
  for (int s = 0; s < ns; ++s) RET_IF(innovation_launch(sh[s], p, false, &count[s]));
  std::vector<mcl_innovation_beam> parts((size_t)ns * p.B);
  long long total = 0;
  for (int s = 0; s < ns; ++s) {
    RET_IF(innovation_fetch(sh[s], p.B, count[s], parts.data() + (size_t)s * p.B, nullptr));
    total += count[s];
  }
  if (innovation_merge_impl(parts.data(), ns, p.B, out) != MCL_OK)
    return fail(sh[0], MCL_ERR_INVALID, "group_ping_innovation: the shards' records do not add up to one sample (do the handles hold one cloud?)");
  *n_sampled = total;
  return MCL_OK;
}

}  // namespace
