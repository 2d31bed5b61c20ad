// mcl_host_match.h -- host side of the ping matching (include/mcl_match.h; kernel: csrc/mcl_match.h; compare, solve, checks
// and derived quantities: mcl_host_pure.h).  The checks, the beam table, the launch geometry and the scratch block are the
// ones of the innovation statistics and the ping information (mcl_host_innovation.h); the poses travel to info_pose as
// mcl_pose_information's do.  mcl_api.hip forwards to match_run.  Nothing here writes a member of the handle but those
// scratch buffers (beamstat_dev, info_pose) and the expected-range buffer every *_expected call shares (the dump).
#pragma once
#include "mcl_host_information.h"
#include "mcl_match.h"

namespace {

static_assert(sizeof(mcl_match_result) == 360 && sizeof(mcl_match_trace) == 192 && sizeof(mcl_match_config) == 72 &&
                  sizeof(mcl_match_derived_t) == 192,
              "include/mcl_match.h's records are whole 64-bit words");
static_assert(MCL_MATCH_MAX_BEAMS == MCL_INNOVATION_MAX_BEAMS, "the text of ping_check_beams");

constexpr size_t MATCH_KEEP_WORDS = (size_t)1 << 23;   // 64 MiB of 64-bit words: a scratch block beyond it is released after the call

struct MatchPing {
  const float* ranges;
  const float* angles;
  int B;
  double sigma, r_max;
  const double* sensor_offset;
  const mcl_match_config* cfg;
};

int match_check(mcl_handle* h, const MatchPing& p, const double* poses, long long M, bool dump) {
  const char* who = "match_ping";
  if (!poses || !p.ranges || !p.angles || !p.cfg) return fail(h, MCL_ERR_INVALID, std::string(who) + ": null argument");
  RET_IF(ping_check_beams(h, who, p.B));
  if (M < 1 || M > MCL_MATCH_MAX_POSES) return fail(h, MCL_ERR_INVALID, std::string(who) + ": M outside 1 ... 65536");
  if (!(p.sigma > 0.0) || !std::isfinite(p.sigma)) return fail(h, MCL_ERR_INVALID, std::string(who) + ": sigma must be positive and finite");
  const char* why = nullptr;
  if (match_config_check_impl(p.cfg, p.r_max, &why) != MCL_OK) return fail(h, MCL_ERR_INVALID, std::string(who) + ": " + why);
  if (dump && (size_t)M * (size_t)(p.cfg->max_iter + 1) * (size_t)(1 + 2 * p.cfg->dims) * (size_t)p.B > (size_t)MCL_MATCH_MAX_DUMP)
    return fail(h, MCL_ERR_INVALID, std::string(who) + ": ranges_out would hold more than 2^26 floats");
  RET_IF(ping_check_state(h, who, false));
  for (long long k = 0; k < 6 * M; ++k)
    if (!std::isfinite(poses[k])) return fail(h, MCL_ERR_INVALID, std::string(who) + ": a pose is not finite");
  return MCL_OK;
}

// mcl_match_ping: upload the poses and the beam table, zero the records, one launch of one workgroup per pose, fetch
int match_run(mcl_handle* h, const MatchPing& p, const double* poses, long long M, mcl_match_result* results_out,
              mcl_match_trace* trace_out, float* ranges_out) {
  RET_IF(match_check(h, p, poses, M, ranges_out != nullptr));
  RET_IF(set_device(h));
  const int B = p.B, T = p.cfg->max_iter + 1, NV = 1 + 2 * p.cfg->dims;
  std::vector<float> beam;
  RET_IF(ping_beam_table(h, "match_ping", p.angles, p.ranges, B, beam));
  RESERVE(h, h->info_pose, 6 * (size_t)M);
  RET_IF(upload(h, h->info_pose, poses, sizeof(double) * 6 * (size_t)M));
  // the scratch block behind the beam records: M results, then (trace) M T rows, all zero
  const size_t res_words = (size_t)M * (sizeof(mcl_match_result) / 8);
  const size_t trace_words = trace_out ? (size_t)M * (size_t)T * (sizeof(mcl_match_trace) / 8) : 0;
  u64* table = nullptr;
  RET_IF(beamstat_prepare(h, beam, B, 1, res_words + trace_words, M, &table));
  const size_t dump_floats = ranges_out ? (size_t)M * (size_t)T * (size_t)NV * (size_t)B : 0;
  if (ranges_out) {
    RESERVE(h, h->exp_dev, dump_floats);
    HIPCHK(h, hipMemsetAsync(h->exp_dev.p, 0xff, sizeof(float) * dump_floats, h->stream));   // (all ones: a NaN)
  }
  MatchArgs ma;
  memset(&ma, 0, sizeof ma);
  fill_frames_and_map(h, p.sensor_offset, p.r_max, ma.m);
  for (int c = 0; c < 6; ++c) ma.m.st[c] = h->info_pose.p + (size_t)c * (size_t)M;
  ma.m.n = M;
  ma.beam = reinterpret_cast<const float4*>(h->beamstat_dev.p);
  ma.results = reinterpret_cast<mcl_match_result*>(table);
  ma.trace = trace_out ? reinterpret_cast<mcl_match_trace*>(table + res_words) : nullptr;
  ma.ranges_out = ranges_out ? h->exp_dev.p : nullptr;
  ma.cfg = *p.cfg;
  ma.jump_q = info_jump_q(p.cfg->steps.jump_max);
  ma.n_beams = B;
  const BeamGeometry g = beam_geometry(B);
  const unsigned grid = (unsigned)M;
  const bool fit_z = p.cfg->dims == 4;
  map_dispatch(h, [&](auto map) {
    constexpr int MAP = decltype(map)::value;
    if (fit_z)
      k_ping_match<MAP, 4><<<grid, g.threads, 0, h->stream>>>(ma);
    else
      k_ping_match<MAP, 3><<<grid, g.threads, 0, h->stream>>>(ma);
  });
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(results_out, table, 8 * res_words, hipMemcpyDeviceToHost, h->stream));
  if (trace_out) HIPCHK(h, hipMemcpyAsync(trace_out, table + res_words, 8 * trace_words, hipMemcpyDeviceToHost, h->stream));
  if (ranges_out) HIPCHK(h, hipMemcpyAsync(ranges_out, h->exp_dev.p, sizeof(float) * dump_floats, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // the scratch block otherwise stays with the handle for good: a debugging trace of many poses (up to 415 MB) is given back
  if (h->beamstat_dev.cap > MATCH_KEEP_WORDS) h->beamstat_dev.reset();
  return MCL_OK;
}

}  // namespace
