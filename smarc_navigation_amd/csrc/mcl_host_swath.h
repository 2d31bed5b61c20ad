// mcl_host_swath.h -- host side of the swath matching (include/mcl_swath.h; kernel: csrc/mcl_swath.h; offsets, checks,
// compare, solve and derived quantities: mcl_host_pure.h).  It is match_run (mcl_host_match.h) with K pings: the same checks
// with the swath's in front of the state's, K beam tables behind each other in the scratch block, the offsets behind the poses
// in info_pose, the same launch geometry (beam_geometry of ONE ping: the kernel walks the pings), the same fetch and the
// same scratch-release rule.  mcl_api.hip forwards to swath_run.  Nothing here writes a member of the handle but those
// scratch buffers (beamstat_dev, info_pose) and the expected-range buffer every *_expected call shares (the dump).
#pragma once
#include "mcl_host_match.h"
#include "mcl_swath.h"

namespace {

static_assert(sizeof(mcl_swath_offset) == 48 && offsetof(mcl_swath_offset, dz) == 16 && offsetof(mcl_swath_offset, roll) == 24 &&
                  offsetof(mcl_swath_offset, dyaw) == 40,
              "include/mcl_swath.h's offset is six doubles");

struct Swath {
  MatchPing p;   // ranges: K x B
  const mcl_swath_offset* offsets;
  int K;
};

int swath_check(mcl_handle* h, const Swath& s, const double* poses, long long M, bool dump) {
  const char* who = "match_swath";
  const MatchPing& p = s.p;
  if (!poses || !p.ranges || !p.angles || !p.cfg || !s.offsets) return fail(h, MCL_ERR_INVALID, std::string(who) + ": null argument");
  const char* why = nullptr;
  if (swath_check_impl(s.K, p.B, s.offsets, &why) != MCL_OK) return fail(h, MCL_ERR_INVALID, std::string(who) + ": " + why);
  if (M < 1 || M > MCL_MATCH_MAX_POSES) return fail(h, MCL_ERR_INVALID, std::string(who) + ": M outside 1 ... 65536");
  if (!(p.sigma > 0.0) || !std::isfinite(p.sigma)) return fail(h, MCL_ERR_INVALID, std::string(who) + ": sigma must be positive and finite");
  if (match_config_check_impl(p.cfg, p.r_max, &why) != MCL_OK) return fail(h, MCL_ERR_INVALID, std::string(who) + ": " + why);
  if (dump && (size_t)M * (size_t)(p.cfg->max_iter + 1) * (size_t)s.K * (size_t)(1 + 2 * p.cfg->dims) * (size_t)p.B > (size_t)MCL_MATCH_MAX_DUMP)
    return fail(h, MCL_ERR_INVALID, std::string(who) + ": ranges_out would hold more than 2^26 floats");
  RET_IF(ping_check_state(h, who, false));
  for (long long k = 0; k < 6 * M; ++k)
    if (!std::isfinite(poses[k])) return fail(h, MCL_ERR_INVALID, std::string(who) + ": a pose is not finite");
  return MCL_OK;
}

// mcl_match_swath: upload the poses with the offsets and the K beam tables, zero the records, one launch of one workgroup
// per pose, fetch
int swath_run(mcl_handle* h, const Swath& s, const double* poses, long long M, mcl_match_result* results_out,
              mcl_match_trace* trace_out, float* ranges_out) {
  RET_IF(swath_check(h, s, poses, M, ranges_out != nullptr));
  RET_IF(set_device(h));
  const MatchPing& p = s.p;
  const int B = p.B, K = s.K, T = p.cfg->max_iter + 1, NV = 1 + 2 * p.cfg->dims;
  // ping k's records at [k B, (k + 1) B): the directions of the one angle table, w that ping's ranges
  std::vector<float> beam(4 * (size_t)K * (size_t)B), one;
  for (int k = 0; k < K; ++k) {
    RET_IF(ping_beam_table(h, "match_swath", p.angles, p.ranges + (size_t)k * (size_t)B, B, one));
    memcpy(beam.data() + 4 * (size_t)k * (size_t)B, one.data(), sizeof(float) * 4 * (size_t)B);
  }
  // the poses and, behind them, the offsets (six doubles each) in one upload
  std::vector<double> up(6 * (size_t)M + 6 * (size_t)K);
  memcpy(up.data(), poses, sizeof(double) * 6 * (size_t)M);
  memcpy(up.data() + 6 * (size_t)M, s.offsets, sizeof(mcl_swath_offset) * (size_t)K);
  RESERVE(h, h->info_pose, up.size());
  RET_IF(upload(h, h->info_pose, up.data(), sizeof(double) * up.size()));
  // the scratch block behind the beam records: M results, then (trace) M T rows, all zero
  const size_t res_words = (size_t)M * (sizeof(mcl_match_result) / 8);
  const size_t trace_words = trace_out ? (size_t)M * (size_t)T * (sizeof(mcl_match_trace) / 8) : 0;
  u64* table = nullptr;
  RET_IF(beamstat_prepare(h, beam, K * B, 1, res_words + trace_words, M, &table));
  const size_t dump_floats = ranges_out ? (size_t)M * (size_t)T * (size_t)K * (size_t)NV * (size_t)B : 0;
  if (ranges_out) {
    RESERVE(h, h->exp_dev, dump_floats);
    HIPCHK(h, hipMemsetAsync(h->exp_dev.p, 0xff, sizeof(float) * dump_floats, h->stream));   // (all ones: a NaN)
  }
  SwathArgs sa;
  memset(&sa, 0, sizeof sa);
  MatchArgs& ma = sa.a;
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
  sa.off = reinterpret_cast<const mcl_swath_offset*>(h->info_pose.p + 6 * (size_t)M);
  sa.n_pings = K;
  const BeamGeometry g = beam_geometry(B);
  const unsigned grid = (unsigned)M;
  const bool fit_z = p.cfg->dims == 4;
  map_dispatch(h, [&](auto map) {
    constexpr int MAP = decltype(map)::value;
    if (fit_z)
      k_swath_match<MAP, 4><<<grid, g.threads, 0, h->stream>>>(sa);
    else
      k_swath_match<MAP, 3><<<grid, g.threads, 0, h->stream>>>(sa);
  });
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(results_out, table, 8 * res_words, hipMemcpyDeviceToHost, h->stream));
  if (trace_out) HIPCHK(h, hipMemcpyAsync(trace_out, table + res_words, 8 * trace_words, hipMemcpyDeviceToHost, h->stream));
  if (ranges_out) HIPCHK(h, hipMemcpyAsync(ranges_out, h->exp_dev.p, sizeof(float) * dump_floats, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->beamstat_dev.cap > MATCH_KEEP_WORDS) h->beamstat_dev.reset();   // (match_run's rule)
  return MCL_OK;
}

}  // namespace
