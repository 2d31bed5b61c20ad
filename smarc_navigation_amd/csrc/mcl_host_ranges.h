// mcl_host_ranges.h -- host side of libmcl_hip.so, part 6: the launcher of the DVL / altimeter range update
// (mcl_ranges.h).  It starts where the MBES plan starts: fill_frames_and_map (mcl_host_update.h).
#pragma once

namespace {

// the beam table (normalise_beams) and the map go into the kernel's argument block; one launch over the particles
// [first, first + count): log-likelihoods into lw_out, or (exp_out) the expected ranges instead
int ranges_launch(mcl_handle* h, const float* ranges, const float* dirs, int B, double sigma, double r_max,
                  const double sensor_offset[6], bool accumulate, double* lw_out, float* exp_out, long long first,
                  long long count) {
  RangesArgs ra;
  memset(&ra, 0, sizeof ra);
  float beam[4 * RANGES_MAX_BEAMS];
  if (normalise_beams(dirs, ranges, B, beam) != MCL_OK)
    return fail(h, MCL_ERR_INVALID, "update_ranges: a beam direction is zero or not finite");
  for (int b = 0; b < B; ++b) ra.beam[b] = make_float4(beam[4 * b], beam[4 * b + 1], beam[4 * b + 2], beam[4 * b + 3]);
  RET_IF(materialise_uniform(h));
  fill_frames_and_map(h, sensor_offset, r_max, ra.m);
  int lg = 0;
  while ((1 << lg) < B) ++lg;
  ra.i0 = first;
  ra.i1 = first + count;
  ra.n_beams = B;
  ra.lg_bp = lg;
  ra.accumulate = accumulate ? 1 : 0;
  ra.sigma = sigma;
  ra.lognorm = std::log(sigma * std::sqrt(2.0 * MCL_PI));
  ra.lw = lw_out;
  ra.exp_out = exp_out;
  const long long per_block = RANGES_THREADS >> lg;
  const unsigned grid = (unsigned)std::min<long long>((count + per_block - 1) / per_block, 1ll << 16);
  if (!exp_out) t_begin(h, MCL_K_UPDATE_MBES);
  map_dispatch(h, [&](auto map) {
    constexpr int MAP = decltype(map)::value;
    if (exp_out)
      k_ranges_update<MAP, true><<<grid, RANGES_THREADS, 0, h->stream>>>(ra);
    else
      k_ranges_update<MAP, false><<<grid, RANGES_THREADS, 0, h->stream>>>(ra);
  });
  if (!exp_out) t_end(h);
  HIPCHK(h, hipGetLastError());
  return MCL_OK;
}

}  // namespace
