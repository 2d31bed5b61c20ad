// mcl_host_acoustic.h -- host side, part 9: the delayed acoustic updates (include/mcl_acoustic.h; kernels:
// mcl_acoustic.h) -- what both calls check and fill in (where the pose comes from, the lever arm, z / roll / pitch) and
// one launcher per update.  mcl_history_bracket is host arithmetic: mcl_host_pure.h.
#pragma once
#include "mcl_acoustic.h"
#include "mcl_host_history.h"

namespace {

static_assert(ACO_MAX_BEACONS == MCL_ACOUSTIC_MAX_BEACONS, "the beacon table of the kernel's argument block");

// The checks of both calls and the shared argument block.  *arm: the transponder is off base_link.
int acoustic_prepare(mcl_handle* h, const char* who, const double offset[3], const double zrp[3], int lag, double frac,
                     bool accumulate, AcoArgs& a, bool* arm) {
  const std::string w(who);
  const char* why = acoustic_pose_check(offset, zrp, lag, frac);
  if (why) return fail(h, MCL_ERR_INVALID, w + ": " + why);
  if (lag >= 0) {
    RET_IF(need_history(h, who));
    if (lag >= h->hist_held) return fail(h, MCL_ERR_INVALID, w + ": lag outside the frames held");
    if (frac > 0.0 && lag + 1 >= h->hist_held) return fail(h, MCL_ERR_INVALID, w + ": frac > 0 needs the frame at lag + 1");
  }
  if (!h->have_state) return fail(h, MCL_ERR_STATE, w + ": no particles (call mcl_init_particles / mcl_set_particles first)");
  if (accumulate) RET_IF(need_weights_to_add(h, who));
  RET_IF(set_device(h));
  if (!zrp) RET_IF(materialise_uniform(h));   // (the particles' own z, roll, pitch are read: ranges_launch does the same)
  memset(&a, 0, sizeof a);
  for (int c = 0; c < 6; ++c) a.st[c] = h->state[h->cur] + (size_t)c * h->n;
  if (lag >= 0) {
    a.link = history_link(h);
    a.g = history_ring(h);
  }
  a.lag = lag;
  a.frac = frac;
  a.own_zrp = zrp ? 0 : 1;
  *arm = offset && (offset[0] != 0.0 || offset[1] != 0.0 || offset[2] != 0.0);
  if (*arm) {
    for (int k = 0; k < 3; ++k) a.off[k] = offset[k];
    if (zrp) {
      double R[9];
      rot_rpy(zrp[1], zrp[2], 0.0, R);   // Ry(pitch) Rx(roll): the kernel turns it by each particle's yaw
      for (int r = 0; r < 3; ++r) a.w[r] = R[r * 3 + 0] * offset[0] + R[r * 3 + 1] * offset[1] + R[r * 3 + 2] * offset[2];
    }
  }
  a.z = zrp ? zrp[0] : 0.0;
  for (int k = 0; k < 12; ++k) a.m2o[k] = h->cfg.m2o[k];
  a.n = (u32)h->n;
  a.accumulate = accumulate ? 1 : 0;
  a.lw = h->lw;
  return MCL_OK;
}

#define ACO_LAUNCH(KERNEL, ...)                                                                  \
  do {                                                                                           \
    const int g_ = grid_for(h->n);                                                               \
    if (lagged && arm) KERNEL<true, true><<<g_, MCL_BLOCK, 0, h->stream>>>(__VA_ARGS__);         \
    else if (lagged) KERNEL<true, false><<<g_, MCL_BLOCK, 0, h->stream>>>(__VA_ARGS__);          \
    else if (arm) KERNEL<false, true><<<g_, MCL_BLOCK, 0, h->stream>>>(__VA_ARGS__);             \
    else KERNEL<false, false><<<g_, MCL_BLOCK, 0, h->stream>>>(__VA_ARGS__);                     \
  } while (0)

int acoustic_finish(mcl_handle* h, bool accumulate) {
  t_end(h);
  HIPCHK(h, hipGetLastError());
  weights_written(h, accumulate ? WEIGHT_MODE_KEEP : MCL_WEIGHT_LOG_SHIFT, SLOTS_NONE);
  return MCL_OK;
}

int fix_launch(mcl_handle* h, const AcoArgs& a, bool arm, const double xy[2], const double cov3[3]) {
  const double det = cov3[0] * cov3[2] - cov3[1] * cov3[1];
  FixArgs f;
  f.gx = xy[0];
  f.gy = xy[1];
  f.ia = cov3[2] / det;
  f.ib = -cov3[1] / det;
  f.ic = cov3[0] / det;
  f.lognorm = 0.5 * std::log((2.0 * MCL_PI) * (2.0 * MCL_PI) * det);
  const bool lagged = a.lag >= 0;
  t_begin(h, MCL_K_UPDATE_GPS);
  ACO_LAUNCH(k_fix_update, a, f);
  return acoustic_finish(h, a.accumulate != 0);
}

int beacon_launch(mcl_handle* h, const AcoArgs& a, bool arm, const double* beacons, const double* ranges, int n_b,
                  double sigma) {
  BeaconArgs f;
  memset(&f, 0, sizeof f);
  for (int b = 0; b < n_b; ++b) {
    if (!(ranges[b] > 0.0)) continue;   // (NaN fails the test)
    for (int c = 0; c < 3; ++c) f.b[f.n_valid][c] = beacons[3 * b + c];
    f.r[f.n_valid++] = ranges[b];
  }
  f.inv_sigma = 1.0 / sigma;
  f.lognorm = (double)f.n_valid * std::log(sigma * std::sqrt(2.0 * MCL_PI));
  const bool lagged = a.lag >= 0;
  t_begin(h, MCL_K_UPDATE_GPS);
  ACO_LAUNCH(k_beacon_update, a, f);
  return acoustic_finish(h, a.accumulate != 0);
}

#undef ACO_LAUNCH

}  // namespace
