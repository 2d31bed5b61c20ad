// mcl_host_recovery.h -- host side of global localisation and kidnap recovery (include/mcl_recovery.h; kernels:
// csrc/mcl_recovery.h): the uniform initialisation, the weight statistics, the random-particle injection.  mcl_api.hip
// forwards to recovery_init_uniform / recovery_weight_stats / recovery_inject.
#pragma once
#include "mcl_host.h"
#include "mcl_recovery.h"

namespace {

// the argument block of k_uniform_state from a caller's box: bounds checked, the MAP frame resolved against cfg.m2o
int uniform_args(mcl_handle* h, const mcl_box* box, uint32_t purpose, uint32_t step, const char* who, UniformArgs& a) {
  const char* reason;
  const int rc = check_box(box, h->cfg.m2o, &reason);
  if (rc != MCL_OK) return fail(h, rc, std::string(who) + ": " + reason);
  const double b[6] = {box->x_min, box->x_max, box->y_min, box->y_max, box->yaw_min, box->yaw_max};
  memset(&a, 0, sizeof a);
  for (int c = 0; c < 3; ++c) {
    a.lo[c] = b[2 * c];
    a.hi[c] = b[2 * c + 1];
    a.w[c] = b[2 * c + 1] - b[2 * c];
  }
  if (box->frame == MCL_FRAME_MAP) {
    const double* m = h->cfg.m2o;
    a.r00 = m[0];
    a.r01 = m[1];
    a.r10 = m[4];
    a.r11 = m[5];
    a.tx = m[3];
    a.ty = m[7];
    a.theta = std::atan2(m[4], m[0]);
    a.xform = !(m[0] == 1.0 && m[1] == 0.0 && m[4] == 0.0 && m[5] == 1.0 && m[3] == 0.0 && m[7] == 0.0);
  }
  a.k0 = (uint32_t)h->cfg.seed;
  a.k1 = (uint32_t)(h->cfg.seed >> 32);
  a.step = step;
  a.purpose = purpose;
  a.gid0 = h->goff;
  return MCL_OK;
}
// REPLAY uniforms (n x per doubles, per <= 6) into the replay buffer
int upload_replay_uniforms(mcl_handle* h, const double* u, int per) {
  RESERVE(h, h->replay_dev, 6 * (size_t)h->n);
  return upload(h, h->replay_dev, u, sizeof(double) * (size_t)per * (size_t)h->n);
}

int recovery_init_uniform(mcl_handle* h, const mcl_box* box, const double* replay_uniforms) {
  UniformArgs a;
  RET_IF(uniform_args(h, box, 5u, 0u, "init_particles_uniform", a));
  const double* rp = nullptr;
  if (h->cfg.rng_mode == MCL_RNG_REPLAY) {
    if (!replay_uniforms) return fail(h, MCL_ERR_INVALID, "init_particles_uniform: REPLAY mode needs n x 3 uniforms");
    RET_IF(upload_replay_uniforms(h, replay_uniforms, 3));
    rp = h->replay_dev;
  }
  RET_IF(state_overwritten(h));
  t_begin(h, MCL_K_NOISE);
  k_uniform_state<false><<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(state_ptrs(h->state[h->cur], h->n), h->n, a, rp, nullptr);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  return MCL_OK;
}

int recovery_weight_stats(mcl_handle* h, mcl_wstats* out) {
  const long long ntiles = (h->n + WS_TILE - 1) / WS_TILE;
  static_assert(sizeof(WsPartial) % sizeof(double) == 0, "the tile records lie behind the result words of one double array");
  RESERVE(h, h->wstats_dev, WS_OUT_WORDS + sizeof(WsPartial) / sizeof(double) * (size_t)ntiles);
  WsPartial* part = reinterpret_cast<WsPartial*>(h->wstats_dev + WS_OUT_WORDS);
  t_begin(h, MCL_K_NORMALISE);
  k_wstats_partial<<<(unsigned)ntiles, MCL_BLOCK, 0, h->stream>>>(h->lw, h->n, h->goff, part);
  k_wstats_final<<<1, MCL_BLOCK, 0, h->stream>>>(part, ntiles, state_ptrs(h->state[h->cur], h->n), h->goff, h->wstats_dev);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  double r[11];
  HIPCHK(h, hipMemcpyAsync(r, h->wstats_dev, sizeof r, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int64_t words[2];
  memcpy(words, r + 3, sizeof words);
  out->n = h->n;
  out->n_live = words[1];
  out->argmax_gid = words[0];
  out->max_lw = r[0];
  out->sum_w = r[1];
  out->sum_w2 = r[2];
  for (int c = 0; c < 6; ++c) out->map_pose[c] = r[5 + c];
  wstats_finish(out);
  return MCL_OK;
}

int recovery_inject(mcl_handle* h, double fraction, const mcl_box* box, const double* replay_uniforms, int64_t* n_injected) {
  UniformArgs a;
  RET_IF(uniform_args(h, box, 6u, h->step_inject, "inject_uniform", a));
  a.fraction = fraction;
  if (h->cfg.rng_mode == MCL_RNG_REPLAY && !replay_uniforms)
    return fail(h, MCL_ERR_INVALID, "inject_uniform: REPLAY mode needs n x 4 uniforms");
  if (fraction == 0.0) {
    if (n_injected) *n_injected = 0;
    return MCL_OK;
  }
  const double* rp = nullptr;
  if (h->cfg.rng_mode == MCL_RNG_REPLAY) {
    RET_IF(upload_replay_uniforms(h, replay_uniforms, 4));
    rp = h->replay_dev;
  }
  RESERVE(h, h->inject_cnt, 1 + MCL_MAX_GRID);
  RET_IF(state_overwritten(h));
  const int grid = grid_for(h->n);
  t_begin(h, MCL_K_NOISE);
  k_uniform_state<true><<<grid, MCL_BLOCK, 0, h->stream>>>(state_ptrs(h->state[h->cur], h->n), h->n, a, rp, h->inject_cnt + 1);
  if (n_injected) k_count_final<<<1, MCL_BLOCK, 0, h->stream>>>(h->inject_cnt + 1, grid, h->inject_cnt);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  h->step_inject++;
  if (n_injected) {
    u64 cnt = 0;
    HIPCHK(h, hipMemcpyAsync(&cnt, h->inject_cnt, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_injected = (int64_t)cnt;
  }
  return MCL_OK;
}

}  // namespace
