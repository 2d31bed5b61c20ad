// mcl_host_regularise.h -- host side, part 12: regularised resampling (include/mcl_regularise.h; kernels:
// mcl_regularise.h) -- the moments, the factor and the jitter queued behind a resample, and the record they leave.
#pragma once
#include "mcl_host_drift.h"

namespace {

static_assert(REG_SUMS_MAX == REG_MAX_DIMS + REG_MAX_PACKED && REG_RES_WORDS == 82, "the record of mcl_regularise_last");

template <int D>
int regularise_launch(mcl_handle* h, bool shrink, double bw, double a, const RegDraw& dr, const double* rp) {
  constexpr int NS = D + D * (D + 1) / 2;
  const size_t n = (size_t)h->n;
  const int g = grid_for(h->n);
  double* st = h->state[h->cur];
  RegPtrs p{};
  p.v[0] = st;
  p.v[1] = st + n;
  p.v[2] = st + 5 * n;
  if (D == 6)
    for (int c = 0; c < 3; ++c) p.v[3 + c] = h->drift_state + (size_t)c * n;
  double* res = h->reg_res;
  t_begin(h, MCL_K_MEAN_COV);
  k_reg_moments<D><<<g, MCL_BLOCK, 0, h->stream>>>(p, h->n, h->reg_part, res + REG_RES_SHIFT);
  k_sum_final<<<NS, MCL_BLOCK, 0, h->stream>>>(h->reg_part, g, res + REG_RES_SUMS);
  k_reg_factor<D><<<1, MCL_WAVE, 0, h->stream>>>(res, h->n);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  t_begin(h, MCL_K_NOISE);
  if (shrink)
    k_reg_apply<D, true><<<g, MCL_BLOCK, 0, h->stream>>>(p, h->n, res, bw, a, dr, rp);
  else
    k_reg_apply<D, false><<<g, MCL_BLOCK, 0, h->stream>>>(p, h->n, res, bw, a, dr, rp);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  return MCL_OK;
}

int regularise_run(mcl_handle* h, const mcl_regularise_config* cfg, const double* replay_normals) {
  const int D = cfg->dims;
  double bw, a;
  RET_IF(regularise_bandwidth_impl(h->n, D, cfg->scale, cfg->shrink, &bw, &a));
  RESERVE(h, h->reg_part, (size_t)REG_SUMS_MAX * MCL_MAX_GRID);
  RESERVE(h, h->reg_res, (size_t)REG_RES_WORDS);
  RegDraw dr;
  dr.k0 = (uint32_t)h->cfg.seed;
  dr.k1 = (uint32_t)(h->cfg.seed >> 32);
  dr.step = h->reg_calls;
  dr.gid0 = h->goff;
  const double* rp = nullptr;
  if (h->cfg.rng_mode == MCL_RNG_REPLAY) {
    RESERVE(h, h->replay_dev, (size_t)D * (size_t)h->n);
    RET_IF(upload(h, h->replay_dev, replay_normals, sizeof(double) * (size_t)D * (size_t)h->n));
    rp = h->replay_dev;
  }
  RET_IF(D == 6 ? regularise_launch<6>(h, cfg->shrink != 0, bw, a, dr, rp) : regularise_launch<3>(h, cfg->shrink != 0, bw, a, dr, rp));
  h->reg_calls++;
  h->reg_dims = D;
  h->reg_h = bw;
  h->reg_a = a;
  return MCL_OK;
}

int regularise_last(mcl_handle* h, mcl_regularise_result* out) {
  double r[REG_RES_WORDS];
  HIPCHK(h, hipMemcpyAsync(r, h->reg_res, sizeof r, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *out = mcl_regularise_result{};
  out->n = h->n;
  out->dims = h->reg_dims;
  out->dead = (int32_t)r[REG_RES_DEAD];
  out->h = h->reg_h;
  out->a = h->reg_a;
  for (int c = 0; c < REG_MAX_DIMS; ++c) {
    out->shift[c] = r[REG_RES_SHIFT + c];
    out->dmean[c] = r[REG_RES_MEAN + c];
  }
  for (int k = 0; k < REG_MAX_PACKED; ++k) {
    out->cov[k] = r[REG_RES_COV + k];
    out->chol[k] = r[REG_RES_CHOL + k];
  }
  return MCL_OK;
}

}  // namespace
