// mcl_host_drift.h -- host side, part 11: the per-particle drift states (include/mcl_drift.h; kernels: mcl_drift.h) -- the
// prior draw, the advance queued before a predict, the gather queued behind every resample's own, the moments.
#pragma once
#include "mcl_host_history.h"

namespace {

static_assert(DRIFT_SUMS * MCL_MAX_GRID == DRIFT_PART_WORDS && DRIFT_RES_WORDS == DRIFT_RESULT_WORDS &&
                  DRIFT_SUMS + 3 <= DRIFT_RES_WORDS,
              "mcl_drift_bytes (mcl_host_pure.h) counts what drift_alloc reserves");

int need_drift(mcl_handle* h, const char* who) {
  if (h->drift_on) return MCL_OK;
  return fail(h, MCL_ERR_STATE, std::string(who) + ": the drift is not enabled (call mcl_drift_enable first)");
}
void drift_free(mcl_handle* h) {
  h->drift_on = false;
  h->drift_step = 0;
  h->drift_state.reset();
  h->drift_part.reset();
  h->drift_res.reset();
}
int drift_alloc(mcl_handle* h) {
  RESERVE(h, h->drift_state, 3 * (size_t)h->n);
  RESERVE(h, h->drift_part, (size_t)DRIFT_SUMS * MCL_MAX_GRID);
  RESERVE(h, h->drift_res, (size_t)DRIFT_RES_WORDS);
  return MCL_OK;
}

// the draw of one call: sq = what multiplies the normals.  *rp = the caller's normals on the device (REPLAY) or nullptr
// (NATIVE; REPLAY with every factor zero: no draw is read)
int drift_draw(mcl_handle* h, const double sq[3], uint32_t step, const double* replay_normals, const char* who, DriftDraw& a,
               const double** rp) {
  for (int c = 0; c < 3; ++c) a.sq[c] = sq[c];
  a.k0 = (uint32_t)h->cfg.seed;
  a.k1 = (uint32_t)(h->cfg.seed >> 32);
  a.step = step;
  a.gid0 = h->goff;
  *rp = nullptr;
  if (h->cfg.rng_mode != MCL_RNG_REPLAY) return MCL_OK;
  const bool any = sq[0] != 0.0 || sq[1] != 0.0 || sq[2] != 0.0;
  if (!any) return MCL_OK;
  if (!replay_normals) return fail(h, MCL_ERR_INVALID, std::string(who) + ": REPLAY mode needs n x 3 normals (a std is not zero)");
  RESERVE(h, h->replay_dev, 3 * (size_t)h->n);
  RET_IF(upload(h, h->replay_dev, replay_normals, sizeof(double) * 3 * (size_t)h->n));
  *rp = h->replay_dev;
  return MCL_OK;
}

int drift_prior(mcl_handle* h, const double* replay_normals, const char* who) {
  DriftDraw a;
  const double* rp;
  RET_IF(drift_draw(h, h->drift_cfg.init_std, 0u, replay_normals, who, a, &rp));
  const size_t n = (size_t)h->n;
  double* d = h->drift_state;
  k_drift_init<<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(d, d + n, d + 2 * n, h->n, a, rp);
  HIPCHK(h, hipGetLastError());
  h->drift_step = 0;
  return MCL_OK;
}

int drift_advance(mcl_handle* h, double dt, const double* replay_normals) {
  const double rt = std::sqrt(dt);
  const double sq[3] = {h->drift_cfg.walk_std[0] * rt, h->drift_cfg.walk_std[1] * rt, h->drift_cfg.walk_std[2] * rt};
  DriftDraw a;
  const double* rp;
  RET_IF(drift_draw(h, sq, h->drift_step + 1u, replay_normals, "drift_advance", a, &rp));
  const size_t n = (size_t)h->n;
  double* st = h->state[h->cur];
  double* d = h->drift_state;
  t_begin(h, MCL_K_PREDICT);
  k_drift_advance<<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(st, st + n, st + 5 * n, d, d + n, d + 2 * n, h->n, dt, a, rp);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  h->drift_step++;
  return MCL_OK;
}

// d'[i] = d[A(i)] behind the gather that just ran (run_resample, run_resample_alt): one launch, in place
int drift_after_resample(mcl_handle* h, bool alt) {
  HistMap m{};
  m.zr = h->zr;
  m.dupes32 = h->dupes32;
  m.cnt = h->cnt;
  m.zcum = h->zcum;
  m.dupes = h->dupes;
  const size_t n = (size_t)h->n;
  double* d = h->drift_state;
  t_begin(h, MCL_K_RESAMPLE);
  if (alt)
    k_drift_gather<true><<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(m, (u32)h->n, d, d + n, d + 2 * n);
  else
    k_drift_gather<false><<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(m, (u32)h->n, d, d + n, d + 2 * n);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  return MCL_OK;
}

int drift_mean_cov(mcl_handle* h, double* mean3, double* cov6) {
  const size_t n = (size_t)h->n;
  const int g = grid_for(h->n);
  const double* d = h->drift_state;
  t_begin(h, MCL_K_MEAN_COV);
  k_drift_moments<<<g, MCL_BLOCK, 0, h->stream>>>(d, d + n, d + 2 * n, h->n, h->drift_part, h->drift_res + DRIFT_SUMS);
  k_sum_final<<<DRIFT_SUMS, MCL_BLOCK, 0, h->stream>>>(h->drift_part, g, h->drift_res);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  double r[DRIFT_RES_WORDS];
  HIPCHK(h, hipMemcpyAsync(r, h->drift_res, sizeof r, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const double N = (double)h->n;
  const double m[3] = {r[0] / N, r[1] / N, r[2] / N};
  if (mean3)
    for (int c = 0; c < 3; ++c) mean3[c] = m[c] + r[DRIFT_SUMS + c];
  if (cov6) {   // xx, xy, xz, yy, yz, zz from the packed lower triangle the kernel leaves
    int k = 0;
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) cov6[k++] = r[3 + reg_packed(b, a)] / N - m[a] * m[b];
  }
  return MCL_OK;
}

}  // namespace
