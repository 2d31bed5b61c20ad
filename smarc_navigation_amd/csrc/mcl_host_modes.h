// mcl_host_modes.h -- host side of the dominant modes (include/mcl_modes.h; kernels: csrc/mcl_modes.h; the lattice check:
// mcl_host_pure.h): histogram, window score, greedy peak selection, the moments inside each peak's window and what the
// host makes of them.  mcl_api.hip forwards to modes_run.  Nothing here writes a member of the handle but its lazily
// reserved buffers.
#pragma once
#include "mcl_host.h"
#include "mcl_recovery.h"   // (k_count_final)

namespace {

// g has passed mode_grid_check_impl, which counted its n_cells; 1 <= k <= MCL_MODES_MAX
int modes_run(mcl_handle* h, const mcl_mode_grid* g, int k, int64_t n_cells, mcl_mode* modes, int32_t* n_modes,
              int64_t* n_outside) {
  const int gp = grid_for(h->n), gc = grid_for(n_cells);
  RESERVE(h, h->modes_hist, (size_t)n_cells);
  RESERVE(h, h->modes_score, (size_t)n_cells);
  RESERVE(h, h->modes_cell, (size_t)h->n);
  RESERVE(h, h->modes_rec, 2 * (size_t)MCL_MAX_GRID);
  RESERVE(h, h->modes_part, (size_t)MODES_MAX_K * MODES_SUMS * MCL_MAX_GRID);
  RESERVE(h, h->modes_res, MODES_RES_WORDS);
  ModeLattice lat;
  lat.x0 = g->x0;
  lat.y0 = g->y0;
  lat.cell = g->cell;
  lat.dyaw = (2.0 * MCL_PI) / (double)g->n_yaw;
  lat.nx = g->nx;
  lat.ny = g->ny;
  lat.n_yaw = g->n_yaw;
  u64* rec_out = h->modes_rec;
  u64* rec_key = h->modes_rec + MCL_MAX_GRID;
  ModePeak* peaks = reinterpret_cast<ModePeak*>(h->modes_res + MODES_RES_PEAKS);
  const StatePtrs st = state_ptrs(h->state[h->cur], h->n);
  t_begin(h, MCL_K_MEAN_COV);
  HIPCHK(h, hipMemsetAsync(h->modes_hist, 0, sizeof(u32) * (size_t)n_cells, h->stream));
  k_modes_hist<<<gp, MCL_BLOCK, 0, h->stream>>>(st, h->n, lat, h->modes_cell, h->modes_hist, rec_out);
  k_count_final<<<1, MCL_BLOCK, 0, h->stream>>>(rec_out, gp, reinterpret_cast<u64*>(h->modes_res + MODES_RES_OUTSIDE));
  k_modes_score<<<gc, MCL_BLOCK, 0, h->stream>>>(h->modes_hist, lat.nx, lat.ny, lat.n_yaw, (u32)n_cells, h->modes_score, rec_key);
  k_modes_peak_final<<<1, MCL_BLOCK, 0, h->stream>>>(rec_key, gc, lat.nx, lat.ny, peaks, 0);
  for (int m = 1; m < k; ++m) {
    k_modes_peak_partial<<<gc, MCL_BLOCK, 0, h->stream>>>(h->modes_score, lat.nx, lat.ny, lat.n_yaw, (u32)n_cells, peaks, m, rec_key);
    k_modes_peak_final<<<1, MCL_BLOCK, 0, h->stream>>>(rec_key, gc, lat.nx, lat.ny, peaks, m);
  }
  k_modes_moments<<<gp, MCL_BLOCK, 0, h->stream>>>(st, h->n, h->modes_cell, lat, peaks, k, h->modes_part);
  k_sum_final<<<k * MODES_SUMS, MCL_BLOCK, 0, h->stream>>>(h->modes_part, gp, h->modes_res);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  double res[MODES_RES_WORDS];
  HIPCHK(h, hipMemcpyAsync(res, h->modes_res, sizeof res, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ModePeak pk[MODES_MAX_K];
  memcpy(pk, res + MODES_RES_PEAKS, sizeof pk);
  if (n_outside) {
    u64 cnt = 0;
    memcpy(&cnt, res + MODES_RES_OUTSIDE, sizeof cnt);
    *n_outside = (int64_t)cnt;
  }
  int found = 0;
  for (; found < k && pk[found].score != 0u; ++found) {
    const double* a = res + found * MODES_SUMS;
    const ModePeak& p = pk[found];
    mcl_mode& o = modes[found];
    const double cnt = a[0];
    const double cx = g->x0 + ((double)p.ix + 0.5) * g->cell, cy = g->y0 + ((double)p.iy + 0.5) * g->cell;
    const double mdx = a[1] / cnt, mdy = a[2] / cnt;
    o.count = (int64_t)cnt;
    o.score = (int64_t)p.score;
    o.ix = p.ix;
    o.iy = p.iy;
    o.iyaw = p.iyaw;
    o.reserved = 0;
    o.mean6[0] = cx + mdx;
    o.mean6[1] = cy + mdy;
    o.mean6[2] = a[3] / cnt;
    o.mean6[3] = a[4] / cnt;
    o.mean6[4] = a[5] / cnt;
    o.mean6[5] = std::atan2(a[6], a[7]);
    o.cov_xy[0] = a[8] / cnt - mdx * mdx;
    o.cov_xy[1] = a[9] / cnt - mdx * mdy;
    o.cov_xy[2] = a[10] / cnt - mdy * mdy;
    o.yaw_R = std::hypot(a[6], a[7]) / cnt;
  }
  *n_modes = found;
  return MCL_OK;
}

}  // namespace
