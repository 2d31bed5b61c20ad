// mcl_host_kld.h -- host side of KLD-sampling across handles (include/mcl_kld.h; kernels: csrc/mcl_kld.h; the device-free
// arithmetic: mcl_kld_pure.h): the occupied cells of the caller's lattice, and the resample of one handle's cloud into
// another's.  mcl_api.hip forwards to kld_bins_run / transfer_run.  kld_bins_run writes no member of the handle but its
// lazily reserved buffers and their bookkeeping; transfer_run writes nothing of src at all.
#pragma once
#include "mcl_host_resample.h"
#include "mcl_kld_pure.h"
#include "mcl_kld.h"

namespace {

static_assert(KLD_LDS_BYTES >= 16 * sizeof(u64), "the reductions' words");

// g has passed kld_grid_check_impl, which counted its n_cells
int kld_bins_run(mcl_handle* h, const mcl_mode_grid* g, int64_t n_cells, int64_t* k, int64_t* n_inside, int64_t* n_outside) {
  const size_t words = (size_t)kld_bitmap_words(n_cells);
  const long long nvec = (long long)(words / 4);
  const int gp = grid_for(h->n), gc = grid_for(nvec);
  RESERVE(h, h->kld_rec, 2 * (size_t)MCL_MAX_GRID + 2);
  // the bitmap is all zero between calls: zeroed when it is allocated or grown, cleaned by k_kld_count where a call set
  // bits -- and cleared here when a call ended early between its mark and its count
  const bool fresh = h->kld_bits.cap < words;
  RESERVE(h, h->kld_bits, words);
  if (fresh || h->kld_dirty) HIPCHK(h, hipMemsetAsync(h->kld_bits, 0, sizeof(u32) * h->kld_bits.cap, h->stream));
  ModeLattice lat;
  lat.x0 = g->x0;
  lat.y0 = g->y0;
  lat.cell = g->cell;
  lat.dyaw = (2.0 * MCL_PI) / (double)g->n_yaw;
  lat.nx = g->nx;
  lat.ny = g->ny;
  lat.n_yaw = g->n_yaw;
  u64* rec = h->kld_rec;
  u64* res = h->kld_rec + 2 * (size_t)MCL_MAX_GRID;
  h->kld_dirty = true;
  t_begin(h, MCL_K_MEAN_COV);
  k_kld_mark<<<gp, MCL_BLOCK, 0, h->stream>>>(state_ptrs(h->state[h->cur], h->n), h->n, lat, h->kld_bits, rec);
  k_kld_count<<<gc, MCL_BLOCK, 0, h->stream>>>(reinterpret_cast<uint4*>(h->kld_bits.p), nvec, rec + MCL_MAX_GRID);
  k_kld_final<<<2, MCL_BLOCK, 0, h->stream>>>(rec, gp, gc, res);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  u64 out[2];
  HIPCHK(h, hipMemcpyAsync(out, res, sizeof out, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->kld_dirty = false;
  if (k) *k = (int64_t)out[1];
  if (n_outside) *n_outside = (int64_t)out[0];
  if (n_inside) *n_inside = (int64_t)h->n - (int64_t)out[0];
  return MCL_OK;
}

// What mcl_resample_into refuses, with nothing touched: nullptr, or the status in *code and the sentence
const char* transfer_refused(const mcl_handle* src, const mcl_handle* dst, int* code) {
  *code = MCL_ERR_UNSUPPORTED;
  if (src->world > 1 || src->comm || dst->world > 1 || dst->comm) return "resample_into: a sharded cloud is not supported";
  if (src->device != dst->device) return "resample_into: the two handles live on different devices";
  *code = MCL_ERR_STATE;
  if (!src->have_state) return "resample_into: src has no particles (call mcl_init_particles / mcl_set_particles first)";
  if (src->drift_on != dst->drift_on) return "resample_into: the drift states are enabled on exactly one of the two handles";
  return nullptr;
}

// src and dst have passed transfer_refused; u53 is the draw.  Everything is queued on dst's stream, behind what src's
// stream held when the call was made; all scratch is dst's.
int transfer_run(mcl_handle* src, mcl_handle* dst, uint64_t u53) {
  const long long N = src->n, M = dst->n;
  const long long ntiles = (N + MCL_SCAN_TILE - 1) / MCL_SCAN_TILE;
  RESERVE(dst, dst->xfer_q, (size_t)N);
  RESERVE(dst, dst->xfer_ncum, (size_t)N);
  RESERVE(dst, dst->xfer_tile, (size_t)ntiles + 1 + MCL_MAX_SLOTS);   // tile sums | the total | the max-lw slots
  RESERVE(dst, dst->xfer_idx, (size_t)M);
  u64* tile = dst->xfer_tile;
  u64* total = tile + ntiles;
  u64* slots = total + 1;
  HIPCHK(dst, hipStreamSynchronize(src->stream));   // (work queued on src is seen)
  RET_IF(state_overwritten(dst));
  t_begin(dst, MCL_K_RESAMPLE);
  // ---- the fixed-point weights mcl_resample on src would decide on, from src's log-weights as they are.
  // The maximum is reduced here into slots of dst's: src's own slots and its max_valid stay what they are.
  HIPCHK(dst, hipMemsetAsync(slots, 0, sizeof(u64) * MCL_MAX_SLOTS, dst->stream));
  QuantArgs qa{};
  qa.n = N;
  qa.slots = slots;
  qa.s = 63 - ceil_log2(N);
  qa.scale = std::ldexp(1.0, qa.s);
  qa.q = dst->xfer_q;
  qa.tile_sum = tile;
  if (src->have_lw) {
    k_max_slots<<<grid_for(N), MCL_BLOCK, 0, dst->stream>>>(src->lw, N, slots);
    qa.lw = src->lw;
    qa.mode = src->weight_mode;
  } else {
    // no pending weights: equal weights -- the rule of "no finite log-likelihood" (empty slots: the maximum is -inf and
    // every q is 2^s, whatever the words read as log-weights hold; the state's x are N doubles that exist)
    qa.lw = src->state[src->cur];
    qa.mode = MCL_WEIGHT_LOG_SHIFT;
  }
  k_quantise_tiles<<<(unsigned)ntiles, MCL_BLOCK, 0, dst->stream>>>(qa);
  k_scan_tile_sums<u64><<<1, 1024, 0, dst->stream>>>(tile, ntiles, total);
  // ---- the offspring CDF for M positions
  CdfArgs ca;
  ca.totals = total;
  ca.rank = 0;
  ca.world = 1;
  ca.n_global = (u64)M;
  ca.u53 = u53;
  ca.shift = nullptr;
  k_offspring_cdf<<<grid_tiles(ntiles), MCL_BLOCK, 0, dst->stream>>>(dst->xfer_q, N, tile, ca, dst->xfer_ncum);
  // ---- the gather
  TransferArgs ta{};
  ta.src = state_ptrs(src->state[src->cur], N);
  ta.dst = state_ptrs(dst->state[dst->cur], M);
  ta.ncum = dst->xfer_ncum;
  ta.n_src = N;
  ta.m = M;
  ta.idx = dst->xfer_idx;
  if (dst->drift_on) {
    for (int c = 0; c < 3; ++c) {
      ta.sdrift[c] = src->drift_state + (size_t)c * N;
      ta.ddrift[c] = dst->drift_state + (size_t)c * M;
    }
    k_transfer_gather<true><<<grid_for(M), MCL_BLOCK, 0, dst->stream>>>(ta);
  } else {
    k_transfer_gather<false><<<grid_for(M), MCL_BLOCK, 0, dst->stream>>>(ta);
  }
  t_end(dst);
  HIPCHK(dst, hipGetLastError());
  HIPCHK(dst, hipStreamSynchronize(dst->stream));   // (src's buffers are no longer read: src may go on)
  dst->have_state = true;
  dst->have_lw = false;
  history_clear(dst);
  dst->step_transfer++;
  dst->have_transfer = true;
  return MCL_OK;
}

}  // namespace
