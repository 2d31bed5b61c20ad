// mcl_host_history.h -- host side, part 8: the particle genealogy (include/mcl_history.h; kernels: mcl_history.h) -- the
// ring of frames, the compose queued behind every resample's gather, the record, the smoother's backward walk and the
// two chases.
#pragma once
#include "mcl_host_resample.h"

namespace {

static_assert(HIST_SUMS * MCL_MAX_GRID == HISTORY_PART_WORDS && HIST_RES_WORDS == HISTORY_RES_WORDS &&
                  HIST_MAX_DEPTH == MCL_HISTORY_MAX_DEPTH && 4 <= HIST_RES_WORDS,
              "mcl_history_bytes (mcl_host_pure.h) counts what history_alloc reserves");

int need_history(mcl_handle* h, const char* who) {
  if (h->hist_on) return MCL_OK;
  return fail(h, MCL_ERR_STATE, std::string(who) + ": history is not enabled (call mcl_history_enable first)");
}
// the link as the kernels take it: nullptr is the identity
const u32* history_link(const mcl_handle* h) { return h->hist_ident ? nullptr : (const u32*)h->hist_link[h->hist_cur]; }
HistRing history_ring(const mcl_handle* h) {
  HistRing g;
  g.parent = h->hist_parent;
  g.xyw = h->hist_xyw;
  g.n = (u32)h->n;
  g.depth = h->hist_depth;
  g.head = h->hist_head;
  return g;
}
int history_frame_index(const mcl_handle* h, int lag) { return (h->hist_head - lag + h->hist_depth) % h->hist_depth; }

void history_clear(mcl_handle* h) {
  h->hist_held = 0;
  h->hist_head = -1;
  h->hist_recorded = 0;
  h->hist_ident = true;
}
void history_free(mcl_handle* h) {
  h->hist_on = false;
  h->hist_depth = 0;
  history_clear(h);
  for (auto& b : h->hist_link) b.reset();
  for (auto& b : h->hist_cnt) b.reset();
  h->hist_parent.reset();
  h->hist_xyw.reset();
  h->hist_part.reset();
  h->hist_res.reset();
  h->hist_stamp.clear();
}
int history_alloc(mcl_handle* h, int depth) {
  const size_t n = (size_t)h->n;
  RESERVE(h, h->hist_link[0], n);
  RESERVE(h, h->hist_link[1], n);
  RESERVE(h, h->hist_cnt[0], n);
  RESERVE(h, h->hist_cnt[1], n);
  RESERVE(h, h->hist_parent, n * (size_t)depth);
  RESERVE(h, h->hist_xyw, 3 * n * (size_t)depth);
  RESERVE(h, h->hist_part, (size_t)HIST_SUMS * MCL_MAX_GRID);
  RESERVE(h, h->hist_res, (size_t)HIST_RES_WORDS * (size_t)depth);
  return MCL_OK;
}

// link' = link o A behind the gather that just ran (run_resample, run_resample_alt): one launch, into the other buffer
int history_after_resample(mcl_handle* h, bool alt) {
  HistMap m{};
  m.zr = h->zr;
  m.dupes32 = h->dupes32;
  m.cnt = h->cnt;
  m.zcum = h->zcum;
  m.dupes = h->dupes;
  const u32* link = history_link(h);
  u32* out = h->hist_link[h->hist_ident ? h->hist_cur : h->hist_cur ^ 1];
  t_begin(h, MCL_K_RESAMPLE);
  if (alt)
    k_history_compose<true><<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(m, link, (u32)h->n, out);
  else
    k_history_compose<false><<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(m, link, (u32)h->n, out);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  if (!h->hist_ident) h->hist_cur ^= 1;
  h->hist_ident = false;
  return MCL_OK;
}

int history_record(mcl_handle* h, double stamp) {
  const int f = (h->hist_head + 1) % h->hist_depth;
  const size_t n = (size_t)h->n;
  const double* st = h->state[h->cur];
  double* fr = h->hist_xyw + (size_t)f * 3 * n;
  t_begin(h, MCL_K_RESAMPLE);
  k_history_record<<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(history_link(h), st, st + n, st + 5 * n, (u32)h->n,
                                                                h->hist_parent + (size_t)f * n, fr, fr + n, fr + 2 * n);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  h->hist_head = f;
  h->hist_stamp[(size_t)f] = stamp;
  if (h->hist_held < h->hist_depth) h->hist_held++;
  h->hist_recorded++;
  h->hist_ident = true;
  return MCL_OK;
}

int history_ancestors(mcl_handle* h, int lag, uint32_t* slots) {
  // (the output borrows the smoother's first count buffer: history_smooth initialises both of its buffers itself, on the
  //  same stream, before it reads them, so nothing this leaves behind is ever read as a count)
  u32* out = h->hist_cnt[0];
  k_history_ancestors<<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(history_link(h), history_ring(h), lag, out);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(slots, out, sizeof(u32) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}

// the backward walk: c_0 from the link, then per frame its sums and the counts of the frame before it
int history_smooth(mcl_handle* h, int lags, mcl_history_est* est) {
  const size_t n = (size_t)h->n;
  const int g = grid_for(h->n);
  t_begin(h, MCL_K_MEAN_COV);
  int cur = 0;
  if (!h->hist_ident) HIPCHK(h, hipMemsetAsync(h->hist_cnt[cur], 0, sizeof(u32) * n, h->stream));
  k_history_count0<<<g, MCL_BLOCK, 0, h->stream>>>(history_link(h), (u32)h->n, h->hist_cnt[cur]);
  for (int k = 0; k < lags; ++k) {
    const int f = history_frame_index(h, k);
    const bool more = k + 1 < lags;
    if (more) HIPCHK(h, hipMemsetAsync(h->hist_cnt[cur ^ 1], 0, sizeof(u32) * n, h->stream));
    const double* fr = h->hist_xyw + (size_t)f * 3 * n;
    double* res = h->hist_res + (size_t)k * HIST_RES_WORDS;
    k_history_frame<<<g, MCL_BLOCK, 0, h->stream>>>(h->hist_cnt[cur], h->hist_parent + (size_t)f * n,
                                                    more ? (u32*)h->hist_cnt[cur ^ 1] : nullptr, fr, fr + n, fr + 2 * n,
                                                    (u32)h->n, h->hist_part, res + HIST_SUMS);
    k_sum_final<<<HIST_SUMS, MCL_BLOCK, 0, h->stream>>>(h->hist_part, g, res);
    cur ^= 1;
  }
  t_end(h);
  HIPCHK(h, hipGetLastError());
  std::vector<double> r((size_t)lags * HIST_RES_WORDS);
  HIPCHK(h, hipMemcpyAsync(r.data(), h->hist_res, sizeof(double) * r.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const double N = (double)h->n;
  for (int k = 0; k < lags; ++k) {
    const double* a = r.data() + (size_t)k * HIST_RES_WORDS;
    mcl_history_est& o = est[k];
    const double mdx = a[0] / N, mdy = a[1] / N;
    o.stamp = h->hist_stamp[(size_t)history_frame_index(h, k)];
    o.n_unique = (int64_t)a[7];   // (a sum of ones below 2^31: exact)
    o.x = mdx + a[HIST_SUMS];
    o.y = mdy + a[HIST_SUMS + 1];
    o.yaw = std::atan2(a[2], a[3]);
    o.yaw_R = std::hypot(a[2], a[3]) / N;
    o.cov_xy[0] = a[4] / N - mdx * mdx;
    o.cov_xy[1] = a[5] / N - mdx * mdy;
    o.cov_xy[2] = a[6] / N - mdy * mdy;
  }
  return MCL_OK;
}

int history_path(mcl_handle* h, long long slot, int lags, double* xyyaw, uint32_t* slots) {
  k_history_path<<<1, MCL_WAVE, 0, h->stream>>>(history_link(h), history_ring(h), (u32)slot, lags, h->hist_res);
  HIPCHK(h, hipGetLastError());
  std::vector<double> r((size_t)lags * 4);
  HIPCHK(h, hipMemcpyAsync(r.data(), h->hist_res, sizeof(double) * r.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < lags; ++k) {
    for (int c = 0; c < 3; ++c) xyyaw[3 * k + c] = r[(size_t)4 * k + c];
    if (slots) slots[k] = (uint32_t)r[(size_t)4 * k + 3];
  }
  return MCL_OK;
}

}  // namespace
