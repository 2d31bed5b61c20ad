// mcl_host_quantile.h -- host side of the exact order statistics (include/mcl_quantile.h; kernels: csrc/mcl_quantile.h;
// keys, threshold, predicate, start and bin choice: mcl_host_pure.h).  mcl_api.hip forwards to quant_run / quant_mass_run /
// quant_key_hist / group_quant_run.  Nothing here writes a member of the handle but its lazily reserved state block.
#pragma once
#include "mcl_host.h"
#include "mcl_quantile.h"

namespace {

// what every call needs of a handle and a query, in the order the header states the errors
int quant_check(mcl_handle* h, const char* who, const mcl_quantile_query* q) {
  if (const char* why = quantile_query_why(q)) return fail(h, MCL_ERR_INVALID, std::string(who) + ": " + why);
  if (!h->have_state)
    return fail(h, MCL_ERR_STATE, std::string(who) + ": no particles (call mcl_init_particles / mcl_set_particles first)");
  if (q->weighted) {
    if (!h->have_lw) return fail(h, MCL_ERR_STATE, std::string(who) + ": weighted, and no log-weights (call an update first)");
    if (h->weight_mode == MCL_WEIGHT_LINEAR)
      return fail(h, MCL_ERR_STATE, std::string(who) + ": weighted, and the pending weights are linear (MCL_WEIGHT_LINEAR), not log-weights");
  }
  return MCL_OK;
}
int quant_thresholds(mcl_handle* h, const char* who, const double* probs, int n_probs, QuantWords* P) {
  if (n_probs < 1 || n_probs > MCL_QUANTILE_MAX) return fail(h, MCL_ERR_INVALID, std::string(who) + ": n_probs outside 1 ... 8");
  for (int k = 0; k < QUANT_MAX_P; ++k) P->w[k] = 0;
  for (int k = 0; k < n_probs; ++k) {
    uint64_t p = 0;
    if (quantile_threshold_impl(probs[k], &p) != MCL_OK)
      return fail(h, MCL_ERR_INVALID, std::string(who) + ": a probability outside [2^-32, 1]");
    P->w[k] = p;
  }
  return MCL_OK;
}
int quant_max_lw_check(mcl_handle* h, const char* who, const mcl_quantile_query* q, double max_lw) {
  if (q->weighted && (std::isnan(max_lw) || max_lw == INFINITY)) return fail(h, MCL_ERR_INVALID, std::string(who) + ": max_lw is NaN or +inf");
  return MCL_OK;
}
QuantQuery quant_query(const mcl_quantile_query* q) {
  QuantQuery r;
  r.quantity = q->quantity;
  r.weighted = q->weighted ? 1 : 0;
  r.cx = q->centre[0];
  r.cy = q->centre[1];
  r.cyaw = q->centre[2];
  return r;
}
int quant_grid(const mcl_handle* h) { return std::min(grid_for(h->n), QUANT_GRID); }
void quant_result(uint64_t key, uint64_t mass, uint64_t total, int64_t n_used, mcl_quantile_result* out) {
  out->total = total;
  out->n_used = n_used;
  if (total == 0) {
    out->value = NAN;
    out->key = 0;
    out->mass = 0;
    return;
  }
  out->value = quant_value(key);
  out->key = key;
  out->mass = mass;
}

// range + plan: the records of this handle's particles reduced into the head of its state block
int quant_range_launch(mcl_handle* h, const QuantQuery& q, int n_probs, const QuantWords& P) {
  RET_IF(set_device(h));
  RESERVE(h, h->quant_dev, QS_WORDS);
  const StatePtrs sp = state_ptrs(h->state[h->cur], h->n);
  const int g = grid_for(h->n);
  if (q.weighted) k_quant_range<true><<<g, MCL_BLOCK, 0, h->stream>>>(sp, h->lw, h->n, q, h->quant_dev);
  else k_quant_range<false><<<g, MCL_BLOCK, 0, h->stream>>>(sp, nullptr, h->n, q, h->quant_dev);
  k_quant_plan<<<1, MCL_BLOCK, 0, h->stream>>>(h->quant_dev, g, n_probs, P);
  return MCL_OK;
}
void quant_hist_kernel(mcl_handle* h, const QuantQuery& q, int round) {
  const StatePtrs sp = state_ptrs(h->state[h->cur], h->n);
  if (q.weighted) k_quant_hist<true><<<quant_grid(h), MCL_BLOCK, 0, h->stream>>>(sp, h->lw, h->n, q, round, h->quant_dev);
  else k_quant_hist<false><<<quant_grid(h), MCL_BLOCK, 0, h->stream>>>(sp, nullptr, h->n, q, round, h->quant_dev);
}

// mcl_cloud_quantiles: range, plan, eight rounds of (hist, pick) back to back -- the rounds below the start return at
// once --, one copy, one synchronisation
int quant_run(mcl_handle* h, const mcl_quantile_query* query, const double* probs, int n_probs, mcl_quantile_result* out) {
  RET_IF(quant_check(h, "cloud_quantiles", query));
  QuantWords P;
  RET_IF(quant_thresholds(h, "cloud_quantiles", probs, n_probs, &P));
  if (h->world > 1)
    return fail(h, MCL_ERR_UNSUPPORTED, "cloud_quantiles: a shard of a larger cloud (world > 1): use mcl_group_cloud_quantiles or the split calls");
  if (query->weighted && h->ng > MCL_QUANTILE_MAX_PARTICLES) return fail(h, MCL_ERR_UNSUPPORTED, "cloud_quantiles: weighted, and more than 2^24 particles");
  const QuantQuery q = quant_query(query);
  t_begin(h, MCL_K_MEAN_COV);
  RET_IF(quant_range_launch(h, q, n_probs, P));
  for (int round = 0; round < QUANT_ROUNDS; ++round) {
    quant_hist_kernel(h, q, round);
    k_quant_pick<<<1, MCL_BLOCK, 0, h->stream>>>(h->quant_dev, round);
  }
  t_end(h);
  HIPCHK(h, hipGetLastError());
  u64 w[QS_HEAD];
  HIPCHK(h, hipMemcpyAsync(w, h->quant_dev, sizeof w, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < n_probs; ++k) quant_result(w[QS_PREFIX + k], w[QS_MK + k], w[QS_S], (int64_t)w[QS_NUSED], out + k);
  return MCL_OK;
}

// mcl_cloud_mass
int quant_mass_run(mcl_handle* h, const mcl_quantile_query* query, double max_lw, const double* values, int n_values,
                   uint64_t* mass, uint64_t* total, int64_t* n_used) {
  RET_IF(quant_check(h, "cloud_mass", query));
  if (n_values < 1 || n_values > MCL_QUANTILE_MAX) return fail(h, MCL_ERR_INVALID, "cloud_mass: n_values outside 1 ... 8");
  QuantWords keys;
  for (int k = 0; k < QUANT_MAX_P; ++k) keys.w[k] = 0;
  for (int k = 0; k < n_values; ++k) {
    if (std::isnan(values[k])) return fail(h, MCL_ERR_INVALID, "cloud_mass: a value is NaN");
    keys.w[k] = quant_key(values[k]);
  }
  RET_IF(quant_max_lw_check(h, "cloud_mass", query, max_lw));
  RET_IF(set_device(h));
  RESERVE(h, h->quant_dev, QS_WORDS);
  const QuantQuery q = quant_query(query);
  const StatePtrs sp = state_ptrs(h->state[h->cur], h->n);
  t_begin(h, MCL_K_MEAN_COV);
  HIPCHK(h, hipMemsetAsync(h->quant_dev + QS_MASS, 0, sizeof(u64) * (QUANT_MAX_P + 2), h->stream));
  if (q.weighted) k_quant_mass<true><<<quant_grid(h), MCL_BLOCK, 0, h->stream>>>(sp, h->lw, h->n, q, max_lw, keys, n_values, h->quant_dev);
  else k_quant_mass<false><<<quant_grid(h), MCL_BLOCK, 0, h->stream>>>(sp, nullptr, h->n, q, 0.0, keys, n_values, h->quant_dev);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  u64 w[QUANT_MAX_P + 2];
  HIPCHK(h, hipMemcpyAsync(w, h->quant_dev + QS_MASS, sizeof w, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < n_values; ++k) mass[k] = w[k];
  *total = w[QUANT_MAX_P];
  *n_used = (int64_t)w[QUANT_MAX_P + 1];
  return MCL_OK;
}

// a hist launch whose plan the host wrote: round, m and one prefix per probability (every probability its own row), queued;
// quant_hist_fetch reads the rows
int quant_hist_launch(mcl_handle* h, const QuantQuery& q, double m, int round, const uint64_t* prefix, int np) {
  RET_IF(set_device(h));
  RESERVE(h, h->quant_dev, QS_WORDS);
  u64 head[QS_HEAD];
  memset(head, 0, sizeof head);
  head[QS_NP] = (u64)np;
  memcpy(head + QS_M, &m, sizeof m);
  for (int k = 0; k < np; ++k) {
    head[QS_PREFIX + k] = prefix[k];
    head[QS_ROW + k] = (u64)k;
  }
  RET_IF(upload(h, h->quant_dev, head, sizeof head));
  t_begin(h, MCL_K_MEAN_COV);
  HIPCHK(h, hipMemsetAsync(h->quant_dev + QS_HIST, 0, sizeof(u64) * QUANT_MAX_P * QUANT_BINS, h->stream));
  quant_hist_kernel(h, q, round);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  return MCL_OK;
}
int quant_hist_fetch(mcl_handle* h, int np, uint64_t* hist /*[np][256]*/) {
  RET_IF(set_device(h));
  HIPCHK(h, hipMemcpyAsync(hist, h->quant_dev + QS_HIST, sizeof(u64) * (size_t)np * QUANT_BINS, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}
// mcl_cloud_key_hist
int quant_key_hist(mcl_handle* h, const mcl_quantile_query* query, double max_lw, uint64_t prefix, int prefix_bits, uint64_t* hist) {
  RET_IF(quant_check(h, "cloud_key_hist", query));
  if (prefix_bits < 0 || prefix_bits > 56 || prefix_bits % 8 != 0) return fail(h, MCL_ERR_INVALID, "cloud_key_hist: prefix_bits is not one of 0, 8, ..., 56");
  if (prefix_bits < 64 && (prefix >> prefix_bits) != 0) return fail(h, MCL_ERR_INVALID, "cloud_key_hist: the prefix has more than prefix_bits bits");
  RET_IF(quant_max_lw_check(h, "cloud_key_hist", query, max_lw));
  RET_IF(quant_hist_launch(h, quant_query(query), query->weighted ? max_lw : 0.0, prefix_bits / 8, &prefix, 1));
  return quant_hist_fetch(h, 1, hist);
}

// mcl_group_cloud_quantiles: the shards' records (maximum, key range, used count), then the rounds from quant_start on,
// each a hist launch per shard with the probabilities' prefixes, the rows added and quant_pick_bin on the sums
int group_quant_run(mcl_handle** sh, int ns, const mcl_quantile_query* query, const double* probs, int n_probs,
                    mcl_quantile_result* out) {
  long long ng = 0;
  for (int s = 0; s < ns; ++s) {
    RET_IF(quant_check(sh[s], "group_cloud_quantiles", query));
    ng += sh[s]->n;
  }
  QuantWords P;
  RET_IF(quant_thresholds(sh[0], "group_cloud_quantiles", probs, n_probs, &P));
  if (query->weighted && ng > MCL_QUANTILE_MAX_PARTICLES) return fail(sh[0], MCL_ERR_UNSUPPORTED, "group_cloud_quantiles: weighted, and more than 2^24 particles");
  const QuantQuery q = quant_query(query);
  for (int s = 0; s < ns; ++s) {
    t_begin(sh[s], MCL_K_MEAN_COV);
    RET_IF(quant_range_launch(sh[s], q, n_probs, P));
    t_end(sh[s]);
    HIPCHK(sh[s], hipGetLastError());
  }
  double m = -INFINITY;
  uint64_t kmin = ~0ull, kmax = 0;
  int64_t n_used = 0;
  for (int s = 0; s < ns; ++s) {
    u64 w[QS_HEAD];
    HIPCHK(sh[s], hipMemcpyAsync(w, sh[s]->quant_dev, sizeof w, hipMemcpyDeviceToHost, sh[s]->stream));
    HIPCHK(sh[s], hipStreamSynchronize(sh[s]->stream));
    double ms;
    memcpy(&ms, w + QS_M, sizeof ms);
    if (ms > m) m = ms;
    kmin = std::min<uint64_t>(kmin, w[QS_KMIN]);
    kmax = std::max<uint64_t>(kmax, w[QS_KMAX]);
    n_used += (int64_t)w[QS_NUSED];
  }
  const QuantStart g = quant_start(kmin, kmax);
  uint64_t prefix[QUANT_MAX_P], below[QUANT_MAX_P], mk[QUANT_MAX_P], S = 0;
  for (int k = 0; k < n_probs; ++k) {
    prefix[k] = g.prefix;
    below[k] = mk[k] = 0;
  }
  std::vector<uint64_t> sum((size_t)n_probs * QUANT_BINS), part((size_t)n_probs * QUANT_BINS);
  for (int round = g.start; round < QUANT_ROUNDS; ++round) {
    for (int s = 0; s < ns; ++s) RET_IF(quant_hist_launch(sh[s], q, m, round, prefix, n_probs));
    std::fill(sum.begin(), sum.end(), 0);
    for (int s = 0; s < ns; ++s) {
      RET_IF(quant_hist_fetch(sh[s], n_probs, part.data()));
      for (size_t t = 0; t < sum.size(); ++t) sum[t] += part[t];
    }
    if (round == g.start)
      for (int d = 0; d < QUANT_BINS; ++d) S += sum[d];   // (every used particle matches the shared prefix: row 0 holds them all)
    for (int k = 0; k < n_probs; ++k) {
      const uint64_t* row = sum.data() + (size_t)k * QUANT_BINS;
      uint64_t cum = 0;
      const int d = quant_pick_bin(row, below[k], S, P.w[k], &cum);
      if (d < 0) {   // (S = 0)
        prefix[k] <<= 8;
        continue;
      }
      prefix[k] = (prefix[k] << 8) | (uint64_t)d;
      below[k] = cum - row[d];
      mk[k] = cum;
    }
  }
  for (int k = 0; k < n_probs; ++k) quant_result(prefix[k], mk[k], S, n_used, out + k);
  return MCL_OK;
}

}  // namespace
