// mcl_host_temper.h -- host side of ESS-targeted tempering (include/mcl_temper.h; kernels: csrc/mcl_temper.h; the
// lattice, the predicate and the round plan: mcl_host_pure.h).  mcl_api.hip forwards to temper_run / temper_sums /
// temper_apply / group_temper_run.
#pragma once
#include "mcl_host.h"
#include "mcl_temper.h"

namespace {

// what every tempering call needs of a handle: pending log-weights that are logarithms
int temper_check(mcl_handle* h, const char* who) {
  if (!h->have_lw) return fail(h, MCL_ERR_STATE, std::string(who) + ": no log-weights (call an update first)");
  if (h->weight_mode == MCL_WEIGHT_LINEAR)
    return fail(h, MCL_ERR_STATE, std::string(who) + ": the pending weights are linear (MCL_WEIGHT_LINEAR), not log-weights");
  return MCL_OK;
}
int temper_target_check(mcl_handle* h, const char* who, long long n_global, long long n_target) {
  if (n_global > MCL_TEMPER_MAX_PARTICLES) return fail(h, MCL_ERR_UNSUPPORTED, std::string(who) + ": more than 2^24 particles");
  if (n_target < 1 || n_target > n_global) return fail(h, MCL_ERR_INVALID, std::string(who) + ": n_target outside 1 ... n_global");
  return MCL_OK;
}
int temper_grid(const mcl_handle* h) { return std::min(grid_for(h->n), TP_SUMS_GRID); }
// the log-weights were scaled: the stored maximum and the residual scheme's cached count no longer describe them
void temper_applied(mcl_handle* h) {
  h->max_valid = false;
  h->residual_k = -1;
}
void temper_result(const u64* w, mcl_temper_result* out) {
  out->j = (int32_t)w[TP_J];
  out->floor_hit = (int32_t)w[TP_FLOOR];
  out->levels_evaluated = (int32_t)w[TP_LEVELS];
  out->reserved = 0;
  out->n_target = (int64_t)w[TP_NT];
  out->n_live = (int64_t)w[TP_NLIVE];
  memcpy(&out->beta, w + TP_BETA_J, sizeof(double));
  memcpy(&out->max_lw, w + TP_M, sizeof(double));
}

// mcl_temper: maximum, three rounds of (sums, pick), apply -- nine launches back to back, the decisions in device memory
int temper_run(mcl_handle* h, long long n_target, bool apply, mcl_temper_result* out) {
  RET_IF(temper_check(h, "temper"));
  if (h->comm) return fail(h, MCL_ERR_UNSUPPORTED, "temper: a handle with an RCCL communicator (use mcl_temper_sums / mcl_temper_apply)");
  if (h->world > 1) return fail(h, MCL_ERR_STATE, "temper: a shard of a larger cloud (use mcl_group_temper or the split calls)");
  RET_IF(temper_target_check(h, "temper", h->ng, n_target));
  RET_IF(set_device(h));
  RESERVE(h, h->temper_dev, TP_WORDS);
  u64* st = h->temper_dev;
  const int gm = grid_for(h->n), gs = temper_grid(h);
  t_begin(h, MCL_K_NORMALISE);
  k_temper_max<<<gm, MCL_BLOCK, 0, h->stream>>>(h->lw, h->n, st);
  k_temper_pick<<<1, MCL_BLOCK, 0, h->stream>>>(st, 0, gm, n_target);
  for (int round = 1; round <= 3; ++round) {
    k_temper_sums<<<gs, MCL_BLOCK, 0, h->stream>>>(h->lw, h->n, st);
    k_temper_pick<<<1, MCL_BLOCK, 0, h->stream>>>(st, round, 0, n_target);
  }
  if (apply) k_temper_apply<<<gm, MCL_BLOCK, 0, h->stream>>>(h->lw, h->n, st, 1.0);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  if (apply) temper_applied(h);
  if (out) {
    u64 w[TP_SUMS];
    HIPCHK(h, hipMemcpyAsync(w, st, sizeof w, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    temper_result(w, out);
  }
  return MCL_OK;
}

// the sums launch of the split form, queued; temper_sums_fetch reads its result
int temper_sums_launch(mcl_handle* h, double max_lw, const int32_t* levels, int n_levels) {
  RET_IF(set_device(h));
  RESERVE(h, h->temper_dev, TP_WORDS);
  u64 plan[TP_PLAN_WORDS];
  memset(plan, 0, sizeof plan);
  plan[TP_NC] = (u64)n_levels;
  for (int k = 0; k < n_levels; ++k) {
    plan[TP_CAND + k] = (u64)levels[k];
    const double b = temper_beta(levels[k]);
    memcpy(plan + TP_BETA + k, &b, sizeof b);
  }
  memcpy(plan + TP_M, &max_lw, sizeof max_lw);
  RET_IF(upload(h, h->temper_dev, plan, sizeof plan));
  t_begin(h, MCL_K_NORMALISE);
  HIPCHK(h, hipMemsetAsync(h->temper_dev + TP_SUMS, 0, sizeof(u64) * 2 * TP_NCAND, h->stream));
  k_temper_sums<<<temper_grid(h), MCL_BLOCK, 0, h->stream>>>(h->lw, h->n, h->temper_dev);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  return MCL_OK;
}
int temper_sums_fetch(mcl_handle* h, int n_levels, uint64_t* s1, uint64_t* s2) {
  RET_IF(set_device(h));
  u64 w[2 * TP_NCAND];
  HIPCHK(h, hipMemcpyAsync(w, h->temper_dev + TP_SUMS, sizeof w, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < n_levels; ++k) {
    s1[k] = w[k];
    s2[k] = w[TP_NCAND + k];
  }
  return MCL_OK;
}
int temper_sums(mcl_handle* h, double max_lw, const int32_t* levels, int32_t n_levels, uint64_t* s1, uint64_t* s2) {
  if (!levels || !s1 || !s2 || n_levels < 1 || n_levels > MCL_TEMPER_MAX_CAND)
    return fail(h, MCL_ERR_INVALID, "temper_sums: bad argument (1 <= n_levels <= 17)");
  for (int k = 0; k < n_levels; ++k)
    if (levels[k] < 0 || levels[k] > MCL_TEMPER_LEVELS) return fail(h, MCL_ERR_INVALID, "temper_sums: a level outside 0 ... 2048");
  if (std::isnan(max_lw) || max_lw == INFINITY) return fail(h, MCL_ERR_INVALID, "temper_sums: max_lw is NaN or +inf");
  RET_IF(temper_check(h, "temper_sums"));
  RET_IF(temper_sums_launch(h, max_lw, levels, n_levels));
  return temper_sums_fetch(h, n_levels, s1, s2);
}

int temper_apply(mcl_handle* h, int32_t j) {
  if (j < 0 || j > MCL_TEMPER_LEVELS) return fail(h, MCL_ERR_INVALID, "temper_apply: level outside 0 ... 2048");
  RET_IF(temper_check(h, "temper_apply"));
  if (j == 0) return MCL_OK;
  RET_IF(set_device(h));
  t_begin(h, MCL_K_NORMALISE);
  k_temper_apply<<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(h->lw, h->n, nullptr, temper_beta(j));
  t_end(h);
  HIPCHK(h, hipGetLastError());
  temper_applied(h);
  return MCL_OK;
}

// mcl_group_temper: the shards' maxima and live counts, then temper_search over the added sums, then the apply
int group_temper_run(mcl_handle** sh, int ns, long long n_target, bool apply, mcl_temper_result* out) {
  long long ng = 0;
  for (int s = 0; s < ns; ++s) {
    RET_IF(temper_check(sh[s], "group_temper"));
    if (sh[s]->comm) return fail(sh[s], MCL_ERR_UNSUPPORTED, "group_temper: a handle with an RCCL communicator");
    ng += sh[s]->n;
  }
  RET_IF(temper_target_check(sh[0], "group_temper", ng, n_target));
  for (int s = 0; s < ns; ++s) {
    mcl_handle* h = sh[s];
    RET_IF(set_device(h));
    RESERVE(h, h->temper_dev, TP_WORDS);
    const int gm = grid_for(h->n);
    t_begin(h, MCL_K_NORMALISE);
    k_temper_max<<<gm, MCL_BLOCK, 0, h->stream>>>(h->lw, h->n, h->temper_dev);
    k_temper_pick<<<1, MCL_BLOCK, 0, h->stream>>>(h->temper_dev, 0, gm, n_target);
    t_end(h);
    HIPCHK(h, hipGetLastError());
  }
  double m = -INFINITY;
  long long live = 0;
  for (int s = 0; s < ns; ++s) {
    u64 w[TP_SUMS];
    RET_IF(pull_sync(sh[s], w, sh[s]->temper_dev, sizeof w));
    double ms;
    memcpy(&ms, w + TP_M, sizeof ms);
    if (ms > m) m = ms;
    live += (long long)w[TP_NLIVE];
  }
  int j = 0, floor_hit = 0, levels = 0;
  RET_IF(temper_search(
      n_target,
      [&](const int32_t* cand, int nc, uint64_t* s1, uint64_t* s2) {
        for (int s = 0; s < ns; ++s) RET_IF(temper_sums_launch(sh[s], m, cand, nc));
        for (int k = 0; k < nc; ++k) s1[k] = s2[k] = 0;
        for (int s = 0; s < ns; ++s) {
          uint64_t p1[MCL_TEMPER_MAX_CAND], p2[MCL_TEMPER_MAX_CAND];
          RET_IF(temper_sums_fetch(sh[s], nc, p1, p2));
          for (int k = 0; k < nc; ++k) {
            s1[k] += p1[k];
            s2[k] += p2[k];
          }
        }
        return (int)MCL_OK;
      },
      &j, &floor_hit, &levels));
  if (apply)
    for (int s = 0; s < ns; ++s) RET_IF(temper_apply(sh[s], j));
  if (out) {
    out->j = j;
    out->floor_hit = floor_hit;
    out->levels_evaluated = levels;
    out->reserved = 0;
    out->n_target = n_target;
    out->n_live = live;
    out->beta = temper_beta(j);
    out->max_lw = m;
  }
  return MCL_OK;
}

}  // namespace
