/* mcl_temper.h -- ESS-targeted likelihood tempering on top of the C ABI in mcl.h (same library, same handle, same
 * conventions; MCL_ABI_VERSION stays 4: nothing declared in mcl.h changes).
 *
 * A ping of hundreds of beams multiplies hundreds of Gaussian factors into every weight: the effective sample size after
 * one update is close to 1 and the resample copies one particle n times.  The cure is to raise the likelihood to a power
 * beta <= 1, chosen PER UPDATE as the largest exponent of a fixed lattice that still leaves a stated effective sample
 * size.  The choice is made on the device, next to the log-weights, and is decided by exact integer sums: the same bits
 * on every run, for every launch geometry and for every split of the cloud into shards.
 *
 * Exponent lattice.  Levels j = 0 ... MCL_TEMPER_LEVELS (2048), beta_j = 2^(-j / 64) = T[j mod 64] * 2^-(j div 64), T[i]
 * the correctly rounded double of 2^(-i / 64) (a table in the library), the power of two applied exactly.  beta_0 = 1,
 * beta_2048 = 2^-32 is the floor, and 2 beta_j = beta_(j - 64) exactly.
 *
 * Sums at a level.  m = the largest finite log-weight of the WHOLE cloud (all shards).  For particle i:
 *     d_i = lw_i - m          e_i = beta_j * d_i                        -- one IEEE double operation each, not fused
 *     q1_i = floor(det_exp(e_i) * 2^32)      q2_i = floor(det_exp(2 e_i) * 2^32)
 * det_exp: the library's deterministic exponential (fma / mul / rint / bit operations only; oracle/mcl_oracle.c states
 * it for the CPU, bit for bit).  S1 = sum q1_i, S2 = sum q2_i as unsigned 64-bit integers; a log-weight that is NaN, -inf
 * or +inf contributes 0 (as in mcl_weight_stats).  Integer sums: exact, whatever the order, tile, grid or shard split.
 *
 * Pass.  Level j passes for a target count n_t (1 <= n_t <= n_global) iff  S1^2 >= n_t * S2 * 2^32  in 128-bit integers,
 * i.e. the effective sample size of the fixed-point weights is >= n_t.  n_global <= 2^24 keeps both sides below 2^112; a
 * larger cloud is refused (MCL_ERR_UNSUPPORTED).
 *
 * Search.  Three rounds; each scans its candidates upwards and takes the first that passes:
 *     round 1   j = 0, 128, ..., 2048        none passes: result 2048, floor_hit = 1.  first pass j1; j1 = 0: result 0
 *     round 2   j1 - 120, j1 - 112, ..., j1 - 8   none passes: j2 = j1.                     first pass j2
 *     round 3   j2 - 7, ..., j2 - 1               none passes: result j2.                   first pass: the result
 * at most 17 + 15 + 7 = 39 levels.  The result is DEFINED by this procedure, not by monotonicity of the effective sample
 * size in beta; the level below the result has always been evaluated and has failed.  levels_evaluated counts every
 * candidate of every round that ran (17, or 17 + 15 + 7).
 *
 * Apply.  lw_i <- beta_j * lw_i: one IEEE product, no shift by m; non-finite values keep every bit; the weight mode of
 * the update stays.  j = 0 stores nothing: every bit of the log-weights, and of the resample that follows, is what it
 * would be without the call.  (mcl_temper decides on the device, so its apply launch is queued before j is known and
 * returns at once when j = 0; mcl_temper_apply and mcl_group_temper know j on the host and launch nothing.)
 *
 * Out of scope: the fused steps (mcl_step_mbes*, and so the roscpp node) resample inside one call and are not tempered;
 * a handle with an RCCL communicator is refused by mcl_temper -- ranks use the split calls (mcl_temper_sums /
 * mcl_temper_apply) and add the integer sums themselves; an in-library collective is not provided.  No multi-GPU machine
 * has run the split calls across processes; mcl_group_temper (one process) is what the tests drive.
 */
#ifndef MCL_TEMPER_H
#define MCL_TEMPER_H
#include "mcl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_TEMPER_LEVELS 2048          /* the floor: beta = 2^-32 */
#define MCL_TEMPER_MAX_CAND 17          /* candidates of one round, levels of one mcl_temper_sums call */
#define MCL_TEMPER_MAX_PARTICLES (1ll << 24)

typedef struct mcl_temper_result {
  int32_t j;                 /* the level, 0 ... 2048 */
  int32_t floor_hit;         /* 1: not even the floor passed (j = 2048) */
  int32_t levels_evaluated;  /* candidates of the rounds that ran */
  int32_t reserved;
  int64_t n_target, n_live;  /* the target count; log-weights that are finite (whole cloud) */
  double beta;               /* beta_j */
  double max_lw;             /* m (-inf: no finite log-weight; then j = 0) */
} mcl_temper_result;

/* ---- pure host arithmetic: no handle, no device */
/* beta_j.  MCL_ERR_INVALID: j outside 0 ... 2048. */
int mcl_temper_beta(int32_t j, double* beta);
/* *pass = (s1^2 >= n_target * s2 * 2^32), exact for every uint64 s1, s2 and every n_target >= 1. */
int mcl_temper_pass(uint64_t s1, uint64_t s2, int64_t n_target, int32_t* pass);
/* The candidates of `round` (1, 2, 3), ascending.  j_prev: ignored in round 1; round 2: j1 (a multiple of 128, 0 ... 2048);
 * round 3: j2 (a multiple of 8, 0 ... 2048).  j_prev = 0 gives no candidates.  MCL_ERR_INVALID otherwise. */
int mcl_temper_candidates(int32_t round, int32_t j_prev, int32_t cand[MCL_TEMPER_MAX_CAND], int32_t* n_cand);

/* ---- one handle: the whole search, on the device (max, three rounds of sums + pick, apply: no host round trip).
 * apply != 0 scales the log-weights.  out may be NULL: the call then does not wait for the GPU.  Timed under
 * MCL_K_NORMALISE.  MCL_ERR_STATE: no pending log-weights (before the first update, after a resample), pending weights
 * declared MCL_WEIGHT_LINEAR (they are no logarithms), a shard of a larger cloud (use mcl_group_temper or the split
 * calls).  MCL_ERR_INVALID: n_target < 1 or > n_global.  MCL_ERR_UNSUPPORTED: a handle with an RCCL communicator,
 * n_global > 2^24. */
int mcl_temper(mcl_handle* h, int64_t n_target, int32_t apply, mcl_temper_result* out);

/* ---- split form, for shards: the caller takes the global maximum from mcl_weight_stats (+ merge), adds the shards'
 * sums, decides with mcl_temper_pass / mcl_temper_candidates and applies the level on every shard.
 * s1[k], s2[k] = THIS shard's sums at levels[k] (each 0 ... 2048; 1 <= n_levels <= 17) relative to max_lw, which must be
 * >= every finite log-weight of the shard (a larger one counts as equal to it); max_lw = -inf: all sums 0;
 * NaN or +inf: MCL_ERR_INVALID.  One synchronisation. */
int mcl_temper_sums(mcl_handle* h, double max_lw, const int32_t* levels, int32_t n_levels, uint64_t* s1, uint64_t* s2);
/* lw_i <- beta_j lw_i on this shard; j = 0 launches nothing.  Does not wait. */
int mcl_temper_apply(mcl_handle* h, int32_t j);

/* ---- several shards in one process: the same search over handles that TOGETHER hold the cloud (n_global = the sum of
 * their sizes; any sizes, any order: the sums do not depend on either), host-driven with one synchronisation per shard
 * per round.  Level and log-weights equal those of mcl_temper on the unsharded cloud bit for bit, for any split.
 * out (optional) as above.  Errors as mcl_temper, on any shard. */
int mcl_group_temper(mcl_handle** shards, int32_t n_shards, int64_t n_target, int32_t apply, mcl_temper_result* out);

#ifdef __cplusplus
}
#endif
#endif /* MCL_TEMPER_H */
