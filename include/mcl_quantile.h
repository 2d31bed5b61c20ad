/* mcl_quantile.h -- exact order statistics of the cloud on top of the C ABI in mcl.h (same library, same handle, same
 * conventions; MCL_ABI_VERSION stays 4: nothing declared in mcl.h changes).
 *
 * A covariance says little about a posterior that is wide, skewed or multi-modal.  What a consumer of a navigation
 * filter asks for is a radius that holds 50 % or 95 % of the posterior (CEP, R95, a horizontal protection level), a
 * heading bound and a robust point estimate: the k-th smallest of n values, optionally weighted by the pending
 * log-weights.  Here that is a selection over order-preserving integer keys with integer masses: exact, and the same
 * bits on every run, for every launch geometry and for every split of the cloud into shards.
 *
 * Quantity of particle i.  Every IEEE double operation is rounded on its own (no contraction).  The centre
 * c = (cx, cy, cyaw) is the caller's, in the state's odom frame, and must be finite.
 *     MCL_Q_X, MCL_Q_Y      x_i, y_i
 *     MCL_Q_YAW_DEV         wrap_pi(yaw_i - cyaw): the library's wrap, (a + pi) mod (2 pi) - pi with the floored modulo
 *                           of the reference (auv_particle.py:48), bit-equal to numpy's %
 *     MCL_Q_ABS_YAW_DEV     fabs of the above
 *     MCL_Q_RADIUS2         dx dx + dy dy with dx = x_i - cx, dy = y_i - cy (two products, one sum).  The caller takes the
 *                           correctly rounded square root of the answer: sqrt is monotonic, the order is the radius's.
 *
 * Key.  K_i = key(v_i + 0.0), key the order-preserving map of a double onto a uint64 (sign bit set: all bits inverted;
 * else the sign bit set).  Adding 0.0 turns -0 into +0: both have one key.  A NaN value takes the particle out of the
 * query; n_used counts the rest.  +inf and -inf are ordinary values.
 *
 * Mass.  Unweighted: q_i = 1.  Weighted: q_i = floor(det_exp(lw_i - m) * 2^32), m the largest finite pending log-weight
 * of the WHOLE cloud, det_exp the library's deterministic exponential: exactly q1 of mcl_temper.h at level 0.  A
 * log-weight that is NaN, -inf or +inf gives 0.  S = sum of q_i over the used particles, a uint64.  Weighted queries need
 * pending log-weights that are logarithms (not MCL_WEIGHT_LINEAR), else MCL_ERR_STATE, and n_global <= 2^24
 * (S < 2^57), else MCL_ERR_UNSUPPORTED.
 *
 * Quantile at probability p.  P = floor(p * 2^32); MCL_ERR_INVALID unless 2^-32 <= p <= 1.  The answer is the smallest
 * key K among the used particles with
 *     2^32 * M(K) >= P * S,        M(K) = sum of q_i over the used particles with K_i <= K,
 * compared in 128-bit integers.  S = 0 (no used particle, or no mass): the value is NaN, mass = 0, status MCL_OK.
 * p = 0.5 on an unweighted cloud is the lower median; p = 1 the maximum; p = 2^-32 the smallest key that carries mass.
 *
 * How.  A most-significant-byte-first radix select over the keys: one reduction finds the smallest and largest key (and
 * m), the leading bytes they share are skipped -- a tracking cloud has x = 512.3... for every particle --, and every
 * further round histograms the next 8 key bits of the particles that still match each probability's prefix (LDS, then
 * global, integer atomics only: the order of integer adds cannot matter) and a one-workgroup kernel picks each
 * probability's bin -- in device memory, no host round trip between the rounds.  Skipping the shared bytes does not change
 * the definition.  The keys are recomputed from the state in every round; nothing of the particle count is stored.
 *
 * Nothing here writes the handle's particles, weights, counters or caches: the filter computes what it computes without
 * the calls.  Launches are timed under MCL_K_MEAN_COV.
 *
 * Out of scope: quantiles of the drift states, Mahalanobis / ellipse quantities, the fused steps, an in-library
 * collective.  No multi-GPU machine has run the split calls (mcl_cloud_mass, mcl_cloud_key_hist) across processes;
 * mcl_group_cloud_quantiles (one process) is what the tests drive.
 */
#ifndef MCL_QUANTILE_H
#define MCL_QUANTILE_H
#include "mcl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_Q_X 0
#define MCL_Q_Y 1
#define MCL_Q_YAW_DEV 2
#define MCL_Q_ABS_YAW_DEV 3
#define MCL_Q_RADIUS2 4
#define MCL_QUANTILE_MAX 8                        /* probabilities of one call, values of one mcl_cloud_mass call */
#define MCL_QUANTILE_MAX_PARTICLES (1ll << 24)    /* weighted queries */

typedef struct mcl_quantile_query {
  int32_t quantity;   /* MCL_Q_* */
  int32_t weighted;   /* 0: every particle counts 1; else by the pending log-weights */
  double centre[3];   /* cx, cy, cyaw (odom frame); finite */
} mcl_quantile_query;

typedef struct mcl_quantile_result {
  double value;     /* the quantile (NaN: S = 0) */
  uint64_t key;     /* its key */
  uint64_t mass;    /* M(key) */
  uint64_t total;   /* S */
  int64_t n_used;   /* particles whose value is not NaN */
} mcl_quantile_result;

/* ---- pure host arithmetic: no handle, no device */
/* *key = key(v + 0.0).  MCL_ERR_INVALID: v is NaN. */
int mcl_quantile_key(double v, uint64_t* key);
/* The inverse, for every uint64: keys below key(-inf) or above key(+inf) are no key of a value and decode to a NaN. */
int mcl_quantile_value(uint64_t key, double* v);
/* *P = floor(p * 2^32).  MCL_ERR_INVALID unless 2^-32 <= p <= 1 (NaN included). */
int mcl_quantile_threshold(double p, uint64_t* P);
/* *reached = (2^32 * mass >= P * total), exact for every uint64 mass, total and P. */
int mcl_quantile_reached(uint64_t mass, uint64_t total, uint64_t P, int32_t* reached);

/* ---- one handle: the quantiles at probs[0 ... n_probs) (1 <= n_probs <= 8; any order, repeats allowed), all found in
 * the same passes; out[k] belongs to probs[k].  One synchronisation, at the end.  Reads the handle, never writes it.
 * MCL_ERR_STATE: no particles yet; weighted without pending log-weights or with linear ones.  MCL_ERR_INVALID: a null
 * pointer, an unknown quantity, a centre that is not finite, n_probs outside 1 ... 8, a probability outside
 * [2^-32, 1].  MCL_ERR_UNSUPPORTED: a shard of a larger cloud (world > 1: use mcl_group_cloud_quantiles or the split
 * calls); weighted with n_global > 2^24. */
int mcl_cloud_quantiles(mcl_handle* h, const mcl_quantile_query* query, const double* probs, int32_t n_probs,
                        mcl_quantile_result* out);

/* ---- the inverse question, in one pass: mass[k] = M(key(values[k])) -- how much of the posterior lies within 5 m of
 * here? --, *total = S, *n_used, of THIS shard alone (no collective; the integers of several shards simply add).
 * 1 <= n_values <= 8; a NaN value is MCL_ERR_INVALID.  max_lw (weighted; ignored otherwise) is the m of the mass rule and
 * must be >= every finite log-weight of the cloud (a larger log-weight counts as equal to it); -inf: all masses 0; NaN or
 * +inf: MCL_ERR_INVALID -- as in mcl_temper_sums.  One synchronisation. */
int mcl_cloud_mass(mcl_handle* h, const mcl_quantile_query* query, double max_lw, const double* values, int32_t n_values,
                   uint64_t* mass, uint64_t* total, int64_t* n_used);

/* ---- shards.  hist[d] = the mass of THIS shard's used particles whose key has the leading prefix_bits bits equal to
 * `prefix` (its low prefix_bits bits; the rest must be 0) and the next 8 bits equal to d.  prefix_bits is one of 0, 8, ...,
 * 56.  max_lw as above.  One synchronisation. */
int mcl_cloud_key_hist(mcl_handle* h, const mcl_quantile_query* query, double max_lw, uint64_t prefix, int32_t prefix_bits,
                       uint64_t hist[256]);
/* Several shards in one process: handles that TOGETHER hold the cloud (n_global = the sum of their sizes; any sizes, any
 * order), host-driven: the shards' maxima and key ranges, then at most eight rounds of added histograms.  The result
 * equals mcl_cloud_quantiles on the unsharded cloud bit for bit, for any split.  No in-library collective. */
int mcl_group_cloud_quantiles(mcl_handle** shards, int32_t n_shards, const mcl_quantile_query* query, const double* probs,
                              int32_t n_probs, mcl_quantile_result* out);

#ifdef __cplusplus
}
#endif
#endif /* MCL_QUANTILE_H */
