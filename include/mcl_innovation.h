/* mcl_innovation.h -- ping innovation statistics and per-beam outlier gating on top of the C ABI in mcl.h (same library,
 * same handle, same conventions; MCL_ABI_VERSION stays 4: nothing declared in mcl.h changes).
 *
 * mcl_update_mbes takes every ping on faith.  Here the ping is first held against the PRIOR cloud, beam by beam: which
 * beams does no hypothesis explain (fish, a bottom-detection failure), is sigma right (the normalised innovation should
 * be about 1 per beam), and does the whole ping disagree with the cloud (a kidnap, a wrong map).  Nothing here changes a
 * weight or a particle: the caller marks the beams it distrusts invalid -- ranges[b] = 0, the convention mcl_update_mbes
 * already has -- and then runs the unchanged update.
 *
 * Definition.  A ping is (r_b, a_b), b < B, 1 <= B <= MCL_INNOVATION_MAX_BEAMS; beam b looks along (0, sin a_b, -cos a_b)
 * in the sensor frame (mcl_innovation_dirs is the float table the kernel reads).  Sensor offset, r_max and the map are as
 * for mcl_update_mbes.
 *
 *   Sample.  The particles whose global id g = global_offset + slot satisfies g mod stride == 0, stride =
 *   ceil(n_global / max_samples), 1 <= max_samples <= MCL_INNOVATION_MAX_SAMPLES (mcl_innovation_sample).  After a resample
 *   the slots hold offspring in ancestor order, so a strided subset is a systematic subsample of an equally weighted
 *   cloud.  The statistics treat the sample as a SET: pending log-weights are ignored by definition.  Call between predict
 *   and update, which is where the node calls it.
 *
 *   Expected range.  For every sampled particle i and every beam b with a valid r_b (r_b > 0; zero, negative and NaN mark
 *   a beam without a return), e_ib is the range of the first hit of the beam with the map, r_max without one: fp64 pose,
 *   fp32 ray in coordinates relative to the particle's own cell -- the arithmetic of mcl_update_ranges for that direction.
 *
 *   Quantisation.  q_ib = rint(((double)r_b - (double)e_ib) * 2^12), clamped to +-2^24: a signed integer in units of
 *   2^-12 m = 0.24 mm.  r_max > MCL_INNOVATION_MAX_RANGE (4096 m) is MCL_ERR_INVALID, so the clamp only ever bites on an
 *   absurd measured range.  |q| <= 2^24, q^2 <= 2^48, and 2^15 samples keep the sum of q^2 within 2^63.
 *
 *   Record of a beam (mcl_innovation_beam), all integers:  n rays cast;  n_miss rays with e = r_max;  n_within rays with
 *   |q| <= q_support = min(floor(support_k sigma 2^12), 2^24);  s1 = sum q;  s2 = sum q^2.  An invalid beam: all zero.
 *
 * Every field is a sum of integers.  The record therefore has the same bits on every run, for every launch geometry and
 * group size, and for every split of the cloud into shards: the shards' records simply add (mcl_innovation_merge).  That
 * argument replaces a fixed reduction tree -- the kernel adds with integer atomics in whatever order the hardware runs.
 *
 * Derived per beam with n > 0 (mcl_innovation_gate; every IEEE operation rounded on its own):
 *     nu      = (double)s1 / ((double)n * 4096)                      mean innovation, metres
 *     V       = (double)(n s2 - s1^2) / (double)(n n) * 2^-24        its variance over the sample, m^2: the numerator is a
 *                                                                   128-bit integer, >= 0 exactly, converted to the nearest
 *                                                                   double (ties to even)
 *     NIS     = nu nu / (V + sigma sigma)                            normalised innovation squared, ~1 on a consistent run
 *     support = (double)n_within / (double)n                         share of the sample that explains the beam
 * A beam with n = 0 has nu = V = NIS = support = 0 and is not valid.
 *
 * Gate (mcl_innovation_gate_config; policy defaults, not tolerances: nis_gate 10.83 -- chi^2_1 at 0.999 --, min_support
 * 0.01, max_gated_fraction 0.25).  Beam b is a CANDIDATE iff NIS_b > nis_gate and support_b < min_support: the mean
 * disagrees and almost no hypothesis explains the beam.  If (double)candidates > max_gated_fraction * (double)n_valid
 * nothing is gated and inconsistent = 1: the ping disagrees with the cloud as a whole, and blinding the filter is the wrong
 * answer to a kidnap.  Otherwise the candidates are gated.
 *
 * Launches take no timing slot (MCL_K_COUNT stays 15).  Out of scope: a weighted variant, the fused steps, an in-library
 * collective (mcl_group_ping_innovation serves shards of one process).
 */
#ifndef MCL_INNOVATION_H
#define MCL_INNOVATION_H
#include "mcl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_INNOVATION_MAX_BEAMS 2048
#define MCL_INNOVATION_MAX_SAMPLES 32768
#define MCL_INNOVATION_DEFAULT_SAMPLES 4096
#define MCL_INNOVATION_MAX_RANGE 4096.0          /* metres: the largest r_max */
#define MCL_INNOVATION_QUANTUM_LOG2 12           /* q is in units of 2^-12 m */
#define MCL_INNOVATION_Q_MAX (1ll << 24)         /* |q| <= 2^24 */

typedef struct mcl_innovation_beam {
  int64_t n;         /* rays cast (0: the beam is invalid, or no particle of this shard is sampled) */
  int64_t n_miss;    /* ... of which e = r_max */
  int64_t n_within;  /* ... of which |q| <= q_support */
  int64_t s1;        /* sum q */
  uint64_t s2;       /* sum q^2 */
} mcl_innovation_beam;

typedef struct mcl_innovation_gate_config {
  double nis_gate;            /* >= 0 */
  double min_support;         /* in [0, 1] */
  double max_gated_fraction;  /* in [0, 1] */
} mcl_innovation_gate_config;

typedef struct mcl_innovation_derived {   /* one beam */
  double nu, var, nis, support;
  int32_t valid;   /* n > 0 */
  int32_t gated;   /* the mask: 1 = set ranges[b] to 0 before the update */
} mcl_innovation_derived;

typedef struct mcl_innovation_verdict {
  int32_t n_valid;       /* beams with n > 0: the degrees of freedom of nis_sum */
  int32_t n_candidates;
  int32_t n_gated;       /* n_candidates, or 0 when inconsistent */
  int32_t inconsistent;
  double nis_sum;        /* sum of NIS_b over the valid beams, in beam order */
  double mean_nu;        /* (sum of nu_b over the valid beams, in beam order) / n_valid; 0 without a valid beam */
} mcl_innovation_verdict;

/* ---- device-free */
/* dirs_out[3 b ...] = the unit direction of beam b as the kernel reads it: (0, sin a, -cos a) in fp64, rounded to float,
 * normalised in fp64, rounded again -- the table mcl_update_ranges would build from the rounded triple.
 * MCL_ERR_INVALID: a null pointer, B outside 1 ... MCL_INNOVATION_MAX_BEAMS, an angle that is not finite. */
int mcl_innovation_dirs(const float* beam_angles, int32_t B, float* dirs_out);
/* *stride = ceil(n_global / max_samples), *count = ceil(n_global / stride): the ids 0, stride, 2 stride, ... below n_global.
 * MCL_ERR_INVALID: n_global < 1, max_samples outside 1 ... 32768, a null pointer. */
int mcl_innovation_sample(int64_t n_global, int32_t max_samples, int64_t* stride, int64_t* count);
/* out[b] = the field-wise sum of parts[p * B + b] over p < n_parts.  MCL_ERR_INVALID: a null pointer, n_parts < 1, B < 1,
 * a part that is no record of the definition (see mcl_innovation_gate), or a sum beyond the bounds above (n > 32768). */
int mcl_innovation_merge(const mcl_innovation_beam* parts, int32_t n_parts, int32_t B, mcl_innovation_beam* out);
/* The derived quantities and the gate.  cfg NULL: the defaults.  per_beam (B entries) may be NULL.  MCL_ERR_INVALID: a null
 * beams / verdict, B < 1, sigma not finite or <= 0, a config outside its ranges, or a record that cannot be a sum of the
 * definition: n outside 0 ... 32768, n_miss or n_within outside 0 ... n, |s1| > n 2^24, s2 > n 2^48, s1^2 > n s2. */
int mcl_innovation_gate(const mcl_innovation_beam* beams, int32_t B, double sigma, const mcl_innovation_gate_config* cfg,
                        mcl_innovation_derived* per_beam, mcl_innovation_verdict* verdict);

/* ---- one handle: the records of THIS shard's sampled particles (a single handle: of the whole sample).  Reads the handle
 * and never writes particles, log-weights, counters or caches (a fused step's deferred z / roll / pitch are stored first, as
 * every range call does).  One synchronisation, at the end.  exp_out (or NULL; production passes NULL): *n_sampled x B
 * floats, sample-major in ascending slot order, e_ib -- the entries of invalid beams are unspecified; room for
 * ceil(n_particles / stride) rows is enough.  *n_sampled: this shard's sampled particles (may be 0).
 * MCL_ERR_INVALID: a null pointer, B outside 1 ... MCL_INNOVATION_MAX_BEAMS, sigma <= 0 or not finite, support_k < 0 or not
 * finite, r_max <= 0 or > 4096, max_samples outside 1 ... 32768, an angle that is not finite.  MCL_ERR_STATE: no map, no
 * particles. */
int mcl_ping_innovation(mcl_handle* h, const float* ranges, const float* beam_angles, int32_t B, double sigma,
                        double support_k, double r_max, const double sensor_offset[6], int32_t max_samples,
                        mcl_innovation_beam* beams_out, float* exp_out, int64_t* n_sampled);
/* Several shards in one process: the shards' records, merged.  Equals mcl_ping_innovation on the unsharded cloud bit for
 * bit.  *n_sampled: the sum over the shards. */
int mcl_group_ping_innovation(mcl_handle** shards, int32_t n_shards, const float* ranges, const float* beam_angles, int32_t B,
                              double sigma, double support_k, double r_max, const double sensor_offset[6],
                              int32_t max_samples, mcl_innovation_beam* beams_out, int64_t* n_sampled);

#ifdef __cplusplus
}
#endif
#endif /* MCL_INNOVATION_H */
