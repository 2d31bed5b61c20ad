/* mcl_information.h -- ping information: what the terrain can fix, per cloud and per pose, on top of the C ABI in mcl.h
 * (same library, same handle, same conventions; MCL_ABI_VERSION stays 4: nothing declared in mcl.h changes).
 *
 * The update of mcl.h is lw_i = -1/2 sum_b ((r_b - e_ib) / sigma)^2.  For that Gaussian range likelihood the Fisher
 * information of one ping about (x, y, yaw) is J = sigma^-2 sum_b g_b g_b^T, g_b the derivative of beam b's expected range
 * with respect to the pose; its inverse is the Cramer-Rao bound of one ping, its smallest eigenvector the direction the
 * terrain cannot fix.  Over a flat seabed J has no horizontal part however many beams the ping has; over a ridge it fixes
 * the across-ridge coordinate only.  Nothing here changes a weight or a particle.
 *
 * Definition.  A ping geometry is (a_b), b < B, 1 <= B <= MCL_INFORMATION_MAX_BEAMS: no measured ranges, information needs
 * none.  Beam b looks along the direction mcl_innovation_dirs gives it; sensor offset, r_max and the map are as for
 * mcl_update_mbes.
 *
 *   Steps.  delta_xy > 0 (metres), delta_yaw > 0 (radians), 0 < jump_max <= r_max, jump_max <= MCL_INFORMATION_MAX_JUMP
 *   (2048 m), r_max <= MCL_INFORMATION_MAX_RANGE (4096 m); all finite.
 *
 *   The six casts.  For a pose p = (x, y, z, roll, pitch, yaw) in the coordinates the particle state is stored in, beam b
 *   is cast from six perturbed states, in this order (the variant index v = 0 ... 5):
 *       x + delta_xy,  x - delta_xy,  y + delta_xy,  y - delta_xy,  yaw + delta_yaw,  yaw - delta_yaw
 *   -- one fp64 addition or subtraction on the stored number -- and then through the unchanged arithmetic of
 *   mcl_ping_innovation (fp64 pose, fp32 ray relative to the perturbed sensor's own cell).  The ranges are e_x+, e_x-,
 *   e_y+, e_y-, e_w+, e_w-.
 *
 *   Misses and jumps.  If any of the six equals r_max the pair (pose, beam) is a MISS.  Otherwise
 *       d_k = rint(((double)e_k+ - (double)e_k-) * 2^12),  k in {x, y, w}
 *   a signed integer in units of 2^-12 m, |d_k| <= 2^24 since 0 <= e <= r_max <= 4096 m.  If any |d_k| > floor(jump_max
 *   2^12) the pair is a JUMP: an occlusion edge, where the range is not differentiable.  Otherwise the pair CONTRIBUTES
 *   its six products d_j d_k.
 *
 *   A record (mcl_information_sums), all integers: n pairs cast, n_miss, n_jump, and over the contributing pairs
 *   sxx, syy, sww (unsigned) and sxy, sxw, syw (signed).
 *   Bound: jump_max <= 2048 m gives |d| <= 2^23 in a contributing pair, |d_j d_k| <= 2^46, and at most 2^15 pairs per
 *   record (MCL_INFORMATION_MAX_SAMPLES samples, or 2^11 beams) keep every sum within 2^61 < 2^63.
 *
 * Every field is a sum of integers, so a record has the same bits on every run, for every launch geometry and group size
 * and for every split of the cloud into shards: the shards' records add (mcl_information_merge).
 *
 * Two accumulations of the same pairs:
 *   per BEAM over a sample of the cloud (mcl_ping_information): the strided sample of mcl_innovation_sample, one record per
 *   beam;
 *   per POSE over the beams (mcl_pose_information): M caller-supplied poses, one record per pose; needs a map, no
 *   particles, and neither reads nor writes the cloud.
 *
 * Derived (mcl_information_matrix; device-free; every IEEE operation rounded on its own, an integer converted to the
 * nearest double).  With delta_x = delta_y = delta_xy, delta_w = delta_yaw, q_jk = (4.0 * delta_j) * delta_k, and the packed
 * order xx, xy, xw, yy, yw, ww:
 *     per_pose = 0, the records are the B beams of a cloud sample:  m_b = n_b - n_miss_b - n_jump_b,
 *         J_jk = (sum over the beams with m_b > 0, in beam order, of (double)S_jk / (((double)m_b * 2^24) * q_jk)) / (sigma * sigma)
 *         -- the sample mean of the ping's information;  hit_share = (double)(sum m_b) / (double)(sum n_b), 0 when sum n_b = 0
 *     per_pose = 1, every record is a pose of its own:
 *         J_jk = (double)S_jk / ((2^24 * q_jk) * (sigma * sigma));   hit_share = (double)m / (double)n, 0 when n = 0
 *   Position information with yaw marginalised, the Schur complement
 *         a = J_xx - J_xw J_xw / J_ww,  b = J_xy - J_xw J_yw / J_ww,  c = J_yy - J_yw J_yw / J_ww      (J_pp itself when J_ww == 0;
 *         each as X - (Y * Z) / J_ww; and a = b = c = 0 when a + c <= 2^-40 (J_xx + J_yy): yaw explains the ranges'
 *         changes altogether, and what the subtraction leaves is rounding)
 *   and in closed form  h = 0.5 * (a + c),  g = 0.5 * (a - c),  lambda_max = h + sqrt(g * g + b * b),
 *   lambda_min = det / lambda_max with det = a * c - b * b (0 when det <= 0),  weak_axis = 0.5 * atan2(2.0 * b, a - c) +
 *   pi / 2 folded into [0, pi): the direction of the lambda_min eigenvector in state coordinates.
 *         crlb_strong = 1 / sqrt(lambda_max),  crlb_weak = 1 / sqrt(lambda_min)
 *   rank_pos = 2, unless lambda_min <= 2^-40 lambda_max: then rank_pos = 1 and crlb_weak = +inf; unless lambda_max is not
 *   positive: then rank_pos = 0, crlb_strong = crlb_weak = +inf, lambda_max = lambda_min = 0 and weak_axis = 0.
 *
 * Launches take no timing slot (MCL_K_COUNT stays 15).  Out of scope: a weighted sample; information about z, roll or
 * pitch; the fused steps; an in-library collective (mcl_group_ping_information serves shards of one process); a
 * posterior-CRLB recursion.
 */
#ifndef MCL_INFORMATION_H
#define MCL_INFORMATION_H
#include "mcl.h"
#include "mcl_innovation.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_INFORMATION_MAX_BEAMS 2048
#define MCL_INFORMATION_MAX_SAMPLES 32768
#define MCL_INFORMATION_DEFAULT_SAMPLES 4096
#define MCL_INFORMATION_MAX_POSES (1 << 20)
#define MCL_INFORMATION_MAX_RANGE 4096.0   /* metres: the largest r_max */
#define MCL_INFORMATION_MAX_JUMP 2048.0    /* metres: the largest jump_max */
#define MCL_INFORMATION_QUANTUM_LOG2 12    /* d is in units of 2^-12 m */

typedef struct mcl_information_sums {
  int64_t n;        /* pairs (pose, beam) cast */
  int64_t n_miss;   /* ... of which one of the six rays found no seabed within r_max */
  int64_t n_jump;   /* ... of which, all six hitting, some |d_k| > floor(jump_max 2^12) */
  uint64_t sxx, syy, sww;   /* over the other pairs: sum d_x d_x, d_y d_y, d_w d_w */
  int64_t sxy, sxw, syw;    /* sum d_x d_y, d_x d_w, d_y d_w */
} mcl_information_sums;

typedef struct mcl_information_steps {
  double delta_xy;   /* metres, > 0 */
  double delta_yaw;  /* radians, > 0 */
  double jump_max;   /* metres, in (0, min(r_max, 2048)] */
} mcl_information_steps;

typedef struct mcl_information_result {
  double J[6];         /* xx, xy, xw, yy, yw, ww: 1/m^2, 1/(m rad), 1/rad^2 */
  double lambda_max, lambda_min;   /* of the 2x2 position information, yaw marginalised */
  double weak_axis;    /* [0, pi): direction of the lambda_min eigenvector, state coordinates */
  double crlb_strong, crlb_weak;   /* metres; +inf where the ping fixes nothing */
  double hit_share;    /* contributing pairs / pairs cast */
  int32_t rank_pos;    /* 0, 1, 2 */
  int32_t reserved;
} mcl_information_result;

/* ---- device-free */
/* out[b] = the field-wise sum of parts[p * B + b] over p < n_parts.  MCL_ERR_INVALID: a null pointer, n_parts < 1, B < 1,
 * a part that is no record of the definition (see mcl_information_matrix), or a sum with n > 32768. */
int mcl_information_merge(const mcl_information_sums* parts, int32_t n_parts, int32_t B, mcl_information_sums* out);
/* The derived quantities.  per_pose == 0: recs are the `count` beams of one cloud sample, out is ONE result; per_pose != 0:
 * out has `count` results, one per record.  MCL_ERR_INVALID: a null pointer, count < 1, sigma / delta_xy / delta_yaw not
 * positive and finite, or a record that cannot be a sum of the definition: n outside 0 ... 32768, n_miss or n_jump negative,
 * n_miss + n_jump > n, a square sum above m 2^46, or a cross sum whose square exceeds the product of its two square sums. */
int mcl_information_matrix(const mcl_information_sums* recs, int32_t count, int32_t per_pose, double sigma, double delta_xy,
                           double delta_yaw, mcl_information_result* out);

/* ---- one handle: the per-beam records of THIS shard's sampled particles (a single handle: of the whole sample).  Reads the
 * handle and never writes particles, log-weights, counters or caches (a fused step's deferred z / roll / pitch are stored
 * first, as every range call does).  One synchronisation, at the end.  ranges_out (or NULL; production passes NULL):
 * *n_sampled x 6 x B floats, sample-major in ascending slot order, then the variant v, then the beam; room for
 * ceil(n_particles / stride) samples is enough.
 * MCL_ERR_INVALID: a null pointer, B outside 1 ... 2048, r_max <= 0 or > 4096, steps outside their ranges, max_samples outside
 * 1 ... 32768, an angle that is not finite.  MCL_ERR_STATE: no map, no particles. */
int mcl_ping_information(mcl_handle* h, const float* beam_angles, int32_t B, double r_max, const double sensor_offset[6],
                         int32_t max_samples, const mcl_information_steps* steps, mcl_information_sums* beams_out,
                         float* ranges_out, int64_t* n_sampled);
/* Several shards in one process: the shards' records, merged.  Equals mcl_ping_information on the unsharded cloud bit for
 * bit.  *n_sampled: the sum over the shards. */
int mcl_group_ping_information(mcl_handle** shards, int32_t n_shards, const float* beam_angles, int32_t B, double r_max,
                               const double sensor_offset[6], int32_t max_samples, const mcl_information_steps* steps,
                               mcl_information_sums* beams_out, int64_t* n_sampled);
/* One record per caller-supplied pose: poses is host SoA, 6 x M doubles (x[M], y[M], z[M], roll[M], pitch[M], yaw[M]) in
 * the coordinates the particle state is stored in, 1 <= M <= 2^20.  The poses travel to a scratch buffer the handle owns;
 * the cloud is neither read nor written, and no particles are needed.  MCL_ERR_INVALID as above, and a pose that is not
 * finite.  MCL_ERR_STATE: no map. */
int mcl_pose_information(mcl_handle* h, const double* poses, int64_t M, const float* beam_angles, int32_t B, double r_max,
                         const double sensor_offset[6], const mcl_information_steps* steps, mcl_information_sums* poses_out);

#ifdef __cplusplus
}
#endif
#endif /* MCL_INFORMATION_H */
