/* mcl_reseed.h -- sensor resetting: replace particles by draws from a mixture of Gaussians, and the rule that turns the
 * fixes of mcl_match_ping / mcl_match_swath into that mixture, on top of mcl_recovery.h and mcl_swath.h (same library, same
 * handle, same conventions; MCL_ABI_VERSION stays 4 and MCL_K_COUNT 15: nothing declared in an existing header changes,
 * and no existing kernel, weight or draw does).
 *
 * mcl_inject_uniform scatters the injected particles over a box: on a survey-sized map, or with a cloud sized for
 * tracking, almost none of them lands inside the basin of the true pose.  Sensor resetting (Lenser and Veloso 2000) draws
 * them from what the measurement itself says: here, from the converged fixes of mcl_match_swath started on a lattice over
 * the map, each with the covariance the terrain gives it.  The injected particles are PROPOSALS: the next pings weigh
 * them, so no ping's likelihood is counted twice.  A handle that never calls mcl_inject_gaussian queues exactly the
 * launches it queued before.
 *
 * Definition of mcl_inject_gaussian.  Everything mcl_inject_uniform says holds, except the draws and the values: the states
 * it may be called in (MCL_ERR_STATE with log-weights pending), fraction == 0 launches nothing and changes nothing, the
 * spatial visiting order is voided, the launches are timed under MCL_K_NOISE, n_injected (optional) is counted on the
 * device and read back with the call's one synchronisation (without it the call does not wait), and a shard of a sharded
 * cloud draws by GLOBAL particle id.
 *   Draws, MCL_RNG_NATIVE.  Philox4x32-10, key = the seed, counter (GLOBAL id, block, step, purpose 9); step = the handle's
 *     injection counter, which mcl_inject_uniform shares: 0 after either init call, +1 per injection OF EITHER KIND that
 *     launched (the purposes differ -- 6 and 9 --, so mcl_inject_uniform's draws keep their bits).
 *       block 0 = (a0, a1, a2, a3):  u_select = U(a0, a1), the rule of mcl_recovery.h;
 *                                    t = ((uint64_t)(a2 >> 5) << 26) | (a3 >> 6), a 53-bit integer
 *       block 1 = (b0, b1, b2, b3):  (xi_0, xi_1) = box_muller(b0, b1),  (xi_2, unused) = box_muller(b2, b3)
 *     -- the library's pairing of words and normals.  Block 1 is evaluated for replaced particles only.
 *   Draws, MCL_RNG_REPLAY.  replay is n x 5 doubles, particle-major: u_select, u_comp, xi_0, xi_1, xi_2, with
 *     t = floor(u_comp 2^53) (exact: a scaling by a power of two).  NULL, or a u_comp outside [0, 1), is MCL_ERR_INVALID.
 *   Selection.  Particle gid is replaced iff u_select < fraction.
 *   Component.  W = sum of the masses, 1 <= W <= 2^31.  r = (t W) >> 53, of the 128-bit product: 0 <= r < W.  The component
 *     is the first c with cum_c > r, cum the inclusive prefix sum of the masses.  Integers only: a component of mass 0 is
 *     never drawn, one of mass m is drawn with probability m / W up to 2^-22 (t has 53 bits, W at most 31).
 *   Value.  With L the component's factor:  z_r = sum_{c <= r} L_rc xi_c, c increasing, starting from the first product;
 *     v_r = mean_r + z_r.  Every product and every sum is one IEEE double operation of its own, not fused (the apply rule
 *     of mcl_regularise.h).  A row of L that is entirely zero gives v_r = mean_r, the mean's own bits (whatever xi is).
 *     r = 0, 1, 2 are x, y, yaw.  Yaw is stored as v if -pi <= v < pi, else wrap_pi(v) (the rule of mcl_drift_advance).
 *   What a replaced particle keeps: its slot's z, roll and pitch, its drift states (mcl_drift.h) and its genealogy links
 *     (mcl_history.h).  Every other particle keeps every bit.
 *   MCL_ERR_INVALID: a null handle or null comps; n_comp outside 1 ... MCL_RESEED_MAX_COMPONENTS; a fraction outside [0, 1]
 *     or not finite; a mean or a factor entry that is not finite; a negative diagonal of L; W = 0 or W > 2^31; in REPLAY
 *     mode a null replay or a u_comp outside [0, 1).  After an error the handle is as it was.
 *
 * Definition of mcl_reseed_select (device-free; one IEEE operation at a time).  From M results of mcl_match_ping or
 * mcl_match_swath, their config and sigma:
 *   1. Result i is a CANDIDATE iff its status is MCL_MATCH_CONVERGED and, with d = mcl_swath_derived(its final record, the
 *      config, sigma):  d.m >= min_beams  and  d.rms <= max_rms.
 *   2. The candidates are ordered by rms ascending, ties by the lower index.  Each in turn is TAKEN unless some fix taken
 *      before it lies within sep_xy of it (sqrt(dx dx + dy dy) <= sep_xy: a root of a sum of two products, not hypot) AND
 *      within sep_yaw (|wrap(yaw - yaw')| <= sep_yaw, the difference wrapped by the library's rule).  Taking stops at
 *      max_components.
 *   3. The covariance of a taken fix over (x, y, yaw), packed (0,0) (1,0) (1,1) (2,0) (2,1) (2,2): cov_scale times the
 *      first six words of d.cov; for a dimension k < 3 in d.dead (the terrain cannot fix it: its d.cov diagonal is +inf) row
 *      and column k become zero and the diagonal dead_std * dead_std (dead_std_xy for x and y, dead_std_yaw for yaw); then
 *      add_std * add_std is added to each diagonal (add_std_xy, add_std_xy, add_std_yaw).
 *   4. chol = mcl_regularise_factor of that covariance, dims 3 (the same function; its dead mask is not kept: a column it
 *      kills is a dimension without spread).
 *   5. mass = 1, reserved = 0, mean = (x, y, yaw) of the result.
 *   6. index_out[c] = i.
 *   7. *n_out = 0 (no candidate) is MCL_OK.
 *   MCL_ERR_INVALID: a null pointer, M outside 1 ... 65536, a config either check refuses, sigma not positive and finite,
 *   a CONVERGED result whose final record mcl_swath_derived refuses or whose pose is not finite.
 *
 * Out of scope: a pose-fix measurement update from the match (it would count pings twice); a prior term in the fit;
 * injecting drift states or z; per-component counts from the device; the ROS nodes; the fused steps; adaptive particle
 * counts.
 */
#ifndef MCL_RESEED_H
#define MCL_RESEED_H
#include "mcl_recovery.h"
#include "mcl_swath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_RESEED_MAX_COMPONENTS 256

typedef struct mcl_reseed_component {
  double mean[3];   /* x, y, yaw in the coordinates the state is stored in (what mcl_match_* returns) */
  double chol[6];   /* lower-triangular factor L of the 3 x 3 covariance, packed (0,0) (1,0) (1,1) (2,0) (2,1) (2,2) */
  uint32_t mass;    /* integer mixture weight; 0 = never drawn */
  uint32_t reserved;
} mcl_reseed_component; /* 80 bytes */

typedef struct mcl_reseed_select_config {
  int32_t max_components;      /* 1 ... 256 */
  int32_t min_beams;           /* contributing beams m of the final record (>= 1) */
  double max_rms;              /* metres; a fix with a larger final rms residual is no candidate (>= 0) */
  double sep_xy, sep_yaw;      /* two fixes closer than both are one hypothesis (>= 0) */
  double cov_scale;            /* multiplies the fix's covariance (> 0) */
  double add_std_xy, add_std_yaw;    /* added in quadrature on the diagonal (>= 0): model error, basin width */
  double dead_std_xy, dead_std_yaw;  /* the spread along a dimension the terrain cannot fix (> 0): e.g. the start lattice's pitch */
} mcl_reseed_select_config; /* 72 bytes */

/* ---- device-free */
/* MCL_OK, or MCL_ERR_INVALID with *reason (or NULL) the rule that is broken. */
int mcl_reseed_select_check(const mcl_reseed_select_config* cfg, const char** reason);
/* The rules of mcl_inject_gaussian for a table of components: MCL_OK, or MCL_ERR_INVALID with *reason (or NULL). */
int mcl_reseed_components_check(const mcl_reseed_component* comps, int32_t n_comp, const char** reason);
/* comps_out and index_out: room for cfg->max_components entries. */
int mcl_reseed_select(const mcl_match_result* results, int64_t M, const mcl_match_config* mcfg, double sigma,
                      const mcl_reseed_select_config* cfg, mcl_reseed_component* comps_out, int64_t* index_out,
                      int32_t* n_out);

/* ---- one handle */
int mcl_inject_gaussian(mcl_handle* h, double fraction, const mcl_reseed_component* comps, int32_t n_comp,
                        const double* replay /* n x 5, REPLAY mode */, int64_t* n_injected);

#ifdef __cplusplus
}
#endif
#endif /* MCL_RESEED_H */
