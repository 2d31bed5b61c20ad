/* mcl_drift.h -- per-particle drift states: a water current and a yaw-rate bias that follow their particle through every
 * resample, on top of the C ABI in mcl.h (same library, same handle, same conventions; MCL_ABI_VERSION stays 4: nothing
 * declared in mcl.h changes, MCL_K_COUNT and mcl_timing are what they were).
 *
 * The predict integrates the odometry's body velocity and yaw rate with white process noise.  The two errors that dominate
 * an AUV's dead reckoning are not white: a water current (a DVL with water track or without lock measures the speed
 * through the water) and a gyro / compass rate bias.  Both are constants that integrate into metres; white noise can only
 * absorb them by widening the cloud on every step.  With the drift enabled every particle carries its own slowly varying
 * (cx, cy, bw); the particles whose drift is right keep agreeing with the fixes, the beacons and the seabed, survive the
 * resamples and take their drift with them: the filter estimates the current as a by-product (mcl_drift_mean_cov).  Off by
 * default; a handle that never enables it queues the launches it always queued.
 *
 * Definition.  State: three doubles per slot, SoA (cx[n], cy[n], bw[n]; 24 B per particle):  cx, cy the current in the
 * ODOM frame [m/s], bw the yaw-rate bias [rad/s].  d_c below is component c of a slot's drift, xi_c its standard normal.
 *   Prior (mcl_drift_enable, mcl_drift_reset).   d_c = init_std[c] * xi_c;  the advance counter k = 0.
 *   Advance (mcl_drift_advance(h, dt), called BEFORE the predict of the same dt -- mcl_predict or a fused mcl_step_mbes*).
 *     dt <= 0: nothing happens and nothing is counted (the predict's own gate), MCL_OK.  Otherwise k = k + 1 and, per slot,
 *     in this order:
 *       1. x   <- x + cx * dt,  y <- y + cy * dt
 *       2. t = yaw + bw * dt;  yaw <- t if -pi <= t < pi, else wrap_pi(t) = (t + pi) mod 2 pi - pi, floored modulo
 *       3. d_c <- d_c + (walk_std[c] * sqrt(dt)) * xi_c           (the product walk_std[c] * sqrt(dt) formed on the host)
 *     Every product and every sum is one IEEE double operation, not fused: a restatement in any language gives the same
 *     bits, also where a sum cancels.
 *     A component whose drift is exactly zero is not stored in steps 1 and 2, and a component whose walk_std is zero is
 *     not stored in step 3: a particle with zero drift keeps every bit of its pose.  z, roll and pitch are neither read
 *     nor written; no slot moves, so the fan sweep's visiting order stays what it was.
 *   Draws.   MCL_RNG_REPLAY: replay_normals is n x 3, particle-major (xi_0, xi_1, xi_2 of slot 0, then slot 1, ...); NULL
 *     is MCL_ERR_INVALID unless every std the call uses is zero (enable / reset: init_std, advance: walk_std).
 *     MCL_RNG_NATIVE: one Philox4x32-10 block, counter (global id, 0, step, purpose 7), key = the seed;  (xi_0, xi_1) =
 *     box_muller(o.x, o.y), (xi_2, unused) = box_muller(o.z, o.w) -- components 0, 1, 2 of the six normals every other
 *     draw of the library makes from its first block.  step 0 is the prior, step k the k-th advance since enable / reset.
 *     A pair whose stds are both zero is not evaluated (its xi are 0).  replay_normals is ignored.
 *   Resample.   While the drift is enabled every resample (mcl_resample with any scheme, mcl_step_mbes,
 *     mcl_step_mbes_landmarks) is followed by one launch behind its gather:  d'[i] = d[A(i)], A the slot map of
 *     mcl_history.h.  In place: a lost slot's ancestor is a surviving slot and a surviving slot is never written, so only
 *     the lost slots store.  Drift and history may be enabled together.
 *   Mean and covariance.   Over the n slots, every slot counting once (pending log-weights are ignored, as in
 *     mcl_pose_modes and mcl_history_smooth: read it after a resample).  With s = the drift of slot 0 and e = d - s:
 *     mean_c = sum e_c / n + s_c;  cov_ab = sum e_a e_b / n - (sum e_a / n)(sum e_b / n).  The sums are one fixed reduction
 *     tree (no floating-point atomics): two calls on the same state agree bit for bit.
 *
 * The drift is NOT touched by mcl_init_particles, mcl_init_particles_uniform, mcl_set_particles or mcl_inject_uniform: a
 * caller who re-initialises the filter calls mcl_drift_reset; an injected particle inherits its slot's drift as it
 * inherits its slot's history.
 *
 * Status codes: MCL_ERR_INVALID for a null handle or argument; MCL_ERR_STATE while the drift is not enabled, for every
 * call but mcl_drift_enable, mcl_drift_bytes and mcl_drift_config_check.
 *
 * Out of scope: sharded clouds (mcl_group_*, communicators), drift terms in the body frame, a DVL scale factor, a fresh
 * drift for injected particles.
 */
#ifndef MCL_DRIFT_H
#define MCL_DRIFT_H
#include "mcl.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcl_drift_config {
  double init_std[3]; /* cx, cy [m/s], bw [rad/s]: the prior, zero mean */
  double walk_std[3]; /* random walk, per sqrt(second) */
} mcl_drift_config;   /* 48 bytes */

/* ---- pure host arithmetic: no handle, no device */
/* *bytes = the device memory mcl_drift_enable allocates on a handle of n particles = 24 n (the state) + 147552 (9 x 2048
 * reduction records and 12 result words of 8 bytes).  (REPLAY draws pass through the handle's replay buffer, which the
 * predict shares.)  MCL_ERR_INVALID: n < 1 or n > 2^31 - 1, null bytes. */
int mcl_drift_bytes(int64_t n, int64_t* bytes);
/* MCL_OK, or MCL_ERR_INVALID with *reason (may be NULL) = a static string naming the first std that is negative, NaN or
 * infinite ("init_std[1] ...", "walk_std[2] ...") or "null config". */
int mcl_drift_config_check(const mcl_drift_config* cfg, const char** reason);

/* Allocate the state and draw the prior.  MCL_ERR_INVALID: a std mcl_drift_config_check refuses; REPLAY mode, a non-zero
 * init_std and no normals.  MCL_ERR_STATE: already enabled (disable first).  MCL_ERR_UNSUPPORTED: a handle
 * mcl_history_enable refuses (world > 1, comm_mode != MCL_COMM_NONE or a communicator).  MCL_ERR_ALLOC: the memory is not
 * there; the drift is then disabled. */
int mcl_drift_enable(mcl_handle* h, const mcl_drift_config* cfg, const double* replay_normals);
/* Redraw the prior (the bits mcl_drift_enable drew: step 0) and zero the advance counter. */
int mcl_drift_reset(mcl_handle* h, const double* replay_normals);
/* Free the buffers; every later call queues exactly the launches a handle that never enabled the drift queues.  One
 * stream synchronisation. */
int mcl_drift_disable(mcl_handle* h);

/* See above.  Asynchronous on the handle's stream; timed under MCL_K_PREDICT.  MCL_ERR_INVALID: dt NaN or infinite;
 * REPLAY mode, dt > 0, a non-zero walk_std and no normals. */
int mcl_drift_advance(mcl_handle* h, double dt, const double* replay_normals);

/* The state, soa3n = cx[n], cy[n], bw[n] (checkpoints, tests).  One synchronisation each. */
int mcl_drift_get(mcl_handle* h, double* soa3n);
int mcl_drift_set(mcl_handle* h, const double* soa3n);

/* mean3 = mean of cx, cy, bw; cov6 = xx xy xw yy yw ww, divided by n (either may be NULL).  Timed under MCL_K_MEAN_COV.
 * One synchronisation. */
int mcl_drift_mean_cov(mcl_handle* h, double mean3[3], double cov6[6]);

#ifdef __cplusplus
}
#endif
#endif /* MCL_DRIFT_H */
