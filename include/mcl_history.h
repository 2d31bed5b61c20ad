/* mcl_history.h -- the genealogy of the particles: ancestor links across resamples and a fixed-lag smoothed track, on top
 * of the C ABI in mcl.h (same library, same handle, same conventions; MCL_ABI_VERSION stays 4: nothing declared in mcl.h
 * changes).
 *
 * Every other estimate of the library is about NOW (mcl_mean_cov, mcl_pose_modes, mcl_weight_stats); mcl_mean_history
 * keeps filtered means, which later pings never correct.  A particle filter holds a better record of the past: trace
 * each of today's particles back through the resamples.  The cloud of their ancestors at an earlier ping is the posterior
 * of that ping's pose given everything measured since (the fixed-lag particle smoother); the ancestors of the best
 * particle are the MAP trajectory; and the number of DISTINCT ancestors left at lag k measures path degeneracy -- "too few
 * particles / too much resampling" --, beside the n_eff of mcl_weight_stats.  While history is enabled the library keeps,
 * on the device, the link every resample computes anyway; it is off by default and costs nothing then.
 *
 * Definition.  All links are integers: a restatement in any language gives the same integers.
 *   Slot map of a resample.   With idx the ancestor vector mcl_get_last_indices returns:  A(i) = i if slot i survived
 *     (the value i occurs in idx), else A(i) = dupes[rank of i among the lost slots, ascending], dupes = idx with the first
 *     occurrence of each distinct value removed, order preserved.  Slot i of the new state holds the pre-resample state of
 *     slot A(i) (plus resampling noise).  Defined for all five schemes.
 *   Link.   n x u32; link[i] = the slot of the NEWEST recorded frame that current slot i descends from.  The identity
 *     after mcl_history_enable, mcl_history_reset and every mcl_history_record.  While history is enabled every resample
 *     (mcl_resample, mcl_step_mbes, mcl_step_mbes_landmarks) composes link'(i) = link(A(i)): one extra launch queued
 *     behind the gather on the handle's stream.  Predicts and updates do not touch it.  Zero, one or several resamples
 *     may lie between two records.
 *   Frame.   mcl_history_record(h, stamp) appends a frame and resets link to the identity.  A frame holds parent = link
 *     (n x u32: slots of the PREVIOUS frame; the first frame after enable or reset holds the identity), the bits of x, y
 *     and yaw of every slot as they are at the call (3 x n x fp64) and the caller's stamp: 28 B per particle.  z, roll
 *     and pitch are not stored: after a predict they are the odometry's on every particle and the caller has them.
 *     Frames live in a ring of `depth` frames; the oldest is overwritten.
 *   Ancestors at lag k (k = 0: the newest frame F).   a_0(i) = link(i);  a_{j+1}(i) = parent_{F-j}[a_j(i)].  Valid for
 *     k < frames held.
 *   Smoothed estimate at lag k.   c_k[s] = #{i : a_k(i) = s} (exact, u32);  n_unique = #{s : c_k[s] > 0};
 *     mean x = sum c (x - x_shift) / n + x_shift with x_shift = the frame's slot-0 x, mean y likewise;
 *     yaw = atan2(sum c sin yaw, sum c cos yaw);  yaw_R = hypot(sum c sin, sum c cos) / n;
 *     cov_xy = {sum c dx^2, sum c dx dy, sum c dy^2} / n about the shift, minus the products of the means of dx and dy.
 *     Every CURRENT particle counts once and pending log-weights are ignored, as in mcl_mean_cov: call it after a
 *     resample.  The sums are a fixed reduction tree (no floating-point atomics): two calls on the same state agree bit
 *     for bit.
 *
 * The state is overwritten, not resampled, by mcl_init_particles, mcl_init_particles_uniform and mcl_set_particles: they
 * clear the frames and reset the link (history stays enabled).  mcl_inject_uniform leaves the lineage as it is -- a
 * replaced particle inherits its slot's past; a caller who wants a clean cut calls mcl_history_reset.
 *
 * Status codes of every call below: MCL_ERR_INVALID for a null handle or argument; MCL_ERR_STATE when history is not
 * enabled (all but enable / disable / bytes).  The queries (frames, ancestors, smooth, path) never write filter state:
 * every call made after them gives the bits it gives without them.
 */
#ifndef MCL_HISTORY_H
#define MCL_HISTORY_H
#include "mcl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_HISTORY_MAX_DEPTH 1024 /* largest ring depth */

typedef struct mcl_history_est {
  double stamp;      /* the frame's stamp */
  int64_t n_unique;  /* distinct ancestors the current particles have in this frame */
  double x, y, yaw;  /* smoothed mean; yaw = circular mean */
  double yaw_R;      /* mean resultant length of the yaws, in [0, 1] */
  double cov_xy[3];  /* xx, xy, yy about the mean, divided by n */
} mcl_history_est;   /* 72 bytes */

/* Pure host arithmetic (no device, no handle): *bytes = the device memory mcl_history_enable(h, depth) allocates on a
 * handle of n particles = 28 n depth (frames) + 16 n (two link buffers, two count buffers) + 80 depth + 131072 (result
 * words, reduction records).  MCL_ERR_INVALID: n < 1 or n > 2^31 - 1 (no handle holds more), depth outside 1 ...
 * MCL_HISTORY_MAX_DEPTH, null bytes. */
int mcl_history_bytes(int64_t n, int32_t depth, int64_t* bytes);

/* Start keeping the genealogy in a ring of `depth` frames (1 ... MCL_HISTORY_MAX_DEPTH); no frames yet, link = identity.
 * On an enabled handle: the same as disable, then enable.  MCL_ERR_UNSUPPORTED: a handle of a sharded cloud (world > 1,
 * comm_mode != MCL_COMM_NONE or a communicator).  MCL_ERR_ALLOC: the memory is not there; history is then disabled. */
int mcl_history_enable(mcl_handle* h, int32_t depth);
/* Free the buffers; every later call queues exactly the launches a handle that never enabled history queues.  MCL_OK
 * when history is not enabled.  One stream synchronisation. */
int mcl_history_disable(mcl_handle* h);
/* Forget the frames (held = recorded = 0) and reset the link to the identity.  No launch. */
int mcl_history_reset(mcl_handle* h);

/* Append a frame (see above).  Asynchronous on the handle's stream.  MCL_ERR_STATE: no particles yet (before
 * mcl_init_particles / mcl_init_particles_uniform / mcl_set_particles).  Timed under MCL_K_RESAMPLE, like the compose. */
int mcl_history_record(mcl_handle* h, double stamp);

/* *held = frames in the ring (<= depth), *recorded = frames recorded since enable / reset / the last init (either may be
 * NULL); stamps (may be NULL): the `held` stamps, newest first.  Host bookkeeping: no synchronisation. */
int mcl_history_frames(mcl_handle* h, int32_t* held, int64_t* recorded, double* stamps);

/* slots[i] = a_lag(i) for the n current slots.  MCL_ERR_INVALID: lag < 0 or lag >= frames held.  One synchronisation. */
int mcl_history_ancestors(mcl_handle* h, int32_t lag, uint32_t* slots);

/* est[k] = the smoothed estimate at lag k, k = 0 ... lags - 1.  MCL_ERR_INVALID: lags < 1 or lags > frames held.  Walks the
 * frames backwards with the descendant counts c_k, not one pointer chase per particle.  Timed under MCL_K_MEAN_COV.  One
 * synchronisation. */
int mcl_history_smooth(mcl_handle* h, int32_t lags, mcl_history_est* est);

/* The trajectory of ONE current slot (0 <= slot < n; e.g. the best particle of mcl_weight_stats for the MAP path):
 * xyyaw[3 k ...] = x, y, yaw of a_k(slot) in the frame at lag k, slots[k] = a_k(slot) (slots may be NULL), k = 0 ...
 * lags - 1.  MCL_ERR_INVALID: slot outside the handle, lags < 1 or lags > frames held.  One synchronisation. */
int mcl_history_path(mcl_handle* h, int64_t slot, int32_t lags, double* xyyaw, uint32_t* slots);

#ifdef __cplusplus
}
#endif
#endif /* MCL_HISTORY_H */
