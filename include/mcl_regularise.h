/* mcl_regularise.h -- regularised resampling: after a resample, jitter every particle with h^2 times the cloud's OWN sample
 * covariance (the regularised particle filter; with shrink, the Liu-West form that keeps the first two moments), on top of
 * the C ABI in mcl.h (same library, same handle, same conventions; MCL_ABI_VERSION stays 4: nothing declared in mcl.h
 * changes, MCL_K_COUNT, mcl_timing and mcl_config are what they were).
 *
 * Every resample ends by adding resampling_noise_covariance, a fixed diagonal covariance typed into a launch file: too
 * wide while the filter tracks, too narrow after a kidnap, blind to the x / y / yaw correlations along the track, and it
 * never touches the drift states of mcl_drift.h.  mcl_regularise, called right after a resample, measures the cloud and
 * jitters pose and drift jointly, with the kernel-density bandwidth for n particles in D dimensions: no knob but a scale.
 * Three small launches behind the resample, no host round trip.  A handle that never calls it queues exactly the launches
 * it always queued.
 *
 * Definition.
 *   Dimensions.  dims = 3: v = (x, y, yaw).  dims = 6: v = (x, y, yaw, cx, cy, bw), the drift of mcl_drift.h, which must
 *     be enabled (MCL_ERR_STATE otherwise).  D = dims below.  z, roll, pitch, the log-weights, the slot order and the
 *     genealogy are neither read for writing nor written.  Every matrix is packed lower-triangular, row by row:
 *     (0,0), (1,0), (1,1), (2,0), ... : 6 words for dims = 3, 21 for dims = 6.
 *   Moments.  Every slot counts once (pending log-weights are ignored, as in mcl_drift_mean_cov: the call belongs after a
 *     resample).  The shift s = the values of slot 0.  e_r(i) = v_r(i) - s_r;  for yaw, t = yaw_i - s_yaw and e = t if
 *     -pi <= t < pi, else wrap_pi(t) = (t + pi) mod 2 pi - pi, floored modulo.  S_r = sum_i e_r,  P_rc = sum_i e_r e_c for
 *     r >= c:  D + D (D + 1) / 2 = 9 or 27 sums, each one fixed reduction tree (the tree of mcl_drift_mean_cov; no
 *     floating-point atomics): two calls on the same state agree bit for bit.  m_r = S_r / n,  C_rc = P_rc / n - m_r m_c.
 *   Factor (mcl_regularise_factor: the device runs the same function).  Every product, sum, quotient and root is one IEEE
 *     double operation, not fused.  For j = 0 .. D - 1:
 *       p = C_jj - sum_{k<j} L_jk^2, k increasing.
 *       If p > C_jj 2^-26:  L_jj = sqrt(p) and, for i > j, L_ij = (C_ij - sum_{k<j} L_ik L_jk) / L_jj, k increasing.
 *       Otherwise column j of L is zero and bit j of `dead` is set.  (The comparison is false for NaN and for C_jj <= 0.)
 *     The threshold is part of the definition: a dimension whose residual variance is below 2^-26 of its own variance
 *     would be jittered by less than 1.3e-4 of its sigma, which is not worth a root of rounding noise.  A constant
 *     dimension has e = 0 exactly, hence a zero row and column of C and of L exactly.
 *   Bandwidth (mcl_regularise_bandwidth; host).  h0 = scale (4 / ((D + 2) n))^(1 / (D + 4)).
 *     shrink = 0: h = h0, a = 1.     shrink = 1: h = min(h0, 1), a = sqrt(1 - h h).
 *   Apply.  Per slot, with xi_0 .. xi_{D-1} its standard normals, every product and sum one IEEE double operation:
 *     z_r = sum_{c<=r} L_rc xi_c, c increasing, starting from the first product.
 *     A dimension whose row of L is entirely zero is neither loaded nor stored.
 *     shrink = 0:  v = cur_r + h z_r.
 *     shrink = 1:  with e_r as in the moments:  t1 = e_r - m_r;  t2 = a t1;  t3 = m_r + t2;  t4 = s_r + t3;  t5 = h z_r;
 *                  v = t4 + t5.
 *     Yaw is stored as v if -pi <= v < pi, else wrap_pi(v) (the rule of mcl_drift_advance).
 *     With shrink = 1 the cloud's mean and covariance are what they were, up to the sampling error of the jitter; with
 *     shrink = 0 the covariance grows by the factor 1 + h^2.
 *   Draws.  MCL_RNG_REPLAY: replay_normals is n x dims, particle-major; NULL is MCL_ERR_INVALID.
 *     MCL_RNG_NATIVE: Philox4x32-10, counter (global id, block, step, purpose 8), key = the seed; step = the number of
 *     earlier mcl_regularise calls on the handle; the six normals are laid out as every other draw of the library lays
 *     them out: (xi_0, xi_1) = box_muller(o.x, o.y), (xi_2, xi_3) = box_muller(o.z, o.w) of block 0, (xi_4, xi_5) =
 *     box_muller(o.x, o.y) of block 1.  dims = 3 evaluates block 0 only and uses xi_0 .. xi_2.  replay_normals is ignored.
 *
 * Status codes: MCL_ERR_INVALID for a null handle or argument, a scale that is not finite or <= 0, dims not 3 or 6;
 * MCL_ERR_STATE for dims = 6 without the drift enabled, and for mcl_regularise_last before any mcl_regularise;
 * MCL_ERR_UNSUPPORTED on a handle mcl_history_enable refuses (world > 1, comm_mode != MCL_COMM_NONE or a communicator).
 *
 * Out of scope: sharded clouds, jittering only the copied slots, z / roll / pitch.
 */
#ifndef MCL_REGULARISE_H
#define MCL_REGULARISE_H
#include "mcl.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcl_regularise_config {
  double scale;   /* multiplies the kernel-density bandwidth; 1 is the textbook value */
  int32_t shrink; /* 0: plain jitter; otherwise: shrink towards the mean first (Liu-West) */
  int32_t dims;   /* 3: x, y, yaw;  6: and cx, cy, bw */
} mcl_regularise_config; /* 16 bytes */

typedef struct mcl_regularise_result {
  int64_t n;
  int32_t dims;
  int32_t dead;     /* bit j: column j of chol is zero */
  double h, a;      /* the bandwidth and the shrink factor the call used */
  double shift[6];  /* s: the values of slot 0 */
  double dmean[6];  /* m: the mean ABOUT the shift (the cloud's mean is shift + dmean; yaw: wrapped) */
  double cov[21];   /* C, packed */
  double chol[21];  /* L, packed */
} mcl_regularise_result; /* 464 bytes; words past dims (6 or 21 packed) are zero */

/* ---- pure host arithmetic: no handle, no device */
/* MCL_OK, or MCL_ERR_INVALID with *reason (may be NULL) = a static string: "null config", "scale must be finite and > 0"
 * or "dims must be 3 (x, y, yaw) or 6 (x, y, yaw, cx, cy, bw)". */
int mcl_regularise_config_check(const mcl_regularise_config* cfg, const char** reason);
/* h and a of the definition.  MCL_ERR_INVALID: n < 1, dims not 3 or 6, scale not finite or <= 0, a null pointer. */
int mcl_regularise_bandwidth(int64_t n, int32_t dims, double scale, int32_t shrink, double* h, double* a);
/* The factor of the definition: cov_packed and chol_packed hold dims (dims + 1) / 2 words.  MCL_ERR_INVALID: dims not 3
 * or 6, a null pointer. */
int mcl_regularise_factor(const double* cov_packed, int32_t dims, double* chol_packed, int32_t* dead);

/* Moments, factor, apply: asynchronous on the handle's stream (NATIVE mode: no synchronisation).  The moments and the
 * factor are timed under MCL_K_MEAN_COV, the apply under MCL_K_NOISE.  The buffers (27 x 2048 reduction records, one
 * result record) are reserved at the first call. */
int mcl_regularise(mcl_handle* h, const mcl_regularise_config* cfg, const double* replay_normals);
/* What the last mcl_regularise measured and used (the record it left on the device).  One synchronisation. */
int mcl_regularise_last(mcl_handle* h, mcl_regularise_result* result);

#ifdef __cplusplus
}
#endif
#endif /* MCL_REGULARISE_H */
