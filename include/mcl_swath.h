/* mcl_swath.h -- swath matching: the Levenberg-Marquardt pose fix of the last K pings on the map as ONE rigid set, on top
 * of mcl_match.h (same library, same handle, same conventions; MCL_ABI_VERSION stays 4 and MCL_K_COUNT 15: nothing declared
 * in an existing header changes, and no weight, no particle and no existing kernel's output does).
 *
 * One MBES ping is a line across the track: what it says about the along-track position is confounded with depth, and
 * mcl_match_ping can end CONVERGED at zero residual a metre off along the track.  K pings that dead reckoning ties rigidly
 * to each other have no such valley, and a yaw error moves the far pings sideways by their lever arm.
 *
 * Definition.
 *   THE SWATH.  K pings, 1 <= K <= MCL_SWATH_MAX_PINGS, that share one table of B beam angles, 1 <= B <= 2048; `ranges` is
 *   K x B, row-major (ping k's beam b at [k B + b]); a beam counts when r > 0, as everywhere; K B <= MCL_SWATH_MAX_BEAMS.
 *
 *   THE OFFSETS.  Ping k carries mcl_swath_offset (dx, dy, dz, roll, pitch, dyaw): dx, dy the position of the vehicle at
 *   ping k relative to the anchor, in the frame turned by the ANCHOR's yaw about the stored z axis; dz added to the
 *   anchor's z; roll, pitch the vehicle's own values at ping k (absolute, not relative); dyaw added to the anchor's yaw.
 *   The anchor is whatever the caller makes it (the node: the newest ping, whose offset is (0, 0, 0, roll, pitch, 0)); no
 *   ping has to be the anchor.  The order of the pings has no meaning: the record below is a sum of integers.
 *
 *   ONE EVALUATION of an anchor pose (x, y, z, yaw).  The 1 + 2 D variants of mcl_match.h are taken ON THE ANCHOR, each
 *   one fp64 addition on the stored number: (x_v, y_v, z_v, yaw_v).  For variant v and ping k, every operation one IEEE
 *   double operation of its own (no contraction):
 *       (s, c) = sincos(yaw_v)
 *       x_k = x_v + (c dx_k - s dy_k)      y_k = y_v + (s dx_k + c dy_k)      z_k = z_v + dz_k      yaw_k = yaw_v + dyaw_k
 *   yaw_k is not wrapped: it only enters a sincos.  Roll and pitch are the offset's.  A coordinate whose offset is exactly
 *   zero keeps the variant's bits: dx_k == 0 and dy_k == 0: nothing is added to x_v and y_v (and no sincos enters);
 *   dz_k == 0: nothing to z_v; dyaw_k == 0: nothing to yaw_v.  Then the unchanged cast arithmetic of mcl_match.h from the
 *   pose (x_k, y_k, z_k, roll_k, pitch_k, yaw_k).  Perturbing the anchor's yaw therefore swings the whole swath about the
 *   anchor.  MISS, JUMP, d_k and rho are those of mcl_match.h per (ping, beam); the record is the same mcl_match_sums,
 *   summed over all K B beams.  So K = 1 with the offset (0, 0, 0, roll, pitch, 0) is mcl_match_ping bit for bit.
 *   The compositions use the device's sincos: they are not restated bit for bit on the host (the last bit of a sincos
 *   moves a ray's origin by less than 1e-12 m).  The INTEGERS are defined over the ranges the device cast, as for
 *   mcl_match_ping; mcl_match_swath's ranges_out hands those out.
 *
 *   Bounds.  n <= 2^14 beams, |d| <= 2^23 in a contributing pair, |rho| <= 2^24:  |S| <= 2^14 2^46 = 2^60,
 *   |C| <= 2^14 2^47 = 2^61, s_rho2 <= 2^14 2^48 = 2^62, |s_rho| <= 2^38 -- every sum stays below 2^63.  The products of
 *   BETTER are below 2^62 2^14 = 2^76 and are compared as 128-bit integers.  The dead test's m grad_floor_q^2 is below 2^38.
 *
 *   BETTER, SOLVE, THE LOOP, the statuses and Derived are those of mcl_match.h word for word, with m the number of
 *   contributing beams of the whole swath; min_beams applies to it.  The loop moves the anchor.  The start poses' roll and
 *   pitch (rows 3 and 4 of `poses`) are not read, but must be finite.
 *
 * Launches take no timing slot.  Out of scope: feeding the fix back into the filter; a prior term; fitting roll and pitch;
 * per-ping beam tables; sharded handles beyond what mcl_pose_information accepts; the fused steps.
 */
#ifndef MCL_SWATH_H
#define MCL_SWATH_H
#include "mcl_match.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_SWATH_MAX_PINGS 64
#define MCL_SWATH_MAX_BEAMS 16384   /* K B */

typedef struct mcl_swath_offset {
  double dx, dy;        /* metres, in the frame turned by the anchor's yaw */
  double dz;            /* metres, added to the anchor's z */
  double roll, pitch;   /* radians, the vehicle's own at this ping */
  double dyaw;          /* radians, added to the anchor's yaw */
} mcl_swath_offset;

/* ---- device-free */
/* The offsets of the vehicle's poses at the K pings (poses6: 6 x K doubles SoA, x[K], y[K], z[K], roll[K], pitch[K], yaw[K],
 * in the coordinates the particle state is stored in -- dead reckoning will do: only differences enter) relative to column
 * `anchor` (0 ... K - 1; -1: the last).  With (s, c) = sincos(yaw_a), u = x_k - x_a, w = y_k - y_a, every operation on its
 * own:  dx = c u + s w,  dy = c w - s u,  dz = z_k - z_a,  dyaw = yaw_k - yaw_a wrapped by the library's rule (kept when
 * -pi <= t < pi, else ((t + pi) mod 2 pi) - pi with the floored modulo);  roll, pitch copied.  The anchor's own row is exact
 * zeros plus its roll and pitch.  MCL_ERR_INVALID: a null pointer, K outside 1 ... 64, anchor outside -1 ... K - 1, a pose
 * that is not finite. */
int mcl_swath_offsets(const double* poses6, int32_t K, int32_t anchor, mcl_swath_offset* out);
/* MCL_OK, or MCL_ERR_INVALID with *reason (or NULL) the rule that is broken: K outside 1 ... 64, B outside 1 ... 2048,
 * K B above 16384, a null table, an offset that is not finite. */
int mcl_swath_check(int32_t K, int32_t B, const mcl_swath_offset* offsets, const char** reason);
/* mcl_match_solve, mcl_match_better and mcl_match_derived (the same arithmetic: one statement of each rule) for the record of
 * a swath: n <= 16384 and the bounds above, where the mcl_match_* functions keep refusing n > 2048. */
int mcl_swath_solve(const mcl_match_sums* rec, const mcl_match_config* cfg, int32_t j, double delta_out[4], int32_t* dead_out);
int mcl_swath_better(const mcl_match_sums* q, const mcl_match_sums* p, int32_t min_beams, int32_t* better);
int mcl_swath_derived(const mcl_match_sums* rec, const mcl_match_config* cfg, double sigma, mcl_match_derived_t* out);

/* ---- one handle.  poses: the anchor's start poses, host SoA 6 x M doubles as for mcl_match_ping, 1 <= M <= 65536; ranges:
 * K x B; offsets: K.  Needs a map, no particles; never reads or writes the cloud, the weights, the counters or the caches.
 * One synchronisation, at the end (an upload above 1 MiB waits for itself first).  results_out: M records, x, y, yaw, z the
 * ANCHOR's.  trace_out (or NULL): M x (max_iter + 1) records as for mcl_match_ping.  ranges_out (or NULL): M x (max_iter + 1)
 * x K x (1 + 2 D) x B floats, [(((i T + t) K + k) NV + v) B + b] with T = max_iter + 1 and NV = 1 + 2 D; entries of
 * evaluations that did not run and of beams that do not count are NaN.  Production passes NULL for both.  The scratch block
 * is mcl_match_ping's and so is its rule: a block above 64 MiB is released before the call returns.
 * MCL_ERR_INVALID: what mcl_match_ping refuses (its B, M, sigma, r_max, config, angles and poses), what mcl_swath_check
 * refuses, a ranges_out of more than 2^26 floats.  MCL_ERR_STATE: no map. */
int mcl_match_swath(mcl_handle* h, const double* poses, int64_t M, const float* ranges, const float* beam_angles, int32_t B,
                    const mcl_swath_offset* offsets, int32_t K, double sigma, double r_max, const double sensor_offset[6],
                    const mcl_match_config* cfg, mcl_match_result* results_out, mcl_match_trace* trace_out, float* ranges_out);

#ifdef __cplusplus
}
#endif
#endif /* MCL_SWATH_H */
