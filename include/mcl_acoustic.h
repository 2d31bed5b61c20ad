/* mcl_acoustic.h -- absolute position measurements that arrive LATE: acoustic (USBL / underwater GPS) position fixes and
 * long-baseline slant ranges to fixed transponders, on top of the C ABI in mcl.h and of the genealogy in mcl_history.h
 * (same library, same handle, same conventions; MCL_ABI_VERSION stays 4: nothing declared in mcl.h changes).
 *
 * An acoustic fix is old when it arrives: travel time, the topside solver and the modem link add up to seconds, which at
 * cruising speed is many sigmas along track.  Weighting today's particles against where the vehicle WAS biases the filter
 * backwards.  The correct update weights each particle by the likelihood of the pose its own ANCESTOR had when the
 * measurement was taken -- and the ancestor links and the ring of recorded frames of mcl_history.h hold exactly that, on
 * the device.  A GPS fix taken at the surface just before a dive and delivered late is the same case.
 *
 * Definition.  (A restatement in any language gives the same numbers up to the rounding of its fp64 sums.)
 *   Pose the measurement is evaluated at, per current slot i:
 *     lag = -1     the particle's own x, y, yaw as they are now.
 *     lag = k >= 0 with a_k(i) as in mcl_history.h and P_k the frame at lag k (0: the newest): x, y, yaw = P_k[a_k(i)].
 *     0 < frac < 1 the pose moves that fraction of the way towards the next older frame along the same lineage:
 *                  a_{k+1} = parent_k[a_k];  x = x_k + frac (x_{k+1} - x_k), y likewise;
 *                  yaw = yaw_k + frac wrap(yaw_{k+1} - yaw_k),  wrap(d) = d - 2 pi ceil((d - pi) / (2 pi)) in (-pi, pi].
 *                  frac = 0 reads one frame only.
 *   z, roll, pitch come from zrp: the same three numbers for every particle (frames do not store them, and after a predict
 *     they are the odometry's on every particle anyway).  zrp == NULL is allowed with lag = -1 only and means each particle's
 *     own components.
 *   Transponder position in the map:
 *     p_i = m2o [x y z 1]' + Rm R(roll, pitch, yaw) offset,    R = Rz(yaw) Ry(pitch) Rx(roll), Rm = the rotation block of
 *     m2o, offset = the transponder in base_link (NULL: zero) -- the sensor origin of mcl_update_ranges without the sensor's
 *     own rotation.
 *   Fix:     d = xy_map - p_i(x, y);   lw_i (+)= -1/2 d' S^-1 d - 1/2 log((2 pi)^2 det S),   S = [xx xy; xy yy] = cov3.
 *   Ranges:  lw_i (+)= -1/2 sum_valid ((r_b - |p_i - b_b|) / sigma)^2 - n_valid log(sigma sqrt(2 pi));  a range <= 0 or NaN
 *            is skipped; with every range skipped the term is 0.
 *   accumulate: as in mcl_update_ranges -- 0: lw_i = term (the weights become log-likelihoods, MCL_WEIGHT_LOG_SHIFT),
 *            1: lw_i += term onto whatever update wrote the weights before (their mode is kept).
 *
 * Status codes.  MCL_ERR_INVALID: a null handle or required argument, a non-finite number, lag < -1, lag >= frames held,
 * frac outside [0, 1), frac > 0 with lag + 1 >= frames held or with lag = -1, zrp == NULL with lag >= 0, and what each call
 * says below.  MCL_ERR_STATE: lag >= 0 while history is not enabled; no particles yet; accumulate with no weights to add
 * to.  lag = -1 works on every handle, the shards of a sharded cloud included (the term is a function of the particle
 * alone); lag >= 0 needs history, which a sharded handle cannot enable.  After an error the handle is as it was.
 *
 * Both updates are one launch on the handle's stream, asynchronous, timed under MCL_K_UPDATE_GPS.  They read the state,
 * the link and the frames and write the log-weights only: particles, mcl_history_ancestors and mcl_history_frames give
 * the same answers before and after.
 */
#ifndef MCL_ACOUSTIC_H
#define MCL_ACOUSTIC_H
#include "mcl.h"
#include "mcl_history.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_ACOUSTIC_MAX_BEACONS 8

/* Position fix.  MCL_ERR_INVALID also unless xx > 0 and det S > 0. */
int mcl_update_fix(mcl_handle* h, const double xy_map[2], const double cov3[3] /* xx xy yy, map frame */,
                   const double offset[3] /* transponder in base_link, NULL = 0 */,
                   const double zrp[3] /* z (odom frame), roll, pitch of the vehicle when measured */,
                   int32_t lag, double frac, int32_t accumulate);

/* Slant ranges to fixed transponders.  MCL_ERR_INVALID also for n_b outside 1 ... MCL_ACOUSTIC_MAX_BEACONS, sigma <= 0, a
 * non-finite beacon coordinate or an infinite range (NaN marks a skipped one). */
int mcl_update_beacon_ranges(mcl_handle* h, const double* beacons_xyz /* n_b x 3, map frame */,
                             const double* ranges /* n_b; <= 0 or NaN = skipped */, int32_t n_b /* 1..8 */,
                             double sigma, const double offset[3], const double zrp[3],
                             int32_t lag, double frac, int32_t accumulate);

/* Where a measurement's stamp falls among the stamps mcl_history_frames returns (newest first, strictly decreasing).
 * Pure host arithmetic: no handle, no device.
 *   s_k >= stamp > s_{k+1}:   *lag = k, *frac = (s_k - stamp) / (s_k - s_{k+1}) in [0, 1), *where = 0
 *   stamp >= s_0:             *lag = 0, *frac = 0, *where = +1   (not older than the newest frame)
 *   stamp <= s_{held-1}:      *lag = held - 1, *frac = 0, *where = -1   (not newer than the oldest; the caller decides
 *                             whether to drop the measurement)
 * The first rule that holds, in the order +1, -1, 0.  MCL_ERR_INVALID: held < 1, a null pointer, a non-finite stamp,
 * stamps that are not strictly decreasing. */
int mcl_history_bracket(const double* stamps_newest_first, int32_t held, double stamp,
                        int32_t* lag, double* frac, int32_t* where);

#ifdef __cplusplus
}
#endif
#endif /* MCL_ACOUSTIC_H */
