/* mcl_kld.h -- KLD-sampling across handles, on top of the C ABI in mcl.h (same library, same handle, same conventions;
 * MCL_ABI_VERSION stays 4 and MCL_K_COUNT 15: nothing declared in mcl.h or in another header changes).
 *
 * A handle's particle count is fixed by mcl_create.  KLD-sampling (Fox, "Adapting the sample size in particle filters
 * through KLD-sampling", IJRR 2003) sizes the cloud by the number k of cells of an (x, y, yaw) lattice that hold a
 * particle.  Here the cloud MOVES BETWEEN HANDLES of different sizes instead of changing a handle's own n:
 *   mcl_kld_bins        counts k on a caller-given lattice (reads the handle, never writes it);
 *   mcl_kld_bound       turns k into the particle count the bound asks for (no device, no handle);
 *   mcl_resample_into   draws dst's particle count from src's weighted cloud (src is left as it was).
 * A handle that never makes these calls queues exactly the launches it queued before.
 *
 * mcl_kld_bins.  The lattice struct and the cell rule are those of mcl_modes.h, word for word: ix = floor((x - x0) /
 *   cell), iy = floor((y - y0) / cell); inside iff 0 <= ix < nx and 0 <= iy < ny; iyaw = floor((yaw + pi) / ((2 pi) /
 *   n_yaw)) reduced into [0, n_yaw) by the floored modulo; every operation an IEEE double operation rounded on its own
 *   (no reciprocal, no fma).  A particle whose x, y or yaw is not finite (or whose yaw quotient overflows), or whose x or
 *   y lies outside the box, belongs to no cell and is counted in n_outside.  Only the limits differ: n_yaw <= 1024 and
 *   nx * ny * n_yaw <= MCL_KLD_MAX_CELLS = 2^27 -- the call keeps one BIT per cell (16 MiB at the limit), where
 *   mcl_pose_modes keeps a count.  k = the number of distinct cells c = (iyaw * ny + iy) * nx + ix that hold at least one
 *   particle; n_inside + n_outside = n.  Like mcl_pose_modes it counts every particle once and ignores pending
 *   log-weights.  The result is an integer that does not depend on the order of anything.
 *
 * mcl_kld_bound.  The Wilson-Hilferty form of Fox's bound, in IEEE doubles, every operation rounded on its own (no
 *   contraction), in exactly this order:
 *     k <= 1: n_min.   Otherwise   a = 2.0 / (9.0 * (k - 1));   t = (1.0 - a) + sqrt(a) * z;
 *     v = ((((k - 1) / (2.0 * epsilon)) * t) * t) * t;   n = ceil(v) clamped into [n_min, n_max]; v not finite: n_max.
 *   z is the upper 1 - delta quantile of the standard normal, supplied by the caller (2.3263478740408408 for delta =
 *   0.01): no inverse normal CDF lives in the library.
 *
 * mcl_resample_into.  N = src's particle count, M = dst's.  q_j, C_j (inclusive sums) and T are the fixed-point weights
 *   mcl_resample on src would decide on (what mcl_get_fixed_weights returns after it: s = 63 - ceil(log2 N), src's weight
 *   mode, a NaN is a particle without weight, no finite value gives equal weights); src without pending weights: equal
 *   weights, q_j = 2^s.  U is a 53-bit uniform: uniform != NULL gives U = floor(u * 2^53); NULL gives the Philox draw of
 *   mcl_resample's own uniform with purpose 10 in place of 3, keyed by DST's seed, its step dst's transfer counter (+ 1
 *   per successful call, reset by mcl_init_particles / mcl_init_particles_uniform on dst).  The draw is the systematic
 *   scheme with M positions:
 *     idx_i = min{ j : (U + i 2^53) T < C_j M 2^53 },  i = 0 .. M - 1      (every comparison between exact integers)
 *   and dst.state[c][i] = src.state[c][idx_i] for all six components: bit copies, NO resampling noise.  With M = N and
 *   the same uniform the indices are those mcl_get_last_indices reports for mcl_resample on src.
 *   Afterwards dst has particles and no pending weights, an enabled history starts clean as after mcl_set_particles, and
 *   its Philox steps of predict, resample and injection keep counting.  Drift (mcl_drift.h) enabled on both handles:
 *   dst's drift states are src's at idx_i; enabled on exactly one: MCL_ERR_STATE.
 *   src: every getter of src and every later call on src returns the bits it would have returned without this call (the
 *   transfer's weights, CDF and indices live in buffers dst owns).
 *   Work queued on src's stream is seen; when the call returns dst may be used.  Each stream is synchronised once.
 */
#ifndef MCL_KLD_H
#define MCL_KLD_H
#include "mcl.h"
#include "mcl_modes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_KLD_MAX_YAW 1024          /* largest n_yaw */
#define MCL_KLD_MAX_CELLS (1 << 27)   /* largest nx * ny * n_yaw */

/* Pure host arithmetic: MCL_OK and *n_cells = nx * ny * n_yaw (n_cells may be NULL), or MCL_ERR_INVALID: a null grid;
 * cell not finite or <= 0; x0 or y0 not finite; nx, ny or n_yaw < 1; n_yaw > 1024; nx * ny * n_yaw > 2^27. */
int mcl_kld_grid_check(const mcl_mode_grid* g, int64_t* n_cells);

/* *k = occupied cells of the lattice g, *n_inside / *n_outside = particles with / without a cell (each output may be
 * NULL).  MCL_ERR_INVALID: a null handle or grid, a grid mcl_kld_grid_check refuses.  MCL_ERR_UNSUPPORTED: a handle of a
 * sharded cloud.  MCL_ERR_STATE: no particles yet.  Timed under MCL_K_MEAN_COV.  One stream synchronisation. */
int mcl_kld_bins(mcl_handle* h, const mcl_mode_grid* g, int64_t* k, int64_t* n_inside, int64_t* n_outside);

/* Pure host arithmetic: the particle count for k occupied cells.  MCL_ERR_INVALID: n null; k < 0; epsilon not finite or
 * <= 0; z not finite or < 0; not 1 <= n_min <= n_max <= 2^31. */
int mcl_kld_bound(int64_t k, double epsilon, double z, int64_t n_min, int64_t n_max, int64_t* n);

/* dst's particles := M draws from src's weighted cloud (see above).  uniform: one double in [0, 1), or NULL.
 * Errors, always with nothing touched -- MCL_ERR_INVALID: a null handle, src == dst, u outside [0, 1);
 * MCL_ERR_UNSUPPORTED: either handle sharded, handles on different devices; MCL_ERR_STATE: src without particles, drift
 * enabled on exactly one of the two.  Timed under MCL_K_RESAMPLE of dst. */
int mcl_resample_into(mcl_handle* src, mcl_handle* dst, const double* uniform);

/* idx[0 .. M): the ancestors (slots of src) of the last transfer into dst.  MCL_ERR_STATE before any transfer. */
int mcl_transfer_last_indices(mcl_handle* dst, int32_t* idx);

#ifdef __cplusplus
}
#endif
#endif /* MCL_KLD_H */
