/* mcl_modes.h -- the dominant modes of the particle cloud, on top of the C ABI in mcl.h (same library, same handle, same
 * conventions; MCL_ABI_VERSION stays 4: nothing declared in mcl.h changes).
 *
 * mcl_mean_cov is the reference's loc_loop: the arithmetic mean over ALL particles, yaw as the plain mean of wrapped
 * angles.  A cloud that holds several hypotheses on purpose (mcl_init_particles_uniform, mcl_inject_uniform:
 * mcl_recovery.h) has a mean that lies between them and on none.  mcl_pose_modes answers the other question: on a
 * caller-given lattice of cells over (x, y, yaw), where are the up to k_max densest places of the cloud, and what are
 * the particle count, the mean pose and the covariance of each?  Like mcl_mean_cov it counts every particle once and
 * ignores pending log-weights; it reads the handle and never writes it: every call made after it gives the bits it
 * gives without it.
 *
 * Definition.  Everything that decides the result is integer arithmetic on cell indices, and the cell of a particle is
 * formed by IEEE double operations each rounded on its own (no reciprocal, no fma): a restatement in any language gives
 * the same integers.
 *   Cell of a particle.   ix = floor((x - x0) / cell),  iy = floor((y - y0) / cell);  inside iff 0 <= ix < nx and
 *     0 <= iy < ny.  iyaw = floor((yaw + pi) / ((2 pi) / n_yaw)) reduced into [0, n_yaw) by the floored modulo: the
 *     state's yaw leaves [-pi, pi) with the resample noise, any yaw with a finite quotient is binned.  A particle whose x,
 *     y or yaw is not finite (or whose yaw quotient overflows), or whose x or y lies outside the box, belongs to no cell
 *     and is counted in n_outside.
 *   Histogram.   H[c] = number of particles in cell c, c = (iyaw * ny + iy) * nx + ix.
 *   Score.   S[c] = sum of H over the window of c: the cells with |dix| <= 1 and |diy| <= 1 that lie inside the box, in
 *     the yaw bins at circular distance <= 1 taken as a SET (n_yaw = 1 or 2: no bin is counted twice).
 *   Modes.   Greedy: mode m is the cell with the largest score among the cells not suppressed, the lowest c on ties;
 *     it suppresses every cell at Chebyshev distance <= 2 from it in (ix, iy, circular iyaw), so the windows of two
 *     modes are disjoint and a particle belongs to at most one mode.  Selection stops after k_max modes or when the best
 *     remaining score is 0; *n_modes is the number found (0 is a valid answer).
 *   Moments of a mode, over the particles whose cell lies in its window:  count (exact);
 *     mean x = cx + sum(x - cx) / count with cx = x0 + (ix + 0.5) cell, mean y likewise; z, roll, pitch: plain means;
 *     yaw = atan2(sum sin yaw, sum cos yaw);  yaw_R = hypot(sum sin, sum cos) / count;
 *     cov_xy = {sum dx^2, sum dx dy, sum dy^2} / count about (cx, cy), minus the products of the means of dx and dy.
 *   The sums are a fixed reduction tree (no floating-point atomics): two calls on the same state agree bit for bit.
 */
#ifndef MCL_MODES_H
#define MCL_MODES_H
#include "mcl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_MODES_MAX 8             /* largest k_max */
#define MCL_MODES_MAX_YAW 64        /* largest n_yaw */
#define MCL_MODES_MAX_CELLS (1 << 24) /* largest nx * ny * n_yaw */

/* the lattice, in the frame of the particle state (ODOM): cells of `cell` metres from (x0, y0), n_yaw bins of the circle */
typedef struct mcl_mode_grid {
  double x0, y0, cell;
  int32_t nx, ny, n_yaw, reserved;
} mcl_mode_grid; /* 40 bytes */

typedef struct mcl_mode {
  int64_t count;       /* particles inside the mode's window */
  int64_t score;       /* the peak cell's score S */
  int32_t ix, iy, iyaw, reserved; /* the peak cell */
  double mean6[6];     /* x, y, z, roll, pitch, yaw; yaw = circular mean */
  double cov_xy[3];    /* xx, xy, yy about the mean, divided by count */
  double yaw_R;        /* mean resultant length of the yaws, in [0, 1] */
} mcl_mode;            /* 112 bytes */

/* Pure host arithmetic (no device, no handle): MCL_OK and *n_cells = nx * ny * n_yaw (n_cells may be NULL), or
 * MCL_ERR_INVALID: a null grid; cell not finite or <= 0; x0 or y0 not finite; nx, ny or n_yaw < 1; n_yaw > 64;
 * nx * ny * n_yaw > 2^24. */
int mcl_mode_grid_check(const mcl_mode_grid* g, int64_t* n_cells);

/* The up to k_max (1 ... 8) modes of the cloud on the lattice g, densest first, into modes[0 .. *n_modes); n_outside
 * (optional): the particles that belong to no cell.  MCL_ERR_INVALID: a null handle, grid, modes or n_modes, k_max
 * outside 1 ... 8, a grid mcl_mode_grid_check refuses.  MCL_ERR_UNSUPPORTED: a handle of a sharded cloud (world > 1).
 * MCL_ERR_STATE: no particles yet (before mcl_init_particles / mcl_init_particles_uniform / mcl_set_particles).
 * Timed under MCL_K_MEAN_COV.  One stream synchronisation. */
int mcl_pose_modes(mcl_handle* h, const mcl_mode_grid* g, int32_t k_max, mcl_mode* modes, int32_t* n_modes,
                   int64_t* n_outside);

#ifdef __cplusplus
}
#endif
#endif /* MCL_MODES_H */
