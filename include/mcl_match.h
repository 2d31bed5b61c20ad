/* mcl_match.h -- ping matching: the Levenberg-Marquardt pose fix of one ping on the map, on top of the C ABI in mcl.h
 * (same library, same handle, same conventions; MCL_ABI_VERSION stays 4: nothing declared in mcl.h changes).
 *
 * mcl_innovation.h holds the residual rho_b = r_b - e_b of a ping against a pose, mcl_information.h the derivative g_b of the
 * expected ranges with respect to the pose, as quantised central differences.  The Gauss-Newton step of the Gaussian range
 * likelihood needs exactly those two: (sum_b g_b g_b^T) delta = sum_b g_b rho_b.  This header puts them together: from a
 * start pose, the pose the ping says the vehicle is at, with a covariance -- without a particle filter.  Nothing here
 * changes a weight or a particle.
 *
 * Definition.  A ping is (r_b, a_b), b < B, 1 <= B <= MCL_MATCH_MAX_BEAMS; a beam counts when r_b > 0 (zero, negative and NaN
 * mark a beam without a return, as everywhere).  Beam directions, sensor offset, r_max, the steps and the map are as for
 * mcl_ping_information.  D = dims is 3: the fix moves (x, y, yaw), or 4: (x, y, yaw, z); the dimensions k = 0 ... 3 are
 * x, y, yaw, z in that order everywhere below, with delta_0 = delta_1 = delta_3 = delta_xy and delta_2 = delta_yaw.
 *
 *   ONE EVALUATION of a pose p = (x, y, z, roll, pitch, yaw), in the coordinates the particle state is stored in.  Every
 *   counting beam is cast 1 + 2 D times, the variant index v = 0 ... 2 D:
 *       v = 0: p itself (the range e_0);  v = 1 ... 6: the six variants of mcl_information.h in its order (x + delta_xy,
 *       x - delta_xy, y + -, yaw + - delta_yaw);  D = 4:  v = 7: z + delta_xy,  v = 8: z - delta_xy
 *   -- each one fp64 addition or subtraction on the stored number, then the unchanged arithmetic of mcl_ping_innovation.
 *   If any of the 1 + 2 D ranges equals r_max the pair is a MISS.  Otherwise d_k = rint(((double)e_k+ - (double)e_k-) 2^12),
 *   the difference of mcl_information.h, k < D; if any |d_k| > floor(jump_max 2^12) the pair is a JUMP.  Otherwise the pair
 *   CONTRIBUTES with rho = the quantised residual of mcl_innovation.h of (r_b, e_0): rint(((double)r_b - (double)e_0) 2^12)
 *   clamped to +-2^24.
 *
 *   A record (mcl_match_sums), all integers: n beams cast, n_miss, n_jump, and over the contributing beams
 *       S[j (j + 1) / 2 + k] = sum d_j d_k, k <= j < D   (packed lower triangle: xx, yx, yy, wx, wy, ww, zx, zy, zw, zz)
 *       C[k] = sum d_k rho, k < D;   s_rho = sum rho;   s_rho2 = sum rho rho
 *   with the entries of dimensions >= D zero.  m = n - n_miss - n_jump is the number of contributing beams.
 *   Bound: jump_max <= 2048 m gives |d| <= 2^23 in a contributing pair, |rho| <= 2^24, and a ping has at most 2^11 beams:
 *   |S| <= 2^11 2^46 = 2^57, |C| <= 2^11 2^47 = 2^58, s_rho2 <= 2^11 2^48 = 2^59, |s_rho| <= 2^35 -- every sum stays
 *   below 2^63, and being a sum of integers has the same bits for every launch geometry and order of addition.
 *
 *   BETTER (mcl_match_better).  A pose with the record q is better than one with the record p, given min_beams, when
 *       m_q >= min_beams  and  s_rho2_q m_p < s_rho2_p m_q
 *   -- the mean square residual falls; the products are below 2^70 and are compared exactly, as 128-bit integers.
 *
 *   SOLVE (mcl_match_solve; device-free).  From a record, the config and the damping exponent j (-20 ... 22), the step
 *   delta[4] and the dead mask.  Every product, sum, quotient and root below is one IEEE double operation of its own (no
 *   contraction), an integer is converted to the nearest double, 2^j and 2^24 are exact:
 *     Dimension k < D is DEAD when S_kk <= m grad_floor_q^2 (integers): the ranges change by no more than grad_floor_q
 *     quanta rms across 2 delta_k -- their own rounding.  Dimensions >= D are dead.  Over the L live dimensions, in
 *     increasing order, compacted to 0 ... L - 1:
 *       A_jk = (double)S_jk / (((4.0 * delta_j) * delta_k) * 2^24),  k <= j      b_k = (double)C_k / ((2.0 * delta_k) * 2^24)
 *       A_kk <- A_kk + 2^j * A_kk
 *       the thresholded Cholesky factor of mcl_regularise.h (mcl_regularise_factor's rule) of the packed A; a column it
 *       kills is dead too, its step 0, and it takes no part in the substitutions
 *       forward:  y_i = (b_i - L_i0 y_0 - ... - L_i,i-1 y_i-1) / L_ii, the subtractions left to right, i increasing
 *       backward: t_i = (y_i - L_i+1,i t_i+1 - ... - L_L-1,i t_L-1) / L_ii, the subtractions in increasing row order, i decreasing
 *     One common scale s = 1, then in this order: h = sqrt(t_x t_x + t_y t_y), if h > step_max_xy: s = step_max_xy / h;
 *     if |t_z| s > step_max_xy: s = step_max_xy / |t_z|;  if |t_yaw| s > step_max_yaw: s = step_max_yaw / |t_yaw|;
 *     delta_k = t_k s when s < 1, else t_k.  A dead dimension gets delta_k = +0.0 exactly.  (h is written as a root of a sum
 *     of two products and not as hypot, whose last bit differs between mathematical libraries.)
 *
 *   THE LOOP, per start pose p_0; roll and pitch never change, z only for D = 4.
 *     1. Evaluate p_0 (evaluation 0).  If m < min_beams: status NO_OVERLAP, the pose is returned unchanged.
 *     2. p = p_0, j = MCL_MATCH_J0 = -10, trials = 0.  Repeat:
 *          if s_rho2 of p is 0:  CONVERGED.
 *          delta = SOLVE(record of p, j).  If every delta_k == 0:  CONVERGED.
 *          if trials == max_iter:  MAX_ITER.
 *          q = p + delta (one fp64 addition per coordinate whose delta_k is not 0; the others keep their bits), yaw wrapped
 *          by the library's rule: t = yaw + delta_yaw is kept when -pi <= t < pi, else ((t + pi) mod 2 pi) - pi with the
 *          floored modulo.  Evaluate q; trials += 1.
 *          if q is BETTER than p:  p = q, accepted += 1, j = max(j - 2, -20), and if sqrt(delta_x delta_x + delta_y delta_y) <
 *            tol_xy and |delta_z| < tol_xy and |delta_yaw| < tol_yaw:  CONVERGED.
 *          else:  j = j + 2, and if j > 20:  STALLED.
 *   So a pose costs at most 1 + max_iter evaluations.  An accepted pose never has a larger mean square residual than the
 *   one before it: the final rms residual is never above the start's.
 *
 *   Derived (mcl_match_derived; device-free, one IEEE operation at a time).  From a record, sigma and the config:
 *     rms = sqrt((double)s_rho2 / (double)m) / 4096   mean = ((double)s_rho / (double)m) / 4096   (metres; 0 when m = 0)
 *     chi2 = (rms / sigma) * (rms / sigma):  chi-square per contributing beam
 *     J, the D x D information without damping, packed as S:  A_jk / (sigma * sigma) over the live dimensions (live as in
 *     SOLVE), 0 in the rows and columns of the dead ones
 *     cov, packed as S: sigma^2 A^-1 over the live dimensions -- from the undamped factor, column by column through the
 *     two substitutions above on the unit vectors, times sigma * sigma; +inf on the diagonal of a dead dimension (one the
 *     factor kills included), 0 in its other entries
 *
 * Launches take no timing slot (MCL_K_COUNT stays 15).  Out of scope: a prior term; feeding the fix back into the filter;
 * roll and pitch; the fused steps; sharded handles beyond what mcl_pose_information accepts.
 */
#ifndef MCL_MATCH_H
#define MCL_MATCH_H
#include "mcl.h"
#include "mcl_information.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_MATCH_MAX_BEAMS 2048
#define MCL_MATCH_MAX_POSES 65536
#define MCL_MATCH_MAX_ITER 32
#define MCL_MATCH_MAX_DUMP (1 << 26)   /* floats of ranges_out */
#define MCL_MATCH_MAX_GRAD_FLOOR 4096  /* quanta */
#define MCL_MATCH_J0 (-10)
#define MCL_MATCH_J_MIN (-20)
#define MCL_MATCH_J_MAX 20

#define MCL_MATCH_CONVERGED 0
#define MCL_MATCH_MAX_ITER_HIT 1
#define MCL_MATCH_STALLED 2
#define MCL_MATCH_NO_OVERLAP 3

typedef struct mcl_match_sums {
  int64_t n;        /* beams cast */
  int64_t n_miss;   /* ... of which one of the 1 + 2 D rays found no seabed within r_max */
  int64_t n_jump;   /* ... of which, all hitting, some |d_k| > floor(jump_max 2^12) */
  int64_t S[10];    /* packed lower triangle of sum d_j d_k over x, y, yaw, z */
  int64_t C[4];     /* sum d_k rho */
  int64_t s_rho;    /* sum rho */
  int64_t s_rho2;   /* sum rho rho */
} mcl_match_sums;

typedef struct mcl_match_config {
  int32_t dims;          /* 3: x, y, yaw;  4: x, y, yaw, z */
  int32_t max_iter;      /* trial evaluations after the start's, 1 ... 32 */
  int32_t min_beams;     /* >= 1 */
  int32_t grad_floor_q;  /* 0 ... 4096 quanta; default 2 */
  double step_max_xy;    /* metres, > 0: the longest horizontal step, and the longest step in z */
  double step_max_yaw;   /* radians, > 0 */
  double tol_xy;         /* metres, >= 0 */
  double tol_yaw;        /* radians, >= 0 */
  mcl_information_steps steps;
} mcl_match_config;

typedef struct mcl_match_result {
  double x, y, yaw, z;   /* the final pose's moved coordinates (z: the start's for dims = 3) */
  int32_t status;        /* MCL_MATCH_CONVERGED ... */
  int32_t evaluations;   /* 1 + trials */
  int32_t accepted;      /* accepted steps */
  int32_t j;             /* the last damping exponent */
  int32_t dead;          /* the dead mask of the last solve (bit k: dimension k), 0 when none ran */
  int32_t reserved;
  mcl_match_sums start;  /* the record at the start pose */
  mcl_match_sums final;  /* the record at the final pose */
} mcl_match_result;

typedef struct mcl_match_trace {
  double x, y, yaw, z;   /* the pose evaluated */
  mcl_match_sums sums;   /* its record */
  int32_t j;             /* the exponent its step was solved with (row 0: MCL_MATCH_J0) */
  int32_t accepted;      /* 1: it became the current pose (row 0: 1 unless NO_OVERLAP) */
} mcl_match_trace;

typedef struct mcl_match_derived_t {
  double rms, mean;      /* metres */
  double chi2;           /* per contributing beam */
  double J[10];          /* packed as S */
  double cov[10];        /* packed as S */
  int32_t dead;
  int32_t m;             /* contributing beams */
} mcl_match_derived_t;

/* ---- device-free */
/* MCL_OK, or MCL_ERR_INVALID with *reason (or NULL) the rule that is broken: dims not 3 or 4, max_iter outside 1 ... 32,
 * min_beams < 1, grad_floor_q outside 0 ... 4096, a step_max not positive and finite, a tol negative or not finite, steps
 * that mcl_ping_information refuses for this r_max. */
int mcl_match_config_check(const mcl_match_config* cfg, double r_max, const char** reason);
/* MCL_ERR_INVALID: a null pointer, a config the check refuses (r_max aside), j outside -20 ... 22, a record that cannot be a
 * sum of the definition (a negative count, n > 2048, n_miss + n_jump > n, a diagonal sum negative or above m 2^46, a sum
 * above its bound). */
int mcl_match_solve(const mcl_match_sums* rec, const mcl_match_config* cfg, int32_t j, double delta_out[4], int32_t* dead_out);
int mcl_match_better(const mcl_match_sums* q, const mcl_match_sums* p, int32_t min_beams, int32_t* better);
int mcl_match_derived(const mcl_match_sums* rec, const mcl_match_config* cfg, double sigma, mcl_match_derived_t* out);

/* ---- one handle.  poses: host SoA, 6 x M doubles (x[M], y[M], z[M], roll[M], pitch[M], yaw[M]) in the coordinates the
 * particle state is stored in, 1 <= M <= 65536.  They travel to a scratch buffer the handle owns; needs a map, no particles;
 * never reads or writes the cloud, the weights, the counters or the caches.  One synchronisation, at the end (a pose upload
 * above 1 MiB waits for itself first, as every large upload of the library does).  sigma only
 * has to be positive and finite: the fix does not depend on it, mcl_match_derived does.
 * results_out: M records.  trace_out (or NULL): M x (max_iter + 1) records, row t of pose i at [i (max_iter + 1) + t]; rows
 * past `evaluations` are zero.  ranges_out (or NULL): M x (max_iter + 1) x (1 + 2 D) x B floats, [((i (max_iter + 1) + t)
 * (1 + 2 D) + v) B + b]; entries of evaluations that did not run and of beams that do not count are NaN.  Production
 * passes NULL for both.  The handle's scratch block holds the results (360 bytes per pose) and the trace (192 bytes per
 * pose and row: up to 415 MB at 65536 poses and max_iter = 32); a block above 64 MiB is released before the call returns.
 * MCL_ERR_INVALID: a null pointer, B outside 1 ... 2048, M outside 1 ... 65536, sigma not positive and finite, r_max <= 0
 * or > 4096, a config mcl_match_config_check refuses, an angle or a pose that is not finite, a ranges_out of more than 2^26
 * floats.  MCL_ERR_STATE: no map. */
int mcl_match_ping(mcl_handle* h, const double* poses, int64_t M, const float* ranges, const float* beam_angles, int32_t B,
                   double sigma, double r_max, const double sensor_offset[6], const mcl_match_config* cfg,
                   mcl_match_result* results_out, mcl_match_trace* trace_out, float* ranges_out);

#ifdef __cplusplus
}
#endif
#endif /* MCL_MATCH_H */
