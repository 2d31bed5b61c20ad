// mcl_acoustic.h -- kernels of the delayed acoustic updates (include/mcl_acoustic.h; gfx950, wave64): a position fix and
// slant ranges to fixed transponders, each evaluated at the pose the particle's own ancestor had when the measurement was
// taken.  One launch per update: a grid-stride loop over the current slots; per slot the chase through link and parent
// (as k_history_ancestors walks it -- the ancestor slot lives in a register, no buffer, no second launch), the gathered
// read of one frame (two with frac > 0), the likelihood in fp64 and the store or accumulate of lw[i].  No LDS, no scratch,
// no atomics; a particle's term depends on its own lineage and the call's arguments only, never on the launch geometry.
//   LAGGED  the pose comes from the frames (lag >= 0) / from the state (lag = -1: no link, no ring)
//   ARM     the transponder sits `offset` away from base_link: yaw is read, one sincos and the rotation / the common case
//           without a lever arm carries neither (and does not read yaw at all)
#pragma once
#include "mcl_history.h"

#define ACO_MAX_BEACONS 8   // MCL_ACOUSTIC_MAX_BEACONS

// what both updates share: where the pose comes from and how it becomes a point of the map
struct AcoArgs {
  const double* st[6];   // the state's columns (lag = -1: x, y, yaw; own_zrp: z, roll, pitch too)
  const u32* link;       // LAGGED: nullptr is the identity
  HistRing g;            // LAGGED
  int lag;
  double frac;           // in [0, 1); > 0: the second frame is read
  int own_zrp;           // 1: z, roll, pitch are the particle's own (lag = -1 only); 0: zrp below on every particle
  double z;
  double w[3];           // ARM, !own_zrp: Ry(pitch) Rx(roll) offset (the host's: the same on every particle)
  double off[3];         // ARM, own_zrp: the offset itself
  double m2o[12];        // rows 0 ... 2 of map <- odom
  u32 n;
  int accumulate;        // 1: lw[i] += term, 0: lw[i] = term
  double* lw;
};
struct FixArgs {
  double gx, gy;         // the fix, map frame
  double ia, ib, ic;     // S^-1 = [ia ib; ib ic]
  double lognorm;        // 1/2 log((2 pi)^2 det S)
};
struct BeaconArgs {
  double b[ACO_MAX_BEACONS][3];   // the VALID beacons, in the caller's order (the host drops the skipped ones)
  double r[ACO_MAX_BEACONS];
  int n_valid;
  double inv_sigma, lognorm;      // lognorm = n_valid log(sigma sqrt(2 pi))
};

#define ACO_TWO_PI 6.283185307179586476925286766559
#define ACO_PI 3.141592653589793238462643383279

// x, y (and with ARM: yaw) of the pose slot i is evaluated at
template <bool LAGGED, bool ARM>
__device__ __forceinline__ void aco_pose(const AcoArgs& a, u32 i, double& x, double& y, double& yaw) {
#pragma clang fp contract(off)
  yaw = 0.0;
  if (!LAGGED) {
    x = a.st[0][i];
    y = a.st[1][i];
    if (ARM) yaw = a.st[5][i];
    return;
  }
  const size_t n = a.g.n;
  u32 s = a.link ? a.link[i] : i;
  for (int j = 0; j < a.lag; ++j) s = a.g.parent[(size_t)hist_frame(a.g, j) * n + s];
  const int f0 = hist_frame(a.g, a.lag);
  const double* p0 = a.g.xyw + (size_t)f0 * 3 * n;
  x = p0[s];
  y = p0[n + s];
  if (ARM) yaw = p0[2 * n + s];
  if (a.frac > 0.0) {   // (the same on every lane)
    const u32 s1 = a.g.parent[(size_t)f0 * n + s];
    const double* p1 = a.g.xyw + (size_t)hist_frame(a.g, a.lag + 1) * 3 * n;
    x = x + a.frac * (p1[s1] - x);
    y = y + a.frac * (p1[n + s1] - y);
    if (ARM) {
      double d = p1[2 * n + s1] - yaw;
      d = d - ACO_TWO_PI * ceil((d - ACO_PI) / ACO_TWO_PI);
      yaw = yaw + a.frac * d;
    }
  }
}

// p = m2o [x y z 1]' + Rm Rz(yaw) (Ry(pitch) Rx(roll) offset)
template <bool ARM>
__device__ __forceinline__ void aco_point(const AcoArgs& a, u32 i, double x, double y, double yaw, double p[3]) {
#pragma clang fp contract(off)
  const double z = a.own_zrp ? a.st[2][i] : a.z;
#pragma unroll
  for (int r = 0; r < 3; ++r) p[r] = a.m2o[r * 4 + 0] * x + a.m2o[r * 4 + 1] * y + a.m2o[r * 4 + 2] * z + a.m2o[r * 4 + 3];
  if (ARM) {
    double w0 = a.w[0], w1 = a.w[1], w2 = a.w[2];
    if (a.own_zrp) {
      double sr, cr, sp, cp;
      sincos(a.st[3][i], &sr, &cr);
      sincos(a.st[4][i], &sp, &cp);
      w0 = cp * a.off[0] + (sp * sr) * a.off[1] + (sp * cr) * a.off[2];
      w1 = cr * a.off[1] - sr * a.off[2];
      w2 = (cp * sr) * a.off[1] + (cp * cr) * a.off[2] - sp * a.off[0];
    }
    double sy, cy;
    sincos(yaw, &sy, &cy);
    const double v0 = cy * w0 - sy * w1, v1 = sy * w0 + cy * w1;
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = p[r] + (a.m2o[r * 4 + 0] * v0 + a.m2o[r * 4 + 1] * v1 + a.m2o[r * 4 + 2] * w2);
  }
}

template <bool LAGGED, bool ARM>
__global__ void __launch_bounds__(MCL_BLOCK) k_fix_update(AcoArgs a, FixArgs f) {
#pragma clang fp contract(off)
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
    double x, y, yaw, p[3];
    aco_pose<LAGGED, ARM>(a, i, x, y, yaw);
    aco_point<ARM>(a, i, x, y, yaw, p);
    const double dx = f.gx - p[0], dy = f.gy - p[1];
    const double q = f.ia * (dx * dx) + 2.0 * (f.ib * (dx * dy)) + f.ic * (dy * dy);
    const double val = -0.5 * q - f.lognorm;
    a.lw[i] = a.accumulate ? a.lw[i] + val : val;
  }
}

template <bool LAGGED, bool ARM>
__global__ void __launch_bounds__(MCL_BLOCK) k_beacon_update(AcoArgs a, BeaconArgs f) {
#pragma clang fp contract(off)
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
    double x, y, yaw, p[3];
    aco_pose<LAGGED, ARM>(a, i, x, y, yaw);
    aco_point<ARM>(a, i, x, y, yaw, p);
    double acc = 0.0;
    for (int b = 0; b < f.n_valid; ++b) {   // (the table sits in the argument block: scalar loads, beacon order)
      const double ex = p[0] - f.b[b][0], ey = p[1] - f.b[b][1], ez = p[2] - f.b[b][2];
      const double e = (f.r[b] - sqrt(ex * ex + ey * ey + ez * ez)) * f.inv_sigma;
      acc = acc + e * e;
    }
    const double val = (0.0 - 0.5 * acc) - f.lognorm;
    a.lw[i] = a.accumulate ? a.lw[i] + val : val;
  }
}
