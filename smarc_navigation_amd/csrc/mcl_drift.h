// mcl_drift.h -- kernels of the per-particle drift states (include/mcl_drift.h; gfx950, wave64): the prior draw, the
// advance queued before a predict, the gather queued behind every resample and the moments.  Streaming kernels, one lane
// per particle, grid-stride; no scratch; LDS only for the moments' words.  The state is SoA: cx[n], cy[n], bw[n].
#pragma once
#include "mcl_kernels.h"
#include "mcl_history.h"
#include "mcl_regularise.h"

#define DRIFT_SUMS 9        // e0, e1, e2, then e_r e_c at 3 + reg_packed(r, c): e0 e0, e1 e0, e1 e1, e2 e0, e2 e1, e2 e2  (e = d - the drift of slot 0)
#define DRIFT_RES_WORDS 12  // the DRIFT_SUMS sums, then the shift (the drift of slot 0)

struct DriftDraw {
  double sq[3];    // what multiplies xi_c: init_std[c] (prior) or walk_std[c] * sqrt(dt) (advance)
  u32 k0, k1;      // Philox key (seed)
  u32 step;        // 0: the prior; k: the k-th advance
  long long gid0;  // global id of local particle 0
};
// xi_0, xi_1, xi_2 of particle i: the caller's normals (n x 3, particle-major) or components 0 .. 2 of native_normals6's
// layout at purpose 7.  A pair whose two factors are zero is not evaluated -- a uniform branch of the kernel arguments.
__device__ __forceinline__ void drift_normals(long long i, const DriftDraw& a, const double* __restrict__ replay, double z[3]) {
  z[0] = z[1] = z[2] = 0.0;
  if (replay) {
#pragma unroll
    for (int c = 0; c < 3; ++c) z[c] = replay[i * 3 + c];
    return;
  }
  const bool p0 = a.sq[0] != 0.0 || a.sq[1] != 0.0, p1 = a.sq[2] != 0.0;
  if (p0 || p1) {
    const u32x4 o = philox4x32((u32)(a.gid0 + i), 0u, a.step, 7u, a.k0, a.k1);
    double unused;
    if (p0) box_muller(o.x, o.y, z[0], z[1]);
    if (p1) box_muller(o.z, o.w, z[2], unused);
  }
}

// ------------------------------------------------------------------ prior
__global__ void __launch_bounds__(MCL_BLOCK) k_drift_init(double* __restrict__ cx, double* __restrict__ cy,
                                                          double* __restrict__ bw, long long n, DriftDraw a,
                                                          const double* __restrict__ replay) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    double z[3];
    drift_normals(i, a, replay, z);
    // (a zero std gives +0.0 whatever the sign of the caller's normal)
    cx[i] = a.sq[0] != 0.0 ? a.sq[0] * z[0] : 0.0;
    cy[i] = a.sq[1] != 0.0 ? a.sq[1] * z[1] : 0.0;
    bw[i] = a.sq[2] != 0.0 ? a.sq[2] * z[2] : 0.0;
  }
}

// ------------------------------------------------------------------ advance
// pose += drift dt, then the drift's random walk (include/mcl_drift.h, steps 1 - 3).  Every product and every sum is one
// IEEE operation of its own (no contraction): a restatement in numpy gives the same bits, also where the sum cancels.
// Six coalesced loads; a store only where a value can have changed: a zero drift component leaves its pose word alone
// (per lane), a zero walk leaves its drift word alone (uniform).  The arithmetic is the predict kernel's noise draw: one
// Philox block, two Box-Muller.
__global__ void __launch_bounds__(MCL_BLOCK) k_drift_advance(double* __restrict__ x, double* __restrict__ y,
                                                             double* __restrict__ yaw, double* __restrict__ cx,
                                                             double* __restrict__ cy, double* __restrict__ bw,
                                                             long long n, double dt, DriftDraw a,
                                                             const double* __restrict__ replay) {
#pragma clang fp contract(off)
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double c0 = cx[i], c1 = cy[i], c2 = bw[i];
    if (c0 != 0.0) x[i] = x[i] + c0 * dt;
    if (c1 != 0.0) y[i] = y[i] + c1 * dt;
    if (c2 != 0.0) {
      const double t = yaw[i] + c2 * dt;
      yaw[i] = (t >= -MCL_PI && t < MCL_PI) ? t : wrap_pi(t);
    }
    double z[3];
    drift_normals(i, a, replay, z);
    if (a.sq[0] != 0.0) cx[i] = c0 + a.sq[0] * z[0];
    if (a.sq[1] != 0.0) cy[i] = c1 + a.sq[1] * z[1];
    if (a.sq[2] != 0.0) bw[i] = c2 + a.sq[2] * z[2];
  }
}

// ------------------------------------------------------------------ the resample hook
// d'[i] = d[A(i)], in place: the ancestor of a lost slot is a surviving slot (its index occurs in the ancestor vector),
// and a surviving slot (A(i) = i) is neither written nor moved -- no lane reads a word another lane writes.  4 B per
// particle (the slot map) and 48 B per lost slot.  (No __restrict__: reads and writes share the three arrays.)
template <bool ALT>
__global__ void __launch_bounds__(MCL_BLOCK) k_drift_gather(HistMap m, u32 n, double* cx, double* cy, double* bw) {
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const u32 a = hist_slot_ancestor<ALT>(m, i, n);   // (< n, and i itself on a slot map that is not sound)
    if (a != i) {
      cx[i] = cx[a];
      cy[i] = cy[a];
      bw[i] = bw[a];
    }
  }
}

// ------------------------------------------------------------------ moments
// The nine sums about the drift of slot 0: mcl_regularise.h's moments of three values, none of them an angle.
__global__ void __launch_bounds__(MCL_BLOCK) k_drift_moments(const double* __restrict__ cx, const double* __restrict__ cy,
                                                             const double* __restrict__ bw, long long n,
                                                             double* __restrict__ part /*[DRIFT_SUMS][grid]*/,
                                                             double* __restrict__ shift_out) {
  static_assert(DRIFT_SUMS == 3 + 3 * (3 + 1) / 2, "the rows moments_about_slot0<3> writes");
  __shared__ double acc[MCL_BLOCK / MCL_WAVE][DRIFT_SUMS];
  const double* const v[3] = {cx, cy, bw};
  moments_about_slot0<3, false>(acc, v, n, blockDim.x, part, shift_out);
}
