// mcl_regularise.h -- kernels of the regularised resampling (include/mcl_regularise.h; gfx950, wave64): the moments of
// (x, y, yaw[, cx, cy, bw]) about slot 0, the factor of their covariance (one lane), and the jitter.  Streaming kernels,
// one lane per particle, grid-stride; no scratch; LDS only for the moments' words.
#pragma once
#include "mcl_kernels.h"
#include "mcl_host_pure.h"

#define REG_SUMS_MAX 27   // D + D (D + 1) / 2 sums: 9 for three dimensions, 27 for six
// the record a call leaves on the device (doubles): mcl_regularise_last copies it
#define REG_RES_SUMS 0                                 // S_0 .. S_{D-1}, then P packed
#define REG_RES_SHIFT REG_SUMS_MAX                     // 6
#define REG_RES_MEAN (REG_RES_SHIFT + REG_MAX_DIMS)    // 6
#define REG_RES_COV (REG_RES_MEAN + REG_MAX_DIMS)      // 21
#define REG_RES_CHOL (REG_RES_COV + REG_MAX_PACKED)    // 21
#define REG_RES_DEAD (REG_RES_CHOL + REG_MAX_PACKED)   // the dead mask, as a double
#define REG_RES_WORDS (REG_RES_DEAD + 1)

struct RegPtrs {
  double* v[REG_MAX_DIMS];   // x, y, yaw, cx, cy, bw (the last three nullptr for three dimensions)
};
struct RegDraw {
  u32 k0, k1;      // Philox key (seed)
  u32 step;        // earlier regularise calls on the handle
  long long gid0;  // global id of local particle 0
};

// e of dimension r (include/mcl_regularise.h): the difference to the shift, the yaw's taken into [-pi, pi)
template <int R>
__device__ __forceinline__ double reg_centre(double v, double s) {
#pragma clang fp contract(off)
  const double t = v - s;
  if (R != 2) return t;
  return (t >= -MCL_PI && t < MCL_PI) ? t : wrap_pi(t);
}

// ------------------------------------------------------------------ moments
// The D + D (D + 1) / 2 sums of D values about slot 0, in the fixed tree of mcl_device.h: rows 0 .. D - 1 the sums of
// e_r, row D + reg_packed(r, c) the sum of e_r e_c; zero terms in the lanes past n.  ANGLE2: dimension 2 is an angle, its
// difference taken into [-pi, pi).  The products are formed where they are summed: D values stay live, not D (D + 1) / 2.
// One body for k_reg_moments (v = x, y, yaw[, cx, cy, bw]) and for k_drift_moments (mcl_drift.h: v = cx, cy, bw); acc and
// block = blockDim.x come from the kernel (mcl_device.h, the fixed tree: blockDim.x is read in kernels only).
template <int D, bool ANGLE2, class V>
__device__ __forceinline__ void moments_about_slot0(double (&acc)[MCL_BLOCK / MCL_WAVE][D + D * (D + 1) / 2],
                                                    const V& v /*[D] pointers*/, long long n, u32 block,
                                                    double* __restrict__ part /*[NS][grid]*/,
                                                    double* __restrict__ shift_out) {
#pragma clang fp contract(off)
  constexpr int NS = D + D * (D + 1) / 2;
  const int lane = threadIdx.x & 63;
  tree_zero(acc);
  double s[D];
#pragma unroll
  for (int r = 0; r < D; ++r) s[r] = v[r][0];
  for (long long base = blockIdx.x * (long long)block + (threadIdx.x & ~63); base < n; base += (long long)gridDim.x * block) {
    const long long i = base + lane;
    double e[D];
#pragma unroll
    for (int r = 0; r < D; ++r) e[r] = 0.0;
    if (i < n) {
#pragma unroll
      for (int r = 0; r < D; ++r) e[r] = (ANGLE2 && r == 2) ? reg_centre<2>(v[r][i], s[r]) : reg_centre<0>(v[r][i], s[r]);
    }
#pragma unroll
    for (int r = 0; r < D; ++r) tree_add(acc, r, e[r]);
#pragma unroll
    for (int r = 0; r < D; ++r) {
#pragma unroll
      for (int c = 0; c <= r; ++c) tree_add(acc, D + reg_packed(r, c), e[r] * e[c]);
    }
  }
  tree_flush(acc, NS, part);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int r = 0; r < D; ++r) shift_out[r] = s[r];
  }
}
template <int D>
__global__ void __launch_bounds__(MCL_BLOCK) k_reg_moments(RegPtrs p, long long n, double* __restrict__ part,
                                                           double* __restrict__ shift_out) {
  __shared__ double acc[MCL_BLOCK / MCL_WAVE][D + D * (D + 1) / 2];
  moments_about_slot0<D, true>(acc, p.v, n, blockDim.x, part, shift_out);
}

// ------------------------------------------------------------------ factor
// One lane: the sums k_sum_final left in res[REG_RES_SUMS ..] become m, C and -- by reg_factor, the function
// mcl_regularise_factor runs on the host -- L and the dead mask, in the same record.  Nothing returns to the host.
template <int D>
__global__ void __launch_bounds__(MCL_WAVE) k_reg_factor(double* __restrict__ res, long long n) {
#pragma clang fp contract(off)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  constexpr int NP = D * (D + 1) / 2;
  const double N = (double)n;
  double m[D];
  __shared__ double C[NP], L[NP];   // (reg_factor indexes them in loops: LDS, not scratch)
#pragma unroll
  for (int r = 0; r < D; ++r) m[r] = res[REG_RES_SUMS + r] / N;
#pragma unroll
  for (int r = 0; r < D; ++r) {
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      const double q = res[REG_RES_SUMS + D + reg_packed(r, c)] / N;
      const double mm = m[r] * m[c];
      C[reg_packed(r, c)] = q - mm;
    }
  }
  const int dead = reg_factor(C, D, L);
#pragma unroll
  for (int r = 0; r < REG_MAX_DIMS; ++r) res[REG_RES_MEAN + r] = r < D ? m[r] : 0.0;
#pragma unroll
  for (int k = 0; k < REG_MAX_PACKED; ++k) {
    res[REG_RES_COV + k] = k < NP ? C[k] : 0.0;
    res[REG_RES_CHOL + k] = k < NP ? L[k] : 0.0;
  }
#pragma unroll
  for (int r = D; r < REG_MAX_DIMS; ++r) res[REG_RES_SHIFT + r] = 0.0;
  res[REG_RES_DEAD] = (double)dead;
}

// ------------------------------------------------------------------ apply
// xi_0 .. xi_{D-1} of particle i: the caller's normals (n x D, particle-major) or native_normals6's layout at purpose 8
// (block 0: xi_0 .. xi_3, block 1: xi_4, xi_5; three dimensions evaluate block 0 only).
template <int D>
__device__ __forceinline__ void reg_normals(long long i, const RegDraw& a, const double* __restrict__ replay, double z[D]) {
  if (replay) {
#pragma unroll
    for (int c = 0; c < D; ++c) z[c] = replay[i * D + c];
    return;
  }
  [[maybe_unused]] double unused;
  const u32x4 o = philox4x32((u32)(a.gid0 + i), 0u, a.step, 8u, a.k0, a.k1);
  box_muller(o.x, o.y, z[0], z[1]);
  if constexpr (D == 3) {
    box_muller(o.z, o.w, z[2], unused);
  } else {
    box_muller(o.z, o.w, z[2], z[3]);
    const u32x4 o1 = philox4x32((u32)(a.gid0 + i), 1u, a.step, 8u, a.k0, a.k1);
    box_muller(o1.x, o1.y, z[4], z[5]);
  }
}

// v_r <- [s_r + (m_r + a (e_r - m_r))  or  v_r] + h (L xi)_r, in place, one lane per slot.  L, m and s are read from the
// record the factor kernel left (uniform: scalar loads).  A dimension whose row of L is zero is neither loaded nor stored
// (a uniform branch); every product and every sum is one IEEE operation of its own (no contraction).
template <int D, bool SHRINK>
__global__ void __launch_bounds__(MCL_BLOCK) k_reg_apply(RegPtrs p, long long n, const double* __restrict__ res, double h,
                                                         double a, RegDraw dr, const double* __restrict__ replay) {
#pragma clang fp contract(off)
  constexpr int NP = D * (D + 1) / 2;
  double L[NP], m[D], s[D];
  bool live[D];
#pragma unroll
  for (int k = 0; k < NP; ++k) L[k] = res[REG_RES_CHOL + k];
#pragma unroll
  for (int r = 0; r < D; ++r) {
    m[r] = res[REG_RES_MEAN + r];
    s[r] = res[REG_RES_SHIFT + r];
    bool any = false;
#pragma unroll
    for (int c = 0; c <= r; ++c) any = any || L[reg_packed(r, c)] != 0.0;
    live[r] = any;
  }
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    double xi[D];
    reg_normals<D>(i, dr, replay, xi);
#pragma unroll
    for (int r = 0; r < D; ++r) {
      if (!live[r]) continue;
      double z = L[reg_packed(r, 0)] * xi[0];
#pragma unroll
      for (int c = 1; c <= r; ++c) {
        const double q = L[reg_packed(r, c)] * xi[c];
        z = z + q;
      }
      const double cur = p.v[r][i];
      const double t5 = h * z;
      double v;
      if (SHRINK) {
        const double e = r == 2 ? reg_centre<2>(cur, s[r]) : reg_centre<0>(cur, s[r]);
        const double t1 = e - m[r];
        const double t2 = a * t1;
        const double t3 = m[r] + t2;
        const double t4 = s[r] + t3;
        v = t4 + t5;
      } else {
        v = cur + t5;
      }
      if (r == 2) v = (v >= -MCL_PI && v < MCL_PI) ? v : wrap_pi(v);
      p.v[r][i] = v;
    }
  }
}
