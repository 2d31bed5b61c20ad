// mcl_recovery.h -- kernels of global localisation and kidnap recovery (include/mcl_recovery.h; gfx950, wave64, fp64):
// k_uniform_state<INJECT> (uniform initialisation / random-particle injection) and the weight statistics
// k_wstats_partial + k_wstats_final.  Streaming kernels; no scratch, LDS only for the reductions' few words.
#pragma once
#include "mcl_kernels.h"

// ------------------------------------------------------------------ uniform state draws
struct UniformArgs {
  double lo[3], hi[3], w[3];   // x, y, yaw: min, max, fl(max - min)
  double r00, r10, r01, r11;   // MCL_FRAME_MAP: rotation block of m2o (its transpose carries map -> odom)
  double tx, ty, theta;        // ... its translation; atan2(r10, r00)
  int xform;                   // 0: the box is in the state's own frame (or m2o is the identity)
  u32 k0, k1, step, purpose;   // Philox key (seed), counter words 2 and 3
  long long gid0;              // global id of local particle 0
  double fraction;             // INJECT: particle replaced iff u_select < fraction
};
// 53-bit uniform in [0, 1) from two 32-bit words (the rule of native_u53, mcl_host_pure.h)
__device__ __forceinline__ double u53_to_double(u32 hi, u32 lo) {
  return (double)(((u64)(hi >> 5) << 26) | (u64)(lo >> 6)) * (1.0 / 9007199254740992.0);
}
// min + u (max - min), the product and the sum each rounded (NOT fused: a restatement in any language gives the same bits)
__device__ __forceinline__ double uniform_in(double u, double lo, double w, double hi) {
#pragma clang fp contract(off)
  const double p = u * w;
  const double v = lo + p;
  return v < hi ? v : hi;
}
// One lane per particle.  INJECT = false: every particle, z = roll = pitch = 0.  INJECT = true: only the particles the
// selection draw picks are written (x, y, yaw); each workgroup leaves the number it replaced in block_cnt[blockIdx.x]
// (ballot counts per wave, added in LDS: no atomics, k_count_final adds the workgroups').
// replay: n x 3 (n x 4 with INJECT) uniforms, particle-major, or nullptr (Philox).
template <bool INJECT>
__global__ void __launch_bounds__(MCL_BLOCK) k_uniform_state(StatePtrs s, long long n, UniformArgs a,
                                                             const double* __restrict__ replay,
                                                             u64* __restrict__ block_cnt) {
  u32 cnt = 0;   // (wave-uniform among the lanes still in the loop; lane 0 leaves last)
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    double u[4];
    if (replay) {
      constexpr int NU = INJECT ? 4 : 3;
#pragma unroll
      for (int c = 0; c < NU; ++c) u[c] = replay[i * NU + c];
      if (!INJECT) u[3] = 0.0;
    } else {
      const u32 gid = (u32)(a.gid0 + i);
      const u32x4 o0 = philox4x32(gid, 0u, a.step, a.purpose, a.k0, a.k1);
      const u32x4 o1 = philox4x32(gid, 1u, a.step, a.purpose, a.k0, a.k1);
      u[0] = u53_to_double(o0.x, o0.y);
      u[1] = u53_to_double(o0.z, o0.w);
      u[2] = u53_to_double(o1.x, o1.y);
      u[3] = u53_to_double(o1.z, o1.w);
    }
    const bool sel = !INJECT || u[3] < a.fraction;
    if constexpr (INJECT) cnt += (u32)__popcll(__ballot(sel));
    if (sel) {
      double x = uniform_in(u[0], a.lo[0], a.w[0], a.hi[0]);
      double y = uniform_in(u[1], a.lo[1], a.w[1], a.hi[1]);
      double yaw = uniform_in(u[2], a.lo[2], a.w[2], a.hi[2]);
      if (a.xform) {
        const double dx = x - a.tx, dy = y - a.ty;
        x = a.r00 * dx + a.r10 * dy;
        y = a.r01 * dx + a.r11 * dy;
        if (a.theta != 0.0) yaw = wrap_pi(yaw - a.theta);
      }
      s.c[0][i] = x;
      s.c[1][i] = y;
      s.c[5][i] = yaw;
      if constexpr (!INJECT) {
        s.c[2][i] = 0.0;
        s.c[3][i] = 0.0;
        s.c[4][i] = 0.0;
      }
    }
  }
  if constexpr (INJECT) {
    __shared__ u32 sh[MCL_BLOCK / MCL_WAVE];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      u64 t = 0;
#pragma unroll
      for (int w = 0; w < MCL_BLOCK / MCL_WAVE; ++w) t += sh[w];
      block_cnt[blockIdx.x] = t;
    }
  }
}
// out[0] = sum of the np workgroup counts (one workgroup)
__global__ void __launch_bounds__(MCL_BLOCK) k_count_final(const u64* __restrict__ block_cnt, int np, u64* __restrict__ out) {
  __shared__ u64 sh[16];
  u64 acc = 0;
  for (int i = threadIdx.x; i < np; i += blockDim.x) acc += block_cnt[i];
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) out[0] = acc;
}

// ------------------------------------------------------------------ weight statistics
// max lw, its particle, sum exp(lw - max), sum exp(2 (lw - max)), the number of finite log-weights -- as a FIXED tree,
// so that the result is a function of (lw, n) alone:
//   k_wstats_partial: one workgroup per tile of WS_TILE consecutive particles (the grid follows from n, no grid stride).
//     Four log-weights per lane in two 16-byte loads; the tile's maximum first (registers -> wave shuffles -> four LDS
//     words), then every weight relative to THAT maximum, summed lane -> wave -> workgroup in a fixed order.  One
//     32-byte record per tile.
//   k_wstats_final (one workgroup): the maximum over the records, then the records' sums rescaled by
//     exp(tile max - max) -- the ONE rescaling a weight ever sees -- and added in index order per lane, then by the same
//     fixed workgroup tree.  Ties of the maximum go to the lowest global id.  Writes the eleven result words.
// A log-weight that is not finite (NaN, +-inf) enters as -inf: weight 0, not live, never the maximum.
#define WS_ITEMS 4
#define WS_TILE (MCL_BLOCK * WS_ITEMS)
#define WS_NO_ARG 0xffffffffu
#define WS_OUT_WORDS 16   // max, sum_w, sum_w2, argmax gid (u64 bits; all ones: none), n_live (u64 bits), pose[6], pad
struct WsPartial {
  double m;       // largest finite log-weight of the tile (-inf: none)
  u64 arg_live;   // its global id (lowest on ties; WS_NO_ARG: none) | finite log-weights of the tile << 32
  double s, s2;   // sum exp(lw - m), sum exp(2 (lw - m))
};
// max / min of a workgroup's values in EVERY thread (sh: one word per wave)
__device__ __forceinline__ double ws_block_max_all(double v, double* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh[0];
#pragma unroll
  for (int w = 1; w < MCL_BLOCK / MCL_WAVE; ++w) r = sh[w] > r ? sh[w] : r;
  return r;
}
__device__ __forceinline__ u32 ws_block_min_all(u32 v, u32* sh) {
  v = wave_min(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  u32 r = sh[0];
#pragma unroll
  for (int w = 1; w < MCL_BLOCK / MCL_WAVE; ++w) r = sh[w] < r ? sh[w] : r;
  return r;
}
__device__ __forceinline__ double ws_finite_or_ninf(double x) {
  return __builtin_fabs(x) < __builtin_inf() ? x : -__builtin_inf();   // (NaN compares false)
}

__global__ void __launch_bounds__(MCL_BLOCK) k_wstats_partial(const double* __restrict__ lw, long long n, long long gid0,
                                                              WsPartial* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double shd[16];
  __shared__ u32 shu[16];
  const long long base = (long long)blockIdx.x * WS_TILE;
  // lane t holds particles base + 2 t, + 1 and base + 512 + 2 t, + 1: every wave load is 1 KiB of consecutive bytes
  double v[WS_ITEMS];
  long long idx[WS_ITEMS];
#pragma unroll
  for (int k = 0; k < WS_ITEMS / 2; ++k) {
    const long long i0 = base + (long long)k * (2 * MCL_BLOCK) + 2 * (long long)threadIdx.x;
    idx[2 * k] = i0;
    idx[2 * k + 1] = i0 + 1;
    if (i0 + 1 < n) {
      const double2 p = *reinterpret_cast<const double2*>(lw + i0);   // (lw is 256-byte aligned, i0 even)
      v[2 * k] = ws_finite_or_ninf(p.x);
      v[2 * k + 1] = ws_finite_or_ninf(p.y);
    } else {
      v[2 * k] = i0 < n ? ws_finite_or_ninf(lw[i0]) : -__builtin_inf();
      v[2 * k + 1] = -__builtin_inf();
    }
  }
  double tm = -__builtin_inf();
  u32 targ = WS_NO_ARG, live = 0;
#pragma unroll
  for (int k = 0; k < WS_ITEMS; ++k) {   // ascending particle ids: `>` keeps the lowest on ties
    if (v[k] > tm) {
      tm = v[k];
      targ = (u32)(gid0 + idx[k]);
    }
    live += v[k] > -__builtin_inf() ? 1u : 0u;
  }
  const double bm = ws_block_max_all(tm, shd);
  const u32 barg = ws_block_min_all(tm == bm ? targ : WS_NO_ARG, shu);   // (no finite weight: every targ is WS_NO_ARG)
  double s = 0.0, s2 = 0.0;
#pragma unroll
  for (int k = 0; k < WS_ITEMS; ++k) {
    const double e = det_exp(v[k] - bm);   // (-inf and NaN -- nothing finite in the tile -- give 0)
    s += e;
    s2 += e * e;
  }
  s = block_sum(s, shd);
  s2 = block_sum(s2, shd);
  live = block_sum(live, shu);
  if (threadIdx.x == 0) {
    WsPartial r;
    r.m = bm;
    r.arg_live = (u64)barg | ((u64)live << 32);
    r.s = s;
    r.s2 = s2;
    part[blockIdx.x] = r;
  }
}

__global__ void __launch_bounds__(MCL_BLOCK) k_wstats_final(const WsPartial* __restrict__ part, long long np, StatePtrs st,
                                                            long long gid0, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double shd[16];
  __shared__ u32 shu[16];
  __shared__ u64 shl[16];
  double tm = -__builtin_inf();
  u32 targ = WS_NO_ARG;
  u64 live = 0;
  for (long long p = threadIdx.x; p < np; p += blockDim.x) {   // ascending tiles = ascending ids: `>` keeps the lowest
    const WsPartial r = part[p];
    if (r.m > tm) {
      tm = r.m;
      targ = (u32)r.arg_live;
    }
    live += r.arg_live >> 32;
  }
  const double gm = ws_block_max_all(tm, shd);
  const u32 garg = ws_block_min_all(tm == gm ? targ : WS_NO_ARG, shu);
  double s = 0.0, s2 = 0.0;
  for (long long p = threadIdx.x; p < np; p += blockDim.x) {
    const double f = det_exp(part[p].m - gm);   // (exactly 1 for the tile(s) that hold the maximum)
    s += part[p].s * f;
    s2 += part[p].s2 * (f * f);
  }
  s = block_sum(s, shd);
  s2 = block_sum(s2, shd);
  live = block_sum(live, shl);
  if (threadIdx.x == 0) {
    out[0] = gm;
    out[1] = s;
    out[2] = s2;
    const bool any = garg != WS_NO_ARG;
    out[3] = __longlong_as_double(any ? (long long)garg : -1ll);
    out[4] = __longlong_as_double((long long)live);
    const long long loc = any ? (long long)garg - gid0 : 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) out[5 + c] = any ? st.c[c][loc] : 0.0;
  }
}
