// mcl_history.h -- kernels of the particle genealogy (include/mcl_history.h; gfx950, wave64): the ancestor link composed
// behind every resample, the frame record, the fixed-lag smoother's backward walk with descendant counts, and the two
// plain chases.  Streaming kernels; no scratch; LDS only for the reductions' words and the path's slots.  Everything that
// decides WHO descends from whom is integer (u32 slots and counts, integer atomics: the order of the adds cannot matter);
// the floating-point sums are a fixed tree.
#pragma once
#include "mcl_kernels.h"
#include "mcl_resample.h"

#define HIST_SUMS 8        // c dx, c dy, c sin, c cos, c dx dx, c dx dy, c dy dy, [c > 0]
#define HIST_RES_WORDS 10  // per lag (doubles): the HIST_SUMS sums, then the frame's shift (x, y of slot 0)
#define HIST_ROUNDS 8      // wave aggregation: distinct slots a wave merges before its lanes add one by one
#define HIST_MAX_DEPTH 1024   // MCL_HISTORY_MAX_DEPTH

// the slot map of the last resample, as the gather read it: which slot's pre-resample state was copied into slot i
//   ALT = false  systematic pipeline (mcl_resample.h): zr[i] = rank of a lost slot or ZR_SURVIVOR, dupes32[rank] = ancestor
//   ALT = true   explicit-index schemes (mcl_resample_alt.h, k_reassign_idx): cnt[i] == 0: lost, zcum[i] - 1 its rank
struct HistMap {
  const u32* zr;        // ALT = false
  const u32* dupes32;
  const u32* cnt;       // ALT = true
  const u32* zcum;
  const int* dupes;
};
template <bool ALT>
__device__ __forceinline__ u32 hist_slot_ancestor(const HistMap& m, u32 i, u32 n) {
  u32 a = i;
  if (ALT) {
    if (m.cnt[i] == 0u) a = (u32)m.dupes[m.zcum[i] - 1u];
  } else {
    const u32 r = m.zr[i];
    if (r != ZR_SURVIVOR) a = m.dupes32[r];
  }
  // A memory-safety guard and nothing else: the resample kernels write slots below n only, so the bound never bites on a
  // sound slot map; on a corrupted one it keeps the gathered read of link inside its buffer (the link is then wrong, as
  // the state the gather copied is).
  return a < n ? a : i;
}

// ------------------------------------------------------------------ compose
// link'(i) = link(A(i)), into the other link buffer (a gathered read of link cannot be done in place).  link == nullptr:
// the link is the identity (right after enable, reset or a record) -- link' = A, without the gathered read.
template <bool ALT>
__global__ void __launch_bounds__(MCL_BLOCK) k_history_compose(HistMap m, const u32* __restrict__ link, u32 n,
                                                               u32* __restrict__ out) {
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const u32 a = hist_slot_ancestor<ALT>(m, i, n);
    out[i] = link ? link[a] : a;
  }
}

// ------------------------------------------------------------------ record
// the frame: parent = link (nullptr: the identity) and the bits of x, y, yaw; the host marks the link as the identity
// again (nothing is written for it)
__global__ void __launch_bounds__(MCL_BLOCK) k_history_record(const u32* __restrict__ link, const double* __restrict__ x,
                                                              const double* __restrict__ y, const double* __restrict__ yaw,
                                                              u32 n, u32* __restrict__ parent, double* __restrict__ fx,
                                                              double* __restrict__ fy, double* __restrict__ fyaw) {
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    parent[i] = link ? link[i] : i;
    fx[i] = x[i];
    fy[i] = y[i];
    fyaw[i] = yaw[i];
  }
}

// ------------------------------------------------------------------ smoothing
// c_0 = histogram of link over the slots of the newest frame (C zeroed by the caller).  The adds are aggregated per wave
// as k_modes_hist's are: after a few resamples a wave's 64 particles descend from a handful of slots.  link == nullptr:
// c_0 = 1 everywhere, plain stores.
__global__ void __launch_bounds__(MCL_BLOCK) k_history_count0(const u32* __restrict__ link, u32 n, u32* __restrict__ C) {
  const int lane = threadIdx.x & 63;
  for (u32 base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += gridDim.x * blockDim.x) {
    const u32 i = base + lane;
    const bool live = i < n;
    if (!link) {
      if (live) C[i] = 1u;
      continue;
    }
    const u32 s = live ? link[i] : 0u;
    bool pending = live;
    for (int r = 0; r < HIST_ROUNDS; ++r) {
      const u64 todo = __ballot(pending);
      if (!todo) break;
      const int leader = __ffsll((long long)todo) - 1;
      const u32 sl = (u32)__builtin_amdgcn_readlane((int)s, leader);
      const bool mine = pending && s == sl;
      const u32 cnt = (u32)__popcll(__ballot(mine));
      if (lane == leader) atomicAdd(&C[sl], cnt);
      pending = pending && !mine;
    }
    if (pending) atomicAdd(&C[s], 1u);
  }
}

// One frame of the backward walk, one pass over its slots: the count-weighted sums of the slots with c > 0, and, when an
// older frame follows, c_next[parent[s]] += c[s] (C_next zeroed by the caller; integer atomics).  The sums are the fixed
// tree of mcl_device.h: the eight terms about slot 0 of the frame, zero in the lanes with c == 0.  A wave whose 64 slots
// all have c == 0 reads their counts and nothing else -- which pays only where whole waves are empty: the surviving
// ancestors are scattered over the slots, and at 1 M particles nearly every wave still holds one 64 frames back
// (measured).
__global__ void __launch_bounds__(MCL_BLOCK) k_history_frame(const u32* __restrict__ C, const u32* __restrict__ parent,
                                                             u32* __restrict__ C_next, const double* __restrict__ fx,
                                                             const double* __restrict__ fy, const double* __restrict__ fyaw,
                                                             u32 n, double* __restrict__ part /*[HIST_SUMS][grid]*/,
                                                             double* __restrict__ shift_out) {
#pragma clang fp contract(off)
  __shared__ double acc[MCL_BLOCK / MCL_WAVE][HIST_SUMS];
  const int lane = threadIdx.x & 63;
  tree_zero(acc);
  const double x0 = fx[0], y0 = fy[0];
  for (u32 base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += gridDim.x * blockDim.x) {
    const u32 s = base + lane;
    const u32 c = s < n ? C[s] : 0u;
    if (!__ballot(c != 0u)) continue;
    double b[4] = {0.0, 0.0, 0.0, 0.0};   // dx, dy, sin, cos (the three products are formed where they are summed)
    if (c != 0u) {
      if (C_next) atomicAdd(&C_next[parent[s]], c);
      b[0] = fx[s] - x0;
      b[1] = fy[s] - y0;
      sincos(fyaw[s], &b[2], &b[3]);
    }
    const double w = (double)c;
#pragma unroll
    for (int j = 0; j < HIST_SUMS; ++j) {
      const double t = j < 4 ? w * b[j] : (j == 4 ? w * (b[0] * b[0]) : (j == 5 ? w * (b[0] * b[1]) : (j == 6 ? w * (b[1] * b[1]) : (c != 0u ? 1.0 : 0.0))));
      tree_add(acc, j, t);
    }
  }
  tree_flush(acc, HIST_SUMS, part);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    shift_out[0] = x0;
    shift_out[1] = y0;
  }
}

// ------------------------------------------------------------------ chases
// the ring of frames as the chases see it: frame `head` is the newest, head - 1 (mod depth) the one before
struct HistRing {
  const u32* parent;     // [depth][n]
  const double* xyw;     // [depth][3][n]
  u32 n;
  int depth, head;
};
__device__ __forceinline__ int hist_frame(const HistRing& g, int lag) {
  const int f = g.head - lag;
  return f < 0 ? f + g.depth : f;
}
// out[i] = a_lag(i): a_0 = link, a_{j+1} = parent_{F-j}[a_j]
__global__ void __launch_bounds__(MCL_BLOCK) k_history_ancestors(const u32* __restrict__ link, HistRing g, int lag,
                                                                 u32* __restrict__ out) {
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += gridDim.x * blockDim.x) {
    u32 a = link ? link[i] : i;
    for (int j = 0; j < lag; ++j) a = g.parent[(size_t)hist_frame(g, j) * g.n + a];
    out[i] = a;
  }
}
// the trajectory of ONE current slot over lags 0 ... lags - 1 (one wave; a diagnostic): lane 0 chases the slots into LDS,
// the wave copies the frames' x, y, yaw.  out: lags x 4 doubles (x, y, yaw, the slot as a double -- exact below 2^53)
__global__ void __launch_bounds__(MCL_WAVE) k_history_path(const u32* __restrict__ link, HistRing g, u32 slot, int lags,
                                                           double* __restrict__ out) {
  __shared__ u32 sl[HIST_MAX_DEPTH];
  if (threadIdx.x == 0) {
    u32 a = link ? link[slot] : slot;
    sl[0] = a;
    for (int j = 0; j + 1 < lags; ++j) {
      a = g.parent[(size_t)hist_frame(g, j) * g.n + a];
      sl[j + 1] = a;
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < lags; k += blockDim.x) {
    const double* f = g.xyw + (size_t)hist_frame(g, k) * 3 * g.n;
    const u32 a = sl[k];
    out[4 * k + 0] = f[a];
    out[4 * k + 1] = f[(size_t)g.n + a];
    out[4 * k + 2] = f[2 * (size_t)g.n + a];
    out[4 * k + 3] = (double)a;
  }
}
