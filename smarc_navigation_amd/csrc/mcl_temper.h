// mcl_temper.h -- kernels of ESS-targeted likelihood tempering (include/mcl_temper.h; gfx950, wave64, fp64):
//   k_temper_max    the largest finite log-weight and the number of finite ones, one record per workgroup
//   k_temper_sums   S1, S2 of every candidate level of a round: each log-weight read once, the candidates evaluated from
//                   registers, integer partials lane -> wave (DPP) -> workgroup (LDS) -> cloud (u64 atomic adds: exact)
//   k_temper_pick   one workgroup: round 0 reduces the maximum and plans round 1; rounds 1-3 compare the sums in 128
//                   bits, take the first pass and plan the next round -- all in device memory, no host round trip
//   k_temper_apply  lw <- beta_j lw, the level read from device memory (or given by the host)
// No floating-point addition anywhere in a reduction.  No scratch; LDS only for the reductions' words.
#pragma once
#include "mcl_kernels.h"
#include "mcl_host_pure.h"

// the state block (u64 words).  TP_NC ... TP_M are what a sums launch reads: one contiguous upload in the split form
#define TP_NC 0          // candidates of the round to run (0: nothing to do)
#define TP_CAND 1        // ... their levels [17]
#define TP_BETA 18       // ... their beta (double bits) [17]
#define TP_M 35          // m: the cloud's largest finite log-weight (double bits; -inf: none)
#define TP_PLAN_WORDS 36
#define TP_J 36          // the level so far / the result
#define TP_BETA_J 37     // beta of the result (double bits), written by the last pick
#define TP_DONE 38
#define TP_FLOOR 39
#define TP_LEVELS 40     // candidates evaluated so far
#define TP_NLIVE 41
#define TP_NT 42
#define TP_SUMS 48       // S1[17], then S2[17]: zero before every sums launch
#define TP_PART 96       // k_temper_max's records: (max bits, live) per workgroup
#define TP_WORDS (TP_PART + 2 * MCL_MAX_GRID)
#define TP_NCAND MCL_TEMPER_MAX_CAND
#define TP_SUMS_GRID 1024   // workgroups of a sums launch at most: 2 x 17 atomic adds each

__device__ __forceinline__ bool temper_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }   // (NaN: false)

__global__ void __launch_bounds__(MCL_BLOCK) k_temper_max(const double* __restrict__ lw, long long n, u64* __restrict__ st) {
  __shared__ double shd[16];
  __shared__ u64 shl[16];
  double m = -__builtin_inf();
  u64 live = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double x = lw[i];
    if (temper_finite(x)) {
      m = x > m ? x : m;
      ++live;
    }
  }
  m = block_max(m, shd, -__builtin_inf());
  live = block_sum(live, shl);
  if (threadIdx.x == 0) {
    st[TP_PART + 2 * blockIdx.x] = (u64)__double_as_longlong(m);
    st[TP_PART + 2 * blockIdx.x + 1] = live;
  }
}

// floor(det_exp(e) 2^32): det_exp(e) <= 1 for e <= 0, the scaling by 2^32 is exact, the conversion truncates
__device__ __forceinline__ u64 temper_q(double e) { return (u64)(det_exp(e) * 4294967296.0); }

__global__ void __launch_bounds__(MCL_BLOCK) k_temper_sums(const double* __restrict__ lw, long long n, u64* __restrict__ st) {
#pragma clang fp contract(off)
  __shared__ u64 sh[MCL_BLOCK / MCL_WAVE][2 * TP_NCAND];
  const int nc = (int)st[TP_NC];   // (wave-uniform: scalar loads)
  if (nc <= 0) return;
  const double m = __longlong_as_double((long long)st[TP_M]);
  const bool have_m = m > -__builtin_inf();
  double beta[TP_NCAND];
#pragma unroll
  for (int c = 0; c < TP_NCAND; ++c) beta[c] = __longlong_as_double((long long)st[TP_BETA + c]);
  u64 a1[TP_NCAND], a2[TP_NCAND];
#pragma unroll
  for (int c = 0; c < TP_NCAND; ++c) a1[c] = a2[c] = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double x = lw[i];
    if (!(have_m && temper_finite(x))) continue;
    double d = x - m;
    d = d < 0.0 ? d : 0.0;   // (a caller's maximum below a log-weight: that weight counts as the maximum)
#pragma unroll
    for (int c = 0; c < TP_NCAND; ++c) {
      if (c < nc) {   // (uniform)
        const double e = beta[c] * d;
        a1[c] += temper_q(e);
        a2[c] += temper_q(e + e);
      }
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < TP_NCAND; ++c) {
    const u64 t1 = wave_sum(a1[c]), t2 = wave_sum(a2[c]);   // (integers: in every lane)
    if (lane == 0) {
      sh[w][c] = t1;
      sh[w][TP_NCAND + c] = t2;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * TP_NCAND) {
    const int c = threadIdx.x % TP_NCAND;
    if (c < nc) {
      u64 t = 0;
#pragma unroll
      for (int k = 0; k < MCL_BLOCK / MCL_WAVE; ++k) t += sh[k][threadIdx.x];
      if (t) atomicAdd(reinterpret_cast<unsigned long long*>(st + TP_SUMS + threadIdx.x), t);
    }
  }
}

// round 0: after k_temper_max over `np` workgroups.  rounds 1 ... 3: after the sums launch of that round.
__global__ void __launch_bounds__(MCL_BLOCK) k_temper_pick(u64* __restrict__ st, int round, int np, long long n_target) {
  __shared__ double shd[16];
  __shared__ u64 shl[16];
  if (round == 0) {
    double m = -__builtin_inf();
    u64 live = 0;
    for (int p = threadIdx.x; p < np; p += blockDim.x) {
      const double v = __longlong_as_double((long long)st[TP_PART + 2 * p]);
      m = v > m ? v : m;
      live += st[TP_PART + 2 * p + 1];
    }
    m = block_max(m, shd, -__builtin_inf());
    live = block_sum(live, shl);
    if (threadIdx.x == 0) {
      st[TP_M] = (u64)__double_as_longlong(m);
      st[TP_NLIVE] = live;
      st[TP_NT] = (u64)n_target;
      st[TP_J] = 0;
      st[TP_BETA_J] = (u64)__double_as_longlong(1.0);
      st[TP_DONE] = 0;
      st[TP_FLOOR] = 0;
      st[TP_LEVELS] = 0;
    }
  }
  if (threadIdx.x != 0) return;
  int j = (int)st[TP_J];
  int done = (int)st[TP_DONE];
  if (round > 0 && !done) {
    const int nc = (int)st[TP_NC];
    int first = -1;
    for (int c = nc - 1; c >= 0; --c)
      if (temper_pass(st[TP_SUMS + c], st[TP_SUMS + TP_NCAND + c], (u64)n_target)) first = (int)st[TP_CAND + c];
    const TemperStep r = temper_next(round, j, first);
    j = r.j;
    done = r.done;
    st[TP_J] = (u64)j;
    st[TP_DONE] = (u64)done;
    st[TP_FLOOR] = st[TP_FLOOR] | (u64)r.floor_hit;
    st[TP_LEVELS] = st[TP_LEVELS] + (u64)nc;
    if (done) st[TP_BETA_J] = (u64)__double_as_longlong(temper_beta(j));
  }
  // the next round's plan, and zero sums for it
  TemperPlan p = {0, 0, 0};
  if (!done && round < 3) p = temper_plan(round + 1, j);
  st[TP_NC] = (u64)(p.count > 0 ? p.count : 0);
  for (int c = 0; c < TP_NCAND; ++c) {
    const bool on = c < p.count;
    const int lev = on ? p.base + p.step * c : 0;
    st[TP_CAND + c] = (u64)lev;
    st[TP_BETA + c] = (u64)__double_as_longlong(on ? temper_beta(lev) : 0.0);
    st[TP_SUMS + c] = 0;
    st[TP_SUMS + TP_NCAND + c] = 0;
  }
}

// st != nullptr: level and beta from the state block; else beta_host (the host knows j > 0)
__global__ void __launch_bounds__(MCL_BLOCK) k_temper_apply(double* __restrict__ lw, long long n, const u64* __restrict__ st,
                                                            double beta_host) {
#pragma clang fp contract(off)
  double beta = beta_host;
  if (st) {
    if (st[TP_J] == 0ull) return;   // (j = 0: not a bit changes)
    beta = __longlong_as_double((long long)st[TP_BETA_J]);
  }
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double x = lw[i];
    if (temper_finite(x)) lw[i] = beta * x;
  }
}
