// mcl_quantile.h -- kernels of the exact order statistics (include/mcl_quantile.h; gfx950, wave64, fp64): a
// most-significant-byte-first radix select over order-preserving 64-bit keys with integer masses.
//   k_quant_range   smallest and largest key, used particles and (weighted) the largest finite log-weight: one record per
//                   workgroup
//   k_quant_plan    one workgroup: reduces the records, skips the leading bytes every key shares (quant_start) and writes
//                   the plan of the first round that runs
//   k_quant_hist    a round: the next 8 key bits of the particles that match a probability's prefix, masses added per wave
//                   (ballot), per workgroup (LDS, u64) and per cloud (global, u64): integer atomics only
//   k_quant_pick    one workgroup: each probability's bin -- the first whose cumulative mass reaches its threshold, a
//                   128-bit compare -- and the next round's prefixes, all in device memory: no host round trip
//   k_quant_mass    the inverse question: the mass at or below up to eight given keys, in one pass
// The keys are recomputed from the state in every round (8 or 16 bytes per particle and round); nothing of
// the particle count is stored.  No floating-point atomics, no floating-point sums.  No scratch.
#pragma once
#include "mcl_kernels.h"
#include "mcl_host_pure.h"

#define QUANT_MAX_P MCL_QUANTILE_MAX
#define QUANT_BINS 256
// the state block (u64 words)
#define QS_NP 0          // probabilities of the call
#define QS_START 1       // the first round that runs (rounds below it return at once)
#define QS_M 2           // m: the cloud's largest finite log-weight (double bits; -inf: none)
#define QS_NUSED 3       // particles whose value is not NaN
#define QS_S 4           // S, known after the first round that runs
#define QS_KMIN 5
#define QS_KMAX 6
#define QS_P 8           // [8] the thresholds
#define QS_PREFIX 16     // [8] the key bytes found so far
#define QS_BELOW 24      // [8] the mass of the keys below the prefix's range
#define QS_MK 32         // [8] the cumulative mass up to and including the picked bin: M(K) after the last round
#define QS_ROW 40        // [8] the histogram row a probability reads: the first probability with the same prefix
#define QS_MASS 48       // k_quant_mass: [8] masses, then the total, then the used count
#define QS_HEAD 64       // what the host reads back
#define QS_HIST 64       // [8][256] the rounds' histograms: zero before every k_quant_hist
#define QS_PART (QS_HIST + QUANT_MAX_P * QUANT_BINS)   // k_quant_range's records: kmin, kmax, used, max lw bits
#define QS_WORDS (QS_PART + 4 * MCL_MAX_GRID)
#define QUANT_GRID 1024        // workgroups of a hist / mass launch at most
#define QUANT_AGG_ROUNDS 4     // wave aggregation: groups of lanes in one bin a wave merges before its lanes add one by one
#define QUANT_AGG_MIN 8        // ... a group smaller than this is not worth a merge

struct QuantQuery {
  int quantity, weighted;
  double cx, cy, cyaw;
};
struct QuantWords {
  u64 w[QUANT_MAX_P];
};

// the quantity of particle i (include/mcl_quantile.h): every operation rounded on its own
__device__ __forceinline__ double quant_quantity(const StatePtrs& s, long long i, const QuantQuery& q) {
#pragma clang fp contract(off)
  if (q.quantity == MCL_Q_X) return s.c[0][i];
  if (q.quantity == MCL_Q_Y) return s.c[1][i];
  if (q.quantity == MCL_Q_RADIUS2) {
    const double dx = s.c[0][i] - q.cx, dy = s.c[1][i] - q.cy;
    const double a = dx * dx, b = dy * dy;
    return a + b;
  }
  const double d = wrap_pi(s.c[5][i] - q.cyaw);
  return q.quantity == MCL_Q_ABS_YAW_DEV ? __builtin_fabs(d) : d;
}
// floor(det_exp(lw - m) 2^32): q1 of csrc/mcl_temper.h at level 0 (beta = 1: the product with it changes no bit)
__device__ __forceinline__ u64 quant_mass(double lw, double m, bool have_m) {
#pragma clang fp contract(off)
  if (!(have_m && __builtin_fabs(lw) < __builtin_inf())) return 0ull;   // (NaN: false)
  double d = lw - m;
  d = d < 0.0 ? d : 0.0;   // (a caller's maximum below a log-weight: that weight counts as the maximum)
  return (u64)(det_exp(d) * 4294967296.0);
}

// ------------------------------------------------------------------ range
template <bool W>
__global__ void __launch_bounds__(MCL_BLOCK) k_quant_range(StatePtrs s, const double* __restrict__ lw, long long n, QuantQuery q,
                                                           u64* __restrict__ st) {
  __shared__ u64 sh[16];
  __shared__ double shd[16];
  u64 kmax = 0ull, nkmin = 0ull, used = 0ull;   // (nkmin = ~kmin: one max reduction serves both)
  double m = -__builtin_inf();
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double v = quant_quantity(s, i, q);
    if (v == v) {
      const u64 k = quant_key(v);
      kmax = k > kmax ? k : kmax;
      nkmin = ~k > nkmin ? ~k : nkmin;
      ++used;
    }
    if (W) {
      const double x = lw[i];
      if (__builtin_fabs(x) < __builtin_inf()) m = x > m ? x : m;
    }
  }
  kmax = block_max(kmax, sh, (u64)0);
  nkmin = block_max(nkmin, sh, (u64)0);
  used = block_sum(used, sh);
  if (W) m = block_max(m, shd, -__builtin_inf());
  if (threadIdx.x == 0) {
    u64* rec = st + QS_PART + 4 * blockIdx.x;
    rec[0] = ~nkmin;
    rec[1] = kmax;
    rec[2] = used;
    rec[3] = (u64)__double_as_longlong(m);
  }
}

// one workgroup, after k_quant_range over `np` workgroups
__global__ void __launch_bounds__(MCL_BLOCK) k_quant_plan(u64* __restrict__ st, int np, int n_probs, QuantWords P) {
  __shared__ u64 sh[16];
  __shared__ double shd[16];
  u64 kmax = 0ull, nkmin = 0ull, used = 0ull;
  double m = -__builtin_inf();
  for (int p = threadIdx.x; p < np; p += blockDim.x) {
    const u64* rec = st + QS_PART + 4 * p;
    nkmin = ~rec[0] > nkmin ? ~rec[0] : nkmin;
    kmax = rec[1] > kmax ? rec[1] : kmax;
    used += rec[2];
    const double v = __longlong_as_double((long long)rec[3]);
    m = v > m ? v : m;
  }
  kmax = block_max(kmax, sh, (u64)0);
  nkmin = block_max(nkmin, sh, (u64)0);
  used = block_sum(used, sh);
  m = block_max(m, shd, -__builtin_inf());
  for (int t = threadIdx.x; t < QUANT_MAX_P * QUANT_BINS; t += blockDim.x) st[QS_HIST + t] = 0ull;
  if (threadIdx.x == 0) {
    const QuantStart g = quant_start(~nkmin, kmax);
    st[QS_NP] = (u64)n_probs;
    st[QS_START] = (u64)g.start;
    st[QS_M] = (u64)__double_as_longlong(m);
    st[QS_NUSED] = used;
    st[QS_S] = 0ull;
    st[QS_KMIN] = ~nkmin;
    st[QS_KMAX] = kmax;
    for (int j = 0; j < QUANT_MAX_P; ++j) {
      st[QS_P + j] = P.w[j];
      st[QS_PREFIX + j] = g.prefix;
      st[QS_BELOW + j] = 0ull;
      st[QS_MK + j] = 0ull;
      st[QS_ROW + j] = 0ull;   // (every probability shares the first round's prefix: one row)
    }
  }
}

// ------------------------------------------------------------------ a round's histogram
// One lane per particle; the 64 lanes of a wave walk the particles together, so every ballot covers whole waves.  Per
// probability that owns a row (QS_ROW[j] == j: no earlier probability has the same prefix) the lanes whose key matches the
// prefix add their mass to LDS row j at the key's next 8 bits.  On a converged cloud most lanes of a wave land in ONE bin
// in the first rounds that run: the first pending lane's bin is read, a ballot finds the lanes in the same bin, and when
// they are QUANT_AGG_MIN or more ONE lane adds their summed mass (unweighted: their number), at most QUANT_AGG_ROUNDS
// times; what is still pending adds lane by lane.  The workgroup's nonzero bins are then added to the cloud's.
template <bool W>
__global__ void __launch_bounds__(MCL_BLOCK) k_quant_hist(StatePtrs s, const double* __restrict__ lw, long long n, QuantQuery q,
                                                          int round, u64* __restrict__ st) {
  __shared__ u64 H[QUANT_MAX_P][QUANT_BINS];
  if (round < (int)st[QS_START]) return;   // (uniform over the launch)
  const int np = (int)st[QS_NP];
  const double m = __longlong_as_double((long long)st[QS_M]);
  const bool have_m = m > -__builtin_inf();
  u64 prefix[QUANT_MAX_P];
  bool own[QUANT_MAX_P];
#pragma unroll
  for (int j = 0; j < QUANT_MAX_P; ++j) {
    prefix[j] = st[QS_PREFIX + j];
    own[j] = j < np && (int)st[QS_ROW + j] == j;
  }
  for (int t = threadIdx.x; t < np * QUANT_BINS; t += blockDim.x) (&H[0][0])[t] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int shift = 56 - 8 * round;
  for (long long base = blockIdx.x * (long long)blockDim.x + (threadIdx.x & ~63); base < n;
       base += (long long)gridDim.x * blockDim.x) {
    const long long i = base + lane;
    bool used = false;
    u64 key = 0ull, mass = 1ull;
    if (i < n) {
      const double v = quant_quantity(s, i, q);
      used = v == v;
      key = quant_key(v);
      if (W) {
        mass = quant_mass(lw[i], m, have_m);
        used = used && mass != 0ull;   // (a particle without mass adds nothing to any bin)
      }
    }
    const u64 hi = round == 0 ? 0ull : key >> (shift + 8);
    const u32 digit = (u32)(key >> shift) & 255u;
#pragma unroll
    for (int j = 0; j < QUANT_MAX_P; ++j) {
      if (!own[j]) continue;   // (uniform)
      bool pending = used && hi == prefix[j];
      for (int r = 0; r < QUANT_AGG_ROUNDS; ++r) {
        const u64 todo = __ballot(pending);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const u32 dl = (u32)__builtin_amdgcn_readlane((int)digit, leader);
        const bool mine = pending && digit == dl;
        const u64 group = __ballot(mine);
        if (__popcll(group) < QUANT_AGG_MIN) break;
        const u64 sum = W ? wave_sum(mine ? mass : 0ull) : (u64)__popcll(group);
        if (lane == leader) atomicAdd(&H[j][dl], sum);
        pending = pending && !mine;
      }
      if (pending) atomicAdd(&H[j][digit], mass);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < np * QUANT_BINS; t += blockDim.x) {
    const u64 v = (&H[0][0])[t];
    if (v) atomicAdd(st + QS_HIST + t, v);
  }
}

// one workgroup, four waves: wave w picks the bins of probabilities w and w + 4; a lane holds four consecutive bins
__global__ void __launch_bounds__(MCL_BLOCK) k_quant_pick(u64* __restrict__ st, int round) {
  const int start = (int)st[QS_START];
  if (round < start) return;   // (uniform over the workgroup)
  const int np = (int)st[QS_NP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = wv; j < np; j += MCL_BLOCK / MCL_WAVE) {
    const u64* row = st + QS_HIST + (size_t)st[QS_ROW + j] * QUANT_BINS + 4 * lane;
    const u64 h0 = row[0], h1 = row[1], h2 = row[2], h3 = row[3];
    const u64 incl = wave_scan_incl(h0 + h1 + h2 + h3);
    // the first round that runs sees every used particle in its one row: the row's sum is S
    const u64 S = round == start ? readlane63(incl) : st[QS_S];
    const u64 P = st[QS_P + j];
    const u64 c0 = st[QS_BELOW + j] + (incl - (h0 + h1 + h2 + h3)) + h0, c1 = c0 + h1, c2 = c1 + h2, c3 = c2 + h3;
    const int first = S == 0ull               ? -1
                      : quant_reached(c0, S, P) ? 0
                      : quant_reached(c1, S, P) ? 1
                      : quant_reached(c2, S, P) ? 2
                      : quant_reached(c3, S, P) ? 3
                                                : -1;
    const u64 hit = __ballot(first >= 0);
    u64 bin = 0ull, cum = 0ull, below = 0ull;
    if (hit) {   // (always, unless S = 0: the last bin's cumulative mass is S and P <= 2^32)
      const int l = __ffsll((long long)hit) - 1;
      const int f = __builtin_amdgcn_readlane(first, l);
      cum = read_lane(f == 0 ? c0 : (f == 1 ? c1 : (f == 2 ? c2 : c3)), l);
      below = cum - read_lane(f == 0 ? h0 : (f == 1 ? h1 : (f == 2 ? h2 : h3)), l);
      bin = (u64)(4 * l + f);
    }
    if (lane == 0) {
      if (j == 0 && round == start) st[QS_S] = S;
      st[QS_PREFIX + j] = (st[QS_PREFIX + j] << 8) | bin;
      st[QS_BELOW + j] = below;
      st[QS_MK + j] = cum;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < np * QUANT_BINS; t += blockDim.x) st[QS_HIST + t] = 0ull;
  if (threadIdx.x == 0)
    for (int j = 0; j < np; ++j) {
      int r = j;
      for (int k = j - 1; k >= 0; --k)
        if (st[QS_PREFIX + k] == st[QS_PREFIX + j]) r = k;
      st[QS_ROW + j] = (u64)r;
    }
}

// ------------------------------------------------------------------ the mass at or below given keys
// st[QS_MASS ...] zero before the launch.  Integer partials lane -> wave (DPP) -> workgroup (LDS) -> cloud (u64 atomics).
template <bool W>
__global__ void __launch_bounds__(MCL_BLOCK) k_quant_mass(StatePtrs s, const double* __restrict__ lw, long long n, QuantQuery q,
                                                          double m, QuantWords keys, int nv, u64* __restrict__ st) {
  __shared__ u64 sh[MCL_BLOCK / MCL_WAVE][QUANT_MAX_P + 2];
  const bool have_m = m > -__builtin_inf();
  u64 a[QUANT_MAX_P + 2];
#pragma unroll
  for (int c = 0; c < QUANT_MAX_P + 2; ++c) a[c] = 0ull;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double v = quant_quantity(s, i, q);
    if (!(v == v)) continue;
    const u64 key = quant_key(v);
    const u64 mass = W ? quant_mass(lw[i], m, have_m) : 1ull;
#pragma unroll
    for (int c = 0; c < QUANT_MAX_P; ++c)
      if (c < nv && key <= keys.w[c]) a[c] += mass;
    a[QUANT_MAX_P] += mass;
    a[QUANT_MAX_P + 1] += 1ull;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < QUANT_MAX_P + 2; ++c) {
    const u64 t = wave_sum(a[c]);
    if (lane == 0) sh[wv][c] = t;
  }
  __syncthreads();
  if (threadIdx.x < QUANT_MAX_P + 2) {
    u64 t = 0ull;
#pragma unroll
    for (int k = 0; k < MCL_BLOCK / MCL_WAVE; ++k) t += sh[k][threadIdx.x];
    if (t) atomicAdd(st + QS_MASS + threadIdx.x, t);
  }
}
