// mcl_kld.h -- kernels of KLD-sampling across handles (include/mcl_kld.h; gfx950, wave64): the occupied cells of an
// (x, y, yaw) lattice as a bitmap (k_kld_mark, k_kld_count, k_kld_final) and the gather of mcl_resample_into
// (k_transfer_gather).  Streaming kernels; no scratch; LDS only for the reductions' words and the gather's bracket
// (KLD_LDS_BYTES at most).  What is counted is integer; the only atomics are non-returning ORs into the bitmap.
#pragma once
#include "mcl_modes.h"   // (ModeLattice, MODES_OUTSIDE: the lattice and the cell rule are those of mcl_pose_modes)

#define KLD_ROUNDS 4        // wave aggregation: distinct bitmap words a wave merges before its lanes OR one by one
#define KLD_LDS_BYTES 128   // the most LDS any kernel of this file uses (16 reduction words of 8 bytes)

// the cell of particle i by the rule of include/mcl_modes.h (subtraction, division, floor, each rounded on its own), or
// MODES_OUTSIDE.  The same statements as k_modes_hist.
__device__ __forceinline__ u32 kld_cell(const StatePtrs& s, long long i, const ModeLattice& g) {
#pragma clang fp contract(off)
  const double fx = __builtin_floor((s.c[0][i] - g.x0) / g.cell);
  const double fy = __builtin_floor((s.c[1][i] - g.y0) / g.cell);
  const double t = __builtin_floor((s.c[5][i] + MCL_PI) / g.dyaw);
  // (NaN fails every comparison; an infinite coordinate or quotient fails its upper bound)
  if (!(fx >= 0.0 && fx < (double)g.nx && fy >= 0.0 && fy < (double)g.ny && __builtin_fabs(t) < __builtin_inf()))
    return MODES_OUTSIDE;
  double m = t;
  if (!(t >= 0.0 && t < (double)g.n_yaw)) {   // floored modulo of an integer-valued double: fmod is exact
    m = fmod(t, (double)g.n_yaw);
    if (m < 0.0) m += (double)g.n_yaw;
  }
  return ((u32)(int)m * (u32)g.ny + (u32)(int)fy) * (u32)g.nx + (u32)(int)fx;
}

__device__ __forceinline__ u32 kld_wave_or(u32 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (u32)__shfl_xor((int)v, o, MCL_WAVE);
  return v;
}

// ------------------------------------------------------------------ mark
// One lane per particle; the 64 lanes of a wave walk the particles together (the loop bound is the wave's), so every
// ballot covers whole waves.  Cell c is bit c & 31 of word c >> 5.  The ORs are aggregated per wave the way k_modes_hist
// aggregates its adds: the first pending lane's word is read, a ballot finds the lanes on the same word, their masks are
// ORed across the wave and ONE lane issues a non-returning atomicOr, at most KLD_ROUNDS times; what is still pending then
// issues its own.  A tracking cloud (a million particles in a few dozen cells: one or two words) issues one or two
// atomics per wave; a wave of spatial neighbours shares its words too.  A round whose leader stood alone on its word
// tells a dispersed wave: it stops merging there (every lane ORs its own bit).  bits[] words past the lattice are never
// touched (c < n_cells by the bounds above).  The particles outside are counted by ballot, one record per workgroup.
__global__ void __launch_bounds__(MCL_BLOCK) k_kld_mark(StatePtrs s, long long n, ModeLattice g, u32* __restrict__ bits,
                                                        u64* __restrict__ block_outside) {
  const int lane = threadIdx.x & 63;
  u32 outside = 0;   // (wave-uniform)
  for (long long base = blockIdx.x * (long long)blockDim.x + (threadIdx.x & ~63); base < n;
       base += (long long)gridDim.x * blockDim.x) {
    const long long i = base + lane;
    const bool live = i < n;
    const u32 c = live ? kld_cell(s, i, g) : MODES_OUTSIDE;
    bool pending = c != MODES_OUTSIDE;
    outside += (u32)__popcll(__ballot(live && !pending));
    const u32 word = c >> 5, bit = 1u << (c & 31u);
    for (int r = 0; r < KLD_ROUNDS; ++r) {
      const u64 todo = __ballot(pending);
      if (!todo) break;
      const int leader = __ffsll((long long)todo) - 1;
      const u32 wl = (u32)__builtin_amdgcn_readlane((int)word, leader);
      const bool mine = pending && word == wl;
      const u64 group = __ballot(mine);
      const u32 mask = kld_wave_or(mine ? bit : 0u);
      if (lane == leader) atomicOr(&bits[wl], mask);
      pending = pending && !mine;
      if (group == (1ull << leader)) break;   // (wave-uniform: a dispersed wave)
    }
    if (pending) atomicOr(&bits[word], bit);
  }
  __shared__ u32 sh[MCL_BLOCK / MCL_WAVE];
  if (lane == 0) sh[threadIdx.x >> 6] = outside;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < MCL_BLOCK / MCL_WAVE; ++w) t += sh[w];
    block_outside[blockIdx.x] = t;
  }
}

// ------------------------------------------------------------------ count and clear
// Streams the bitmap's nvec 16-byte vectors (the words behind the lattice's last are zero and stay zero), popcounts them
// and writes zero back over every vector that holds a set bit: the bitmap is clean for the next call without a memset
// per call.  One count per workgroup, no atomics.
__global__ void __launch_bounds__(MCL_BLOCK) k_kld_count(uint4* __restrict__ bits, long long nvec,
                                                         u64* __restrict__ block_cnt) {
  __shared__ u64 sh[16];
  u64 acc = 0;
  for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < nvec; v += (long long)gridDim.x * blockDim.x) {
    const uint4 x = bits[v];
    if (x.x | x.y | x.z | x.w) {
      acc += (u64)(__popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w));
      bits[v] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = acc;
}
// out[b] = sum of the np[b] workgroup counts of row b (the scheme of k_count_final; workgroup 0: the outside counts of
// k_kld_mark, workgroup 1: the cell counts of k_kld_count)
__global__ void __launch_bounds__(MCL_BLOCK) k_kld_final(const u64* __restrict__ rec, int np0, int np1, u64* __restrict__ out) {
  __shared__ u64 sh[16];
  const u64* row = rec + (size_t)blockIdx.x * MCL_MAX_GRID;
  const int np = blockIdx.x == 0 ? np0 : np1;
  u64 acc = 0;
  for (int i = threadIdx.x; i < np; i += blockDim.x) acc += row[i];
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// ------------------------------------------------------------------ the gather of mcl_resample_into
// ncum[j] = offspring CDF of src's N particles for M positions (k_offspring_cdf with M for the particle count):
// idx_i = min{ j : ncum[j] > i }.  One lane per output slot.  A workgroup's slots [i0, i1) have their ancestors in
// [idx(i0), idx(i1 - 1)]: two lanes of the first wave find that bracket with a binary search each over all of ncum and
// leave it in LDS; every lane then searches inside it (for M >= N the bracket is at most the workgroup's width), copies
// its six -- with DRIFT nine -- doubles and writes idx_i.  A CDF that never exceeds i (no weight at all) ends at N - 1.
struct TransferArgs {
  StatePtrs src, dst;
  const double* sdrift[3];   // DRIFT: src's cx, cy, bw
  double* ddrift[3];         // ... dst's
  const u32* ncum;
  long long n_src, m;
  int* idx;                  // m: out
};
__device__ __forceinline__ long long transfer_search(const u32* __restrict__ ncum, long long lo, long long hi, u32 i) {
  while (lo < hi) {   // min j in [lo, hi] with ncum[j] > i, or hi
    const long long mid = lo + ((hi - lo) >> 1);
    if (ncum[mid] > i)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}
template <bool DRIFT>
__global__ void __launch_bounds__(MCL_BLOCK) k_transfer_gather(TransferArgs a) {
  __shared__ long long br[2];
  for (long long base = blockIdx.x * (long long)blockDim.x; base < a.m; base += (long long)gridDim.x * blockDim.x) {
    const long long last = (base + blockDim.x < a.m ? base + blockDim.x : a.m) - 1;
    if (threadIdx.x < 2) br[threadIdx.x] = transfer_search(a.ncum, 0, a.n_src - 1, (u32)(threadIdx.x == 0 ? base : last));
    __syncthreads();
    const long long i = base + threadIdx.x;
    if (i < a.m) {
      const long long j = transfer_search(a.ncum, br[0], br[1], (u32)i);
#pragma unroll
      for (int c = 0; c < 6; ++c) a.dst.c[c][i] = a.src.c[c][j];
      if (DRIFT) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.ddrift[c][i] = a.sdrift[c][j];
      }
      a.idx[i] = (int)j;
    }
    __syncthreads();   // (br is rewritten by the next pass)
  }
}
