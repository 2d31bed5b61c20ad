// mcl_modes.h -- kernels of mcl_pose_modes (include/mcl_modes.h; gfx950, wave64): the (x, y, yaw) histogram of the cloud,
// its 3 x 3 x 3 window score with the greedy peak selection, and the moments of the particles inside each peak's window.
// Streaming kernels; no scratch; LDS only for the reductions' words.  Everything that decides WHICH cells are peaks is
// integer (u32 counts, integer atomics: the order of the adds cannot matter); the floating-point sums are a fixed tree.
#pragma once
#include "mcl_kernels.h"

#define MODES_OUTSIDE 0xffffffffu   // cell id of a particle that belongs to no cell
#define MODES_MAX_K 8               // MCL_MODES_MAX
#define MODES_SUMS 11               // count, dx, dy, z, roll, pitch, sin, cos, dx dx, dx dy, dy dy
#define MODES_ROUNDS 8              // wave aggregation: distinct cells a wave merges before its lanes add one by one
#define MODES_RES_WORDS 120         // result block (doubles): MODES_MAX_K x MODES_SUMS sums | the peaks | n_outside
#define MODES_RES_PEAKS 88
#define MODES_RES_OUTSIDE 112

struct ModeLattice {
  double x0, y0, cell, dyaw;   // dyaw = (2 pi) / n_yaw, formed once on the host
  int nx, ny, n_yaw;
};
struct ModePeak {
  u32 score, c;   // score 0: no peak (selection has stopped)
  int ix, iy, iyaw;
  int pad;
};
static_assert(sizeof(ModePeak) == 24 && MODES_RES_PEAKS + MODES_MAX_K * sizeof(ModePeak) / 8 == MODES_RES_OUTSIDE &&
                  MODES_MAX_K * MODES_SUMS == MODES_RES_PEAKS && MODES_RES_OUTSIDE < MODES_RES_WORDS,
              "layout of the result block");

__device__ __forceinline__ int modes_circ_dist(int a, int b, int n_yaw) {
  const int d = a > b ? a - b : b - a;
  return d < n_yaw - d ? d : n_yaw - d;
}
// (ix, iy, iyaw) of the linear cell id c = (iyaw ny + iy) nx + ix
__device__ __forceinline__ void modes_decode(u32 c, int nx, int ny, int& ix, int& iy, int& iyaw) {
  const u32 r = c / (u32)nx;
  ix = (int)(c - r * (u32)nx);
  iyaw = (int)(r / (u32)ny);
  iy = (int)(r - (u32)iyaw * (u32)ny);
}
// score and cell of a selection key: the larger score wins, then the LOWER cell id
__device__ __forceinline__ u64 modes_key(u32 score, u32 c) { return ((u64)score << 32) | (u64)(0xffffffffu - c); }

// ------------------------------------------------------------------ histogram
// One lane per particle; the 64 lanes of a wave walk the particles together (the loop bound is the wave's), so every
// ballot below covers whole waves.  The cell rule of include/mcl_modes.h: subtraction, division, floor, each rounded on its
// own.  cell_id[i] keeps the particle's cell for the moments pass.
// The adds into H are aggregated per wave first: the first pending lane's cell is read, a ballot finds the lanes in the
// same cell, ONE lane adds their number, at most MODES_ROUNDS times; what is still pending then adds 1 per lane.  A
// tracking cloud (a million particles in a few dozen cells) issues a handful of atomics per wave instead of 64 on a few
// addresses.  The particles outside are counted by ballot per wave, four LDS words, one record per workgroup.
__global__ void __launch_bounds__(MCL_BLOCK) k_modes_hist(StatePtrs s, long long n, ModeLattice g,
                                                          u32* __restrict__ cell_id, u32* __restrict__ H,
                                                          u64* __restrict__ block_outside) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  u32 outside = 0;   // (wave-uniform)
  for (long long base = blockIdx.x * (long long)blockDim.x + (threadIdx.x & ~63); base < n;
       base += (long long)gridDim.x * blockDim.x) {
    const long long i = base + lane;
    const bool live = i < n;
    u32 c = MODES_OUTSIDE;
    if (live) {
      const double fx = __builtin_floor((s.c[0][i] - g.x0) / g.cell);
      const double fy = __builtin_floor((s.c[1][i] - g.y0) / g.cell);
      const double t = __builtin_floor((s.c[5][i] + MCL_PI) / g.dyaw);
      // (NaN fails every comparison; an infinite coordinate or quotient fails its upper bound)
      if (fx >= 0.0 && fx < (double)g.nx && fy >= 0.0 && fy < (double)g.ny && __builtin_fabs(t) < __builtin_inf()) {
        double m = t;
        if (!(t >= 0.0 && t < (double)g.n_yaw)) {   // floored modulo of an integer-valued double: fmod is exact
          m = fmod(t, (double)g.n_yaw);
          if (m < 0.0) m += (double)g.n_yaw;
        }
        c = ((u32)(int)m * (u32)g.ny + (u32)(int)fy) * (u32)g.nx + (u32)(int)fx;
      }
      cell_id[i] = c;
    }
    bool pending = c != MODES_OUTSIDE;
    outside += (u32)__popcll(__ballot(live && !pending));
    for (int r = 0; r < MODES_ROUNDS; ++r) {
      const u64 todo = __ballot(pending);
      if (!todo) break;
      const int leader = __ffsll((long long)todo) - 1;
      const u32 cl = (u32)__builtin_amdgcn_readlane((int)c, leader);
      const bool mine = pending && c == cl;
      const u32 cnt = (u32)__popcll(__ballot(mine));
      if (lane == leader) atomicAdd(&H[cl], cnt);
      pending = pending && !mine;
    }
    if (pending) atomicAdd(&H[c], 1u);
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

// ------------------------------------------------------------------ score and peak selection
// S[c] = sum of H over the window of c, written densely (n_cells words: the later selection rounds read S alone), and
// the first round's per-workgroup best {score, lowest c} -- nothing is suppressed yet.
__global__ void __launch_bounds__(MCL_BLOCK) k_modes_score(const u32* __restrict__ H, int nx, int ny, int n_yaw,
                                                           u32 n_cells, u32* __restrict__ S, u64* __restrict__ rec) {
  __shared__ u64 sh[16];
  // the yaw bins at circular distance <= 1 as a set: n_yaw >= 3: {-1, 0, +1}; 2: {0, +1}; 1: {0}
  const int w_lo = n_yaw >= 3 ? -1 : 0, w_hi = n_yaw >= 2 ? 1 : 0;
  u64 best = 0;
  for (u32 c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cells; c += gridDim.x * blockDim.x) {
    int ix, iy, iyaw;
    modes_decode(c, nx, ny, ix, iy, iyaw);
    const int x_lo = ix > 0 ? ix - 1 : 0, x_hi = ix + 1 < nx ? ix + 1 : nx - 1;
    const int y_lo = iy > 0 ? iy - 1 : 0, y_hi = iy + 1 < ny ? iy + 1 : ny - 1;
    u32 sum = 0;
    for (int dw = w_lo; dw <= w_hi; ++dw) {
      int w = iyaw + dw;
      w = w < 0 ? w + n_yaw : (w >= n_yaw ? w - n_yaw : w);
      for (int y = y_lo; y <= y_hi; ++y) {
        const u32* row = H + ((size_t)w * ny + y) * nx;
        for (int x = x_lo; x <= x_hi; ++x) sum += row[x];
      }
    }
    S[c] = sum;
    const u64 key = modes_key(sum, c);
    if (sum != 0u && key > best) best = key;
  }
  best = block_max(best, sh, (u64)0);
  if (threadIdx.x == 0) rec[blockIdx.x] = best;
}
// round m >= 1: the best cell outside the suppression regions (Chebyshev distance <= 2 in ix, iy, circular iyaw) of the
// m peaks found so far -- they lie in device memory, where k_modes_peak_final left them: no host round trip per round
__global__ void __launch_bounds__(MCL_BLOCK) k_modes_peak_partial(const u32* __restrict__ S, int nx, int ny, int n_yaw,
                                                                  u32 n_cells, const ModePeak* __restrict__ peaks, int m,
                                                                  u64* __restrict__ rec) {
  __shared__ u64 sh[16];
  __shared__ int pk[MODES_MAX_K][3];
  __shared__ int npk;
  if (threadIdx.x == 0) {
    int k = 0;
    for (int p = 0; p < m; ++p)
      if (peaks[p].score != 0u) {
        pk[k][0] = peaks[p].ix;
        pk[k][1] = peaks[p].iy;
        pk[k][2] = peaks[p].iyaw;
        ++k;
      }
    npk = k;
  }
  __syncthreads();
  const int np = npk;
  u64 best = 0;
  for (u32 c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cells; c += gridDim.x * blockDim.x) {
    const u32 sc = S[c];
    const u64 key = modes_key(sc, c);
    if (sc == 0u || key <= best) continue;   // (only a cell that would win is worth decoding)
    int ix, iy, iyaw;
    modes_decode(c, nx, ny, ix, iy, iyaw);
    bool free_cell = true;
    for (int p = 0; p < np; ++p) {
      const int dx = ix - pk[p][0], dy = iy - pk[p][1];
      if (dx >= -2 && dx <= 2 && dy >= -2 && dy <= 2 && modes_circ_dist(iyaw, pk[p][2], n_yaw) <= 2) free_cell = false;
    }
    if (free_cell) best = key;
  }
  best = block_max(best, sh, (u64)0);
  if (threadIdx.x == 0) rec[blockIdx.x] = best;
}
// one workgroup: the best of the np workgroup records becomes peak m (score 0: nothing left)
__global__ void __launch_bounds__(MCL_BLOCK) k_modes_peak_final(const u64* __restrict__ rec, int np, int nx, int ny,
                                                                ModePeak* __restrict__ peaks, int m) {
  __shared__ u64 sh[16];
  u64 best = 0;
  for (int i = threadIdx.x; i < np; i += blockDim.x) best = rec[i] > best ? rec[i] : best;
  best = block_max(best, sh, (u64)0);
  if (threadIdx.x == 0) {
    ModePeak p;
    p.score = (u32)(best >> 32);
    p.c = p.score ? 0xffffffffu - (u32)best : 0u;
    modes_decode(p.c, nx, ny, p.ix, p.iy, p.iyaw);
    p.pad = 0;
    peaks[m] = p;
  }
}

// ------------------------------------------------------------------ moments
// One pass over the particles with the stored cell ids.  A particle lies in at most one window (the windows are
// disjoint).  The sums are the fixed tree of mcl_device.h, row m * MODES_SUMS + j for term j of mode m: per wave
// iteration and per mode that has a particle in the wave, the eleven terms, zero in the lanes outside that mode's window.
__global__ void __launch_bounds__(MCL_BLOCK) k_modes_moments(StatePtrs s, long long n, const u32* __restrict__ cell_id,
                                                             ModeLattice g, const ModePeak* __restrict__ peaks, int k,
                                                             double* __restrict__ part /*[k][MODES_SUMS][grid]*/) {
#pragma clang fp contract(off)
  __shared__ double acc[MCL_BLOCK / MCL_WAVE][MODES_MAX_K * MODES_SUMS];
  __shared__ int pk[MODES_MAX_K][4];      // ix, iy, iyaw, score != 0
  __shared__ double ctr[MODES_MAX_K][2];  // the peak cell's centre
  const int lane = threadIdx.x & 63;
  tree_zero(acc);
  if (threadIdx.x < k) {
    const ModePeak p = peaks[threadIdx.x];
    pk[threadIdx.x][0] = p.ix;
    pk[threadIdx.x][1] = p.iy;
    pk[threadIdx.x][2] = p.iyaw;
    pk[threadIdx.x][3] = p.score != 0u;
    ctr[threadIdx.x][0] = g.x0 + ((double)p.ix + 0.5) * g.cell;
    ctr[threadIdx.x][1] = g.y0 + ((double)p.iy + 0.5) * g.cell;
  }
  __syncthreads();   // (pk, ctr.  A barrier of its own: with the peaks set up ahead of tree_zero's, 83 VGPRs instead of 62)
  for (long long base = blockIdx.x * (long long)blockDim.x + (threadIdx.x & ~63); base < n;
       base += (long long)gridDim.x * blockDim.x) {
    const long long i = base + lane;
    const u32 c = i < n ? cell_id[i] : MODES_OUTSIDE;
    int mode = -1;
    if (c != MODES_OUTSIDE) {
      int ix, iy, iyaw;
      modes_decode(c, g.nx, g.ny, ix, iy, iyaw);
      for (int m = 0; m < k; ++m) {
        const int dx = ix - pk[m][0], dy = iy - pk[m][1];
        if (pk[m][3] && dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1 && modes_circ_dist(iyaw, pk[m][2], g.n_yaw) <= 1) mode = m;
      }
    }
    if (!__ballot(mode >= 0)) continue;
    // the seven terms the eleven are made of (the three products are formed where they are summed: fewer live registers)
    double b[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (mode >= 0) {
      sincos(s.c[5][i], &b[5], &b[6]);
      b[0] = s.c[0][i] - ctr[mode][0];
      b[1] = s.c[1][i] - ctr[mode][1];
      b[2] = s.c[2][i];
      b[3] = s.c[3][i];
      b[4] = s.c[4][i];
    }
    for (int m = 0; m < k; ++m) {
      if (!__ballot(mode == m)) continue;
      const bool in = mode == m;
#pragma unroll
      for (int j = 0; j < MODES_SUMS; ++j) {
        const double t = j == 0 ? 1.0 : (j < 8 ? b[j - 1] : (j == 8 ? b[0] * b[0] : (j == 9 ? b[0] * b[1] : b[1] * b[1])));
        tree_add(acc, m * MODES_SUMS + j, in ? t : 0.0);
      }
    }
  }
  tree_flush(acc, k * MODES_SUMS, part);
}
