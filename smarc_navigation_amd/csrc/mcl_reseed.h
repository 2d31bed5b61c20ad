// mcl_reseed.h -- kernel of the sensor resetting (include/mcl_reseed.h; gfx950, wave64, fp64): k_inject_gaussian replaces
// the particles a selection draw picks by draws from a mixture of at most 256 Gaussians over (x, y, yaw).
//   One lane per particle over a grid stride, as k_uniform_state<true> (csrc/mcl_recovery.h), whose counting scheme it
//   shares: ballot counts per wave, added in LDS, one word per workgroup for k_count_final.  No atomics, no scratch.
//   The component table lives in LDS: every lane looks up ITS OWN component, a divergent read that the scalar cache cannot
//   serve and that would cost a vector-memory round trip per word from global memory.  The host uploads it in the layout
//   the kernel keeps it in -- nine rows (mean x, y, yaw; L00, L10, L11, L20, L21, L22) of RESEED_ROW doubles, one column
//   per component (structure of arrays: lanes with different components read different banks; records of 72 bytes would
//   stride the banks by 18), then RESEED_ROW prefix sums `cum` as 32-bit words, padded with W -- and every workgroup copies
//   the used columns with 16-byte loads, then waits at ONE barrier before the first use.  RESEED_LDS_BYTES = 19 472 bytes:
//   eight workgroups of four waves fit a CU's 160 KiB, which is the 32-waves-per-CU cap -- the table costs no occupancy.
//   The component is found by a binary search over the 256 words of cum: eight steps, no branch, the same trip count
//   in every lane.  Philox block 1 and the Box-Muller pair are evaluated under the selection only: a lane whose
//   u_select >= fraction neither draws its normals nor touches the state.
#pragma once
#include "mcl_kernels.h"
#include "mcl_host_pure.h"
#include "mcl_recovery.h"

#define RESEED_ROW MCL_RESEED_MAX_COMPONENTS
#define RESEED_ROWS 9   // mean[3], chol[6]
#define RESEED_TAB_BYTES (RESEED_ROWS * RESEED_ROW * 8 + RESEED_ROW * 4)   // what the host uploads: 19 456
#define RESEED_TAB_WORDS (RESEED_TAB_BYTES / 8)
// the kernel's whole LDS: the table and the four wave counts (tests/test_reseed_isa.py holds the code object to it)
#define RESEED_LDS_BYTES (RESEED_TAB_BYTES + 16)

struct ReseedArgs {
  u32 k0, k1, step;    // Philox key (seed) and counter word 2; the purpose is 9
  int n_comp;          // 1 ... 256
  long long gid0;      // global id of local particle 0
  double fraction;     // particle replaced iff u_select < fraction
  u64 W;               // sum of the masses, 1 ... 2^31
};

// replay: n x 5 doubles (u_select, u_comp, xi_0, xi_1, xi_2), particle-major, or nullptr (Philox, purpose 9).
// tab: RESEED_TAB_BYTES, 16-byte aligned.  block_cnt[blockIdx.x]: the particles this workgroup replaced.
__global__ void __launch_bounds__(MCL_BLOCK) k_inject_gaussian(StatePtrs s, long long n, ReseedArgs a,
                                                               const double* __restrict__ tab,
                                                               const double* __restrict__ replay,
                                                               u64* __restrict__ block_cnt) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double sh_tab[RESEED_TAB_WORDS];
  __shared__ u32 sh_cnt[MCL_BLOCK / MCL_WAVE];
  {
    // the used columns of the nine rows (two doubles per load), then all of cum (four words per load)
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(tab);
    uint4* dst = reinterpret_cast<uint4*>(sh_tab);
    const int half = (a.n_comp + 1) >> 1;
    for (int k = threadIdx.x; k < RESEED_ROWS * half; k += MCL_BLOCK) {
      const int row = k / half, j = k - row * half;
      dst[row * (RESEED_ROW / 2) + j] = src[row * (RESEED_ROW / 2) + j];
    }
    constexpr int CUM0 = RESEED_ROWS * RESEED_ROW / 2;   // (in 16-byte units)
    for (int k = threadIdx.x; k < RESEED_ROW / 4; k += MCL_BLOCK) dst[CUM0 + k] = src[CUM0 + k];
  }
  __syncthreads();
  const u32* cum = reinterpret_cast<const u32*>(sh_tab + RESEED_ROWS * RESEED_ROW);
  u32 cnt = 0;   // (wave-uniform among the lanes still in the loop; lane 0 leaves last)
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const u32 gid = (u32)(a.gid0 + i);
    double u_select;
    u64 t;
    if (replay) {
      u_select = replay[i * 5];
      t = (u64)(replay[i * 5 + 1] * 9007199254740992.0);
    } else {
      const u32x4 o0 = philox4x32(gid, 0u, a.step, 9u, a.k0, a.k1);
      u_select = u53_to_double(o0.x, o0.y);
      t = ((u64)(o0.z >> 5) << 26) | (u64)(o0.w >> 6);
    }
    const bool sel = u_select < a.fraction;
    cnt += (u32)__popcll(__ballot(sel));
    if (sel) {
      double xi[3];
      if (replay) {
        xi[0] = replay[i * 5 + 2];
        xi[1] = replay[i * 5 + 3];
        xi[2] = replay[i * 5 + 4];
      } else {
        [[maybe_unused]] double unused;
        const u32x4 o1 = philox4x32(gid, 1u, a.step, 9u, a.k0, a.k1);
        box_muller(o1.x, o1.y, xi[0], xi[1]);
        box_muller(o1.z, o1.w, xi[2], unused);
      }
      const u32 r = reseed_rank(t, a.W);
      u32 c = 0;   // the number of components with cum <= r = the first with cum > r
#pragma unroll
      for (u32 step = RESEED_ROW / 2; step > 0; step >>= 1) c += cum[c + step - 1] <= r ? step : 0u;
      // (c <= 255 whatever r is: every read below stays inside the table; r < W = the last word of cum puts c below n_comp)
      double m[3], L[6];
#pragma unroll
      for (int k = 0; k < 3; ++k) m[k] = sh_tab[k * RESEED_ROW + c];
#pragma unroll
      for (int k = 0; k < 6; ++k) L[k] = sh_tab[(3 + k) * RESEED_ROW + c];
      double v[3];
#pragma unroll
      for (int rr = 0; rr < 3; ++rr) {
        bool any = false;
        double z = L[reg_packed(rr, 0)] * xi[0];
        any = L[reg_packed(rr, 0)] != 0.0;
#pragma unroll
        for (int cc = 1; cc <= rr; ++cc) {
          const double q = L[reg_packed(rr, cc)] * xi[cc];
          z = z + q;
          any = any || L[reg_packed(rr, cc)] != 0.0;
        }
        const double sum = m[rr] + z;
        v[rr] = any ? sum : m[rr];
      }
      s.c[0][i] = v[0];
      s.c[1][i] = v[1];
      s.c[5][i] = (v[2] >= -MCL_PI && v[2] < MCL_PI) ? v[2] : wrap_pi(v[2]);
    }
  }
  if ((threadIdx.x & 63) == 0) sh_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 tot = 0;
#pragma unroll
    for (int w = 0; w < MCL_BLOCK / MCL_WAVE; ++w) tot += sh_cnt[w];
    block_cnt[blockIdx.x] = tot;
  }
}
