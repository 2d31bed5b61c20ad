// mcl_kld_pure.h -- the device-free arithmetic of KLD-sampling (include/mcl_kld.h), in the style of mcl_host_pure.h (no HIP
// header: mcl_host_kld.h includes it, and `make host-asan-kld` compiles it with plain g++ under ASan + UBSan): the lattice
// check of mcl_kld_bins, the bound of mcl_kld_bound, the 53-bit uniform and the argument check of mcl_resample_into.
#pragma once
#include "mcl_host_pure.h"
#include "../../include/mcl_kld.h"

namespace {

// mcl_kld_grid_check: the rules of mode_grid_check_impl with the limits of a bitmap (one bit per cell)
int kld_grid_check_impl(const mcl_mode_grid* g, int64_t* n_cells, const char** reason) {
  const char* why = nullptr;
  if (!g) why = "null grid";
  else if (!std::isfinite(g->cell) || !(g->cell > 0.0)) why = "cell must be finite and > 0";
  else if (!std::isfinite(g->x0) || !std::isfinite(g->y0)) why = "x0 or y0 is not finite";
  else if (g->nx < 1 || g->ny < 1 || g->n_yaw < 1) why = "nx, ny and n_yaw must be >= 1";
  else if (g->n_yaw > MCL_KLD_MAX_YAW) why = "n_yaw > 1024";
  else if ((int64_t)g->nx * (int64_t)g->ny > MCL_KLD_MAX_CELLS ||   // (each factor < 2^31: neither product overflows)
           (int64_t)g->nx * (int64_t)g->ny * (int64_t)g->n_yaw > MCL_KLD_MAX_CELLS)
    why = "more than 2^27 cells";
  if (reason) *reason = why;
  if (why) return MCL_ERR_INVALID;
  if (n_cells) *n_cells = (int64_t)g->nx * (int64_t)g->ny * (int64_t)g->n_yaw;
  return MCL_OK;
}

// mcl_kld_bound: the Wilson-Hilferty form of Fox's bound.  Every operation a double operation rounded on its own, in the
// order include/mcl_kld.h states: a restatement in any language gives the same integer.
int kld_bound_impl(int64_t k, double epsilon, double z, int64_t n_min, int64_t n_max, int64_t* n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!n || k < 0 || !std::isfinite(epsilon) || !(epsilon > 0.0) || !std::isfinite(z) || z < 0.0 || n_min < 1 ||
      n_min > n_max || n_max > ((int64_t)1 << 31))
    return MCL_ERR_INVALID;
  if (k <= 1) {
    *n = n_min;
    return MCL_OK;
  }
  const double km1 = (double)(k - 1);
  const double a = 2.0 / (9.0 * km1);
  const double sa = std::sqrt(a);
  const double saz = sa * z;
  const double t = (1.0 - a) + saz;
  const double e2 = 2.0 * epsilon;
  double v = km1 / e2;
  v = v * t;
  v = v * t;
  v = v * t;
  if (!std::isfinite(v)) {
    *n = n_max;
    return MCL_OK;
  }
  const double c = std::ceil(v);
  if (c >= (double)n_max) *n = n_max;        // (n_min, n_max <= 2^31: exact as doubles)
  else if (c <= (double)n_min) *n = n_min;
  else *n = (int64_t)c;
  return MCL_OK;
}

// the 53-bit uniform of native_u53 (mcl_host_pure.h) with the purpose as an argument: mcl_resample_into draws with 10
uint64_t native_u53_purpose(uint64_t seed, uint32_t step, uint32_t purpose) {
  uint32_t o[4];
  philox_host(0xFFFFFFFFu, 0u, step, purpose, (uint32_t)seed, (uint32_t)(seed >> 32), o);
  return ((uint64_t)(o[0] >> 5) << 26) | (uint64_t)(o[1] >> 6);
}
constexpr uint32_t KLD_TRANSFER_PURPOSE = 10u;

// U of mcl_resample_into: the caller's uniform, or the draw of dst's seed at dst's transfer counter; false: u outside [0, 1)
bool kld_transfer_u53(const double* uniform, uint64_t seed, uint32_t step, uint64_t* u53) {
  if (uniform) {
    if (!(uniform[0] >= 0.0 && uniform[0] < 1.0)) return false;
    *u53 = (uint64_t)std::floor(uniform[0] * 9007199254740992.0);
  } else {
    *u53 = native_u53_purpose(seed, step, KLD_TRANSFER_PURPOSE);
  }
  return true;
}

// words of the bitmap of mcl_kld_bins: one bit per cell, a whole number of 16-byte vectors
int64_t kld_bitmap_words(int64_t n_cells) { return ((n_cells + 127) / 128) * 4; }

}  // namespace
