// mcl_host_reseed.h -- host side of the sensor resetting (include/mcl_reseed.h; kernel: csrc/mcl_reseed.h): the table of
// components checked, laid out as the kernel keeps it and uploaded, the REPLAY draws, the launch.  mcl_api.hip forwards
// mcl_inject_gaussian to reseed_inject; the device-free entry points go to mcl_host_pure.h.
#pragma once
#include "mcl_host.h"
#include "mcl_host_recovery.h"
#include "mcl_reseed.h"

namespace {

int reseed_inject(mcl_handle* h, double fraction, const mcl_reseed_component* comps, int n_comp, const double* replay,
                  int64_t* n_injected) {
  uint64_t W = 0;
  if (const char* why = reseed_components_why(comps, n_comp, &W)) return fail(h, MCL_ERR_INVALID, std::string("inject_gaussian: ") + why);
  const bool rp_mode = h->cfg.rng_mode == MCL_RNG_REPLAY;
  if (rp_mode) {
    if (!replay) return fail(h, MCL_ERR_INVALID, "inject_gaussian: REPLAY mode needs n x 5 draws");
    for (long long i = 0; i < h->n; ++i)
      if (!(replay[5 * i + 1] >= 0.0 && replay[5 * i + 1] < 1.0)) return fail(h, MCL_ERR_INVALID, "inject_gaussian: a u_comp outside [0, 1)");
  }
  if (fraction == 0.0) {
    if (n_injected) *n_injected = 0;
    return MCL_OK;
  }
  // the table as k_inject_gaussian keeps it: nine rows of RESEED_ROW doubles, then cum as 32-bit words padded with W
  alignas(16) unsigned char tab[RESEED_TAB_BYTES];
  memset(tab, 0, sizeof tab);
  double* rows = reinterpret_cast<double*>(tab);
  uint32_t* cum = reinterpret_cast<uint32_t*>(tab + RESEED_ROWS * RESEED_ROW * sizeof(double));
  uint64_t acc = 0;
  for (int c = 0; c < RESEED_ROW; ++c) {
    if (c < n_comp) {
      for (int k = 0; k < 3; ++k) rows[k * RESEED_ROW + c] = comps[c].mean[k];
      for (int k = 0; k < 6; ++k) rows[(3 + k) * RESEED_ROW + c] = comps[c].chol[k];
      acc += comps[c].mass;
    }
    cum[c] = (uint32_t)acc;   // (W <= 2^31)
  }
  RESERVE(h, h->reseed_tab, (size_t)RESEED_TAB_WORDS);
  RESERVE(h, h->inject_cnt, 1 + MCL_MAX_GRID);
  RET_IF(upload(h, h->reseed_tab, tab, sizeof tab));
  const double* rp = nullptr;
  if (rp_mode) {
    RET_IF(upload_replay_uniforms(h, replay, 5));
    rp = h->replay_dev;
  }
  ReseedArgs a;
  memset(&a, 0, sizeof a);
  a.k0 = (uint32_t)h->cfg.seed;
  a.k1 = (uint32_t)(h->cfg.seed >> 32);
  a.step = h->step_inject;
  a.n_comp = n_comp;
  a.gid0 = h->goff;
  a.fraction = fraction;
  a.W = W;
  RET_IF(state_overwritten(h));
  const int grid = grid_for(h->n);
  t_begin(h, MCL_K_NOISE);
  k_inject_gaussian<<<grid, MCL_BLOCK, 0, h->stream>>>(state_ptrs(h->state[h->cur], h->n), h->n, a, h->reseed_tab, rp, h->inject_cnt + 1);
  if (n_injected) k_count_final<<<1, MCL_BLOCK, 0, h->stream>>>(h->inject_cnt + 1, grid, h->inject_cnt);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  h->step_inject++;
  if (n_injected) {
    u64 cnt = 0;
    HIPCHK(h, hipMemcpyAsync(&cnt, h->inject_cnt, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_injected = (int64_t)cnt;
  }
  return MCL_OK;
}

}  // namespace
