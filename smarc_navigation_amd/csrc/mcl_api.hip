// mcl_api.hip -- host side of libmcl_hip.so: the C ABI declared in include/mcl.h.
// C++ host code that owns the device buffers, orders kernels on one HIP stream per handle and
// runs the shard-exchange steps over RCCL (one process per GPU) or device copies (LOCAL group).
// The machinery is in mcl_host*.h (one translation unit); this file is the entry points.
#include "mcl_host.h"
#include "mcl_host_resample.h"
#include "mcl_host_moments.h"
#include "mcl_host_update.h"
#include "mcl_host_landmarks.h"
#include "mcl_host_ranges.h"
#include "mcl_host_step.h"
#include "mcl_host_history.h"
#include "mcl_host_acoustic.h"
#include "mcl_host_temper.h"
#include "mcl_host_drift.h"
#include "mcl_host_regularise.h"
#include "mcl_host_quantile.h"
#include "mcl_host_innovation.h"
#include "mcl_host_information.h"
#include "mcl_host_match.h"
#include "mcl_host_swath.h"
#include "mcl_host_recovery.h"
#include "mcl_host_reseed.h"
#include "mcl_host_modes.h"
#include "mcl_host_kld.h"

// dead-reckoning integrator (host only; uses euler_from_quat above)
#include "mcl_dr_impl.h"
// bathymetry map builder (uses rot_rpy above)
#include "mcl_gridmap.h"

// ============================================================================================ C ABI
extern "C" {

int mcl_abi_version(void) { return MCL_ABI_VERSION; }

const char* mcl_status_string(int s) {
  switch (s) {
    case MCL_OK: return "ok";
    case MCL_ERR_INVALID: return "invalid argument";
    case MCL_ERR_NO_DEVICE: return "no gfx950 HIP device";
    case MCL_ERR_HIP: return "HIP runtime error";
    case MCL_ERR_UNSUPPORTED: return "unsupported";
    case MCL_ERR_STATE: return "bad call order";
    case MCL_ERR_COMM: return "RCCL error";
    case MCL_ERR_ALLOC: return "allocation failed";
  }
  return "unknown status";
}

const char* mcl_last_error(const mcl_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int mcl_matrix_from_tf(const double translation[3], const double quaternion[4], double m16[16]) {
  return matrix_from_tf_impl(translation, quaternion, m16);
}

int mcl_device_count(int* count) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  if (count) *count = n;
  return MCL_OK;
}

int mcl_create(const mcl_config* cfg, mcl_handle** out) {
  if (!cfg || !out) {
    g_create_err = "mcl_create: null argument";
    return MCL_ERR_INVALID;
  }
  *out = nullptr;
  if (cfg->n_particles < 1 || cfg->n_particles > 0x7fffffffll) {
    g_create_err = "mcl_create: n_particles out of range";
    return MCL_ERR_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    g_create_err = "mcl_create: no HIP device visible (this library has no CPU fallback)";
    return MCL_ERR_NO_DEVICE;
  }
  if (cfg->device < 0 || cfg->device >= ndev) {
    g_create_err = "mcl_create: device ordinal out of range";
    return MCL_ERR_INVALID;
  }
  hipDeviceProp_t prop;
  memset(&prop, 0, sizeof prop);
  if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_create_err = std::string("mcl_create: device is not gfx950 (found ") + prop.gcnArchName + ")";
    return MCL_ERR_NO_DEVICE;
  }
  mcl_handle* h = new mcl_handle();
  h->cfg = *cfg;
  h->n = cfg->n_particles;
  h->world = cfg->world > 1 ? cfg->world : 1;
  h->rank = h->world > 1 ? cfg->rank : 0;
  h->ng = cfg->n_global > 0 ? cfg->n_global : cfg->n_particles;
  h->goff = h->world > 1 ? cfg->global_offset : 0;
  h->device = cfg->device;
  memset(&h->tacc, 0, sizeof h->tacc);
  {
    auto on = [](const char* name) {
      const char* v = getenv(name);
      return v && v[0] == '1';
    };
    auto env_tristate = [](const char* name) {   // -1 not set, 1 for "1...", else 0
      const char* v = getenv(name);
      return !v ? -1 : (v[0] == '1' ? 1 : 0);
    };
    h->env_debug_work = getenv("MCL_DEBUG_WORK") != nullptr;
    h->env_sort = env_tristate("MCL_SORT_VISITS");
    h->env_sweep = env_tristate("MCL_SWEEP");
    h->env_slice = env_tristate("MCL_SLICE");
    h->env_slice_group = env_tristate("MCL_SLICE_GROUP");
    h->env_handover_slice = env_tristate("MCL_HANDOVER_SLICE");
    h->env_visit = env_tristate("MCL_VISIT");
    h->env_sweep_uniform = env_tristate("MCL_SWEEP_UNIFORM");
    if (const char* sv = getenv("MCL_SWEEP_STEP_CAP")) h->env_sweep_step_cap = std::max(0, atoi(sv));
    if (const char* sv = getenv("MCL_SWEEP_WAVE_CAP")) h->env_sweep_wave_cap = std::max(0, atoi(sv));
    if (const char* sv = getenv("MCL_VISIT_BINS")) {
      int b[3] = {0, 0, 0};
      if (sscanf(sv, "%d,%d,%d", &b[0], &b[1], &b[2]) == 3 && b[0] >= 1 && b[1] >= 1 && b[2] >= 1 &&
          (long long)b[0] * b[1] * b[2] <= VISIT_MAX_BINS && (b[0] * b[1] * b[2]) % 64 == 0)
        for (int c = 0; c < 3; ++c) h->visit_nb[c] = b[c];
    }
    if (const char* sv = getenv("MCL_VISIT_RANGE")) {
      const double r = atof(sv);
      if (r >= 0.5 && r <= 16.0) h->visit_range = (float)r;
    }
    if (const char* sv = getenv("MCL_VISIT_MIN_N")) h->visit_min_n = std::max(1ll, atoll(sv));
    if (const char* sv = getenv("MCL_INNOVATION_GROUP")) h->env_innov_group = std::max(0, atoi(sv));
    if (const char* sv = getenv("MCL_INFORMATION_GROUP")) h->env_info_group = std::max(0, atoi(sv));
    if (const char* sv = getenv("MCL_SWEEP_NSUB")) h->env_nsub = (sv[0] == '2' || sv[0] == '4') ? sv[0] - '0' : 1;
    h->env_force_comm = on("MCL_FORCE_COMM");
    if (const char* ex = getenv("MCL_EXCHANGE")) h->exch_allgather = strcmp(ex, "allgather") == 0;
    if (const char* fi = getenv("MCL_FAULT_INJECT")) h->fault_step = strcmp(fi, "step_after_predict") == 0;
    h->env_no_overlap = on("MCL_NO_OVERLAP");
  }
  if (h->ng > 0xffffffffll || h->goff + h->n > h->ng || h->rank >= h->world) {
    g_create_err = "mcl_create: inconsistent shard geometry";
    delete h;
    return MCL_ERR_INVALID;
  }
  if (h->world > 1 && (h->ng != h->n * h->world || h->goff != h->n * h->rank)) {
    g_create_err = "mcl_create: shards must be equal-sized contiguous blocks (n_global = world * n_particles)";
    delete h;
    return MCL_ERR_INVALID;
  }
  // (on a failure mcl_destroy releases the stream; the buffers free themselves with the handle)
#define CREATE_CHK(status)                                                 \
  do {                                                                     \
    const int rc_ = (status);                                              \
    if (rc_ != MCL_OK) {                                                   \
      g_create_err = std::string(#status " failed: ") + hipGetErrorString(hipGetLastError()); \
      mcl_destroy(h);                                                      \
      return rc_;                                                          \
    }                                                                      \
  } while (0)
  CREATE_CHK(hip_status(hipSetDevice(h->device)));
  CREATE_CHK(hip_status(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)));
  const size_t n = (size_t)h->n, ng = (size_t)h->ng;
  h->ntiles_loc = (h->n + MCL_SCAN_TILE - 1) / MCL_SCAN_TILE;
  h->ntiles_glob = (h->ng + MCL_SCAN_TILE - 1) / MCL_SCAN_TILE;
  CREATE_CHK(h->state[0].reserve(6 * n));
  CREATE_CHK(h->state[1].reserve(6 * n));
  if (h->world > 1 && h->exch_allgather) CREATE_CHK(h->state_glob.reserve(6 * ng));
  CREATE_CHK(h->lw.reserve(n));
  CREATE_CHK(h->q.reserve(n));
  CREATE_CHK(h->ncum.reserve(ng));
  CREATE_CHK(h->zcum.reserve(ng));
  CREATE_CHK(h->tile64.reserve((size_t)(h->ntiles_loc + 1)));
  CREATE_CHK(h->tile32.reserve((size_t)(h->ntiles_glob + 1)));
  CREATE_CHK(h->part.reserve(MOM_COUNT * MCL_MAX_GRID));
  CREATE_CHK(h->scal.reserve(64));
  CREATE_CHK(h->zr.reserve(n));
  CREATE_CHK(h->dupes32.reserve(ng));
  CREATE_CHK(h->desc.reserve((size_t)(h->ntiles_glob + 1)));
  CREATE_CHK(h->ctrl.reserve(CTRL_BYTES));
  CREATE_CHK(h->totals.reserve((size_t)(h->world + 1)));
  CREATE_CHK(h->host_pin.reserve(RING_STRIDE * MEAN_RING));
  if (hipHostGetDevicePointer((void**)&h->host_pin_dev, h->host_pin, 0) != hipSuccess) h->host_pin_dev = nullptr;
  CREATE_CHK(hip_status(hipMemsetAsync(h->state[0], 0, sizeof(double) * 6 * n, h->stream)));
  CREATE_CHK(hip_status(hipMemsetAsync(h->state[1], 0, sizeof(double) * 6 * n, h->stream)));
  CREATE_CHK(hip_status(hipMemsetAsync(h->scal, 0, sizeof(double) * 64, h->stream)));
  CREATE_CHK(hip_status(hipMemsetAsync(h->desc, 0, sizeof(u64) * h->desc.cap, h->stream)));
  CREATE_CHK(hip_status(hipMemsetAsync(h->ctrl, 0, CTRL_BYTES, h->stream)));
  CREATE_CHK(hip_status(hipMemsetAsync(h->totals, 0, sizeof(u64) * h->totals.cap, h->stream)));
  CREATE_CHK(hip_status(hipStreamSynchronize(h->stream)));
#undef CREATE_CHK
  *out = h;
  return MCL_OK;
}

int mcl_destroy(mcl_handle* h) {
  if (!h) return MCL_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  t_collect(h);
  for (auto& e : h->ev_pool) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  comm_teardown(h, false);
  if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
  if (h->ev_state_ready) (void)hipEventDestroy(h->ev_state_ready);
  if (h->ev_gather_done) (void)hipEventDestroy(h->ev_gather_done);
  if (h->copy_stream) {
    (void)hipStreamSynchronize(h->copy_stream);
    (void)hipStreamDestroy(h->copy_stream);
  }
  for (auto& e : h->ev_stage)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : h->ev_upd)
    if (e) (void)hipEventDestroy(e);
  for (auto& sl : h->pin_ring)
    if (sl.ev) (void)hipEventDestroy(sl.ev);
  mesh_free(h->mesh);
  landmarks_free(h->landmarks);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;   // (its buffers free themselves: here, with the handle's device current)
  return MCL_OK;
}

int mcl_init_particles(mcl_handle* h, const double* replay_normals) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  const double* rp = nullptr;
  if (h->cfg.rng_mode == MCL_RNG_REPLAY) {
    if (!replay_normals) return fail(h, MCL_ERR_INVALID, "init_particles: REPLAY mode needs n x 6 normals");
    RET_IF(upload_replay(h, replay_normals));
    rp = h->replay_dev;
  }
  RET_IF(state_overwritten(h));
  NoiseArgs a = noise_args(h, h->cfg.init_cov, 0u, 0u);
  t_begin(h, MCL_K_NOISE);
  k_add_noise<<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(state_ptrs(h->state[h->cur], h->n), h->n, a, rp, 1);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  filter_restarted(h);
  h->have_state = true;
  history_clear(h);
  return MCL_OK;
}

int mcl_predict(mcl_handle* h, const mcl_odom* odom, double dt, const double* replay_normals) {
  if (!h || !odom) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  RET_IF(cancel_state_gather(h));
  return do_predict(h, odom, dt, replay_normals);
}

int mcl_update_gps(mcl_handle* h, double gx_map, double gy_map) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  if (!(h->cfg.meas_std > 0.0)) return fail(h, MCL_ERR_INVALID, "update_gps: meas_std must be > 0");
  GpsArgs a;
  for (int k = 0; k < 4; ++k) {
    a.r0[k] = h->cfg.m2o[k];
    a.r1[k] = h->cfg.m2o[4 + k];
  }
  const double s2 = h->cfg.meas_std * h->cfg.meas_std;
  a.gx = gx_map;
  a.gy = gy_map;
  a.inv_s2 = 1.0 / s2;
  a.lognorm = std::log(2.0 * MCL_PI * s2);
  t_begin(h, MCL_K_UPDATE_GPS);
  k_gps_logw<<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(state_ptrs(h->state[h->cur], h->n), h->n, a, h->lw);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  weights_written(h, MCL_WEIGHT_LINEAR_FLOOR, SLOTS_NONE);
  return MCL_OK;
}

int mcl_set_map_grid(mcl_handle* h, const float* z, int32_t nx, int32_t ny, double ox, double oy, double res) {
  if (!h || !z || nx < 2 || ny < 2 || !(res > 0.0)) return fail(h, MCL_ERR_INVALID, "set_map_grid: bad argument");
  RET_IF(set_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (nx > (1 << 21) || ny > (1 << 21)) return fail(h, MCL_ERR_UNSUPPORTED, "set_map_grid: more than 2^21 nodes a side");
  h->map_kind = -1;   // (no map until everything below has succeeded: include/mcl.h)
  h->grid.reset();
  h->grid_pad.reset();
  const size_t cnt = (size_t)nx * (size_t)ny;
  RESERVE(h, h->grid, cnt);
  HIPCHK(h, hipMemcpy(h->grid, z, sizeof(float) * cnt, hipMemcpyHostToDevice));
  RESERVE(h, h->grid_pad, padded_heights_count(nx, ny));
  HIPCHK(h, upload_padded_heights(z, nx, ny, h->grid_pad));
  float mn = z[0], mx = z[0];
  for (size_t k = 1; k < cnt; ++k) {
    if (z[k] < mn) mn = z[k];
    if (z[k] > mx) mx = z[k];
  }
  h->gnx = nx;
  h->gny = ny;
  h->gox = ox;
  h->goy = oy;
  h->gres = res;
  h->gzmin = mn;
  h->gzmax = mx;
  h->gslope_max = grid_slope_max(z, nx, ny, res);
  h->map_kind = 0;
  h->map_xy[0] = ox;
  h->map_xy[1] = ox + (nx - 1) * res;
  h->map_xy[2] = oy;
  h->map_xy[3] = oy + (ny - 1) * res;
  return MCL_OK;
}

int mcl_set_map_mesh(mcl_handle* h, const float* verts, int64_t nv, const uint32_t* tris, int64_t nt) {
  return mcl_set_map_mesh_ex(h, verts, nv, tris, nt, 0u);
}

int mcl_set_map_mesh_ex(mcl_handle* h, const float* verts, int64_t nv, const uint32_t* tris, int64_t nt,
                        uint32_t flags) {
  if (!h || !verts || !tris || nv < 3 || nt < 1) return fail(h, MCL_ERR_INVALID, "set_map_mesh: bad argument");
  RET_IF(set_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->map_kind = -1;   // (no map until everything below has succeeded: include/mcl.h)
  mesh_free(h->mesh);
  h->mesh = nullptr;
  std::string err;
  // (a structured mesh is cast as a soup only on request: the slice's vertex records are built then)
  int rc = mesh_build(verts, nv, tris, nt, (flags & (MCL_MESH_GENERAL | MCL_MESH_UNSTRUCTURED)) != 0, &h->mesh, &err);
  if (rc != MCL_OK) {
    h->err = err;
    return rc;
  }
  {
    double lo[2] = {verts[0], verts[1]}, hi[2] = {verts[0], verts[1]};
    for (int64_t i = 1; i < nv; ++i)
      for (int c = 0; c < 2; ++c) {
        lo[c] = std::min(lo[c], (double)verts[3 * i + c]);
        hi[c] = std::max(hi[c], (double)verts[3 * i + c]);
      }
    h->map_xy[0] = lo[0];
    h->map_xy[1] = hi[0];
    h->map_xy[2] = lo[1];
    h->map_xy[3] = hi[1];
  }
  h->mesh_heightfield = (flags & MCL_MESH_HEIGHTFIELD) != 0;
  h->force_general_mesh = (flags & (MCL_MESH_GENERAL | MCL_MESH_UNSTRUCTURED)) != 0;
  h->mesh_no_sweep = (flags & MCL_MESH_GENERAL) != 0;
  if (h->mesh_heightfield && h->mesh->n_vertical > 0) {
    h->err = "set_map_mesh: MCL_MESH_HEIGHTFIELD declared but the mesh has vertical faces";
    h->mesh_heightfield = false;
    return MCL_ERR_INVALID;
  }
  h->map_kind = 1;
  return MCL_OK;
}

int mcl_update_mbes(mcl_handle* h, const float* ranges, const float* beam_angles, int32_t B, double sigma,
                    double r_max, const double sensor_offset[6]) {
  if (!h || !ranges || !beam_angles || B < 1 || !(sigma > 0.0) || !(r_max > 0.0))
    return fail(h, MCL_ERR_INVALID, "update_mbes: bad argument");
  RET_IF(set_device(h));
  RET_IF(upload_beams(h, ranges, beam_angles, B));
  MbesPlan plan;
  RET_IF(plan_mbes(h, B, sigma, r_max, sensor_offset, nullptr, plan));
  RET_IF(run_mbes(h, plan, false));
  weights_written(h, MCL_WEIGHT_LOG_SHIFT, SLOTS_SET0);
  return MCL_OK;
}

int mcl_mbes_expected(mcl_handle* h, int64_t first, int64_t count, const float* beam_angles, int32_t B,
                      double r_max, const double sensor_offset[6], float* out) {
  if (!h || !beam_angles || !out || B < 1 || first < 0 || count < 1 || first + count > h->n)
    return fail(h, MCL_ERR_INVALID, "mbes_expected: bad argument");
  RET_IF(set_device(h));
  RET_IF(upload_beams(h, nullptr, beam_angles, B));
  const size_t need = (size_t)count * (size_t)B;
  RESERVE(h, h->exp_dev, need);
  const MbesExpect expect{h->exp_dev, first, count};
  MbesPlan plan;
  RET_IF(plan_mbes(h, B, 1.0, r_max, sensor_offset, &expect, plan));
  RET_IF(run_mbes(h, plan, false));
  HIPCHK(h, hipMemcpyAsync(out, h->exp_dev, sizeof(float) * need, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}

int mcl_set_landmarks(mcl_handle* h, const double* xyz, int64_t n_landmarks) {
  if (!h || !xyz || n_landmarks < 1) return fail(h, MCL_ERR_INVALID, "set_landmarks: bad argument");
  RET_IF(set_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  landmarks_free(h->landmarks);
  h->landmarks = new LandmarkDev();
  h->landmarks->host_xyz.assign(xyz, xyz + 3 * n_landmarks);
  return MCL_OK;
}

int mcl_set_landmark_noise(mcl_handle* h, const double* cov6, const double Q6[6]) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(need_feature_map(h, "set_landmark_noise"));
  RET_IF(set_device(h));
  LandmarkDev* L = h->landmarks;
  const size_t n = L->host_xyz.size() / 3;
  L->host_cov.clear();
  L->lam_cov_max = 0.0;
  if (cov6) {
    for (size_t i = 0; i < n; ++i) {
      const double* s = cov6 + 6 * i;
      if (!(s[0] >= 0.0 && s[3] >= 0.0 && s[5] >= 0.0) || !(sym3_det(s) >= 0.0))
        return fail(h, MCL_ERR_INVALID, "set_landmark_noise: landmark covariance not positive semi-definite");
      L->lam_cov_max = std::max(L->lam_cov_max, sym3_lam_bound(s));
    }
    L->host_cov.assign(cov6, cov6 + 6 * n);
  }
  L->have_q = Q6 != nullptr;
  if (Q6) {
    if (!(sym3_det(Q6) > 0.0) || !(Q6[0] > 0.0)) return fail(h, MCL_ERR_INVALID, "set_landmark_noise: Q must be positive definite");
    for (int k = 0; k < 6; ++k) L->Q[k] = Q6[k];
  }
  L->maha = cov6 != nullptr || Q6 != nullptr;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  L->built_for = -1.0;  // the covariances travel with the next grid build
  return MCL_OK;
}

int mcl_update_landmarks(mcl_handle* h, const double* det_xyz, int32_t n_det, double sigma, int32_t k, double gate,
                         const double sensor_offset[6], int32_t accumulate) {
  if (!h) return MCL_ERR_INVALID;
  const LandmarkObs o = {det_xyz, n_det, sigma, k, gate, sensor_offset};
  RET_IF(landmarks_prepare(h, o, "update_landmarks"));
  if (accumulate) RET_IF(need_weights_to_add(h, "update_landmarks"));
  return landmarks_launch(h, o, accumulate != 0, false);
}

int mcl_update_landmarks_assign(mcl_handle* h, const double* det_xyz, int32_t n_det, double sigma, int32_t k_cand,
                                double gate, double new_mh_dist, const double sensor_offset[6], int32_t accumulate,
                                int32_t* assign_out, int64_t n_keep) {
  if (!h || !det_xyz || n_det < 1 || n_det > LM_SUB || !(sigma > 0.0) || k_cand < 1 || k_cand > LA_KC || !(gate > 0.0) ||
      !(new_mh_dist >= 0.0) || n_keep < 0 || (n_keep > 0 && !assign_out))
    return fail(h, MCL_ERR_INVALID, "update_landmarks_assign: bad argument (n_det <= 16, 1 <= k_cand <= 8)");
  RET_IF(need_feature_map(h, "update_landmarks_assign"));
  if (accumulate) RET_IF(need_weights_to_add(h, "update_landmarks_assign"));
  RET_IF(set_device(h));
  RET_IF(ensure_landmark_grid(h, sigma, gate));
  const LandmarkObs o = {det_xyz, n_det, sigma, k_cand, gate, sensor_offset};
  return landmarks_assign_launch(h, o, new_mh_dist, accumulate != 0, assign_out, n_keep);
}

int mcl_update_ranges(mcl_handle* h, const float* ranges, const float* dirs, int32_t n_beams, double sigma, double r_max,
                      const double sensor_offset[6], int32_t accumulate) {
  if (!h) return MCL_ERR_INVALID;
  if (!ranges || !dirs || n_beams < 1 || n_beams > RANGES_MAX_BEAMS || !(sigma > 0.0) || !(r_max > 0.0))
    return fail(h, MCL_ERR_INVALID, "update_ranges: bad argument (1 <= n_beams <= 16, sigma > 0, r_max > 0)");
  RET_IF(set_device(h));
  RET_IF(need_map(h, "update_ranges"));
  if (accumulate) RET_IF(need_weights_to_add(h, "update_ranges"));
  RET_IF(ranges_launch(h, ranges, dirs, n_beams, sigma, r_max, sensor_offset, accumulate != 0, h->lw, nullptr, 0, h->n));
  weights_written(h, accumulate ? WEIGHT_MODE_KEEP : MCL_WEIGHT_LOG_SHIFT, SLOTS_NONE);
  return MCL_OK;
}

int mcl_ranges_expected(mcl_handle* h, int64_t first, int64_t count, const float* dirs, int32_t n_beams, double r_max,
                        const double sensor_offset[6], float* out) {
  if (!h) return MCL_ERR_INVALID;
  if (!dirs || !out || n_beams < 1 || n_beams > RANGES_MAX_BEAMS || !(r_max > 0.0) || first < 0 || count < 1 ||
      first + count > h->n)
    return fail(h, MCL_ERR_INVALID, "ranges_expected: bad argument");
  RET_IF(set_device(h));
  RET_IF(need_map(h, "ranges_expected"));
  const size_t need = (size_t)count * (size_t)n_beams;
  RESERVE(h, h->exp_dev, need);
  RET_IF(ranges_launch(h, nullptr, dirs, n_beams, 1.0, r_max, sensor_offset, false, nullptr, h->exp_dev, first, count));
  HIPCHK(h, hipMemcpyAsync(out, h->exp_dev, sizeof(float) * need, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}

int mcl_resample(mcl_handle* h, const double* uniforms, int64_t n_uniforms, const double* replay_normals) {
  if (!h) return MCL_ERR_INVALID;
  if (h->world > 1 && !h->comm)
    return fail(h, MCL_ERR_STATE, "resample: multi-shard handle needs mcl_comm_init or mcl_group_resample");
  if (h->cfg.rng_mode == MCL_RNG_REPLAY && !replay_normals)
    return fail(h, MCL_ERR_INVALID, "resample: REPLAY mode needs n x 6 normals");
  const double* rn[1] = {replay_normals};
  return run_resample(&h, 1, uniforms, n_uniforms, rn);
}

int mcl_resample_prepare(mcl_handle* h, int64_t* n_uniforms) {
  if (!h || !n_uniforms) return MCL_ERR_INVALID;
  if (!h->have_lw) return fail(h, MCL_ERR_STATE, "resample_prepare: no weights (call an update first)");
  RET_IF(set_device(h));
  int rc;
  *n_uniforms = uniforms_needed(h, &rc);
  return rc;
}

int mcl_group_resample(mcl_handle** shards, int32_t ns, const double* uniforms, int64_t n_uniforms,
                       const double* const* replay_normals) {
  if (!shards || ns < 1) return MCL_ERR_INVALID;
  for (int s = 0; s < ns; ++s)
    if (!shards[s] || shards[s]->world != ns || shards[s]->rank != s)
      return fail(shards[0], MCL_ERR_INVALID, "group_resample: shards must be ranks 0..n-1 of one world");
  return run_resample(shards, ns, uniforms, n_uniforms, replay_normals);
}

int mcl_mean_cov(mcl_handle* h, double mean6[6], double* yaw_mean, double cov9[9]) {
  if (!h || !mean6 || !cov9) return MCL_ERR_INVALID;
  if (h->world > 1 && !h->comm) return fail(h, MCL_ERR_STATE, "mean_cov: multi-shard handle needs a communicator");
  RET_IF(run_mean_cov_async(&h, 1));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  finish_mean_cov(h, mean6, yaw_mean, cov9);
  return MCL_OK;
}

int mcl_mean_cov_async(mcl_handle* h) {
  if (!h) return MCL_ERR_INVALID;
  if (h->world > 1 && !h->comm) return fail(h, MCL_ERR_STATE, "mean_cov: multi-shard handle needs a communicator");
  return run_mean_cov_async(&h, 1);
}

int mcl_group_mean_cov(mcl_handle** shards, int32_t ns, double mean6[6], double* yaw_mean, double cov9[9]) {
  if (!shards || ns < 1 || !mean6 || !cov9) return MCL_ERR_INVALID;
  RET_IF(run_mean_cov_async(shards, ns));
  for (int s = 0; s < ns; ++s) {
    RET_IF(set_device(shards[s]));
    HIPCHK(shards[s], hipStreamSynchronize(shards[s]->stream));
  }
  finish_mean_cov(shards[0], mean6, yaw_mean, cov9);
  return MCL_OK;
}

int mcl_last_mean_cov(mcl_handle* h, double mean6[6], double* yaw_mean, double cov9[9]) {
  if (!h || !mean6 || !cov9) return MCL_ERR_INVALID;
  if (!h->have_meancov) return fail(h, MCL_ERR_STATE, "last_mean_cov: nothing computed yet");
  RET_IF(set_device(h));
  RET_IF(flush_pending_moments(h));   // (one process per GPU: the last fused step's sums may still be per shard -- a collective)
  HIPCHK(h, hipStreamSynchronize(h->stream));
  finish_mean_cov(h, mean6, yaw_mean, cov9);
  return MCL_OK;
}

int mcl_mean_history(mcl_handle* h, int64_t last_k, double* mean6_out) {
  if (!h || !mean6_out || last_k < 1) return MCL_ERR_INVALID;
  if (last_k > h->mean_count || last_k > MEAN_RING) return fail(h, MCL_ERR_INVALID, "mean_history: not that many results kept");
  RET_IF(set_device(h));
  RET_IF(flush_pending_moments(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (long long k = 0; k < last_k; ++k) {
    double yaw, cov9[9];
    finish_mean_cov(h, mean6_out + 6 * k, &yaw, cov9, h->mean_count - last_k + k);
  }
  return MCL_OK;
}

int mcl_get_poses(mcl_handle* h, double* pose7) {
  if (!h || !pose7) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  RESERVE(h, h->pose7, 7 * (size_t)h->n);
  k_poses<<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(state_ptrs(h->state[h->cur], h->n), h->n, h->pose7);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(pose7, h->pose7, sizeof(double) * 7 * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}

int mcl_get_particles(mcl_handle* h, double* soa, double* w) {
  if (!h || !soa) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  HIPCHK(h, hipMemcpyAsync(soa, h->state[h->cur], sizeof(double) * 6 * (size_t)h->n, hipMemcpyDeviceToHost,
                           h->stream));
  if (w) {
    if (!h->have_cdf) return fail(h, MCL_ERR_STATE, "get_particles: weights exist only after a resample");
    RESERVE(h, h->wnorm, (size_t)h->n);
    k_normalised_weights<<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(h->q, h->n, h->totals, h->world, h->qshift_cur, h->wnorm);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(w, h->wnorm, sizeof(double) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}

int mcl_set_particles(mcl_handle* h, const double* soa) {
  if (!h || !soa) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  RET_IF(state_overwritten(h));
  HIPCHK(h, hipMemcpyAsync(h->state[h->cur], soa, sizeof(double) * 6 * (size_t)h->n, hipMemcpyHostToDevice,
                           h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->have_state = true;
  history_clear(h);
  return MCL_OK;
}

int mcl_get_log_weights(mcl_handle* h, double* lw) {
  if (!h || !lw) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  HIPCHK(h, hipMemcpyAsync(lw, h->lw, sizeof(double) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}

int mcl_set_log_weights(mcl_handle* h, const double* lw, int32_t weight_mode) {
  if (!h || !lw || weight_mode < 0 || weight_mode > 2) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  HIPCHK(h, hipMemcpyAsync(h->lw, lw, sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  weights_written(h, weight_mode, SLOTS_NONE);
  return MCL_OK;
}

int mcl_get_last_indices(mcl_handle* h, int32_t* idx) {
  if (!h || !idx) return MCL_ERR_INVALID;
  if (!h->have_cdf && !h->idx_explicit) return fail(h, MCL_ERR_STATE, "get_last_indices: no resample yet");
  RET_IF(set_device(h));
  RESERVE(h, h->idx, (size_t)h->n);
  if (!h->idx_explicit) RET_IF(ensure_global_cdf(h));
  if (!h->idx_explicit) {
    k_indices<<<grid_for(h->n), MCL_BLOCK, 0, h->stream>>>(h->ncum, h->ng, h->goff, h->n, h->idx);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipMemcpyAsync(idx, h->idx, sizeof(int) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}

int mcl_get_last_offspring_cdf(mcl_handle* h, uint32_t* ncum) {
  if (!h || !ncum) return MCL_ERR_INVALID;
  if (!h->have_cdf) return fail(h, MCL_ERR_STATE, "get_last_offspring_cdf: no resample yet");
  RET_IF(set_device(h));
  RET_IF(ensure_global_cdf(h));
  HIPCHK(h, hipMemcpyAsync(ncum, h->ncum, sizeof(u32) * (size_t)h->ng, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}

int mcl_get_fixed_weights(mcl_handle* h, uint64_t* q, uint64_t* total) {
  if (!h || !q) return MCL_ERR_INVALID;
  if (!h->have_cdf) return fail(h, MCL_ERR_STATE, "get_fixed_weights: no resample yet");
  RET_IF(set_device(h));
  HIPCHK(h, hipMemcpyAsync(q, h->q, sizeof(u64) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
  std::vector<u64> t(h->world);
  HIPCHK(h, hipMemcpyAsync(t.data(), h->totals, sizeof(u64) * (size_t)h->world, hipMemcpyDeviceToHost, h->stream));
  u64 shift = 0;   // (a shard of several processes keeps its weights at its own exponent: mcl_resample.h, k_shift_scan)
  if (h->qshift_cur) HIPCHK(h, hipMemcpyAsync(&shift, h->qshift_cur, sizeof(u64), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (shift)
    for (long long i = 0; i < h->n; ++i) q[i] = shift >= 64 ? 0 : q[i] >> shift;
  if (total) {
    u64 T = 0;
    for (u64 v : t) T += v;
    *total = T;
  }
  return MCL_OK;
}

namespace {
// a fused step that ends between its predict and its gather: the z, roll, pitch stores that kernel left to the gather
// are made now, on every shard it ran on; the error text `failed` holds survives that
int abandon_step(mcl_handle* failed, mcl_handle** sh, int n, int rc) {
  const std::string keep = failed->err;
  for (int t = 0; t < n; ++t) (void)materialise_uniform(sh[t]);
  failed->err = keep;
  return rc;
}
// the fused step of one handle (mcl_step_mbes; with a landmark observation: mcl_step_mbes_landmarks)
int step_mbes_impl(mcl_handle* h, const StepIn& in) {
  if (!h || !in.odom || !in.ranges || !in.beam_angles) return MCL_ERR_INVALID;
  RET_IF(step_check(h, in, false));
  RET_IF(step_stage(h, in));
  // (systematic scheme: the gather of this call substitutes z, roll, pitch -- the predict kernel does not store them)
  const bool sys = h->cfg.resample_scheme == MCL_RESAMPLE_SYSTEMATIC || h->cfg.resample_scheme == MCL_RESAMPLE_NAIVE;
  int rc = step_front(h, in, sys, true);
  if (rc != MCL_OK) {
    const std::string keep = h->err;
    (void)cancel_state_gather(h);
    (void)materialise_uniform(h);
    h->err = keep;
    return rc;
  }
  // resample; the gather pass also accumulates the sums of update_loc_pose of the new state
  rc = run_resample(&h, 1, nullptr, 0, nullptr, sys);
  if (rc != MCL_OK) return abandon_step(h, &h, 1, rc);
  return sys ? collect_fused_moments(&h, 1) : run_mean_cov_async(&h, 1);
}

int group_step_mbes_impl(mcl_handle** shards, int32_t ns, const StepIn& in) {
  if (!shards || ns < 1 || !in.odom || !in.ranges || !in.beam_angles) return MCL_ERR_INVALID;
  for (int s = 0; s < ns; ++s)
    if (!shards[s] || shards[s]->world != ns || shards[s]->rank != s)
      return fail(shards[0], MCL_ERR_INVALID, std::string(in.who) + ": shards must be ranks 0..n-1 of one world");
  for (int s = 0; s < ns; ++s) RET_IF(step_check(shards[s], in, true));
  // everything that can fail before a kernel is queued, for EVERY shard first: a later shard's failure must not find
  // earlier shards with a predict in flight whose z / roll / pitch stores were deferred to the gather
  for (int s = 0; s < ns; ++s) RET_IF(step_stage(shards[s], in));
  for (int s = 0; s < ns; ++s) {
    mcl_handle* h = shards[s];
    int rc = set_device(h);
    if (rc == MCL_OK) rc = step_front(h, in, true, false);   // (no overlapped gather in a LOCAL group: device copies)
    if (rc != MCL_OK) return abandon_step(h, shards, s + 1, rc);
  }
  const int rc = run_resample(shards, ns, nullptr, 0, nullptr, true);
  if (rc != MCL_OK) return abandon_step(shards[0], shards, ns, rc);
  return collect_fused_moments(shards, ns);
}
}  // namespace

int mcl_step_mbes(mcl_handle* h, const mcl_odom* odom, double dt, const float* ranges, const float* beam_angles,
                  int32_t B, double sigma, double r_max, const double sensor_offset[6]) {
  return step_mbes_impl(h, StepIn{odom, dt, ranges, beam_angles, B, sigma, r_max, sensor_offset, nullptr, "step_mbes"});
}

int mcl_step_mbes_landmarks(mcl_handle* h, const mcl_odom* odom, double dt, const float* ranges, const float* beam_angles,
                            int32_t B, double sigma, double r_max, const double sensor_offset[6], const double* det_xyz,
                            int32_t n_det, double lm_sigma, int32_t k, double gate, const double lm_sensor_offset[6]) {
  const LandmarkObs o = {det_xyz, n_det, lm_sigma, k, gate, lm_sensor_offset};
  return step_mbes_impl(h, StepIn{odom, dt, ranges, beam_angles, B, sigma, r_max, sensor_offset, &o, "step_mbes_landmarks"});
}

int mcl_group_step_mbes(mcl_handle** shards, int32_t ns, const mcl_odom* odom, double dt, const float* ranges,
                        const float* beam_angles, int32_t B, double sigma, double r_max, const double sensor_offset[6]) {
  return group_step_mbes_impl(shards, ns,
                              StepIn{odom, dt, ranges, beam_angles, B, sigma, r_max, sensor_offset, nullptr, "group_step_mbes"});
}

int mcl_group_step_mbes_landmarks(mcl_handle** shards, int32_t ns, const mcl_odom* odom, double dt, const float* ranges,
                                  const float* beam_angles, int32_t B, double sigma, double r_max,
                                  const double sensor_offset[6], const double* det_xyz, int32_t n_det, double lm_sigma,
                                  int32_t k, double gate, const double lm_sensor_offset[6]) {
  const LandmarkObs o = {det_xyz, n_det, lm_sigma, k, gate, lm_sensor_offset};
  return group_step_mbes_impl(
      shards, ns, StepIn{odom, dt, ranges, beam_angles, B, sigma, r_max, sensor_offset, &o, "group_step_mbes_landmarks"});
}

int mcl_exchange_plan(int32_t world, const uint32_t* lost, const uint32_t* surplus, int32_t rank, uint32_t* send_off,
                      uint32_t* send_cnt, uint32_t* recv_off, uint32_t* recv_cnt) {
  return exchange_plan_impl(world, lost, surplus, rank, send_off, send_cnt, recv_off, recv_cnt);
}

int mcl_exchange_stats(mcl_handle* h, int64_t* states_sent, int64_t* lost_slots, int32_t reset) {
  if (!h) return MCL_ERR_INVALID;
  if (states_sent) *states_sent = (int64_t)h->ex_sent;
  if (lost_slots) *lost_slots = (int64_t)h->ex_lost;
  if (reset) h->ex_sent = h->ex_lost = 0;
  return MCL_OK;
}

int mcl_exchange_ops(mcl_handle* h, int64_t* p2p_ops, int64_t* resamples, int32_t reset) {
  if (!h) return MCL_ERR_INVALID;
  if (p2p_ops) *p2p_ops = (int64_t)h->ex_ops;
  if (resamples) *resamples = (int64_t)h->ex_rounds;
  if (reset) h->ex_ops = h->ex_rounds = 0;
  return MCL_OK;
}

int mcl_sync(mcl_handle* h) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}

int mcl_resample_indices(int32_t scheme, const double* weights, int64_t n, const double* uniforms,
                         int64_t n_uniforms, int32_t device, int32_t* out) {
  if (!weights || !out || n < 1) return MCL_ERR_INVALID;
  mcl_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.n_particles = n;
  cfg.device = device;
  cfg.resample_scheme = scheme;
  cfg.rng_mode = MCL_RNG_REPLAY;
  mcl_handle* h = nullptr;
  int rc = mcl_create(&cfg, &h);
  if (rc != MCL_OK) return rc;
  rc = mcl_set_log_weights(h, weights, MCL_WEIGHT_LINEAR);
  if (rc == MCL_OK) {
    if (scheme != MCL_RESAMPLE_SYSTEMATIC && scheme != MCL_RESAMPLE_NAIVE) {
      int64_t need = 0;
      rc = mcl_resample_prepare(h, &need);
      if (rc == MCL_OK) rc = alt_indices(h, uniforms, n_uniforms);
      if (rc == MCL_OK) rc = mcl_get_last_indices(h, out);
      if (rc != MCL_OK) g_create_err = h->err;
    } else if (uint64_t u53 = 0; sample_u53(h->cfg, 0u, uniforms, n_uniforms, &u53)) {
      g_create_err = "resample_indices: systematic needs one uniform in [0,1)";
      rc = MCL_ERR_INVALID;
    } else {
      rc = phase_quantise(h, true);
      if (rc == MCL_OK) rc = phase_cdf(h, u53);
      if (rc == MCL_OK) {
        h->have_cdf = true;
        h->cdf_global = true;
        rc = mcl_get_last_indices(h, out);
      }
      if (rc != MCL_OK) g_create_err = h->err;
    }
  } else {
    g_create_err = h->err;
  }
  mcl_destroy(h);
  return rc;
}

int mcl_comm_unique_id(char id[128]) {
  if (!id) return MCL_ERR_INVALID;
  ncclUniqueId uid;
  static_assert(sizeof(ncclUniqueId) <= 128, "unique id size");
  if (ncclGetUniqueId(&uid) != ncclSuccess) {
    g_create_err = "ncclGetUniqueId failed";
    return MCL_ERR_COMM;
  }
  memset(id, 0, 128);
  memcpy(id, &uid, sizeof uid);
  return MCL_OK;
}

namespace {
// wait for an event with a deadline; 0 = done, 1 = timed out, negative = HIP error
int wait_event_ms(hipEvent_t ev, int timeout_ms) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipSuccess) return 0;
    if (e != hipErrorNotReady) return -1;
    if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > timeout_ms)
      return 1;
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}
}  // namespace

int mcl_comm_init_ex(mcl_handle* h, const char id[128], uint32_t flags) {
  if (!h || !id) return MCL_ERR_INVALID;
  if (h->world < 2 && !h->env_force_comm) return MCL_OK;  // MCL_FORCE_COMM=1: test hook, 1-rank communicator
  if (h->comm) return fail(h, MCL_ERR_STATE, "comm_init: communicator exists (mcl_comm_shutdown first)");
  RET_IF(set_device(h));
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof uid);
  NCCLCHK(h, ncclCommInitRank(&h->comm, h->world, uid, h->rank));
  if (h->exch_allgather) RESERVE(h, h->state_glob, 6 * (size_t)h->ng);
  // second communicator + stream for the overlapped state all-gather (MCL_EXCHANGE=allgather only: the O(n)
  // exchange ships a few per cent of a shard and has nothing worth hiding); optional
  const bool overlap = h->exch_allgather && !(flags & MCL_COMM_NO_OVERLAP) && !h->env_no_overlap;
  if (overlap && ncclCommSplit(h->comm, 0, h->rank, &h->comm2, nullptr) == ncclSuccess && h->comm2) {
    if (!h->comm_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
    if (!h->ev_state_ready) HIPCHK(h, hipEventCreateWithFlags(&h->ev_state_ready, hipEventDisableTiming));
    if (!h->ev_gather_done) HIPCHK(h, hipEventCreateWithFlags(&h->ev_gather_done, hipEventDisableTiming));
  } else {
    h->comm2 = nullptr;
  }
  return MCL_OK;
}

int mcl_comm_init(mcl_handle* h, const char id[128]) { return mcl_comm_init_ex(h, id, 0u); }

int mcl_comm_ranks(mcl_handle* h, int32_t* ranks, int32_t* overlap) {
  if (!h || !ranks) return MCL_ERR_INVALID;
  if (overlap) *overlap = h->comm2 ? 1 : 0;
  if (!h->comm) {
    *ranks = 1;
    return MCL_OK;
  }
  RET_IF(set_device(h));
  // every rank contributes 1: the sum is the number of ranks RCCL really connected
  int* d = (int*)(h->totals + h->world);  // scratch word behind the shard totals
  const int one = 1;
  HIPCHK(h, hipMemcpyAsync(d, &one, sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  NCCLCHK(h, ncclAllReduce(d, d, 1, ncclInt32, ncclSum, h->comm, h->stream));
  int got = 0;
  HIPCHK(h, hipMemcpyAsync(&got, d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *ranks = got;
  return MCL_OK;
}

int mcl_comm_selftest(mcl_handle* h, int32_t timeout_ms) {
  if (!h) return MCL_ERR_INVALID;
  if (!h->comm) return MCL_OK;
  if (timeout_ms < 1) timeout_ms = 1;
  RET_IF(set_device(h));
  // the exact concurrency pattern of mcl_step_mbes: the 6-array state all-gather on the second
  // communicator/stream while the first communicator runs its all-reduce + all-gathers, three rounds
  hipEvent_t done = nullptr;
  HIPCHK(h, hipEventCreateWithFlags(&done, hipEventDisableTiming));
  int rc = MCL_OK;
  for (int round = 0; round < 3 && rc == MCL_OK; ++round) {
    rc = start_state_gather(h);
    if (rc != MCL_OK) break;
    ncclResult_t e = ncclAllReduce(h->scal + 24, h->scal + 24, 1, ncclDouble, ncclMax, h->comm, h->stream);
    if (e == ncclSuccess) e = ncclAllGather(h->totals + h->rank, h->totals, 1, ncclUint64, h->comm, h->stream);
    if (e == ncclSuccess && h->exch_allgather)
      e = ncclAllGather(h->ncum + h->goff, h->ncum, (size_t)h->n, ncclUint32, h->comm, h->stream);
    if (e == ncclSuccess && !h->exch_allgather && h->world > 1) {
      // the O(n) exchange's pattern: the hand-over records all-gathered, then grouped point-to-point transfers
      // (here: one word to the next rank, one from the previous)
      RET_IF(alloc_lsx(h));
      e = ncclAllGather(h->lsx + 4 * (size_t)h->rank, h->lsx, 4, ncclUint64, h->comm, h->stream);
      if (e == ncclSuccess) e = ncclGroupStart();
      if (e == ncclSuccess) e = ncclSend(h->totals + h->rank, 1, ncclUint64, (h->rank + 1) % h->world, h->comm, h->stream);
      if (e == ncclSuccess) e = ncclRecv(h->totals + h->world, 1, ncclUint64, (h->rank + h->world - 1) % h->world, h->comm, h->stream);
      if (e == ncclSuccess) e = ncclGroupEnd();
    }
    if (e != ncclSuccess) {
      h->err = std::string("comm_selftest: ") + ncclGetErrorString(e);
      rc = MCL_ERR_COMM;
      break;
    }
    (void)cancel_state_gather(h);
    (void)hipEventRecord(done, h->stream);
    const int w = wait_event_ms(done, timeout_ms);
    if (w != 0) {
      h->err = w > 0 ? "comm_selftest: collectives did not complete before the deadline (communicators aborted)"
                     : "comm_selftest: HIP error while waiting";
      comm_teardown(h, true);
      rc = MCL_ERR_COMM;
    }
  }
  (void)hipEventDestroy(done);
  return rc;
}

int mcl_comm_shutdown(mcl_handle* h, int32_t abort) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  if (!abort) RET_IF(flush_pending_moments(h));   // (while the communicator is still there)
  if (!abort && h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));
  if (!abort && h->comm_stream) HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  comm_teardown(h, abort != 0);
  (void)flush_pending_moments(h);   // (aborted with an entry open: it is marked NaN)
  return MCL_OK;
}

int mcl_mbes_last_path(mcl_handle* h, int32_t* path, int64_t* handed_over, int64_t* deferred_groups) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int cnt[2] = {0, 0};  // groups the fast kernel left to the general one; particles the sweep handed over
  HIPCHK(h, hipMemcpy(cnt, h->ctrl + CTRL_WORK, sizeof cnt, hipMemcpyDeviceToHost));
  if (path) *path = h->sweep_now ? 1 : (h->slice_now ? 2 : 0);
  if (handed_over) *handed_over = (h->sweep_now || h->slice_now) ? cnt[1] : 0;
  if (deferred_groups) {
    *deferred_groups = cnt[0];
    if (h->slice_now && h->slice_group_ran && h->slice_loose) {
      // the fan slice over groups of spatial neighbours: groups it left to the per-particle kernel
      int loose = 0;
      HIPCHK(h, hipMemcpy(&loose, h->ctrl + CTRL_LOOSE, sizeof loose, hipMemcpyDeviceToHost));
      *deferred_groups = loose;
    } else if (h->slice_now) {
      *deferred_groups = -1;   // (no groups: every particle cast on its own)
    }
  }
  return MCL_OK;
}

int mcl_mbes_last_handover(mcl_handle* h, int64_t* by_slice, int64_t* by_traversal) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int first = 0, second = 0;
  HIPCHK(h, hipMemcpy(&first, h->ctrl + CTRL_DEFER, sizeof first, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(&second, h->ctrl + CTRL_DEFER2, sizeof second, hipMemcpyDeviceToHost));
  const bool staged = h->sweep_now && h->handover_slice_now;
  if (!h->sweep_now && !h->slice_now) first = 0;
  if (by_slice) *by_slice = staged ? first - second : 0;
  if (by_traversal) *by_traversal = staged ? second : first;
  return MCL_OK;
}

int mcl_mbes_visit_order(mcl_handle* h, uint32_t* slots, int32_t* sorted) {
  if (!h || !slots) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (sorted) *sorted = h->pose_visit ? 1 : 0;
  if (!h->pose_visit || !h->pose_dev) {
    for (long long i = 0; i < h->n; ++i) slots[i] = (uint32_t)i;
    return MCL_OK;
  }
  std::vector<MbesPose> rec((size_t)h->n);
  HIPCHK(h, hipMemcpy(rec.data(), h->pose_dev, sizeof(MbesPose) * (size_t)h->n, hipMemcpyDeviceToHost));
  for (long long i = 0; i < h->n; ++i) slots[i] = rec[(size_t)i].slot;
  return MCL_OK;
}

// ---- global localisation and kidnap recovery (include/mcl_recovery.h; host: mcl_host_recovery.h, kernels: csrc/mcl_recovery.h)
int mcl_map_bounds(mcl_handle* h, double xy_min_max[4]) {
  if (!h || !xy_min_max) return MCL_ERR_INVALID;
  RET_IF(need_map(h, "map_bounds"));
  for (int k = 0; k < 4; ++k) xy_min_max[k] = h->map_xy[k];
  return MCL_OK;
}

int mcl_init_particles_uniform(mcl_handle* h, const mcl_box* box, const double* replay_uniforms) {
  if (!h) return MCL_ERR_INVALID;
  if (!box) return fail(h, MCL_ERR_INVALID, "init_particles_uniform: null box");
  RET_IF(set_device(h));
  RET_IF(recovery_init_uniform(h, box, replay_uniforms));
  filter_restarted(h);
  h->have_state = true;
  history_clear(h);
  return MCL_OK;
}

int mcl_weight_stats(mcl_handle* h, mcl_wstats* out) {
  if (!h || !out) return MCL_ERR_INVALID;
  if (!h->have_lw) return fail(h, MCL_ERR_STATE, "weight_stats: no log-weights (call an update first)");
  RET_IF(set_device(h));
  return recovery_weight_stats(h, out);
}

int mcl_weight_stats_merge(const mcl_wstats* parts, int32_t n_parts, mcl_wstats* out) {
  return weight_stats_merge_impl(parts, n_parts, out);
}

int mcl_inject_uniform(mcl_handle* h, double fraction, const mcl_box* box, const double* replay_uniforms,
                       int64_t* n_injected) {
  if (!h) return MCL_ERR_INVALID;
  if (!box) return fail(h, MCL_ERR_INVALID, "inject_uniform: null box");
  if (!(fraction >= 0.0 && fraction <= 1.0)) return fail(h, MCL_ERR_INVALID, "inject_uniform: fraction outside [0, 1]");
  if (h->have_lw) return fail(h, MCL_ERR_STATE, "inject_uniform: log-weights pending (resample first: they describe the particles as they are)");
  RET_IF(set_device(h));
  return recovery_inject(h, fraction, box, replay_uniforms, n_injected);
}

// ---- dominant modes of the cloud (include/mcl_modes.h; host: mcl_host_modes.h, kernels: csrc/mcl_modes.h)
int mcl_mode_grid_check(const mcl_mode_grid* g, int64_t* n_cells) { return mode_grid_check_impl(g, n_cells, nullptr); }

int mcl_pose_modes(mcl_handle* h, const mcl_mode_grid* g, int32_t k_max, mcl_mode* modes, int32_t* n_modes,
                   int64_t* n_outside) {
  if (!h) return MCL_ERR_INVALID;
  if (!g || !modes || !n_modes) return fail(h, MCL_ERR_INVALID, "pose_modes: null argument");
  if (k_max < 1 || k_max > MCL_MODES_MAX) return fail(h, MCL_ERR_INVALID, "pose_modes: k_max outside 1 ... 8");
  int64_t n_cells = 0;
  const char* reason = nullptr;
  if (mode_grid_check_impl(g, &n_cells, &reason) != MCL_OK) return fail(h, MCL_ERR_INVALID, std::string("pose_modes: ") + reason);
  if (h->world > 1) return fail(h, MCL_ERR_UNSUPPORTED, "pose_modes: a sharded cloud (world > 1) is not supported");
  if (!h->have_state) return fail(h, MCL_ERR_STATE, "pose_modes: no particles (call mcl_init_particles / mcl_set_particles first)");
  RET_IF(set_device(h));
  return modes_run(h, g, k_max, n_cells, modes, n_modes, n_outside);
}

// ---- particle genealogy (include/mcl_history.h; host: mcl_host_history.h, kernels: csrc/mcl_history.h)
int mcl_history_bytes(int64_t n, int32_t depth, int64_t* bytes) { return history_bytes_impl(n, depth, bytes); }

int mcl_history_disable(mcl_handle* h) {
  if (!h) return MCL_ERR_INVALID;
  if (!h->hist_on) return MCL_OK;
  RET_IF(set_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (a compose or a record in flight still writes the buffers)
  history_free(h);
  return MCL_OK;
}

int mcl_history_enable(mcl_handle* h, int32_t depth) {
  if (!h) return MCL_ERR_INVALID;
  if (depth < 1 || depth > MCL_HISTORY_MAX_DEPTH) return fail(h, MCL_ERR_INVALID, "history_enable: depth outside 1 ... 1024");
  if (h->world > 1 || h->cfg.comm_mode != MCL_COMM_NONE || h->comm)
    return fail(h, MCL_ERR_UNSUPPORTED, "history_enable: a sharded cloud is not supported");
  RET_IF(set_device(h));   // (the ring is allocated on the handle's device, whichever is current in the caller's thread)
  RET_IF(mcl_history_disable(h));
  const int rc = history_alloc(h, depth);
  if (rc != MCL_OK) {
    const std::string keep = h->err;
    history_free(h);
    h->err = keep;
    return rc;
  }
  h->hist_stamp.assign((size_t)depth, 0.0);
  h->hist_depth = depth;
  history_clear(h);
  h->hist_on = true;
  return MCL_OK;
}

int mcl_history_reset(mcl_handle* h) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(need_history(h, "history_reset"));
  history_clear(h);
  return MCL_OK;
}

int mcl_history_record(mcl_handle* h, double stamp) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(need_history(h, "history_record"));
  if (!h->have_state) return fail(h, MCL_ERR_STATE, "history_record: no particles (call mcl_init_particles / mcl_set_particles first)");
  RET_IF(set_device(h));
  return history_record(h, stamp);
}

int mcl_history_frames(mcl_handle* h, int32_t* held, int64_t* recorded, double* stamps) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(need_history(h, "history_frames"));
  if (held) *held = h->hist_held;
  if (recorded) *recorded = h->hist_recorded;
  if (stamps)
    for (int k = 0; k < h->hist_held; ++k) stamps[k] = h->hist_stamp[(size_t)history_frame_index(h, k)];
  return MCL_OK;
}

int mcl_history_ancestors(mcl_handle* h, int32_t lag, uint32_t* slots) {
  if (!h) return MCL_ERR_INVALID;
  if (!slots) return fail(h, MCL_ERR_INVALID, "history_ancestors: null argument");
  RET_IF(need_history(h, "history_ancestors"));
  if (lag < 0 || lag >= h->hist_held) return fail(h, MCL_ERR_INVALID, "history_ancestors: lag outside the frames held");
  RET_IF(set_device(h));
  return history_ancestors(h, lag, slots);
}

int mcl_history_smooth(mcl_handle* h, int32_t lags, mcl_history_est* est) {
  if (!h) return MCL_ERR_INVALID;
  if (!est) return fail(h, MCL_ERR_INVALID, "history_smooth: null argument");
  RET_IF(need_history(h, "history_smooth"));
  if (lags < 1 || lags > h->hist_held) return fail(h, MCL_ERR_INVALID, "history_smooth: lags outside the frames held");
  RET_IF(set_device(h));
  return history_smooth(h, lags, est);
}

int mcl_history_path(mcl_handle* h, int64_t slot, int32_t lags, double* xyyaw, uint32_t* slots) {
  if (!h) return MCL_ERR_INVALID;
  if (!xyyaw) return fail(h, MCL_ERR_INVALID, "history_path: null argument");
  RET_IF(need_history(h, "history_path"));
  if (slot < 0 || slot >= h->n) return fail(h, MCL_ERR_INVALID, "history_path: slot outside the handle");
  if (lags < 1 || lags > h->hist_held) return fail(h, MCL_ERR_INVALID, "history_path: lags outside the frames held");
  RET_IF(set_device(h));
  return history_path(h, slot, lags, xyyaw, slots);
}

// ---- delayed acoustic updates (include/mcl_acoustic.h; host: mcl_host_acoustic.h, kernels: csrc/mcl_acoustic.h)
int mcl_update_fix(mcl_handle* h, const double xy_map[2], const double cov3[3], const double offset[3], const double zrp[3],
                   int32_t lag, double frac, int32_t accumulate) {
  if (!h) return MCL_ERR_INVALID;
  if (!xy_map || !cov3) return fail(h, MCL_ERR_INVALID, "update_fix: null argument");
  if (!std::isfinite(xy_map[0]) || !std::isfinite(xy_map[1]) || !std::isfinite(cov3[0]) || !std::isfinite(cov3[1]) ||
      !std::isfinite(cov3[2]) || !(cov3[0] > 0.0) || !(cov3[0] * cov3[2] - cov3[1] * cov3[1] > 0.0) ||
      !std::isfinite(cov3[0] * cov3[2] - cov3[1] * cov3[1]))
    return fail(h, MCL_ERR_INVALID, "update_fix: the fix must be finite and its covariance positive definite");
  AcoArgs a;
  bool arm = false;
  RET_IF(acoustic_prepare(h, "update_fix", offset, zrp, lag, frac, accumulate != 0, a, &arm));
  return fix_launch(h, a, arm, xy_map, cov3);
}

int mcl_update_beacon_ranges(mcl_handle* h, const double* beacons_xyz, const double* ranges, int32_t n_b, double sigma,
                             const double offset[3], const double zrp[3], int32_t lag, double frac, int32_t accumulate) {
  if (!h) return MCL_ERR_INVALID;
  if (!beacons_xyz || !ranges || n_b < 1 || n_b > MCL_ACOUSTIC_MAX_BEACONS || !(sigma > 0.0) || !std::isfinite(sigma))
    return fail(h, MCL_ERR_INVALID, "update_beacon_ranges: bad argument (1 <= n_b <= 8, sigma > 0)");
  for (int b = 0; b < n_b; ++b)
    if (!std::isfinite(beacons_xyz[3 * b]) || !std::isfinite(beacons_xyz[3 * b + 1]) || !std::isfinite(beacons_xyz[3 * b + 2]) ||
        std::isinf(ranges[b]))
      return fail(h, MCL_ERR_INVALID, "update_beacon_ranges: a beacon is not finite or a range is infinite");
  AcoArgs a;
  bool arm = false;
  RET_IF(acoustic_prepare(h, "update_beacon_ranges", offset, zrp, lag, frac, accumulate != 0, a, &arm));
  return beacon_launch(h, a, arm, beacons_xyz, ranges, n_b, sigma);
}

int mcl_history_bracket(const double* stamps_newest_first, int32_t held, double stamp, int32_t* lag, double* frac,
                        int32_t* where) {
  return history_bracket_impl(stamps_newest_first, held, stamp, lag, frac, where);
}

// ---- ESS-targeted tempering (include/mcl_temper.h; host: mcl_host_temper.h, kernels: csrc/mcl_temper.h)
int mcl_temper_beta(int32_t j, double* beta) { return temper_beta_impl(j, beta); }

int mcl_temper_pass(uint64_t s1, uint64_t s2, int64_t n_target, int32_t* pass) { return temper_pass_impl(s1, s2, n_target, pass); }

int mcl_temper_candidates(int32_t round, int32_t j_prev, int32_t cand[MCL_TEMPER_MAX_CAND], int32_t* n_cand) {
  return temper_candidates_impl(round, j_prev, cand, n_cand);
}

int mcl_temper(mcl_handle* h, int64_t n_target, int32_t apply, mcl_temper_result* out) {
  if (!h) return MCL_ERR_INVALID;
  return temper_run(h, n_target, apply != 0, out);
}

int mcl_temper_sums(mcl_handle* h, double max_lw, const int32_t* levels, int32_t n_levels, uint64_t* s1, uint64_t* s2) {
  if (!h) return MCL_ERR_INVALID;
  return temper_sums(h, max_lw, levels, n_levels, s1, s2);
}

int mcl_temper_apply(mcl_handle* h, int32_t j) {
  if (!h) return MCL_ERR_INVALID;
  return temper_apply(h, j);
}

int mcl_group_temper(mcl_handle** shards, int32_t ns, int64_t n_target, int32_t apply, mcl_temper_result* out) {
  if (!shards || ns < 1) return MCL_ERR_INVALID;
  for (int s = 0; s < ns; ++s)
    if (!shards[s]) return MCL_ERR_INVALID;
  return group_temper_run(shards, ns, n_target, apply != 0, out);
}

// ---- per-particle drift states (include/mcl_drift.h; host: mcl_host_drift.h, kernels: csrc/mcl_drift.h)
int mcl_drift_bytes(int64_t n, int64_t* bytes) { return drift_bytes_impl(n, bytes); }

int mcl_drift_config_check(const mcl_drift_config* cfg, const char** reason) { return drift_config_check_impl(cfg, reason); }

int mcl_drift_disable(mcl_handle* h) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(need_drift(h, "drift_disable"));
  RET_IF(set_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (an advance or a gather in flight still writes the buffers)
  drift_free(h);
  return MCL_OK;
}

int mcl_drift_enable(mcl_handle* h, const mcl_drift_config* cfg, const double* replay_normals) {
  if (!h) return MCL_ERR_INVALID;
  const char* why = nullptr;
  if (drift_config_check_impl(cfg, &why) != MCL_OK) return fail(h, MCL_ERR_INVALID, std::string("drift_enable: ") + why);
  if (h->drift_on) return fail(h, MCL_ERR_STATE, "drift_enable: already enabled (call mcl_drift_disable first)");
  if (h->world > 1 || h->cfg.comm_mode != MCL_COMM_NONE || h->comm)
    return fail(h, MCL_ERR_UNSUPPORTED, "drift_enable: a sharded cloud is not supported");
  RET_IF(set_device(h));
  h->drift_cfg = *cfg;
  int rc = drift_alloc(h);
  if (rc == MCL_OK) rc = drift_prior(h, replay_normals, "drift_enable");
  if (rc != MCL_OK) {
    const std::string keep = h->err;
    (void)hipStreamSynchronize(h->stream);
    drift_free(h);
    h->err = keep;
    return rc;
  }
  h->drift_on = true;
  return MCL_OK;
}

int mcl_drift_reset(mcl_handle* h, const double* replay_normals) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(need_drift(h, "drift_reset"));
  RET_IF(set_device(h));
  return drift_prior(h, replay_normals, "drift_reset");
}

int mcl_drift_advance(mcl_handle* h, double dt, const double* replay_normals) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(need_drift(h, "drift_advance"));
  if (!std::isfinite(dt)) return fail(h, MCL_ERR_INVALID, "drift_advance: dt is not finite");
  if (!(dt > 0.0)) return MCL_OK;   // (the predict's gate: nothing moves, nothing is counted)
  RET_IF(set_device(h));
  return drift_advance(h, dt, replay_normals);
}

int mcl_drift_get(mcl_handle* h, double* soa3n) {
  if (!h) return MCL_ERR_INVALID;
  if (!soa3n) return fail(h, MCL_ERR_INVALID, "drift_get: null argument");
  RET_IF(need_drift(h, "drift_get"));
  RET_IF(set_device(h));
  HIPCHK(h, hipMemcpyAsync(soa3n, h->drift_state, sizeof(double) * 3 * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}

int mcl_drift_set(mcl_handle* h, const double* soa3n) {
  if (!h) return MCL_ERR_INVALID;
  if (!soa3n) return fail(h, MCL_ERR_INVALID, "drift_set: null argument");
  RET_IF(need_drift(h, "drift_set"));
  RET_IF(set_device(h));
  HIPCHK(h, hipMemcpyAsync(h->drift_state, soa3n, sizeof(double) * 3 * (size_t)h->n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MCL_OK;
}

int mcl_drift_mean_cov(mcl_handle* h, double mean3[3], double cov6[6]) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(need_drift(h, "drift_mean_cov"));
  RET_IF(set_device(h));
  return drift_mean_cov(h, mean3, cov6);
}

// ---- regularised resampling (include/mcl_regularise.h; host: mcl_host_regularise.h, kernels: csrc/mcl_regularise.h)
int mcl_regularise_config_check(const mcl_regularise_config* cfg, const char** reason) {
  return regularise_config_check_impl(cfg, reason);
}

int mcl_regularise_bandwidth(int64_t n, int32_t dims, double scale, int32_t shrink, double* h, double* a) {
  return regularise_bandwidth_impl(n, dims, scale, shrink, h, a);
}

int mcl_regularise_factor(const double* cov_packed, int32_t dims, double* chol_packed, int32_t* dead) {
  return regularise_factor_impl(cov_packed, dims, chol_packed, dead);
}

int mcl_regularise(mcl_handle* h, const mcl_regularise_config* cfg, const double* replay_normals) {
  if (!h) return MCL_ERR_INVALID;
  if (const char* why = regularise_config_why(cfg)) return fail(h, MCL_ERR_INVALID, std::string("regularise: ") + why);
  if (h->world > 1 || h->cfg.comm_mode != MCL_COMM_NONE || h->comm)
    return fail(h, MCL_ERR_UNSUPPORTED, "regularise: a sharded cloud is not supported");
  if (cfg->dims == 6 && !h->drift_on)
    return fail(h, MCL_ERR_STATE, "regularise: dims = 6 needs the drift (call mcl_drift_enable first, or pass dims = 3)");
  if (h->cfg.rng_mode == MCL_RNG_REPLAY && !replay_normals)
    return fail(h, MCL_ERR_INVALID, "regularise: REPLAY mode needs n x dims normals");
  RET_IF(set_device(h));
  return regularise_run(h, cfg, replay_normals);
}

int mcl_regularise_last(mcl_handle* h, mcl_regularise_result* result) {
  if (!h) return MCL_ERR_INVALID;
  if (!result) return fail(h, MCL_ERR_INVALID, "regularise_last: null argument");
  if (h->reg_dims == 0) return fail(h, MCL_ERR_STATE, "regularise_last: no mcl_regularise call yet");
  RET_IF(set_device(h));
  return regularise_last(h, result);
}

// ---- exact order statistics (include/mcl_quantile.h; host: mcl_host_quantile.h, kernels: csrc/mcl_quantile.h)
int mcl_quantile_key(double v, uint64_t* key) { return quantile_key_impl(v, key); }

int mcl_quantile_value(uint64_t key, double* v) { return quantile_value_impl(key, v); }

int mcl_quantile_threshold(double p, uint64_t* P) { return quantile_threshold_impl(p, P); }

int mcl_quantile_reached(uint64_t mass, uint64_t total, uint64_t P, int32_t* reached) {
  return quantile_reached_impl(mass, total, P, reached);
}

int mcl_cloud_quantiles(mcl_handle* h, const mcl_quantile_query* query, const double* probs, int32_t n_probs,
                        mcl_quantile_result* out) {
  if (!h) return MCL_ERR_INVALID;
  if (!query || !probs || !out) return fail(h, MCL_ERR_INVALID, "cloud_quantiles: null argument");
  return quant_run(h, query, probs, n_probs, out);
}

int mcl_cloud_mass(mcl_handle* h, const mcl_quantile_query* query, double max_lw, const double* values, int32_t n_values,
                   uint64_t* mass, uint64_t* total, int64_t* n_used) {
  if (!h) return MCL_ERR_INVALID;
  if (!query || !values || !mass || !total || !n_used) return fail(h, MCL_ERR_INVALID, "cloud_mass: null argument");
  return quant_mass_run(h, query, max_lw, values, n_values, mass, total, n_used);
}

int mcl_cloud_key_hist(mcl_handle* h, const mcl_quantile_query* query, double max_lw, uint64_t prefix, int32_t prefix_bits,
                       uint64_t hist[256]) {
  if (!h) return MCL_ERR_INVALID;
  if (!query || !hist) return fail(h, MCL_ERR_INVALID, "cloud_key_hist: null argument");
  return quant_key_hist(h, query, max_lw, prefix, prefix_bits, hist);
}

int mcl_group_cloud_quantiles(mcl_handle** shards, int32_t ns, const mcl_quantile_query* query, const double* probs,
                              int32_t n_probs, mcl_quantile_result* out) {
  if (!shards || ns < 1) return MCL_ERR_INVALID;
  for (int s = 0; s < ns; ++s)
    if (!shards[s]) return MCL_ERR_INVALID;
  if (!query || !probs || !out) return fail(shards[0], MCL_ERR_INVALID, "group_cloud_quantiles: null argument");
  return group_quant_run(shards, ns, query, probs, n_probs, out);
}

// ---- ping innovation statistics and the per-beam gate (include/mcl_innovation.h; host: mcl_host_innovation.h, kernel:
// csrc/mcl_innovation.h)
int mcl_innovation_dirs(const float* beam_angles, int32_t B, float* dirs_out) { return innovation_dirs_impl(beam_angles, B, dirs_out); }

int mcl_innovation_sample(int64_t n_global, int32_t max_samples, int64_t* stride, int64_t* count) {
  return innovation_sample_impl(n_global, max_samples, stride, count);
}

int mcl_innovation_merge(const mcl_innovation_beam* parts, int32_t n_parts, int32_t B, mcl_innovation_beam* out) {
  return innovation_merge_impl(parts, n_parts, B, out);
}

int mcl_innovation_gate(const mcl_innovation_beam* beams, int32_t B, double sigma, const mcl_innovation_gate_config* cfg,
                        mcl_innovation_derived* per_beam, mcl_innovation_verdict* verdict) {
  return innovation_gate_impl(beams, B, sigma, cfg, per_beam, verdict);
}

int mcl_ping_innovation(mcl_handle* h, const float* ranges, const float* beam_angles, int32_t B, double sigma,
                        double support_k, double r_max, const double sensor_offset[6], int32_t max_samples,
                        mcl_innovation_beam* beams_out, float* exp_out, int64_t* n_sampled) {
  if (!h) return MCL_ERR_INVALID;
  if (!beams_out || !n_sampled) return fail(h, MCL_ERR_INVALID, "ping_innovation: null argument");
  const InnovPing p = {ranges, beam_angles, B, sigma, support_k, r_max, sensor_offset, max_samples};
  return innovation_run(h, p, beams_out, exp_out, n_sampled);
}

int mcl_group_ping_innovation(mcl_handle** shards, int32_t ns, const float* ranges, const float* beam_angles, int32_t B,
                              double sigma, double support_k, double r_max, const double sensor_offset[6],
                              int32_t max_samples, mcl_innovation_beam* beams_out, int64_t* n_sampled) {
  if (!shards || ns < 1) return MCL_ERR_INVALID;
  for (int s = 0; s < ns; ++s)
    if (!shards[s]) return MCL_ERR_INVALID;
  if (!beams_out || !n_sampled) return fail(shards[0], MCL_ERR_INVALID, "group_ping_innovation: null argument");
  const InnovPing p = {ranges, beam_angles, B, sigma, support_k, r_max, sensor_offset, max_samples};
  return group_innovation_run(shards, ns, p, beams_out, n_sampled);
}

// ---- ping information (include/mcl_information.h; host: mcl_host_information.h, kernel: csrc/mcl_information.h)
int mcl_information_merge(const mcl_information_sums* parts, int32_t n_parts, int32_t B, mcl_information_sums* out) {
  return information_merge_impl(parts, n_parts, B, out);
}

int mcl_information_matrix(const mcl_information_sums* recs, int32_t count, int32_t per_pose, double sigma, double delta_xy,
                           double delta_yaw, mcl_information_result* out) {
  return information_matrix_impl(recs, count, per_pose, sigma, delta_xy, delta_yaw, out);
}

int mcl_ping_information(mcl_handle* h, const float* beam_angles, int32_t B, double r_max, const double sensor_offset[6],
                         int32_t max_samples, const mcl_information_steps* steps, mcl_information_sums* beams_out,
                         float* ranges_out, int64_t* n_sampled) {
  if (!h) return MCL_ERR_INVALID;
  if (!beams_out || !n_sampled) return fail(h, MCL_ERR_INVALID, "ping_information: null argument");
  const InfoPing p = {beam_angles, B, r_max, sensor_offset, steps};
  return information_run(h, p, max_samples, beams_out, ranges_out, n_sampled);
}

int mcl_group_ping_information(mcl_handle** shards, int32_t ns, const float* beam_angles, int32_t B, double r_max,
                               const double sensor_offset[6], int32_t max_samples, const mcl_information_steps* steps,
                               mcl_information_sums* beams_out, int64_t* n_sampled) {
  if (!shards || ns < 1) return MCL_ERR_INVALID;
  for (int s = 0; s < ns; ++s)
    if (!shards[s]) return MCL_ERR_INVALID;
  if (!beams_out || !n_sampled) return fail(shards[0], MCL_ERR_INVALID, "group_ping_information: null argument");
  const InfoPing p = {beam_angles, B, r_max, sensor_offset, steps};
  return group_information_run(shards, ns, p, max_samples, beams_out, n_sampled);
}

int mcl_pose_information(mcl_handle* h, const double* poses, int64_t M, const float* beam_angles, int32_t B, double r_max,
                         const double sensor_offset[6], const mcl_information_steps* steps, mcl_information_sums* poses_out) {
  if (!h) return MCL_ERR_INVALID;
  if (!poses_out) return fail(h, MCL_ERR_INVALID, "pose_information: null argument");
  const InfoPing p = {beam_angles, B, r_max, sensor_offset, steps};
  return pose_information_run(h, p, poses, M, poses_out);
}

// ---- ping matching (include/mcl_match.h; host: mcl_host_match.h, kernel: csrc/mcl_match.h)
int mcl_match_config_check(const mcl_match_config* cfg, double r_max, const char** reason) {
  return match_config_check_impl(cfg, r_max, reason);
}

int mcl_match_solve(const mcl_match_sums* rec, const mcl_match_config* cfg, int32_t j, double delta_out[4], int32_t* dead_out) {
  return match_solve_impl(rec, cfg, j, delta_out, dead_out);
}

int mcl_match_better(const mcl_match_sums* q, const mcl_match_sums* p, int32_t min_beams, int32_t* better) {
  return match_better_impl(q, p, min_beams, better);
}

int mcl_match_derived(const mcl_match_sums* rec, const mcl_match_config* cfg, double sigma, mcl_match_derived_t* out) {
  return match_derived_impl(rec, cfg, sigma, out);
}

int mcl_match_ping(mcl_handle* h, const double* poses, int64_t M, const float* ranges, const float* beam_angles, int32_t B,
                   double sigma, double r_max, const double sensor_offset[6], const mcl_match_config* cfg,
                   mcl_match_result* results_out, mcl_match_trace* trace_out, float* ranges_out) {
  if (!h) return MCL_ERR_INVALID;
  if (!results_out) return fail(h, MCL_ERR_INVALID, "match_ping: null argument");
  const MatchPing p = {ranges, beam_angles, B, sigma, r_max, sensor_offset, cfg};
  return match_run(h, p, poses, M, results_out, trace_out, ranges_out);
}

// ---- swath matching (include/mcl_swath.h; host: mcl_host_swath.h, kernel: csrc/mcl_swath.h)
int mcl_swath_offsets(const double* poses6, int32_t K, int32_t anchor, mcl_swath_offset* out) {
  return swath_offsets_impl(poses6, K, anchor, out);
}

int mcl_swath_check(int32_t K, int32_t B, const mcl_swath_offset* offsets, const char** reason) {
  return swath_check_impl(K, B, offsets, reason);
}

int mcl_swath_solve(const mcl_match_sums* rec, const mcl_match_config* cfg, int32_t j, double delta_out[4], int32_t* dead_out) {
  return match_solve_impl(rec, cfg, j, delta_out, dead_out, MCL_SWATH_MAX_BEAMS);
}

int mcl_swath_better(const mcl_match_sums* q, const mcl_match_sums* p, int32_t min_beams, int32_t* better) {
  return match_better_impl(q, p, min_beams, better, MCL_SWATH_MAX_BEAMS);
}

int mcl_swath_derived(const mcl_match_sums* rec, const mcl_match_config* cfg, double sigma, mcl_match_derived_t* out) {
  return match_derived_impl(rec, cfg, sigma, out, MCL_SWATH_MAX_BEAMS);
}

int mcl_match_swath(mcl_handle* h, const double* poses, int64_t M, const float* ranges, const float* beam_angles, int32_t B,
                    const mcl_swath_offset* offsets, int32_t K, double sigma, double r_max, const double sensor_offset[6],
                    const mcl_match_config* cfg, mcl_match_result* results_out, mcl_match_trace* trace_out, float* ranges_out) {
  if (!h) return MCL_ERR_INVALID;
  if (!results_out) return fail(h, MCL_ERR_INVALID, "match_swath: null argument");
  const Swath s = {{ranges, beam_angles, B, sigma, r_max, sensor_offset, cfg}, offsets, K};
  return swath_run(h, s, poses, M, results_out, trace_out, ranges_out);
}

// ---- sensor resetting (include/mcl_reseed.h; host: mcl_host_reseed.h, kernel: csrc/mcl_reseed.h)
int mcl_reseed_select_check(const mcl_reseed_select_config* cfg, const char** reason) {
  return reseed_select_check_impl(cfg, reason);
}

int mcl_reseed_components_check(const mcl_reseed_component* comps, int32_t n_comp, const char** reason) {
  return reseed_components_check_impl(comps, n_comp, reason);
}

int mcl_reseed_select(const mcl_match_result* results, int64_t M, const mcl_match_config* mcfg, double sigma,
                      const mcl_reseed_select_config* cfg, mcl_reseed_component* comps_out, int64_t* index_out,
                      int32_t* n_out) {
  return reseed_select_impl(results, M, mcfg, sigma, cfg, comps_out, index_out, n_out);
}

int mcl_inject_gaussian(mcl_handle* h, double fraction, const mcl_reseed_component* comps, int32_t n_comp,
                        const double* replay, int64_t* n_injected) {
  if (!h) return MCL_ERR_INVALID;
  if (!comps) return fail(h, MCL_ERR_INVALID, "inject_gaussian: null components");
  if (!(fraction >= 0.0 && fraction <= 1.0)) return fail(h, MCL_ERR_INVALID, "inject_gaussian: fraction outside [0, 1]");
  if (h->have_lw) return fail(h, MCL_ERR_STATE, "inject_gaussian: log-weights pending (resample first: they describe the particles as they are)");
  RET_IF(set_device(h));
  return reseed_inject(h, fraction, comps, n_comp, replay, n_injected);
}

// ---- KLD-sampling across handles (include/mcl_kld.h; host: mcl_host_kld.h, kernels: csrc/mcl_kld.h)
int mcl_kld_grid_check(const mcl_mode_grid* g, int64_t* n_cells) { return kld_grid_check_impl(g, n_cells, nullptr); }

int mcl_kld_bound(int64_t k, double epsilon, double z, int64_t n_min, int64_t n_max, int64_t* n) {
  return kld_bound_impl(k, epsilon, z, n_min, n_max, n);
}

int mcl_kld_bins(mcl_handle* h, const mcl_mode_grid* g, int64_t* k, int64_t* n_inside, int64_t* n_outside) {
  if (!h) return MCL_ERR_INVALID;
  if (!g) return fail(h, MCL_ERR_INVALID, "kld_bins: null grid");
  int64_t n_cells = 0;
  const char* reason = nullptr;
  if (kld_grid_check_impl(g, &n_cells, &reason) != MCL_OK) return fail(h, MCL_ERR_INVALID, std::string("kld_bins: ") + reason);
  if (h->world > 1) return fail(h, MCL_ERR_UNSUPPORTED, "kld_bins: a sharded cloud (world > 1) is not supported");
  if (!h->have_state) return fail(h, MCL_ERR_STATE, "kld_bins: no particles (call mcl_init_particles / mcl_set_particles first)");
  RET_IF(set_device(h));
  return kld_bins_run(h, g, n_cells, k, n_inside, n_outside);
}

int mcl_resample_into(mcl_handle* src, mcl_handle* dst, const double* uniform) {
  if (!src || !dst) return MCL_ERR_INVALID;
  if (src == dst) return fail(dst, MCL_ERR_INVALID, "resample_into: src and dst are the same handle");
  uint64_t u53 = 0;
  if (!kld_transfer_u53(uniform, dst->cfg.seed, dst->step_transfer, &u53)) return fail(dst, MCL_ERR_INVALID, "resample_into: u not in [0,1)");
  int code = MCL_OK;
  if (const char* why = transfer_refused(src, dst, &code)) return fail(dst, code, why);
  RET_IF(set_device(dst));
  return transfer_run(src, dst, u53);
}

int mcl_transfer_last_indices(mcl_handle* dst, int32_t* idx) {
  if (!dst || !idx) return MCL_ERR_INVALID;
  if (!dst->have_transfer) return fail(dst, MCL_ERR_STATE, "transfer_last_indices: no transfer into this handle yet");
  RET_IF(set_device(dst));
  HIPCHK(dst, hipMemcpyAsync(idx, dst->xfer_idx, sizeof(int) * (size_t)dst->n, hipMemcpyDeviceToHost, dst->stream));
  HIPCHK(dst, hipStreamSynchronize(dst->stream));
  return MCL_OK;
}

int mcl_timing_enable(mcl_handle* h, int32_t on) {
  if (!h) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  t_collect(h);
  h->timing = on != 0;
  return MCL_OK;
}

int mcl_timing_get(mcl_handle* h, mcl_timing* out) {
  if (!h || !out) return MCL_ERR_INVALID;
  RET_IF(set_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  t_collect(h);
  *out = h->tacc;
  memset(&h->tacc, 0, sizeof h->tacc);
  return MCL_OK;
}

}  // extern "C"

#ifdef SWEEP_TIMELINE
// debug builds only (tools/sweep_timeline.py): the per-wave clock records of the last sweep launch
extern "C" int mcl_debug_sweep_timeline(unsigned long long* out, int n_waves) {
  if (n_waves > SWEEP_TL_WAVES) n_waves = SWEEP_TL_WAVES;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sweep_tl), (size_t)n_waves * 6 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

