// mcl_host_landmarks.h -- host side of libmcl_hip.so, part 5: the landmark updates (mcl_landmarks.h).  A plan --
// landmarks_prepare: argument checks and the cell grid for this gate radius -- and one launcher per kernel:
// landmarks_launch (k_landmark_update; alone or inside the fused step) and landmarks_assign_launch (k_landmark_assign).
#pragma once

namespace {

// one landmark observation (mcl_update_landmarks' arguments; the assignment update: k = k_cand)
struct LandmarkObs {
  const double* det;
  int n_det;
  double sigma;
  int k;
  double gate;
  const double* so;
};
int landmarks_upload(mcl_handle* h, const LandmarkObs& o) {
  RESERVE(h, h->det_dev, 3 * (size_t)o.n_det);
  return upload(h, h->det_dev, o.det, sizeof(double) * 3 * (size_t)o.n_det);
}
void landmark_noise_args(const LandmarkDev* L, double sigma, LandmarkArgs& a) {
  a.maha = L->maha ? 1 : 0;
  a.lmcov = L->lmcov;
  landmark_q(L->have_q ? L->Q : nullptr, sigma, a.Q);
  a.logdet_q = std::log(sym3_det(a.Q));
  a.lognorm = 1.5 * std::log(2.0 * MCL_PI) + 0.5 * a.logdet_q;  // isotropic: 3/2 log 2pi + 3 log sigma
}
// the cell grid depends on the gate radius only: rebuilt (the stream drained first -- the old arrays may still be read by
// a kernel in flight) only when that changes
int ensure_landmark_grid(mcl_handle* h, double sigma, double gate) {
  LandmarkDev* L = h->landmarks;
  double Q[6];
  landmark_q(L->have_q ? L->Q : nullptr, sigma, Q);
  const double radius = landmark_gate_radius(L->maha, L->lam_cov_max, Q, sigma, gate);
  if (L->built_for == radius && L->lm) return MCL_OK;
  std::string err;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int rc = landmarks_build(L, radius, &err);
  if (rc != MCL_OK) h->err = err;
  return rc;
}
// argument checks and the cell grid.  (A grid rebuild drains the stream, so the fused step calls this BEFORE its predict.)
// ride: the fused step -- the detections are not copied here; they wait for the beam table's staged copy of the same
// step (upload_sweep_beams; landmarks_launch copies them itself if the update took a path without that table)
int landmarks_prepare(mcl_handle* h, const LandmarkObs& o, const char* who, bool ride = false) {
  if (!o.det || o.n_det < 1 || !(o.sigma > 0.0) || o.k < 1 || o.k > LM_MAX_K || !(o.gate > 0.0))
    return fail(h, MCL_ERR_INVALID, std::string(who) + ": bad argument (1 <= k <= 4)");
  RET_IF(need_feature_map(h, who));
  RET_IF(set_device(h));
  RET_IF(ensure_landmark_grid(h, o.sigma, o.gate));
  h->det_ride = nullptr;
  h->det_ride_dev = nullptr;
  if (ride) {
    h->det_ride = o.det;
    h->det_ride_n = o.n_det;
  }
  return MCL_OK;   // (landmarks_launch copies detections that did not ride)
}
// what both kernels read: the state as stored, frames, detections (det_dev: on the device), cell grid, noise, k, lw
void landmark_args(const mcl_handle* h, const LandmarkObs& o, const double* det_dev, bool accumulate, LandmarkArgs& a) {
  static const double zero6[6] = {0, 0, 0, 0, 0, 0};
  const double* so = o.so ? o.so : zero6;
  const LandmarkDev* L = h->landmarks;
  memset(&a, 0, sizeof a);   // (uni_mask = 0, max_slots = nullptr: the state is read as stored)
  for (int c = 0; c < 6; ++c) a.st[c] = h->state[h->cur] + (size_t)c * h->n;
  a.n = h->n;
  for (int q = 0; q < 12; ++q) a.m2o[q] = h->cfg.m2o[q];
  for (int q = 0; q < 3; ++q) a.off_t[q] = so[q];
  rot_rpy(so[3], so[4], so[5], a.off_R);
  a.det = det_dev;
  a.n_det = o.n_det;
  a.lm = L->lm;
  a.cell_start = L->cell_start;
  a.nb_cell = L->nb_cell;
  a.nb_list = L->nb_list;
  a.gx = L->gx;
  a.gy = L->gy;
  a.x0 = L->x0;
  a.y0 = L->y0;
  a.inv_cs = 1.0 / L->cs;
  a.inv_s2 = 1.0 / (o.sigma * o.sigma);
  a.gate = o.gate;
  landmark_noise_args(L, o.sigma, a);
  a.k = o.k;
  a.accumulate = accumulate ? 1 : 0;
  a.lw = h->lw;
}
// the k-NN landmark likelihood of every particle.  fused: inside mcl_step_mbes_landmarks -- the predict kernel of the
// same call may have left z, roll, pitch unstored (uni_deferred), and the kernel leaves max lw in the second slot set
int landmarks_launch(mcl_handle* h, const LandmarkObs& o, bool accumulate, bool fused) {
  // the detections: where the beam table's copy of this step left them, or (an update without that table: no sweep)
  // copied now
  const double* det = h->det_ride_dev;
  if (!det) {
    RET_IF(landmarks_upload(h, o));
    det = h->det_dev;
  }
  h->det_ride = nullptr;
  h->det_ride_dev = nullptr;
  LandmarkArgs a;
  landmark_args(h, o, det, accumulate, a);
  a.uni_mask = (fused && h->uni_deferred) ? UNI_ZRP : 0u;
  for (int c = 0; c < 3; ++c) a.uni[c] = h->uni_val[c];
  a.max_slots = fused ? (u64*)(h->ctrl + CTRL_SLOTS2) : nullptr;   // (zeroed with the whole block by this step's predict / pose launch)
  t_begin(h, MCL_K_UPDATE_LANDMARKS);
  long long blocks = (h->n + 255) / 256;   // (a wave per 64 particles, four waves per workgroup)
  if (blocks > 16384) blocks = 16384;
  if (a.maha)
    k_landmark_update<true><<<(unsigned)blocks, 256, 0, h->stream>>>(a);
  else
    k_landmark_update<false><<<(unsigned)blocks, 256, 0, h->stream>>>(a);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  weights_written(h, accumulate ? WEIGHT_MODE_KEEP : MCL_WEIGHT_LOG_SHIFT, fused ? SLOTS_SET1 : SLOTS_NONE);
  return MCL_OK;
}
// the joint assignment of the detections of every particle (o.k candidates per detection), its log-likelihood into lw and
// the choices of the first n_keep particles into assign_out: every particle gets a conflict-free answer or a worklist
// entry; then the solver runs over the worklist (its grid strides over the device-side count)
int landmarks_assign_launch(mcl_handle* h, const LandmarkObs& o, double new_mh_dist, bool accumulate, int32_t* assign_out,
                            long long n_keep) {
  h->det_ride = nullptr;   // (detections a failed fused step left waiting are not this call's)
  h->det_ride_dev = nullptr;
  RET_IF(landmarks_upload(h, o));
  if (n_keep > h->n) n_keep = h->n;
  if (n_keep > 0) RESERVE(h, h->asg_dev, (size_t)n_keep * (size_t)o.n_det);
  RESERVE(h, h->lm_worklist, (size_t)h->n + 1);
  LandmarkAssignArgs aa;
  landmark_args(h, o, h->det_dev, accumulate, aa.base);
  aa.orig = h->landmarks->orig;
  aa.new_mh = new_mh_dist;
  aa.k_cand = o.k;
  aa.assign_out = n_keep > 0 ? h->asg_dev.p : nullptr;
  aa.n_keep = n_keep;
  aa.worklist = h->lm_worklist;
  aa.work_count = h->lm_worklist + h->n;
  HIPCHK(h, hipMemsetAsync(aa.work_count, 0, sizeof(int), h->stream));
  t_begin(h, MCL_K_UPDATE_LANDMARKS);
  long long blocks = (h->n + LA_PER_BLOCK - 1) / LA_PER_BLOCK;
  if (blocks > 32768) blocks = 32768;
  k_landmark_assign<false><<<(unsigned)blocks, LA_PER_BLOCK * LM_SUB, 0, h->stream>>>(aa);
  k_landmark_assign<true><<<(unsigned)std::min<long long>(blocks, 2048), LA_PER_BLOCK * LM_SUB, 0, h->stream>>>(aa);
  t_end(h);
  HIPCHK(h, hipGetLastError());
  if (n_keep > 0) {
    HIPCHK(h, hipMemcpyAsync(assign_out, aa.assign_out, sizeof(int) * (size_t)n_keep * o.n_det, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  weights_written(h, accumulate ? WEIGHT_MODE_KEEP : MCL_WEIGHT_LOG_SHIFT, SLOTS_NONE);
  return MCL_OK;
}

}  // namespace
