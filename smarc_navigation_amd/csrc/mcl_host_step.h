// mcl_host_step.h -- host side of libmcl_hip.so, part 7: the front half of the fused step -- checks, staging, then
// predict + MBES update (+ landmark update) -- written once for one handle (mcl_step_mbes*) and for a LOCAL group of
// shards (mcl_group_step_mbes*).  The callers (mcl_api.hip) resample and keep their own unwinding.
#pragma once

namespace {

// what the four entry points pass through
struct StepIn {
  const mcl_odom* odom;
  double dt;
  const float *ranges, *beam_angles;
  int B;
  double sigma, r_max;
  const double* sensor_offset;
  const LandmarkObs* lm;   // the landmark observation of the same ping, or nullptr
  const char* who;
};

// the checks of one handle.  sharded: a shard of a LOCAL group (no communicator needed; the systematic scheme only)
int step_check(mcl_handle* h, const StepIn& in, bool sharded) {
  const std::string w(in.who);
  if (h->cfg.rng_mode != MCL_RNG_NATIVE) return fail(h, MCL_ERR_INVALID, w + ": NATIVE rng only");
  if (!sharded && h->world > 1 && !h->comm) return fail(h, MCL_ERR_STATE, w + ": multi-shard handle needs mcl_comm_init");
  if (in.B < 1 || !(in.sigma > 0.0) || !(in.r_max > 0.0)) return fail(h, MCL_ERR_INVALID, w + ": bad argument");
  RET_IF(need_map(h, in.who));
  if (sharded && h->cfg.resample_scheme != MCL_RESAMPLE_SYSTEMATIC && h->cfg.resample_scheme != MCL_RESAMPLE_NAIVE)
    return fail(h, MCL_ERR_UNSUPPORTED, w + ": only the systematic scheme is sharded");
  return in.lm ? need_feature_map(h, in.who) : MCL_OK;
}

// everything that can fail before a kernel is queued.  The beam table first (the group classification in the predict's
// pose kernel follows the two extreme beams); the landmarks after it: upload_beams forgets detections an earlier call
// left waiting
int step_stage(mcl_handle* h, const StepIn& in) {
  RET_IF(set_device(h));
  RET_IF(upload_beams(h, in.ranges, in.beam_angles, in.B));
  return in.lm ? landmarks_prepare(h, *in.lm, in.who, true) : MCL_OK;
}

// predict and updates, up to the resample; the first failure.  defer_uniform: the gather of this call substitutes z,
// roll, pitch -- the predict kernel does not store them, and the caller materialises them on any way out but that gather.
// overlap_gather: the state all-gather of the resample starts behind the predict, under the ray-cast
int step_front(mcl_handle* h, const StepIn& in, bool defer_uniform, bool overlap_gather) {
  MbesPlan plan;
  RET_IF(plan_mbes(h, in.B, in.sigma, in.r_max, in.sensor_offset, nullptr, plan));
  // predict writes the MBES pose records of the new state in the same pass (the map and sensor offset are known here)
  bool pose_done = false;
  RET_IF(do_predict(h, in.odom, in.dt, nullptr, &plan.args, &pose_done, defer_uniform));
  if (h->fault_step) return fail(h, MCL_ERR_STATE, std::string(in.who) + ": injected fault after predict");
  if (overlap_gather) RET_IF(start_state_gather(h));
  RET_IF(run_mbes(h, plan, pose_done));   // (the sweep leaves max lw in the slots)
  weights_written(h, MCL_WEIGHT_LOG_SHIFT, SLOTS_SET0);
  // the landmark likelihood of the same ping on top (BASELINE config 5): reads the state the predict left (z, roll,
  // pitch from the odometry when that kernel did not store them), leaves max lw in the second slot set
  return in.lm ? landmarks_launch(h, *in.lm, true, true) : MCL_OK;
}

}  // namespace
