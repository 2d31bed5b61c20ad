// mcl_host.h -- host side of libmcl_hip.so, part 1: the handle (device buffers, streams, communicators, caches) and
// the helpers every other part uses (error macros, launch geometry, timing regions, Philox on the host, uploads).
// One translation unit: mcl_api.hip includes mcl_host.h, mcl_host_resample.h, mcl_host_moments.h, mcl_host_update.h,
// mcl_host_landmarks.h, mcl_host_ranges.h, mcl_host_step.h, mcl_host_history.h, mcl_host_acoustic.h, mcl_host_temper.h,
// mcl_host_drift.h, mcl_host_regularise.h, mcl_host_quantile.h, mcl_host_innovation.h (with the pipeline of the two ping
// statistics), mcl_host_information.h (which includes it), mcl_host_recovery.h, mcl_host_modes.h, mcl_host_kld.h
// in this order and then defines the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mcl.h"
#include "mcl_host_pure.h"
#include "mcl_kernels.h"
#include "mcl_mbes.h"
#include "mcl_sweep.h"
#include "mcl_slice.h"
#include "mcl_mesh.h"
#include "mcl_resample.h"
#include "mcl_resample_alt.h"
#include "mcl_landmarks.h"
#include "mcl_ranges.h"
#include "mcl_modes.h"
#include "mcl_history.h"
#include "mcl_drift.h"
#include "mcl_regularise.h"

#define MEAN_RING 4096
#define RING_STRIDE 20  // doubles per mean/cov result: 16 payload + [16] format tag + [17..19] the two-pass form's shift
// control block layout (bytes)
#define CTRL_SLOTS 0                       // MCL_MAX_SLOTS u64
#define CTRL_WORK (8 * MCL_MAX_SLOTS)      // int: groups deferred by the fast MBES kernel
#define CTRL_DEFER (CTRL_WORK + 4)         // int: particles the fan sweep handed to the general kernel
#define CTRL_LOOSE (CTRL_WORK + 8)         // int: groups the fan slice's group kernel left to the per-particle kernel
#define CTRL_T_QUANT (CTRL_WORK + 12)      // u32 tickets, self-resetting
#define CTRL_T_EXPAND (CTRL_WORK + 16)
#define CTRL_T_GATHER (CTRL_WORK + 20)
#define CTRL_T_VISIT (CTRL_WORK + 24)
#define CTRL_DEFER2 (CTRL_WORK + 28)       // int: particles the fan slice, as the TIN sweep's hand-over kernel, handed on to the general kernel
#define CTRL_SLOTS2 1024                   // a second set of MCL_MAX_SLOTS u64: max lw after the fused landmark update
#define CTRL_BYTES 2048

namespace {

thread_local std::string g_create_err;

struct TimedRegion {
  hipEvent_t a, b;
  int k;
  bool open;
};

// where the resample gather leaves the 13 moment sums of a fused step (decided by plan_gather, read by
// collect_fused_moments)
//   SCAL          scal[32..47]: reduced over the shards, then copied to the ring
//   SHARD_RECORD  the shard's record: they ride with the NEXT step's all-gather
//   RING_DIRECT   single shard: the kernel's last block writes the pinned ring entry itself
enum MomentsDest { MOMENTS_SCAL, MOMENTS_SHARD_RECORD, MOMENTS_RING_DIRECT };

}  // namespace

struct mcl_handle {
  mcl_config cfg;
  long long n = 0, ng = 0, goff = 0;
  int rank = 0, world = 1;
  int device = 0;
  hipStream_t stream = nullptr;
  // particle state: two ping-pong SoA buffers of 6*n doubles; multi-shard: a global copy
  DevBuf<double> state[2];
  int cur = 0;
  DevBuf<double> state_glob;  // 6*ng (world > 1)
  DevBuf<double> lw;          // n log-weights
  DevBuf<double> wnorm;       // n (lazily)
  DevBuf<u64> q;              // n fixed-point weights
  DevBuf<u32> ncum;           // ng offspring CDF (global)
  DevBuf<u32> zcum;           // ng scratch (generic keep/lost/dupes of the explicit-index schemes)
  DevBuf<u32> zr;             // n: rank of a lost slot among the lost slots, or ZR_SURVIVOR
  DevBuf<u32> dupes32;        // ng: dupes[k] = ancestor copied into the k-th lost slot
  DevBuf<u64> desc;           // ntiles_glob look-back descriptors
  DevBuf<unsigned char> ctrl; // control block: max-lw slots | MBES work counter | kernel tickets (CTRL_* offsets)
  u32 epoch = 0;                 // look-back epoch (one per k_cdf_expand launch)
  bool max_valid = false;        // the slots hold max lw of the current log-weights
  int slot_set = 0;              // ... which set: 0 = CTRL_SLOTS (MBES kernels, k_max_slots), 1 = CTRL_SLOTS2 (fused landmark update)
  bool pose_ready = false;       // pose_dev already holds the records of the current state (fused predict)
  DevBuf<u64> tile64;
  DevBuf<u32> tile32;
  long long ntiles_loc = 0, ntiles_glob = 0;
  DevBuf<double> part;     // reduction partials [7][MCL_MAX_GRID]
  DevBuf<double> scal;     // device scalars: [0] max lw, [8..27] the two-pass ring entry (sums7, [15] sum ez, [16..21] cov6, [22..23] sum ex, ey, [24] tag 0, [25..27] shift), [32..47] the fused sums
  DevBuf<u64> totals;      // device, world entries (+1 scratch)
  DevBuf<int> idx;         // n (lazily)
  DevBuf<double> replay_dev;
  DevBuf<double> pose7;
  double* host_pin_dev = nullptr;  // device-side address of host_pin (kernels write results into the ring directly)
  MomentsDest moments_dest = MOMENTS_SCAL;   // of the last gather
  PinBuf<double> host_pin;  // pinned ring: MEAN_RING entries of RING_STRIDE doubles (run_mean_cov_async / k_resample_gather say what lies where)
  long long mean_count = 0;     // number of mean/cov results produced so far
  // MBES
  DevBuf<float2> beam_sc;
  DevBuf<float> ranges_dev;
  DevBuf<float> exp_dev;   // expected ranges (mcl_mbes_expected, mcl_ranges_expected), grown on demand
  DevBuf<MbesPose> pose_dev;
  DevBuf<MbesGroup> mbes_groups;  // one record per group of MBES_WAVES particles
  // visiting order for dispersed clouds: Morton keys, radix sort (rocPRIM), permutation
  DevBuf<u32> sort_keys, sort_keys_out, sort_idx, mbes_perm;
  DevBuf<unsigned char> sort_tmp;
  size_t sort_tmp_bytes = 0;
  // pinned ring of 4 slots x 4 ints, one slot per MBES update: [0] groups the natural-order classification deferred,
  // [1] particles the sweep handed to the general kernel.  An update reads
  // the slot of the update TWO before it, after waiting for that update's event (long since complete when the host
  // runs ahead): the visiting-order and grid-size decisions are a function of the filter's history, never of timing.
  PinBuf<int> work_host;
  hipEvent_t ev_upd[4] = {nullptr, nullptr, nullptr, nullptr};
  unsigned long long upd_seq = 0;
  int env_sort = -1;            // MCL_SORT_VISITS=0/1 forces the decision (tests, A/B)
  DevBuf<int> mbes_worklist;  // ngroups + 1 ints; [ngroups] is the counter
  DevBuf<int> lm_worklist;    // n + 1 ints; [n] is the counter (landmark assignment: particles with clashes)
  // alternative resamplers (lazily allocated)
  DevBuf<u64> cq;       // inclusive scan of q
  DevBuf<u64> u53;      // uniforms as 53-bit integers
  DevBuf<u32> cnt, first, flags, fcum, copies, ccum;
  DevBuf<int> dupes;
  DevBuf<double> cs, chunk, uni_dev;
  long long residual_k = -1;  // copies count cached by mcl_resample_prepare
  bool idx_explicit = false;  // last resample produced idx[] directly (non-systematic)
  int beams_cap = 0;   // beams beam_sc AND ranges_dev have room for (the angle cache describes them): committed when both exist
  std::vector<float> beam_cache;  // last uploaded angles
  int beam_lo = -1, beam_hi = -1;  // extreme-angle beams (footprint shortcut)
  bool beams_sorted = false;
  // fan sweep (mcl_sweep.h)
  std::vector<float> ranges_host;   // last uploaded ranges (the sweep's beam table is built from them)
  bool sweep_angles_ok = false;     // ascending, finite, |a| <= 85 degrees
  int b_split = 0;
  int sweep_cap = 0;
  // the table travels on its own stream into alternating device buffers, so the 12 KiB copy of ping k + 1 overlaps
  // the kernels of ping k instead of standing between two steps (4 us of copy + its launch gaps)
  DevBuf<float> sweep_buf[2];   // a SweepBlock each (mcl_host_update.h)
  PinBuf<float> sweep_stage[2];   // pinned staging, one per buffer
  hipEvent_t ev_stage[2] = {nullptr, nullptr};
  bool stage_used[2] = {false, false};
  int sweep_sel = 0;
  hipStream_t copy_stream = nullptr;
  DevBuf<u32> defer_idx;         // particles the sweep hands to k_mbes_cast<., ., 2>
  DevBuf<u32> defer2_idx;        // TIN with holes: what the fan slice -- the sweep's hand-over kernel there -- declines in turn
  int env_handover_slice = -1;      // MCL_HANDOVER_SLICE=0: the ray traversal takes the TIN sweep's hand-overs even on meshes with holes (A/B)
  int env_sweep_step_cap = 0;       // MCL_SWEEP_STEP_CAP=n: the lattice walk gives up after n steps (tests of the step-limit path; 0: the walk's own limit)
  int env_sweep_wave_cap = 0;       // MCL_SWEEP_WAVE_CAP=n: the wave-level bound of the assembly walk loop (tests; 0: derived from r_max, the resolution and the step cap)
  int env_sweep_uniform = -1;       // MCL_SWEEP_UNIFORM=1: waves of the lattice sweep whose lanes share a path share the walk (mcl_sweep.h; default off: the scalar unit makes it slower than the per-lane loop)
  DevBuf<unsigned long long> sweep_work_dev;   // MCL_DEBUG_WORK: the lattice sweep's (shared, all) walk steps per wave, 64 words
  DevBuf<unsigned> reasons_dev;  // -DSWEEP_REASONS builds: why the sweep declined (16 counters)
  // spatial visiting order of the sweep (mcl_kernels.h: VisitArgs): prepared by the fused step's gather, used by the
  // next fused predict
  DevBuf<u32> visit_okey, visit_base;
  DevBuf<unsigned short> visit_cnt;
  DevBuf<u64> visit_desc;
  u32 visit_epoch = 0;
  DevBuf<VisitPar> visit_par;    // two entries: read / written alternately
  unsigned visit_flip = 0;
  bool gather_attr_set = false;     // k_resample_gather<true, true, true> may use its 112 KiB of dynamic LDS
  bool visit_ready = false;         // okey / hist / binbase describe the slots of the current state
  bool pose_visit = false;          // pose_dev lies in visiting order (written by the last fused predict)
  int env_visit = -1;               // MCL_VISIT=0/1 forces the decision (tests, A/B)
  int visit_nb[3] = {16, 32, 8};    // MCL_VISIT_BINS=x,y,yaw  (measured at 1 M x 512, sweep us: 8,8,8 277; 16,16,8 268; 16,16,16 265; 16,32,8 263)
  float visit_range = 2.5f;         // MCL_VISIT_RANGE: bins span mean +- range * sigma  (headline sweep us -- 4: 260.5, 3: 257.2, 2.5: 257.1; the tempered filter -- 4: 300, 3: 294, 2: 288)
  long long visit_min_n = 393216;   // MCL_VISIT_MIN_N: smaller shards are visited in slot order (the order costs ~20 us per step whatever
                                    // the size -- a launch, a second gather pass, scattered record stores --: measured worth +5 us at
                                    // 524 288 x 512, -9 us at 65 536 x 256)
  int env_sweep = -1;               // MCL_SWEEP=0/1 forces the decision (tests, A/B)
  int env_nsub = 0;                 // MCL_SWEEP_NSUB=1/2/4 forces the lanes per particle side (A/B)
  bool sweep_now = false;           // the fan sweep casts the current / last update (decided by plan_mbes)
  bool slice_now = false;           // ... the fan slice (mcl_slice.h) casts it
  bool handover_slice_now = false;  // the last update's sweep hand-overs went through the fan slice first (TIN with holes)
  int env_slice = -1;               // MCL_SLICE=0 keeps the ray traversal on triangle soups (tests, A/B)
  int env_slice_group = -1;         // MCL_SLICE_GROUP=0: the fan slice casts every particle on its own (no shared candidate lists)
  DevBuf<u32> slice_loose;       // k_mbes_slice_group: the groups of SLICE_G pose records it left to k_mbes_slice
  bool slice_attr_set = false;
  bool slice_group_ran = false;     // the last sliced update went through k_mbes_slice_group first
  size_t slice_attr_bytes = 0;
  DevBuf<float> grid;
  DevBuf<float> grid_pad;   // the same heights inside a one-node ring of NaNs (fan sweep: MbesArgs::grid_pad)
  int gnx = 0, gny = 0;
  double gox = 0, goy = 0, gres = 1;
  float gzmin = 0, gzmax = 0;
  double gslope_max = 0;       // steepest patch gradient of the height grid (the fan sweep's tilt bound)
  MeshDev* mesh = nullptr;
  LandmarkDev* landmarks = nullptr;
  DevBuf<double> det_dev;   // 3 x detections, grown on demand
  // fused landmark step: the detections ride in the per-ping beam table's staged copy (its own stream, under the previous
  // step's kernels) instead of a copy on the compute stream in front of the predict
  const double* det_ride = nullptr;      // host detections waiting for the next table upload (3 x det_ride_n doubles)
  int det_ride_n = 0, det_ride_cap = 0;  // ... their count; room for them behind either table buffer
  const double* det_ride_dev = nullptr;  // where that upload put them (device), until the landmark kernel is launched
  int map_kind = -1;  // 0 grid, 1 mesh
  bool mesh_heightfield = false;
  bool force_general_mesh = false;  // MCL_MESH_GENERAL / MCL_MESH_UNSTRUCTURED: no structured-mesh fast path
  bool mesh_no_sweep = false;       // MCL_MESH_GENERAL: triangle-record traversal only (no adjacency sweep either)
  // bookkeeping
  int weight_mode = 0;
  bool have_lw = false, have_cdf = false, have_meancov = false;
  uint32_t step_predict = 0, step_resample = 0;
  // global localisation / recovery (include/mcl_recovery.h)
  uint32_t step_inject = 0;       // Philox step of the next mcl_inject_uniform / mcl_inject_gaussian; reset by both init calls
  double map_xy[4] = {0, 0, 0, 0};  // footprint of the map (x_min, x_max, y_min, y_max; MAP frame), valid while map_kind >= 0
  DevBuf<double> wstats_dev;   // weight statistics: WS_OUT_WORDS result words, then one 32-byte record per tile (lazily)
  DevBuf<u64> inject_cnt;      // injection: the replaced-particle total, then one count per workgroup (lazily)
  DevBuf<double> reseed_tab;   // sensor resetting (include/mcl_reseed.h): the component table of csrc/mcl_reseed.h, RESEED_TAB_WORDS (lazily)
  DevBuf<u64> temper_dev;      // tempering (include/mcl_temper.h): the state block of csrc/mcl_temper.h, TP_WORDS (lazily)
  // dominant modes (include/mcl_modes.h; all lazily)
  bool have_state = false;     // the particles were initialised (either init call, mcl_set_particles)
  DevBuf<u32> modes_hist;      // H: particles per cell of the caller's lattice
  DevBuf<u32> modes_score;     // S: the window sums of H, dense
  DevBuf<u32> modes_cell;      // n: the cell id of every particle (MODES_OUTSIDE: none)
  DevBuf<u64> modes_rec;       // per-workgroup records: MCL_MAX_GRID outside counts, then MCL_MAX_GRID selection keys
  DevBuf<double> modes_part;   // per-workgroup moment sums [k][MODES_SUMS][grid]
  DevBuf<double> modes_res;    // MODES_RES_WORDS: the summed moments, the peaks, the outside count
  // KLD-sampling across handles (include/mcl_kld.h; all lazily)
  DevBuf<u32> kld_bits;        // mcl_kld_bins: one bit per cell of the caller's lattice; all zero between calls
  bool kld_dirty = false;      // ... unless a call ended between its mark and its count: the next one clears the bitmap
  DevBuf<u64> kld_rec;         // per-workgroup records: MCL_MAX_GRID outside counts, MCL_MAX_GRID cell counts, then the two sums
  uint32_t step_transfer = 0;  // mcl_resample_into with this handle as dst: successful calls so far, the Philox step of the next one
  bool have_transfer = false;  // xfer_idx holds the ancestors of a transfer
  DevBuf<u64> xfer_q;          // the transfer's scratch, sized by SRC: fixed-point weights (n_src)
  DevBuf<u64> xfer_tile;       // ... tile sums, the total, MCL_MAX_SLOTS max-lw slots
  DevBuf<u32> xfer_ncum;       // ... offspring CDF for this handle's n positions (n_src)
  DevBuf<int> xfer_idx;        // n: the ancestors of the last transfer
  // particle genealogy (include/mcl_history.h; all allocated by mcl_history_enable, freed by mcl_history_disable)
  bool hist_on = false;
  int hist_depth = 0, hist_held = 0, hist_head = -1;   // ring: frames held, index of the newest (-1: none)
  long long hist_recorded = 0;
  bool hist_ident = true;      // the link is the identity (nothing is stored for it: enable, reset, every record)
  int hist_cur = 0;            // which link buffer holds the link when it is not the identity
  DevBuf<u32> hist_link[2];    // n each: link, and where the next compose writes link'
  DevBuf<u32> hist_parent;     // depth x n: the frames' parent slots
  DevBuf<double> hist_xyw;     // depth x 3 x n: the frames' x, y, yaw
  DevBuf<u32> hist_cnt[2];     // n each: descendant counts of the frame the walk is at / of the one before it
  DevBuf<double> hist_part;    // per-workgroup sums [HIST_SUMS][grid]
  DevBuf<double> hist_res;     // depth x HIST_RES_WORDS: the smoother's sums per lag (and the path's records)
  std::vector<double> hist_stamp;   // depth: the frames' stamps
  // per-particle drift states (include/mcl_drift.h; all allocated by mcl_drift_enable, freed by mcl_drift_disable)
  bool drift_on = false;
  mcl_drift_config drift_cfg = {};
  uint32_t drift_step = 0;     // advances since enable / reset: the Philox step of the last one (0: the prior's)
  DevBuf<double> drift_state;  // 3 x n: cx, cy, bw
  DevBuf<double> drift_part;   // per-workgroup sums [DRIFT_SUMS][grid]
  DevBuf<double> drift_res;    // DRIFT_RES_WORDS: the summed moments, the shift
  // regularised resampling (include/mcl_regularise.h; both buffers reserved by the first mcl_regularise)
  uint32_t reg_calls = 0;      // regularise calls so far: the Philox step of the next one
  int32_t reg_dims = 0;        // of the last call (0: there was none)
  double reg_h = 0.0, reg_a = 0.0;   // ... its bandwidth and shrink factor
  DevBuf<double> reg_part;     // per-workgroup sums [REG_SUMS_MAX][grid]
  DevBuf<double> reg_res;      // REG_RES_WORDS: the record of the last call (sums, shift, mean, cov, factor, dead mask)
  DevBuf<u64> quant_dev;       // order statistics (include/mcl_quantile.h): the state block of csrc/mcl_quantile.h, QS_WORDS (lazily)
  DevBuf<u64> beamstat_dev;    // ping innovation and ping information (mcl_host_innovation.h: beamstat_prepare): B beam records of 16 bytes, then
                               // the 5 x B, 9 x B or 9 x M accumulators of the call in flight (lazily; dead once that call has fetched)
  int env_innov_group = 0;     // MCL_INNOVATION_GROUP=n: particles per workgroup of k_innovation (A/B; 0: innovation_group decides)
  DevBuf<double> info_pose;    // ping information: the 6 x M poses of mcl_pose_information (lazily)
  int env_info_group = 0;      // MCL_INFORMATION_GROUP=n: poses per workgroup of k_information (A/B; 0: information_group decides)
  bool timing = false;
  std::vector<TimedRegion> regions;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  mcl_timing tacc;
  ncclComm_t comm = nullptr;
  // overlap of the pre-resample state all-gather with the measurement update (second communicator,
  // second stream); falls back to an in-line gather when the split is unavailable
  ncclComm_t comm2 = nullptr;
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_state_ready = nullptr, ev_gather_done = nullptr;
  bool gather_inflight = false;
  // z, roll, pitch of every particle are the odometry's right after motion_pred: the exchange leaves them out
  bool uni_valid = false;       // true from a predict until the state is written by anything else
  double uni_val[3] = {0, 0, 0};
  unsigned gather_uni_mask = 0; // components the state exchange of THIS resample skipped: written by start_state_gather,
                                // exchange_cdf_state / exchange_cdf_state_group and launch_pack, read by plan_gather (which
                                // substitutes uni_val), cleared by finish_resample
  bool fault_step = false;      // MCL_FAULT_INJECT=step_after_predict (tests): the fused step fails after its predict
  bool uni_deferred = false;    // fused step in flight: the predict kernel did NOT store z, roll, pitch (the gather of
                                // the same call substitutes them; materialise_uniform() on any other way out)
  // O(n)-per-rank resample exchange: hand-over records {L | S << 32, x0, y0, z0} of every shard,
  // surplus copies packed for the peers, copies received for this shard's lost slots
  bool exch_allgather = false;   // MCL_EXCHANGE=allgather: the all-gather exchange of rounds 1-2 instead
  // one collective for "maximum, then totals" (mcl_resample.h: k_quantise_tiles' records, k_shift_scan)
  DevBuf<u64> shrec;          // device: world x SHREC_WORDS all-gathered shard records, then the shift word
  DevBuf<unsigned short> tile_bits;   // device: ntiles_loc x 64 bit counts of this shard's tiles
  const u64* qshift_cur = nullptr;       // the shift the weights in `q` are read with (nullptr: none) -- set by every resample
  bool shrec_dirty = false;              // a launch that accumulates into the record is queued and k_shift_scan (which zeroes it) is not
  // the fused step's moments ride with the NEXT step's records instead of an all-reduce of their own:
  bool mom_pending = false;              // a ring entry is reserved whose sums still lie, per shard, in the records
  long long mom_pending_entry = -1;      // ... which one (index into the result ring, before the modulo)
  DevBuf<u64> lsx;            // device, world x 4 words
  PinBuf<u64, hipHostMallocMapped | hipHostMallocCoherent> lsx_host;   // pinned (fine-grained: the host polls it while kernels run), world x 4 words + the sequence word k_publish_ls writes last
  u64* lsx_host_dev = nullptr;   // its device-side address
  u64 ls_seq = 0;
  DevBuf<double> xsend;       // 6 doubles per entry: xsend.cap / 6 copies
  DevBuf<double> xrecv;       // 6 x n
  std::vector<u32> ex_L, ex_S;   // per shard, filled by exchange_ls
  std::vector<u32> ex_Lpre, ex_Spre;
  unsigned long long ex_sent = 0, ex_lost = 0;  // particle states sent to peers / lost slots, summed over the resamples
  unsigned long long ex_ops = 0, ex_rounds = 0; // point-to-point operations (sends + receives) issued, likewise; exchanges
  int ex_nship = 6;                             // doubles per exchanged copy (3 right after a predict: x, y, yaw)
  bool cdf_global = false;       // ncum holds the GLOBAL offspring CDF (else only this shard's slice)
  std::vector<mcl_handle*> group;  // LOCAL group this shard was last resampled in (lazy CDF all-gather)
  // environment switches, read once in mcl_create (never on the per-measurement path)
  bool env_debug_work = false, env_force_comm = false, env_no_overlap = false;
  // pinned staging so that asynchronous uploads never read caller-owned pageable memory after the call returns
  struct PinSlot {
    PinBuf<unsigned char> buf;
    hipEvent_t ev = nullptr;  // recorded after the async copy out of this slot
    bool used = false;
  } pin_ring[8];
  unsigned pin_next = 0;
  DevBuf<int> asg_dev;  // landmark assignment output (cached, grown on demand)
  std::string err;
};

namespace {

#define HIPCHK(h, call)                                                                        \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      char buf_[512];                                                                          \
      snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      (h)->err = buf_;                                                                         \
      return MCL_ERR_HIP;                                                                      \
    }                                                                                          \
  } while (0)
// room for `count` elements in a DevBuf / PinBuf of the handle (mcl_buffer.h: within its capacity nothing happens; the
// contents are not kept; a failure leaves the buffer empty): MCL_ERR_ALLOC when the memory is not there, else MCL_ERR_HIP
#define RESERVE(h, buf, count)                                                                 \
  do {                                                                                         \
    const int rc_ = (buf).reserve(count);                                                      \
    if (rc_ != MCL_OK) {                                                                       \
      char buf_[512];                                                                          \
      snprintf(buf_, sizeof buf_, "%s.reserve(%s) failed: %s (%s:%d)", #buf, #count, hipGetErrorString(hipGetLastError()), __FILE__, __LINE__); \
      (h)->err = buf_;                                                                         \
      return rc_;                                                                              \
    }                                                                                          \
  } while (0)
#define NCCLCHK(h, call)                                                                       \
  do {                                                                                         \
    ncclResult_t e_ = (call);                                                                  \
    if (e_ != ncclSuccess) {                                                                   \
      char buf_[512];                                                                          \
      snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, ncclGetErrorString(e_), __FILE__, __LINE__); \
      (h)->err = buf_;                                                                         \
      return MCL_ERR_COMM;                                                                     \
    }                                                                                          \
  } while (0)
#define RET_IF(x)           \
  do {                      \
    int rc_ = (x);          \
    if (rc_ != MCL_OK) return rc_; \
  } while (0)

int fail(mcl_handle* h, int code, const char* msg) {
  if (h) h->err = msg;
  return code;
}
int fail(mcl_handle* h, int code, const std::string& msg) { return fail(h, code, msg.c_str()); }

int grid_for(long long n, int block = MCL_BLOCK) {
  long long g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > MCL_MAX_GRID) g = MCL_MAX_GRID;
  return (int)g;
}
int grid_tiles(long long ntiles) {
  if (ntiles < 1) ntiles = 1;
  return (int)(ntiles > MCL_MAX_GRID ? MCL_MAX_GRID : ntiles);
}

StatePtrs state_ptrs(double* base, long long n) {
  StatePtrs s;
  for (int c = 0; c < 6; ++c) s.c[c] = base + (size_t)c * n;
  return s;
}

void t_begin(mcl_handle* h, int k) {
  if (!h->timing) return;
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (!h->ev_pool.empty()) {
    ev = h->ev_pool.back();
    h->ev_pool.pop_back();
  } else {
    // timing-only events: no system-scope fence when they are recorded (a default event releases / acquires at system
    // scope -- a cache write-back and invalidate around every timed region, which made the regions ~20 % longer than
    // the kernels inside them are under rocprofv3)
    if (hipEventCreateWithFlags(&ev.first, hipEventDisableSystemFence) != hipSuccess) (void)hipEventCreate(&ev.first);
    if (hipEventCreateWithFlags(&ev.second, hipEventDisableSystemFence) != hipSuccess) (void)hipEventCreate(&ev.second);
  }
  (void)hipEventRecord(ev.first, h->stream);
  h->regions.push_back(TimedRegion{ev.first, ev.second, k, true});
}
// closes the innermost open region (regions nest: MCL_K_MBES_MAIN inside MCL_K_UPDATE_MBES)
void t_end(mcl_handle* h) {
  if (!h->timing) return;
  for (size_t r = h->regions.size(); r-- > 0;)
    if (h->regions[r].open) {
      h->regions[r].open = false;
      (void)hipEventRecord(h->regions[r].b, h->stream);
      return;
    }
}
void t_collect(mcl_handle* h) {
  for (auto& r : h->regions) {
    float ms = 0.f;
    if (r.open) (void)hipEventRecord(r.b, h->stream);  // (an error return left it open)
    (void)hipEventSynchronize(r.b);
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    h->tacc.ms[r.k] += ms;
    h->tacc.launches[r.k] += 1;
    h->ev_pool.push_back({r.a, r.b});
  }
  h->regions.clear();
}

NoiseArgs noise_args(const mcl_handle* h, const double cov[6], uint32_t purpose, uint32_t step) {
  NoiseArgs a;
  for (int c = 0; c < 6; ++c) a.sq[c] = std::sqrt(cov[c]);
  a.k0 = (uint32_t)h->cfg.seed;
  a.k1 = (uint32_t)(h->cfg.seed >> 32);
  a.step = step;
  a.purpose = purpose;
  a.gid0 = h->goff;
  return a;
}

// Host -> device upload that honours "the caller owns every host buffer" (include/mcl.h): when the call
// returns the caller may overwrite `src`.  Small payloads (ranges, detections, uniforms) are copied into a
// ring of pinned slots and travel asynchronously; large ones (REPLAY normals: the parity path, not the
// production path) are copied synchronously.
int upload(mcl_handle* h, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return MCL_OK;
  if (bytes > (1u << 20)) {
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
  }
  mcl_handle::PinSlot& sl = h->pin_ring[h->pin_next++ % 8u];
  if (sl.used) HIPCHK(h, hipEventSynchronize(sl.ev));
  if (sl.buf.cap < bytes) {
    size_t cap = 4096;
    while (cap < bytes) cap <<= 1;
    RESERVE(h, sl.buf, cap);
  }
  if (!sl.ev) HIPCHK(h, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
  memcpy(sl.buf, src, bytes);
  HIPCHK(h, hipMemcpyAsync(dst, sl.buf, bytes, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipEventRecord(sl.ev, h->stream));
  sl.used = true;
  return MCL_OK;
}

int upload_replay(mcl_handle* h, const double* normals) {
  RESERVE(h, h->replay_dev, 6 * (size_t)h->n);
  return upload(h, h->replay_dev, normals, sizeof(double) * 6 * (size_t)h->n);
}

int set_device(mcl_handle* h) {
  HIPCHK(h, hipSetDevice(h->device));
  return MCL_OK;
}

// z, roll, pitch (components 2, 3, 4) are the same three numbers on every particle of every shard: mcl_handle::uni_valid
constexpr unsigned UNI_ZRP = 0x1cu;
unsigned uni_mask(const mcl_handle* h) { return h->uni_valid ? UNI_ZRP : 0u; }
// the components a state exchange that skips `mask` ships, ascending; returns how many
int shipped_components(unsigned mask, int ship[6]) {
  int nship = 0;
  for (int c = 0; c < 6; ++c) {
    ship[c] = 0;
    if (!((mask >> c) & 1u)) ship[nship++] = c;
  }
  return nship;
}

// New log-weights were written (every update, mcl_set_log_weights): the ONE place that says what they are.
// mode: the new weight_mode, or WEIGHT_MODE_KEEP when the update accumulated onto the weights that were there.
// slots: which slot set the kernel that wrote them left max lw in -- SLOTS_NONE: neither, ensure_max_slots reduces.
// (A stale max_valid would make the resample quantise against the wrong maximum, silently.)
enum WeightSlots { SLOTS_NONE, SLOTS_SET0, SLOTS_SET1 };
constexpr int WEIGHT_MODE_KEEP = -1;
void weights_written(mcl_handle* h, int mode, WeightSlots slots) {
  if (mode != WEIGHT_MODE_KEEP) h->weight_mode = mode;
  h->have_lw = true;
  h->max_valid = slots != SLOTS_NONE;
  if (slots != SLOTS_NONE) h->slot_set = slots == SLOTS_SET1 ? 1 : 0;
  h->residual_k = -1;
}

// The particle state was overwritten by something that is neither a predict nor a resample (init, set_particles,
// injection): an overlapped gather of the old state is forgotten, z / roll / pitch are no longer the odometry's and the
// visiting order no longer describes the slots.  (A stale uni_valid would put the old odometry back, silently.)
int cancel_state_gather(mcl_handle* h);   // (mcl_host_resample.h)
int state_overwritten(mcl_handle* h) {
  RET_IF(cancel_state_gather(h));
  h->uni_valid = false;
  h->visit_ready = false;
  return MCL_OK;
}
// particle genealogy (mcl_host_history.h): the compose behind a resample's gather -- alt: the explicit-index schemes'
// slot map -- and the clean start when the state is overwritten by an init call or mcl_set_particles
int history_after_resample(mcl_handle* h, bool alt);
void history_clear(mcl_handle* h);
// per-particle drift (mcl_host_drift.h): d'[i] = d[A(i)] behind the same gather, by the same slot map
int drift_after_resample(mcl_handle* h, bool alt);
// The filter starts again from fresh particles (both init calls): the Philox steps count from 0, no weights, no CDF.
void filter_restarted(mcl_handle* h) {
  h->step_predict = h->step_resample = h->step_inject = h->step_transfer = 0;
  h->have_lw = h->have_cdf = false;
}

// What a call needs to have been there before it: MCL_ERR_STATE with the one sentence that says what to call first.
int need_map(mcl_handle* h, const char* who) {
  if (h->map_kind >= 0) return MCL_OK;
  return fail(h, MCL_ERR_STATE, std::string(who) + ": no map (call mcl_set_map_grid/mesh first)");
}
int need_feature_map(mcl_handle* h, const char* who) {
  if (h->landmarks) return MCL_OK;
  return fail(h, MCL_ERR_STATE, std::string(who) + ": no feature map (call mcl_set_landmarks first)");
}
int need_weights_to_add(mcl_handle* h, const char* who) {
  if (h->have_lw) return MCL_OK;
  return fail(h, MCL_ERR_STATE, std::string(who) + ": nothing to accumulate onto");
}

// the communicators go (destroyed, or aborted after a collective that hung); an overlapped gather goes with them
void comm_teardown(mcl_handle* h, bool abort) {
  if (h->comm2) (void)(abort ? ncclCommAbort(h->comm2) : ncclCommDestroy(h->comm2));
  if (h->comm) (void)(abort ? ncclCommAbort(h->comm) : ncclCommDestroy(h->comm));
  h->comm2 = nullptr;
  h->comm = nullptr;
  h->gather_inflight = false;
}

}  // namespace
