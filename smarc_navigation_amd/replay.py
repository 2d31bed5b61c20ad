#!/usr/bin/env python3
"""Recorded-stream replay + evaluation.

Replays a recorded input stream (own .npz format, no rosbag dependency) through the node class
(smarc_navigation_amd/auv_pf.py: the same callbacks the rospy wrapper registers) and scores the
result the way the reference's visual_tools.py does: time-synchronised (GPS, DR, PF) samples accumulated per
callback (odom_cb, visual_tools.py:27-37,80-110), the two error series it plots (:127,:135) and its shutdown
summary (finish_hld :61-76: path length of the three tracks and the norm of each track's final position),
plus the RMSE between the PF mean pose and a reference track (the "pose RMSE vs ref" of the metric).

Stream file (np.savez): stamp[n], v[n,3], wz[n], q[n,4], z[n]  (odometry, /sam/dr/odom);
optional gps_idx[k], gps_xy_utm[k,2]; optional mbes_idx[m], mbes_ranges[m,B], mbes_angles[B],
mbes_range_max; optional dr_xyz[n,3] (dead-reckoning track), truth_xyz[n,3]; t0; optional map_z, map_origin,
map_res (a height grid the stream carries: replayed over when no map is given).
A raw-sensor file (ev_t, ev_kind, ev_data as synth.raw_sensor_events makes them; optional gps_map,
pressure_tf) is first run through the dead-reckoning integrator (--raw).

    python -m smarc_navigation_amd.replay stream.npz --particles 65536 [--map-grid map.npz] [--out traj.csv]

rosbag input (BASELINE config 1 is "rosbag replay"): `--bag` reads a ROS 1 bag (format 2.0, rosbag_io.py: no ROS
installation needed) and runs its messages IN RECORDED ORDER through the node's callbacks -- what `rosbag play` into
the live node does (the reference reads its bags with rosbag.Bag(...).read_messages(),
auv_ekf_localization/rosbags/rosbag_handler.py:8-19):

    python -m smarc_navigation_amd.replay run.bag --bag --odom-topic /sam/dr/odom --gps-topic /sam/dr/gps \
        --mbes-topic /sam/mbes_scan --particles 128
"""
import argparse
import json
import math

import numpy as np


def track_metrics(vec):
    """visual_tools.py:61-76 for one 3 x n track: summed segment lengths and |last position|."""
    vec = np.asarray(vec, dtype=np.float64)
    dist = 0.
    for i in range(1, vec.shape[1]):
        dist += np.linalg.norm(vec[:, i] - vec[:, i - 1])
    final = float(np.linalg.norm(vec[:, -1])) if vec.shape[1] else 0.0
    return float(dist), final


class ApproximateTimeSync(object):
    """The time synchroniser visual_tools.py:27-37 relies on: ros_comm's message_filters
    ApproximateTimeSynchronizer (Python implementation, ROS melodic / noetic 1.14-1.16; a third-party
    dependency, not part of the reference repository), restated from its published algorithm:
    every topic keeps the last `queue_size` messages by stamp; when a message arrives, the other topics'
    stamps within `slop` of it are collected, sorted by distance, and the first combination (itertools
    product order: nearest candidates first) whose span is < slop and whose messages are all still queued
    is delivered and removed.  add(topic_index, stamp, msg) returns the delivered tuple or None."""

    def __init__(self, n_topics, queue_size, slop):
        self.queues = [dict() for _ in range(n_topics)]
        self.queue_size, self.slop = int(queue_size), float(slop)

    def add(self, index, stamp, msg):
        import itertools
        q = self.queues[index]
        q[stamp] = msg
        while len(q) > self.queue_size:
            del q[min(q)]
        others = self.queues[:index] + self.queues[index + 1:]
        cands = []
        for oq in others:
            ts = sorted(((s, abs(s - stamp)) for s in oq if abs(s - stamp) <= self.slop), key=lambda x: x[1])
            if not ts:
                return None
            cands.append([s for s, _ in ts])
        for vv in itertools.product(*cands):
            vv = list(vv)
            vv.insert(index, stamp)
            if (max(vv) - min(vv)) < self.slop and all(t in qq for qq, t in zip(self.queues, vv)):
                out = tuple(qq[t] for qq, t in zip(self.queues, vv))
                for qq, t in zip(self.queues, vv):
                    del qq[t]
                return out
        return None


class DRStats(object):
    """Mirror of visual_tools.py's DRStatsVisualization (the reference's evaluation node): GPS fix (utm),
    dead-reckoning odometry and PF odometry, time-synchronised (queue 20, slop 20 s, :27-37), accumulated per
    sample (odom_cb :80-110: the fix is transformed utm -> odom frame with z = 0; the three 3 x k arrays START
    with a zero column, :48-50), scored at shutdown (finish_hld :61-76) and as the two error series the node
    plots (visualize :127,:135).  `utm2odom`: 4x4, or None while the transform is unavailable (the triple
    is then dropped like the node drops it, :108-109)."""

    def __init__(self, queue_size=20, slop=20.0):
        self.sync = ApproximateTimeSync(3, queue_size, slop)
        self.filter_cnt = 1
        self.gps_odom_vec = np.zeros((3, 1))
        self.dr_odom_vec = np.zeros((3, 1))
        self.pf_odom_vec = np.zeros((3, 1))
        self.utm2odom = None

    def odom_cb(self, gps_xyz_utm, dr_xyz, pf_xyz):
        if self.utm2odom is None:
            return False
        g = np.asarray(self.utm2odom, dtype=np.float64).dot([gps_xyz_utm[0], gps_xyz_utm[1], 0.0, 1.0])[:3]
        self.gps_odom_vec = np.hstack((self.gps_odom_vec, g.reshape((3, 1))))
        self.dr_odom_vec = np.hstack((self.dr_odom_vec, np.asarray(dr_xyz, dtype=np.float64).reshape((3, 1))))
        self.pf_odom_vec = np.hstack((self.pf_odom_vec, np.asarray(pf_xyz, dtype=np.float64).reshape((3, 1))))
        self.filter_cnt += 1
        return True

    def add(self, topic, stamp, xyz):
        """topic: 0 gps (utm), 1 dead reckoning, 2 particle filter; runs odom_cb on every synchronised triple"""
        hit = self.sync.add(topic, float(stamp), np.asarray(xyz, dtype=np.float64))
        return self.odom_cb(*hit) if hit is not None else False

    def error_series(self):
        """|gps - pf| and |gps - dr| per accumulated sample (visual_tools.py:127,:135)"""
        return (np.linalg.norm(self.gps_odom_vec - self.pf_odom_vec, axis=0),
                np.linalg.norm(self.gps_odom_vec - self.dr_odom_vec, axis=0))

    def finish_hld(self):
        """the six numbers the node prints at shutdown (visual_tools.py:61-76)"""
        out = {}
        for name, vec in (('GPS', self.gps_odom_vec), ('DR', self.dr_odom_vec), ('PF', self.pf_odom_vec)):
            out[name + ' distance'], out[name + ' final error'] = track_metrics(vec)
        return out


def pose_rmse(est_xy, ref_xy):
    d = np.asarray(est_xy, dtype=np.float64) - np.asarray(ref_xy, dtype=np.float64)
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


class SmoothTrack(object):
    """The fixed-lag smoothed track of a replay (include/mcl_history.h): history is enabled with depth lag + 1 and one
    frame is recorded per resampled ping.  At every record the lag-0 estimate is the FILTERED pose of that ping (the mean of
    the cloud the resample left); once lag + 1 frames are held, the estimate at lag `lag` -- that ping's pose given the
    `lag` pings measured since -- leaves the window and is final.  finish() emits the tail: the frames still in the window,
    smoothed by whatever followed them.  Every entry carries n_unique, the distinct ancestors the cloud had in its frame.

    Cost: one mcl_history_smooth per record -- a walk over ONE frame while the window fills (the filtered pose alone), over
    all lag + 1 frames once it is full (the walk that reaches lag `lag` passes every frame between) -- and one
    synchronisation each: the smoother's price times the ping count, fine for an offline replay, not for a live node.

    A re-initialisation of the particles in mid-stream (mcl_init_particles, mcl_set_particles) clears the ring: the pings
    still in the window can no longer be smoothed.  They are emitted with their filtered pose and n_unique = -1."""

    def __init__(self, engine, lag):
        self.e, self.lag = engine, int(lag)
        self.e.history_enable(self.lag + 1)
        self.idx, self.stamp, self.filtered = [], [], []
        self.smoothed, self.n_unique = [], []
        self._recorded = 0

    def record(self, idx, stamp):
        """call right after a resample (ping `idx` of the stream, at `stamp`)"""
        self.e.history_record(stamp)
        held, recorded, _ = self.e.history_frames()
        if recorded != self._recorded + 1:       # the ring was cleared under us: what was in the window stays unsmoothed
            self._cut()
        self._recorded = recorded
        full = held == self.lag + 1
        est = self.e.history_smooth(held if full else 1)
        self.idx.append(int(idx))
        self.stamp.append(float(stamp))
        self.filtered.append([est[0].x, est[0].y, est[0].yaw])
        if full:
            self._emit(est[self.lag])

    def _emit(self, est):
        self.smoothed.append([est.x, est.y, est.yaw])
        self.n_unique.append(est.n_unique)

    def _cut(self):
        for k in range(len(self.smoothed), len(self.filtered)):
            self.smoothed.append(list(self.filtered[k]))
            self.n_unique.append(-1)

    def finish(self):
        """the tail, then the arrays: dict(idx, stamp, filtered_xyyaw[m,3], smoothed_xyyaw[m,3], n_unique[m], lag)"""
        held, recorded = self.e.history_frames()[:2] if self.idx else (0, 0)
        if recorded != self._recorded:
            self._cut()
        elif held:
            est = self.e.history_smooth(held)
            first = held - 2 if held == self.lag + 1 else held - 1   # (a full window's oldest frame is out already)
            for k in range(first, -1, -1):
                self._emit(est[k])
        return dict(idx=np.array(self.idx, dtype=np.int64), stamp=np.array(self.stamp),
                    filtered_xyyaw=np.array(self.filtered).reshape(-1, 3), smoothed_xyyaw=np.array(self.smoothed).reshape(-1, 3),
                    n_unique=np.array(self.n_unique, dtype=np.int64), lag=self.lag)


def smooth_summary(track, stream, summary):
    """what a smoothed track adds to a replay's summary: pings, the smallest n_unique and -- with truth in the stream --
    the smoothed track's pose RMSE beside the filtered one's, both at the resampled pings"""
    summary['smooth_lag'], summary['smooth_pings'] = int(track['lag']), int(len(track['idx']))
    if len(track['idx']):
        live = track['n_unique'][track['n_unique'] >= 0]      # (-1: a ping whose lineage a re-initialisation cut)
        summary['smooth_n_unique_min'] = int(live.min()) if len(live) else 0
        if 'truth_xyz' in stream:
            ref = np.asarray(stream['truth_xyz'])[track['idx']][:, :2]
            summary['filtered_rmse_vs_truth'] = pose_rmse(track['filtered_xyyaw'][:, :2], ref)
            summary['smoothed_rmse_vs_truth'] = pose_rmse(track['smoothed_xyyaw'][:, :2], ref)


def odom_stream_from_raw(t, kind, data, gps_map=None, pressure_tf=None, dvl_period=0.2, dr_period=0.02):
    """Raw IMU / DVL / depth / thruster events (synth.raw_sensor_events format) -> the odometry stream
    `replay` consumes, through the dead-reckoning integrator (dr.py): one sample
    per published timer tick, stamped with the tick's event time.  Also returns the map -> odom
    transform the integrator fixed from the first usable GPS fix (4x4) for the filter's m2o."""
    from . import dr, synth
    from . import auv_pf as node
    ticks, m2o = dr.replay_events(t, kind, data, gps_map=gps_map, pressure_tf=pressure_tf, dvl_period=dvl_period,
                                  dr_period=dr_period)
    tick_t = np.asarray(t)[np.asarray(kind) == synth.EV_TICK]
    pub = ticks[:, 0] > 0
    stream = dict(stamp=tick_t[pub], v=ticks[pub, 8:11], wz=ticks[pub, 13], q=ticks[pub, 4:8], z=ticks[pub, 3],
                  dr_xyz=ticks[pub, 1:4])
    if pub.any():
        stream['t0'] = float(stream['stamp'][0]) - dr_period
    m2o_mat = None if np.isnan(m2o).any() else node.matrix_from_tf(m2o[0:3], m2o[3:7])
    return stream, m2o_mat


FIX_SMOOTH_CLASH = ('acoustic fixes (--fix-period) and the smoothed track (--smooth) both keep the particle genealogy, and one '
                    'ring has one owner: run them separately')


def make_fixes(stream, m2o, period, latency, std, seed=0):
    """Synthetic acoustic fixes of a stream WITH TRUTH: every `period` seconds the truth position of that sample, taken
    into the map frame, plus N(0, std^2 I) (seeded), stamped with the sample's time and delivered `latency` seconds later.
    Returns a list of (deliver_at, stamp, x_map, y_map), in delivery order."""
    if 'truth_xyz' not in stream:
        raise ValueError('acoustic fixes are made from the truth track: the stream has no truth_xyz')
    rs = np.random.RandomState(seed)
    M = np.identity(4) if m2o is None else np.asarray(m2o, dtype=np.float64)
    stamp, truth = np.asarray(stream['stamp'], dtype=np.float64), np.asarray(stream['truth_xyz'], dtype=np.float64)
    out, due = [], float(stamp[0]) + float(period)
    for k in range(len(stamp)):
        if stamp[k] < due:
            continue
        due += float(period)
        p = M.dot([truth[k, 0], truth[k, 1], truth[k, 2], 1.0])[:2] + float(std) * rs.randn(2)
        out.append((float(stamp[k]) + float(latency), float(stamp[k]), float(p[0]), float(p[1])))
    return out


# the node parameters a synthetic stream is replayed with (`synth[:N]`): the noise the stream was made with -- fixes of
# 0.5 m, a tight start, little process noise and no resampling noise -- instead of the reference's launch defaults (a fix
# of 1 cm and a metre of resampling noise, under which no drift can be told from the jitter)
SYNTH_PARAMS = dict(measurement_std=0.5, init_covariance='[0.01, 0.01, 0.0, 0.0, 0.0, 0.0001]',
                    motion_covariance='[0.0001, 0.0001, 0.0, 0.0, 0.0, 0.000001]',
                    resampling_noise_covariance='[0.0, 0.0, 0.0, 0.0, 0.0, 0.0]')


def synthetic_stream(n_steps=3000, current=(0.0, 0.0), yaw_rate_bias=0.0, gps_every=50, gps_sigma=0.5, seed=0, mbes_every=0,
                     beams=64, mbes_sigma=0.1, mbes_range_max=100.0, outliers=None):
    """A stream made here instead of read from a file (`synth` / `synth:N` on the command line): synth.odom_stream with a
    water current and a yaw-rate bias the odometry does not see, the truth track, and a GPS fix of gps_sigma metres every
    gps_every samples (identity frames: utm = map = odom).  drift_truth = (cx, cy, bw) is what drift states should find.
    mbes_every = K > 0 (needs the GPU): also a multibeam ping of `beams` beams every K samples over synth.bathymetry_grid's
    default map, which the stream then carries (map_z, map_origin, map_res): the ranges the library expects at the truth,
    with mbes_sigma metres of noise and, outliers = (fraction, shorten_m), that share of the beams shorten_m short
    (synth.noisy_pings: both from seeds of their own, so the rest of the stream keeps its numbers; mbes_outliers marks them)."""
    from . import synth
    st = synth.odom_stream(int(n_steps), current=current, yaw_rate_bias=yaw_rate_bias)
    idx, xy = synth.gps_fixes(st['truth'], np.identity(4), every=int(gps_every), sigma=float(gps_sigma), seed=int(seed) + 2)
    st.update(truth_xyz=st['truth'][:, :3].copy(), gps_idx=idx, gps_xy_utm=xy,
              drift_truth=np.array([float(current[0]), float(current[1]), float(yaw_rate_bias)]))
    if mbes_every > 0:
        from . import engine
        origin, res = (-64.0, -256.0), 1.0
        z = synth.bathymetry_grid(512, 512, res, origin)
        at = np.arange(int(mbes_every) - 1, int(n_steps), int(mbes_every))
        ba = synth.beam_angles(int(beams))
        cast = engine.Engine(at.size, rng_mode=engine.RNG_REPLAY)
        cast.set_map_grid(z, origin, res)
        cast.set_particles(np.ascontiguousarray(st['truth'][at].T))
        clean = cast.mbes_expected(0, at.size, ba, float(mbes_range_max))
        cast.close()
        ranges, hit = synth.noisy_pings(clean, mbes_sigma, mbes_range_max, outliers, seed=int(seed) + 4)
        st.update(mbes_idx=at, mbes_ranges=ranges, mbes_angles=ba, mbes_range_max=float(mbes_range_max), mbes_outliers=hit,
                  map_z=z, map_origin=np.array(origin), map_res=res)
    return st


def innovation_summary(nis_rows, nu_rows):
    """what --innovation adds to a summary, from the per-beam NIS and nu of every ping (NaN: the beam had no return): the
    run's mean NIS per beam -- about 1 when sigma is right, well above when it is too small --, their mean, the mean nu"""
    nis, nu = np.asarray(nis_rows, dtype=np.float64), np.asarray(nu_rows, dtype=np.float64)
    out = dict(innovation_pings=int(nis.shape[0]))
    seen = np.isfinite(nis)
    if seen.any():
        count = seen.sum(axis=0)
        per_beam = np.where(seen, nis, 0.0).sum(axis=0) / np.maximum(count, 1)     # (0 for a beam that never had a return)
        out['innovation_nis_per_beam'] = [float(v) for v in per_beam]
        out['innovation_mean_nis'] = float(per_beam[count > 0].mean())
        out['innovation_mean_nu'] = float(nu[seen].mean())
    return out


def credible_summary(prob, radii, est_xyz, truth_xyz=None):
    """what --credible adds to a summary: the probability, the median of the stated radii and, against a truth, the share of
    the published poses whose true position lay inside the stated radius -- the filter's calibration; a well-tuned filter
    gives about `prob`.  A radius that is NaN (no particle with a position) contains nothing."""
    radii = np.asarray(radii, dtype=np.float64)
    out = dict(credible_prob=float(prob), credible_pings=int(radii.size))
    if truth_xyz is not None and radii.size:
        fin = radii[np.isfinite(radii)]
        err = np.hypot(np.asarray(est_xyz)[:, 0] - np.asarray(truth_xyz)[:, 0], np.asarray(est_xyz)[:, 1] - np.asarray(truth_xyz)[:, 1])
        out['credible_radius_median'] = float(np.median(fin)) if fin.size else float('nan')
        out['credible_containment'] = float(np.mean(err <= radii))
    return out


def information_summary(log):
    """what a node with mbes_information_every > 0 adds to a summary, from its information_log (one row per asked ping:
    stamp, crlb_strong, crlb_weak, weak_axis, rank_pos, hit_share): the pings asked, the medians of the one-ping Cramer-Rao
    bounds (metres; None -- JSON has no infinity -- where more than half of the pings fix nothing along that axis), the
    share of pings whose position information is rank-deficient, and the rows themselves"""
    def num(v):
        return float(v) if np.isfinite(v) else None
    rows = np.asarray(log, dtype=np.float64).reshape(-1, 6)
    out = dict(information_pings=int(rows.shape[0]))
    if rows.shape[0]:
        out['information_crlb_strong_median'] = num(np.median(rows[:, 1]))
        out['information_crlb_weak_median'] = num(np.median(rows[:, 2]))
        out['information_rank_deficient_share'] = float(np.mean(rows[:, 4] < 2))
        out['information_hit_share_mean'] = float(np.mean(rows[:, 5]))
        out['information_per_ping'] = [dict(stamp=float(r[0]), crlb_strong=num(r[1]), crlb_weak=num(r[2]),
                                            weak_axis=float(r[3]), rank_pos=int(r[4]), hit_share=float(r[5])) for r in rows]
    return out


def _fix_log_summary(prefix, log, truth_xy):
    """the summary keys of a log of pose fixes (match_log, swath_log: one row per call: stamp, status, x, y, yaw, rms,
    evaluations, and the published pose x, y, yaw the fix started from), named prefix_*"""
    ok = np.array([r[1] == 'CONVERGED' for r in log], dtype=bool)
    rms = np.array([r[5] for r in log], dtype=np.float64)
    out = {prefix + '_calls': len(log), prefix + '_converged_share': float(ok.mean()) if len(log) else 0.0,
           prefix + '_rms_residual_median': float(np.median(rms[ok])) if ok.any() else None,
           prefix + '_rmse_xy': None, prefix + '_filter_rmse_xy': None}
    if truth_xy is not None and ok.any():
        t = np.asarray(truth_xy, dtype=np.float64)[ok]
        fix = np.array([[r[2], r[3]] for r in log], dtype=np.float64)[ok]
        own = np.array([[r[7], r[8]] for r in log], dtype=np.float64)[ok]
        out[prefix + '_rmse_xy'], out[prefix + '_filter_rmse_xy'] = pose_rmse(fix, t), pose_rmse(own, t)
    return out


def match_summary(log, truth_xy=None):
    """what a node with mbes_match_every > 0 adds to a summary, from its match_log (one row per call: stamp, status, x, y,
    yaw, rms, evaluations, and the published pose x, y, yaw the fix started from): the calls, the share of them that
    converged, the median rms residual of the converged fixes (metres) and -- with truth_xy, the stream's truth at the
    pings of the calls -- the RMSE of the converged fixes against it, beside the filter's own at the same pings"""
    return _fix_log_summary('match', log, truth_xy)


def swath_summary(log, truth_xy=None):
    """what a node with mbes_swath_pings > 0 adds to a summary, from its swath_log (rows as match_log's): match_summary's
    figures as swath_calls, swath_converged_share, swath_rms_residual_median, swath_rmse_xy beside swath_filter_rmse_xy"""
    return _fix_log_summary('swath', log, truth_xy)


def replay(stream, params=None, m2o=None, utm2map=None, grid=None, mesh=None, publish_every=5, smooth_lag=0,
           fix_period=0.0, fix_latency=0.0, fix_seed=0, innovation=False):
    """Drive the node with a recorded stream; returns dict(pf_xyz[n_pub,3], pub_idx, summary).  smooth_lag > 0: also
    out['smooth'], the lag-smooth_lag smoothed track beside the filtered one, one entry per resample of the node
    (SmoothTrack; the node's particle genealogy: include/mcl_history.h).  fix_period > 0 (a stream with truth_xyz): acoustic
    fixes every fix_period seconds with the node's `fix_std` of noise, delivered fix_latency seconds late to fix_cb
    (make_fixes); the node's `fix_history_depth` decides whether they are applied to the past or to the present; the
    summary gains fixes_applied, fixes_dropped and fix_mean_lag (mean age of the applied fixes, seconds).  innovation: every
    ping is first held against the cloud (Engine.ping_innovation, include/mcl_innovation.h; nothing of the filter changes)
    and the summary gains innovation_summary's keys: what to tune the node's mbes_std with.  A node with mbes_gate_nis > 0
    adds gate_pings, gate_n_gated, gate_inconsistent; one with mbes_information_every > 0 adds information_summary's keys.
    One with mbes_match_every > 0 adds match_summary's keys (the fixes of include/mcl_match.h against the stream's truth),
    one with mbes_swath_pings > 0 swath_summary's (include/mcl_swath.h).
    A stream that carries its map (map_z, map_origin, map_res) is replayed over it when neither grid nor mesh is given."""
    from . import auv_pf as node
    from . import msgs
    if smooth_lag > 0 and fix_period > 0:
        raise ValueError(FIX_SMOOTH_CLASH)
    tr = node.RecordingTransport(utm2map)
    pf = node.auv_pf(params or {}, m2o_mat=m2o, transport=tr)
    if grid is None and mesh is None and 'map_z' in stream:
        grid = dict(z=stream['map_z'], origin=tuple(float(v) for v in stream['map_origin']), res=stream['map_res'])
    if grid is not None:
        pf.set_map_grid(grid['z'], grid['origin'], float(grid['res']))
    if mesh is not None:
        pf.set_map_mesh(mesh['verts'], mesh['tris'])
    n = len(stream['stamp'])
    inn_nis, inn_nu, n_inconsistent, match_at, swath_at = [], [], 0, [], []
    pf.start_timing(float(stream['t0']) if 't0' in stream else float(stream['stamp'][0]) - 0.02)
    gps_at = {int(k): j for j, k in enumerate(stream['gps_idx'])} if 'gps_idx' in stream else {}
    mbes_at = {int(k): j for j, k in enumerate(stream['mbes_idx'])} if 'mbes_idx' in stream else {}
    pub_idx, pf_xyz, cred_r = [], [], []
    stats = DRStats() if ('gps_idx' in stream and 'dr_xyz' in stream) else None
    fixes = make_fixes(stream, m2o, fix_period, fix_latency, pf.fix_std, fix_seed) if fix_period > 0 else []
    next_fix = 0
    smooth, at = None, [0]
    if smooth_lag > 0:
        # every resample of the node -- whichever callback asked for it -- is followed by a record
        smooth = SmoothTrack(pf.particles, smooth_lag)
        node_resample = pf.resample

        def resample_and_record(weights):
            node_resample(weights)
            smooth.record(at[0], pf.time)
        pf.resample = resample_and_record
    if stats is not None:
        # visual_tools transforms the fix into the odom frame: (map <- odom)^-1 (map <- utm)
        u2m = np.identity(4) if utm2map is None else np.asarray(utm2map, dtype=np.float64)
        stats.utm2odom = np.linalg.inv(np.identity(4) if m2o is None else np.asarray(m2o, dtype=np.float64)).dot(u2m)
    for k in range(n):
        at[0] = k
        pf.odom_callback(msgs.odometry_from_stream(stream, k))
        if stats is not None:
            stats.add(1, stream['stamp'][k], stream['dr_xyz'][k])
            if k in gps_at:
                stats.add(0, stream['stamp'][k], list(stream['gps_xy_utm'][gps_at[k]]) + [0.0])
        if k in gps_at:
            g = msgs.Odometry()
            g.pose.pose.position.x = float(stream['gps_xy_utm'][gps_at[k]][0])
            g.pose.pose.position.y = float(stream['gps_xy_utm'][gps_at[k]][1])
            pf.dive_cb(msgs.Bool(False))
            pf.gps_odom_cb(g)
        if k in mbes_at:
            ang = np.asarray(stream['mbes_angles'], dtype=np.float64)
            scan = msgs.LaserScan(stream['mbes_ranges'][mbes_at[k]], float(ang[0]),
                                  float(ang[1] - ang[0]) if ang.size > 1 else 0.0,
                                  float(stream['mbes_range_max']) if 'mbes_range_max' in stream else 100.0)
            if innovation and pf.old_time and pf.has_map:
                inn = pf.particles.ping_innovation(np.asarray(scan.ranges, dtype=np.float32), ang.astype(np.float32),
                                                   pf.mbes_std, float(scan.range_max), pf.mbes_sensor_offset)
                inn_nis.append(np.where(inn.valid, inn.nis, np.nan))
                inn_nu.append(np.where(inn.valid, inn.nu, np.nan))
            calls, matched, swathed = pf.gate_calls, pf.match_calls, pf.swath_calls
            pf.mbes_cb(scan)
            if pf.match_calls > matched:
                match_at.append(k)
            if pf.swath_calls > swathed:
                swath_at.append(k)
            if pf.gate_calls > calls and pf.last_innovation.inconsistent:
                n_inconsistent += 1
        while next_fix < len(fixes) and fixes[next_fix][0] <= stream['stamp'][k]:
            f = msgs.Odometry()
            f.header = msgs.Header(pf.map_frame, msgs.Time(fixes[next_fix][1]))
            f.pose.pose.position.x, f.pose.pose.position.y = fixes[next_fix][2], fixes[next_fix][3]
            pf.fix_cb(f)
            next_fix += 1
        if (k + 1) % publish_every == 0 or k == n - 1:
            pf.loc_loop(None)
            p = tr.odom_corrected[-1].pose.pose.position
            pub_idx.append(k)
            pf_xyz.append([p.x, p.y, p.z])
            if pf.credible_prob > 0.0:
                cred_r.append(float(pf.last_credible['radius']))
            if stats is not None:
                stats.add(2, stream['stamp'][k], [p.x, p.y, p.z])
    pf_xyz = np.array(pf_xyz)
    summary = {}
    if fix_period > 0:
        summary['fixes_applied'], summary['fixes_dropped'] = int(pf.fixes_applied), int(pf.fixes_dropped)
        summary['fix_mean_lag'] = float(pf.fix_lag_sum / pf.fixes_applied) if pf.fixes_applied else 0.0
    if pf.temper_ess_ratio > 0.0:
        # likelihood tempering (include/mcl_temper.h): the exponents the resamplings of this run were given
        b = pf.temper_betas
        summary['temper_ess_ratio'], summary['temper_resamplings'] = float(pf.temper_ess_ratio), int(len(b))
        summary['tempered_updates'] = int(pf.tempered_updates)
        summary['temper_beta_mean'] = float(np.mean(b)) if b else 1.0
        summary['temper_beta_min'] = float(np.min(b)) if b else 1.0
    if pf.estimate_drift:
        # drift states (include/mcl_drift.h): the cloud's mean (cx, cy, bw) at the last published pose, and how far its
        # current is from the one the stream was made with
        summary['drift_mean'] = [float(x) for x in pf.drift_mean]
        if 'drift_truth' in stream:
            t = np.asarray(stream['drift_truth'], dtype=np.float64)
            summary['drift_error'] = float(np.hypot(pf.drift_mean[0] - t[0], pf.drift_mean[1] - t[1]))
            summary['drift_bias_error'] = float(abs(pf.drift_mean[2] - t[2]))
    if pf.regularise_scale > 0.0:
        # regularised resampling (include/mcl_regularise.h): how many resamplings were jittered, with which bandwidth
        summary['regularise_scale'], summary['regularise_shrink'] = float(pf.regularise_scale), bool(pf.regularise_shrink)
        summary['regularise_calls'] = int(pf.regularise_calls)
        summary['regularise_h_mean'] = float(np.mean(pf.regularise_hs)) if pf.regularise_hs else 0.0
    if pf.credible_prob > 0.0:
        # credible region (include/mcl_quantile.h): the radius that held credible_prob of the cloud about every published pose
        out_cred = np.array(cred_r)
        summary.update(credible_summary(pf.credible_prob, out_cred, pf_xyz,
                                        np.asarray(stream['truth_xyz'])[pub_idx] if 'truth_xyz' in stream else None))
    if innovation:
        summary.update(innovation_summary(inn_nis, inn_nu))
    if pf.mbes_gate_nis > 0.0:
        # per-beam outlier gate (include/mcl_innovation.h): pings gated, beams marked invalid, pings that disagreed as a whole
        summary['mbes_gate_nis'], summary['gate_pings'] = float(pf.mbes_gate_nis), int(pf.gate_calls)
        summary['gate_n_gated'], summary['gate_inconsistent'] = int(pf.gated_beams), int(n_inconsistent)
    if pf.mbes_information_every > 0:
        # ping information (include/mcl_information.h): what every K-th ping could tell the cloud where it stood
        summary['mbes_information_every'] = int(pf.mbes_information_every)
        summary.update(information_summary(pf.information_log))
    if pf.mbes_match_every > 0:
        # ping matching (include/mcl_match.h): where every K-th ping alone says the vehicle is, against the stream's truth
        summary['mbes_match_every'] = int(pf.mbes_match_every)
        summary.update(match_summary(pf.match_log, np.asarray(stream['truth_xyz'])[match_at][:, :2] if 'truth_xyz' in stream else None))
    if pf.mbes_swath_pings > 0:
        # swath matching (include/mcl_swath.h): where the last K pings together say the vehicle is, against the stream's truth
        summary['mbes_swath_pings'], summary['mbes_swath_every'] = int(pf.mbes_swath_pings), int(pf.mbes_swath_every)
        summary.update(swath_summary(pf.swath_log, np.asarray(stream['truth_xyz'])[swath_at][:, :2] if 'truth_xyz' in stream else None))
    summary['pf_distance'], summary['pf_final'] = track_metrics(pf_xyz.T)
    for name in ('dr_xyz', 'truth_xyz'):
        if name in stream:
            ref = np.asarray(stream[name])[pub_idx]
            tag = name.split('_')[0]
            summary[tag + '_distance'], summary[tag + '_final'] = track_metrics(ref.T)
            summary['pf_rmse_vs_' + tag] = pose_rmse(pf_xyz[:, :2], ref[:, :2])
    out = dict(pf_xyz=pf_xyz, pub_idx=np.array(pub_idx), summary=summary)
    if smooth is not None:
        out['smooth'] = smooth.finish()
        smooth_summary(out['smooth'], stream, summary)
    if stats is not None:
        out['stats'] = stats
        out['err_gps_pf'], out['err_gps_dr'] = stats.error_series()
        summary['visual_tools'] = stats.finish_hld()
    return out


def stream_to_bag(path, stream, odom_topic='/sam/dr/odom', gps_topic='/sam/dr/gps', mbes_topic='/sam/mbes_scan',
                  dive_topic='/dive', compression='none'):
    """A stream file's content as a rosbag 2.0 file (rosbag_io.write_bag): one nav_msgs/Odometry per sample, the GPS
    fixes (nav_msgs/Odometry in utm, preceded once by std_msgs/Bool false on the dive topic -- the node ignores fixes
    while `diving`, auv_pf.py:103,126) and the pings (sensor_msgs/LaserScan) right after the sample they belong to."""
    from . import msgs, rosbag_io
    out = []
    n = len(stream['stamp'])
    gps_at = {int(k): j for j, k in enumerate(stream['gps_idx'])} if 'gps_idx' in stream else {}
    mbes_at = {int(k): j for j, k in enumerate(stream['mbes_idx'])} if 'mbes_idx' in stream else {}
    surfaced = False
    for k in range(n):
        t = float(stream['stamp'][k])
        od = msgs.odometry_from_stream(stream, k)
        od.header.frame_id, od.child_frame_id = 'sam/odom', 'sam/base_link'
        out.append((odom_topic, 'nav_msgs/Odometry', od, t))
        if k in gps_at:
            if not surfaced:
                out.append((dive_topic, 'std_msgs/Bool', msgs.Bool(False), t))
                surfaced = True
            g = msgs.Odometry()
            g.header.stamp, g.header.frame_id = msgs.Time(t), 'utm'
            g.pose.pose.position.x = float(stream['gps_xy_utm'][gps_at[k]][0])
            g.pose.pose.position.y = float(stream['gps_xy_utm'][gps_at[k]][1])
            out.append((gps_topic, 'nav_msgs/Odometry', g, t))
        if k in mbes_at:
            ang = np.asarray(stream['mbes_angles'], dtype=np.float64)
            scan = msgs.LaserScan(np.asarray(stream['mbes_ranges'][mbes_at[k]], np.float32), float(ang[0]),
                                  float(ang[1] - ang[0]) if ang.size > 1 else 0.0,
                                  float(stream['mbes_range_max']) if 'mbes_range_max' in stream else 100.0)
            scan.header.stamp, scan.header.frame_id = msgs.Time(t), 'sam/mbes_link'
            out.append((mbes_topic, 'sensor_msgs/LaserScan', scan, t))
    rosbag_io.write_bag(path, out, compression=compression)
    return len(out)


def replay_bag(path, params=None, m2o=None, utm2map=None, grid=None, mesh=None, odom_topic='/sam/dr/odom',
               gps_topic='/sam/dr/gps', mbes_topic='/sam/mbes_scan', mbes_cloud_topic=None, dive_topic='/dive',
               lm_detect_topic=None, publish_period=0.1, t0=None):
    """BASELINE config 1, literally: a recorded ROS 1 bag's messages in recorded order through the node's callbacks
    (odom_callback, gps_odom_cb, dive_cb, mbes_cb, mbes_pc_cb, lm_detect_cb), loc_loop every `publish_period` seconds
    of bag time (auv_pf.py:114: a 10 Hz timer).  Returns dict(pf_xyz[k,3], pf_stamp[k], counts{topic: messages},
    summary); no ROS installation is needed (rosbag_io.Bag)."""
    from . import auv_pf as node
    from . import rosbag_io
    tr = node.RecordingTransport(utm2map)
    pf = node.auv_pf(params or {}, m2o_mat=m2o, transport=tr)
    if grid is not None:
        pf.set_map_grid(grid['z'], grid['origin'], float(grid['res']))
    if mesh is not None:
        pf.set_map_mesh(mesh['verts'], mesh['tris'])
    route = {odom_topic: pf.odom_callback, gps_topic: pf.gps_odom_cb, dive_topic: pf.dive_cb, mbes_topic: pf.mbes_cb}
    if mbes_cloud_topic:
        route[mbes_cloud_topic] = pf.mbes_pc_cb
    if lm_detect_topic:
        route[lm_detect_topic] = pf.lm_detect_cb
    counts, pf_xyz, pf_stamp = {}, [], []
    started, next_pub, last_t = False, None, None
    for topic, msg, t in rosbag_io.Bag(path).read_messages(topics=list(route)):
        if not started:
            # "Start timing now" (auv_pf.py:96-98): the node is up before the first message
            pf.start_timing(float(t0) if t0 is not None else t - 0.02)
            next_pub, started = t + publish_period, True
        while t >= next_pub:   # the 10 Hz timer, in bag time
            pf.loc_loop(None)
            p = tr.odom_corrected[-1].pose.pose.position
            pf_xyz.append([p.x, p.y, p.z])
            pf_stamp.append(next_pub)
            next_pub += publish_period
        route[topic](msg)
        counts[topic] = counts.get(topic, 0) + 1
        last_t = t
    if started:
        pf.loc_loop(None)
        p = tr.odom_corrected[-1].pose.pose.position
        pf_xyz.append([p.x, p.y, p.z])
        pf_stamp.append(last_t)
    pf_xyz = np.array(pf_xyz).reshape(-1, 3)
    summary = {'messages': counts}
    if len(pf_xyz):
        summary['pf_distance'], summary['pf_final'] = track_metrics(pf_xyz.T)
    return dict(pf_xyz=pf_xyz, pf_stamp=np.array(pf_stamp), counts=counts, summary=summary, node=pf)


def replay_recover(stream, grid=None, mesh=None, particles=65536, seed=0, sigma=1.0, m2o=None, yaw=(-np.pi, np.pi),
                   process_cov=(0.01, 0.01, 0, 0, 0, 1e-4), resample_cov=(0.04, 0.04, 0, 0, 0, 1e-3), alpha_slow=0.001,
                   alpha_fast=0.1, max_fraction=0.1, inject=True, estimate='mean', mode_cell=1.0, mode_n_yaw=36,
                   smooth_lag=0, credible=0.0, reseed=0, reseed_pitch=4.0, reseed_n_yaw=8, reseed_yaw_window=None,
                   reseed_select=None, kld=0.0, kld_sizes=None, kld_cell=0.5, kld_n_yaw=36):
    """Global localisation with kidnap recovery on a recorded stream (--recover): the cloud starts uniform over the map's
    footprint, and every ping runs the separate calls  predict ... -> update_mbes -> weight_stats -> resample ->
    inject_uniform(fraction)  with the fraction of recovery.AugmentedMCL (the likelihood per valid beam, a short-term
    against a long-term average).  The node class is not involved.  estimate='mean' publishes mcl_mean_cov's pose;
    'mode' the heaviest cluster's (mode 0 of mcl_pose_modes on a lattice of mode_cell metres x mode_n_yaw bins over the
    map's footprint) when there is one, otherwise the mean; 'median' the component-wise median of x and y (exact order
    statistics, include/mcl_quantile.h; z is the mean's).  credible = P > 0: after every ping also the radius that holds P
    of the cloud about the published pose (out['credible_radius']); with a truth the summary gains credible_radius_median
    and credible_containment (credible_summary).  Returns dict(pf_xyz[m,3] published pose after every ping,
    pub_idx, fractions[m], injected[m], log_lik_per_beam[m], n_eff[m], summary).  smooth_lag > 0: also out['smooth'], the
    lag-smooth_lag smoothed track (SmoothTrack), one entry per ping; an injected particle inherits its slot's past.
    reseed = K > 0: sensor resetting (recovery.SensorResetting, include/mcl_reseed.h) instead of the uniform injection: a
    ring of the last K pings with the odometry's poses at them (the stream's twist integrated without noise), offsets by
    swath_offsets, a swath match from a lattice of reseed_pitch metres x reseed_n_yaw yaws (over the full circle, or with
    reseed_yaw_window W within +-W of the odometry's heading) and the injection at its fixes (reseed_select: the keywords of
    engine.make_reseed_select_config); the summary gains reseed_calls, reseed_fallbacks, reseed_components_median and,
    with a truth, first_ping_within_1m_after_kidnap (the first ping from which the published pose stays within 1 m of the
    truth after it was last farther away; None if it never does).  reseed = 0 is the path and the summary of before.
    kld = EPS > 0: KLD-sampling across handles (adaptive.AdaptiveCloud, include/mcl_kld.h) with the KL error EPS: one engine
    per size of kld_sizes (default: particles, particles / 8, / 64, / 512, down to 256), each with its own copy of the map;
    the cloud starts on the largest, every resample counts the occupied cells of a lattice of kld_cell metres x kld_n_yaw
    bins and moves the cloud to the size adaptive.KldLadder asks for, and a positive injection fraction takes it back to
    the largest first.  The summary gains kld_sizes_used, kld_final_size and kld_moves, out['kld_trace'] the (ping, k,
    bound, size) rows.  kld = 0 is the path and the summary of before."""
    from . import adaptive
    from . import engine as eng
    from . import recovery
    from .auv_pf import euler_from_quaternion
    if not 0 <= int(reseed) <= eng.SWATH_MAX_PINGS:
        raise ValueError('replay_recover: reseed must be 0 ... %d pings' % eng.SWATH_MAX_PINGS)
    if 'mbes_idx' not in stream or (grid is None and mesh is None):
        raise ValueError('replay_recover: needs a stream with MBES pings and a map')
    if estimate not in ('mean', 'mode', 'median'):
        raise ValueError("replay_recover: estimate must be 'mean', 'mode' or 'median'")
    if not 0.0 <= credible <= 1.0:
        raise ValueError('replay_recover: credible must lie in [0, 1]')
    if not (0.0 <= float(kld) and math.isfinite(float(kld))):
        raise ValueError('replay_recover: kld must be a finite KL error >= 0')
    cloud = None
    if float(kld) > 0.0:
        if smooth_lag > 0:
            raise ValueError('replay_recover: the genealogy of --smooth lives in one handle; not with kld')
        sizes = sorted(set(int(s) for s in kld_sizes)) if kld_sizes else sorted(
            set(max(int(particles) >> sh, min(256, int(particles))) for sh in (0, 3, 6, 9)))
        if not sizes or sizes[0] < 1:
            raise ValueError('replay_recover: kld_sizes must be positive')
        engines = [eng.Engine(s, process_cov=process_cov, resample_cov=resample_cov, m2o=m2o, seed=seed) for s in sizes]
        e = cloud = adaptive.AdaptiveCloud(engines, adaptive.KldLadder(sizes, float(kld)), kld_cell, kld_n_yaw)
    else:
        e = eng.Engine(int(particles), process_cov=process_cov, resample_cov=resample_cov, m2o=m2o, seed=seed)
    if grid is not None:
        e.set_map_grid(grid['z'], grid['origin'], float(grid['res']))
    else:
        e.set_map_mesh(mesh['verts'], mesh['tris'])
    e.init_particles_uniform(yaw=yaw)
    smooth = SmoothTrack(e, smooth_lag) if smooth_lag > 0 else None
    lattice = e.mode_grid(mode_cell, mode_n_yaw) if estimate == 'mode' else None
    aug = recovery.AugmentedMCL(alpha_slow, alpha_fast, max_fraction)
    resetting, reseed_components = None, []
    if int(reseed) > 0:
        resetting = recovery.SensorResetting(aug, eng.make_reseed_select_config(**dict(reseed_select or {})), reseed_pitch,
                                             reseed_n_yaw, reseed_yaw_window, pings=int(reseed))
        dr = [0.0] * 6   # the odometry's own pose: of x and y only differences enter, the heading is its quaternion's
    mbes_at = {int(k): j for j, k in enumerate(stream['mbes_idx'])}
    ang = np.asarray(stream['mbes_angles'], dtype=np.float32)
    r_max = float(stream['mbes_range_max']) if 'mbes_range_max' in stream else 100.0
    t_prev = float(stream['t0']) if 't0' in stream else float(stream['stamp'][0]) - 0.02
    out = dict(pf_xyz=[], pub_idx=[], fractions=[], injected=[], log_lik_per_beam=[], n_eff=[])
    if credible > 0.0:
        out['credible_radius'] = []
    for k in range(len(stream['stamp'])):
        t = float(stream['stamp'][k])
        e.predict(stream['v'][k], float(stream['wz'][k]), stream['q'][k], float(stream['z'][k]), t - t_prev, stamp=t)
        if resetting is not None:   # the noise-free motion model (synth.odom_stream's): the twist turned by the sample's attitude
            dt = t - t_prev
            roll, pitch, hd = [float(a) for a in euler_from_quaternion(stream['q'][k])]
            cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(hd), math.sin(hd)
            vx, vy, vz = [float(c) * dt for c in stream['v'][k]]
            dr = [dr[0] + cy * cp * vx + (cy * sp * sr - sy * cr) * vy + (cy * sp * cr + sy * sr) * vz,
                  dr[1] + sy * cp * vx + (sy * sp * sr + cy * cr) * vy + (sy * sp * cr - cy * sr) * vz,
                  float(stream['z'][k]), float(roll), float(pitch), hd]
        t_prev = t
        if k not in mbes_at:
            continue
        ranges = np.asarray(stream['mbes_ranges'][mbes_at[k]], dtype=np.float32)
        e.update_mbes(ranges, ang, sigma, r_max)
        if resetting is not None:
            resetting.push(ranges, dr)
        st = e.weight_stats()
        out['log_lik_per_beam'].append(aug.observe(st, int(np.count_nonzero(ranges > 0))))
        out['n_eff'].append(st.n_eff)
        e.resample()
        if smooth is not None:
            smooth.record(k, t)
        frac = aug.fraction() if inject else 0.0
        out['fractions'].append(frac)
        if cloud is not None and frac > 0.0:
            cloud.to_top()
        if resetting is not None:
            out['injected'].append(resetting.step(e, ang, sigma, r_max) if frac > 0.0 else 0)
            if frac > 0.0 and not resetting.last['fallback']:
                reseed_components.append(resetting.last['components'])
        else:
            out['injected'].append(e.inject_uniform(frac, yaw=yaw) if frac > 0.0 else 0)
            if frac > 0.0:
                aug.injected()
        pose = e.mean_cov()[0][:3]
        if lattice is not None:
            modes = e.pose_modes(mode_cell, k=1, grid=lattice)[0]
            if modes:
                pose = modes[0].mean[:3]
        if estimate == 'median':
            pose = np.array([e.cloud_quantiles('x', [0.5])[0].value, e.cloud_quantiles('y', [0.5])[0].value, pose[2]])
        if credible > 0.0:
            r2 = e.cloud_quantiles('radius2', [credible], (float(pose[0]), float(pose[1]), 0.0))[0].value
            out['credible_radius'].append(math.sqrt(r2))
        out['pf_xyz'].append(pose)
        out['pub_idx'].append(k)
    track = smooth.finish() if smooth is not None else None
    e.close()
    if cloud is not None:
        out['kld_trace'] = list(cloud.trace)
    for name in out:
        out[name] = np.array(out[name])
    summary = dict(pings=len(out['pub_idx']), injected_total=int(out['injected'].sum()) if len(out['injected']) else 0)
    if len(out['pf_xyz']):
        summary['pf_distance'], summary['pf_final'] = track_metrics(out['pf_xyz'].T)
        if 'truth_xyz' in stream:
            ref = np.asarray(stream['truth_xyz'])[out['pub_idx']]
            summary['final_error_vs_truth'] = float(np.linalg.norm(out['pf_xyz'][-1, :2] - ref[-1, :2]))
    if resetting is not None:
        summary.update(reseed_calls=resetting.calls, reseed_fallbacks=resetting.fallbacks,
                       reseed_components_median=float(np.median(reseed_components)) if reseed_components else 0.0)
        if 'truth_xyz' in stream and len(out['pf_xyz']):
            err = np.linalg.norm(out['pf_xyz'][:, :2] - np.asarray(stream['truth_xyz'])[out['pub_idx']][:, :2], axis=1)
            far = np.flatnonzero(err > 1.0)
            first = 0 if far.size == 0 else int(far[-1]) + 1
            summary['first_ping_within_1m_after_kidnap'] = first if first < err.size else None
    if cloud is not None:
        summary.update(kld_sizes_used=sorted(set(int(r[3]) for r in cloud.trace)),
                       kld_final_size=int(cloud.trace[-1][3]) if cloud.trace else int(cloud.ladder.sizes[-1]),
                       kld_moves=int(cloud.moves))
    if credible > 0.0:
        summary.update(credible_summary(credible, out['credible_radius'], out['pf_xyz'],
                                        np.asarray(stream['truth_xyz'])[out['pub_idx']]
                                        if 'truth_xyz' in stream and len(out['pub_idx']) else None))
    if track is not None:
        out['smooth'] = track
        smooth_summary(track, stream, summary)
    out['summary'] = summary
    return out


def save_smooth(out_path, res):
    """--smooth with --out: the smoothed track as a CSV of its own beside the filtered one (OUT.smooth.csv)"""
    tr = res.get('smooth')
    if tr is None:
        return
    np.savetxt(out_path + '.smooth.csv',
               np.column_stack([tr['idx'], tr['stamp'], tr['filtered_xyyaw'], tr['smoothed_xyyaw'], tr['n_unique']]).reshape(-1, 9),
               delimiter=',', header='step,stamp,filtered_x,filtered_y,filtered_yaw,smoothed_x,smoothed_y,smoothed_yaw,n_unique')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('stream', help='a stream file (npz), or synth[:N]: a synthetic stream of N samples (3000) with the truth '
                                   'and a GPS fix of 0.5 m every second (synthetic_stream), replayed with SYNTH_PARAMS')
    ap.add_argument('--particles', type=int, default=4096)
    ap.add_argument('--map-grid', help='npz with z, origin, res')
    ap.add_argument('--out', help='CSV of the published mean pose')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--raw', action='store_true', help='the file holds raw sensor events: integrate them first')
    ap.add_argument('--bag', action='store_true', help='the file is a ROS 1 bag (format 2.0): replay its messages in recorded order')
    ap.add_argument('--odom-topic', default='/sam/dr/odom')
    ap.add_argument('--gps-topic', default='/sam/dr/gps')
    ap.add_argument('--mbes-topic', default='/sam/mbes_scan')
    ap.add_argument('--dive-topic', default='/dive')
    ap.add_argument('--recover', action='store_true',
                    help='global localisation with kidnap recovery (replay_recover): uniform start over the map, '
                         'augmented-MCL injection; needs --map-grid and MBES pings in the stream')
    ap.add_argument('--sigma', type=float, default=None,
                    help='MBES range sigma: of --recover (default 1.0), or the node\'s mbes_std of the plain replay (default: the '
                         'node\'s own, 0.2)')
    ap.add_argument('--innovation', action='store_true',
                    help='hold every ping against the cloud before its update (include/mcl_innovation.h) and add the run\'s mean '
                         'normalised innovation squared per beam and the mean innovation to the summary: about 1 and about 0 '
                         'when --sigma is right')
    ap.add_argument('--gate-nis', type=float, default=0.0, metavar='G',
                    help='the node\'s mbes_gate_nis: beams whose normalised innovation squared exceeds G while almost no particle '
                         'explains them are marked invalid before the update (10.83: chi^2_1 at 0.999); 0: off')
    ap.add_argument('--information', type=int, nargs='?', const=1, default=0, metavar='EVERY',
                    help='the node\'s mbes_information_every: before every EVERY-th ping (default: every ping) ask how much a ping '
                         'of that geometry can tell the cloud where it stands (include/mcl_information.h); the summary gains a '
                         'row per asked ping, the medians of the one-ping Cramer-Rao bounds along the strong and the weak axis '
                         'and the share of pings whose position information is rank-deficient; 0: off')
    ap.add_argument('--match', type=int, nargs='?', const=1, default=0, metavar='EVERY',
                    help='the node\'s mbes_match_every: after the update of every EVERY-th ping (default: every ping) fit that '
                         'ping alone to the map from the published pose (include/mcl_match.h); nothing is fed back; the summary '
                         'gains match_calls, match_converged_share, match_rmse_xy (against the stream\'s truth, beside the '
                         'filter\'s own match_filter_rmse_xy) and match_rms_residual_median; plain stream replay only; 0: off')
    ap.add_argument('--swath', type=int, nargs='+', default=None, metavar='K',
                    help='--swath K [EVERY]: the node\'s mbes_swath_pings and mbes_swath_every: after the update of every EVERY-th '
                         'ping (default: every ping) fit the last K pings, tied by the odometry, to the map as one rigid set from the '
                         'published pose (include/mcl_swath.h); nothing is fed back; the summary gains swath_calls, '
                         'swath_converged_share, swath_rmse_xy (beside the filter\'s own swath_filter_rmse_xy) and '
                         'swath_rms_residual_median -- with --match, match_rmse_xy stands beside them; plain stream replay only')
    ap.add_argument('--reseed', type=int, default=0, metavar='K',
                    help='--recover: sensor resetting (include/mcl_reseed.h): inject at the fixes of a swath match of the last K '
                         'pings started on a lattice over the map, instead of uniformly; the summary gains reseed_calls, '
                         'reseed_fallbacks, reseed_components_median and first_ping_within_1m_after_kidnap; 0: off')
    ap.add_argument('--reseed-pitch', type=float, default=4.0, metavar='P', help='--reseed: the lattice\'s spacing in metres')
    ap.add_argument('--reseed-yaw-window', type=float, default=None, metavar='W',
                    help='--reseed: start yaws within +-W radians of the odometry\'s heading (a compass) instead of the full circle')
    ap.add_argument('--kld', type=float, default=0.0, metavar='EPS',
                    help='--recover: KLD-sampling across handles (include/mcl_kld.h) with the KL error EPS: the cloud moves '
                         'between engines of the sizes of --kld-sizes as the occupied cells of its lattice ask')
    ap.add_argument('--kld-sizes', type=int, nargs='+', default=None, metavar='N',
                    help='--kld: the particle counts of the ladder (default: --particles and its 8th, 64th, 512th)')
    ap.add_argument('--kld-cell', type=float, default=0.5, metavar='C', help='--kld: the cell of the lattice in metres')
    ap.add_argument('--kld-n-yaw', type=int, default=36, metavar='Y', help='--kld: the yaw bins of the lattice')
    ap.add_argument('--mbes-every', type=int, default=0, metavar='K',
                    help='synthetic streams: a multibeam ping every K samples over a synthetic map the stream carries')
    ap.add_argument('--outliers', type=float, nargs=2, default=None, metavar=('FRACTION', 'SHORTEN_M'),
                    help='synthetic streams with --mbes-every: that share of the beams comes back SHORTEN_M metres short')
    ap.add_argument('--credible', type=float, default=0.0, metavar='P',
                    help='after every published pose also ask the cloud for the radius that holds the share P of the posterior '
                         'about it (the node\'s credible_prob, include/mcl_quantile.h); with a truth the summary gains '
                         'credible_radius_median and credible_containment, the share of poses whose true position lay inside '
                         'the stated radius (a well-tuned filter gives about P); 0: off')
    ap.add_argument('--estimate', choices=('mean', 'mode', 'median'), default='mean',
                    help='--recover: publish the mean pose, the heaviest cluster of the cloud (mcl_pose_modes), or the component-wise '
                         'median of x and y (mcl_cloud_quantiles)')
    ap.add_argument('--smooth', type=int, default=0, metavar='LAG',
                    help='also emit the fixed-lag smoothed track: every resampled ping as the LAG pings after it correct it '
                         '(particle genealogy, include/mcl_history.h); --out then writes it next to the filtered track')
    ap.add_argument('--fix-period', type=float, default=0.0, metavar='S',
                    help='make an acoustic position fix from the truth track every S seconds (a stream with truth_xyz)')
    ap.add_argument('--fix-latency', type=float, default=0.0, metavar='S', help='deliver each fix S seconds after its stamp')
    ap.add_argument('--fix-std', type=float, default=1.0, metavar='M', help='noise of the fixes and the std the node gives them')
    ap.add_argument('--fix-history-depth', type=int, default=0, metavar='N',
                    help='the node keeps N frames of the particles\' past and applies each fix at its stamp '
                         '(include/mcl_acoustic.h); 0: to the cloud as it is when the fix arrives')
    ap.add_argument('--temper-ess', type=float, default=0.0, metavar='RATIO',
                    help='temper every likelihood to an effective sample size of at least RATIO x particles before its '
                         'resampling (the node\'s temper_ess_ratio, include/mcl_temper.h); the summary reports the mean and '
                         'the minimum exponent; 0: off')
    ap.add_argument('--estimate-drift', action='store_true',
                    help='every particle carries a water current and a yaw-rate bias (the node\'s estimate_drift, '
                         'include/mcl_drift.h); the summary gains drift_mean, and drift_error against a synthetic stream')
    ap.add_argument('--drift-init-std', type=float, nargs=3, default=None, metavar=('CX', 'CY', 'BW'),
                    help='the prior\'s standard deviations [m/s, m/s, rad/s] (the node\'s drift_init_std)')
    ap.add_argument('--drift-walk-std', type=float, nargs=3, default=None, metavar=('CX', 'CY', 'BW'),
                    help='the random walk\'s, per sqrt(second) (the node\'s drift_walk_std)')
    ap.add_argument('--regularise', type=float, default=0.0, metavar='SCALE',
                    help='after every resampling jitter each particle with h^2 x the cloud\'s own covariance, h = SCALE x the '
                         'kernel-density bandwidth (the node\'s regularise_scale, include/mcl_regularise.h; 1.0 is the '
                         'textbook value); the summary gains regularise_scale and the mean h; 0: off')
    ap.add_argument('--no-regularise-shrink', action='store_true',
                    help='plain jitter: do not shrink towards the mean first (the node\'s regularise_shrink = false)')
    ap.add_argument('--current', type=float, nargs=2, default=(0.0, 0.0), metavar=('CX', 'CY'),
                    help='synthetic streams: a water current [m/s, odom frame] the odometry does not see')
    ap.add_argument('--yaw-rate-bias', type=float, default=0.0, metavar='B',
                    help='synthetic streams: a yaw-rate bias [rad/s] the odometry does not see')
    a = ap.parse_args(argv)
    synthetic = a.stream == 'synth' or a.stream.startswith('synth:')
    if (tuple(a.current) != (0.0, 0.0) or a.yaw_rate_bias != 0.0) and not synthetic:
        ap.error('--current / --yaw-rate-bias: only with a synthetic stream (synth[:N])')
    if synthetic and (a.bag or a.raw or a.recover):
        ap.error('synth[:N]: only with the plain stream replay')
    if (a.estimate_drift or a.drift_init_std or a.drift_walk_std) and (a.bag or a.recover):
        ap.error('--estimate-drift: only with the plain stream replay')
    if (a.drift_init_std or a.drift_walk_std) and not a.estimate_drift:
        ap.error('--drift-init-std / --drift-walk-std need --estimate-drift')
    if not (a.regularise >= 0.0 and np.isfinite(a.regularise)):
        ap.error('--regularise: SCALE must be finite and >= 0')
    if (a.regularise > 0 or a.no_regularise_shrink) and (a.bag or a.recover):
        ap.error('--regularise: only with the plain stream replay')
    if a.no_regularise_shrink and not a.regularise > 0:
        ap.error('--no-regularise-shrink needs --regularise SCALE')
    if not 0.0 <= a.credible <= 1.0:
        ap.error('--credible: P must lie in [0, 1]')
    if not (a.gate_nis >= 0.0 and np.isfinite(a.gate_nis)):
        ap.error('--gate-nis: G must be finite and >= 0')
    if (a.gate_nis > 0 or a.innovation) and (a.bag or a.recover):
        ap.error('--gate-nis / --innovation: only with the plain stream replay')
    if a.information < 0 or (a.information > 0 and (a.bag or a.recover)):
        ap.error('--information: EVERY >= 0, and only with the plain stream replay')
    if a.match < 0 or (a.match > 0 and (a.bag or a.recover)):
        ap.error('--match: EVERY >= 0, and only with the plain stream replay')
    if a.swath is not None and (len(a.swath) > 2 or a.swath[0] < 1 or a.swath[0] > 64 or (len(a.swath) == 2 and a.swath[1] < 1)
                                or a.bag or a.recover):
        ap.error('--swath K [EVERY]: 1 <= K <= 64, EVERY >= 1, and only with the plain stream replay')
    if not 0 <= a.reseed <= 64 or (a.reseed > 0 and not a.recover) or not a.reseed_pitch > 0.0 or (
            a.reseed_yaw_window is not None and not 0.0 < a.reseed_yaw_window <= np.pi):
        ap.error('--reseed K: 0 <= K <= 64, only with --recover; --reseed-pitch P > 0; --reseed-yaw-window 0 < W <= pi')
    kld_given = a.kld != 0.0 or a.kld_sizes is not None
    if (kld_given and not a.recover) or not (a.kld >= 0.0 and np.isfinite(a.kld)) or (a.kld_sizes is not None and (
            a.kld == 0.0 or min(a.kld_sizes) < 1)) or not a.kld_cell > 0.0 or not 1 <= a.kld_n_yaw <= 1024 or (a.kld > 0 and a.smooth > 0):
        ap.error('--kld EPS > 0, only with --recover and without --smooth; --kld-sizes N >= 1 with --kld; --kld-cell C > 0; '
                 '--kld-n-yaw 1 ... 1024')
    if a.sigma is not None and not (a.sigma > 0.0 and np.isfinite(a.sigma)):
        ap.error('--sigma must be finite and > 0')
    if (a.mbes_every != 0 or a.outliers is not None) and not synthetic:
        ap.error('--mbes-every / --outliers: only with a synthetic stream (synth[:N])')
    if a.mbes_every < 0 or (a.outliers is not None and not (a.mbes_every > 0 and 0.0 <= a.outliers[0] <= 1.0 and a.outliers[1] >= 0.0)):
        ap.error('--mbes-every K > 0; --outliers FRACTION in [0, 1] and SHORTEN_M >= 0, with --mbes-every')
    if a.credible > 0 and a.bag:
        ap.error('--credible: not with --bag')
    if not 0.0 <= a.temper_ess <= 1.0:
        ap.error('--temper-ess: RATIO must lie in [0, 1]')
    if a.temper_ess > 0 and (a.bag or a.recover):
        ap.error('--temper-ess: only with the plain stream replay')
    if a.smooth < 0 or a.smooth >= 1024:
        ap.error('--smooth: LAG must be 0 ... 1023')
    if a.fix_period > 0 and a.smooth > 0:
        ap.error(FIX_SMOOTH_CLASH)
    if a.fix_period > 0 and (a.bag or a.recover):
        ap.error('--fix-period: only with the plain stream replay')
    if a.fix_period < 0 or a.fix_latency < 0 or not a.fix_std > 0 or not 0 <= a.fix_history_depth <= 1024:
        ap.error('--fix-period / --fix-latency >= 0, --fix-std > 0, --fix-history-depth 0 ... 1024')
    if a.bag:
        grid = dict(np.load(a.map_grid)) if a.map_grid else None
        res = replay_bag(a.stream, dict(particle_count=a.particles, seed=a.seed), grid=grid, odom_topic=a.odom_topic,
                         gps_topic=a.gps_topic, mbes_topic=a.mbes_topic, dive_topic=a.dive_topic)
        if a.out:
            np.savetxt(a.out, np.column_stack([res['pf_stamp'], res['pf_xyz']]), delimiter=',', header='stamp,x,y,z')
        print(json.dumps(res['summary']))
        return
    if synthetic:
        stream = synthetic_stream(int(a.stream[6:]) if a.stream[5:6] == ':' else 3000, a.current, a.yaw_rate_bias, seed=a.seed,
                                  mbes_every=a.mbes_every, outliers=a.outliers)
    else:
        stream = dict(np.load(a.stream, allow_pickle=False))
    m2o = None
    if a.raw:
        ptf = stream.get('pressure_tf')
        if ptf is not None and np.isnan(ptf).any():
            ptf = None
        stream, m2o = odom_stream_from_raw(stream['ev_t'], stream['ev_kind'], stream['ev_data'],
                                           gps_map=stream.get('gps_map'), pressure_tf=ptf)
    grid = dict(np.load(a.map_grid)) if a.map_grid else None
    if a.recover:
        res = replay_recover(stream, grid=grid, particles=a.particles, seed=a.seed, sigma=1.0 if a.sigma is None else a.sigma, m2o=m2o,
                             estimate=a.estimate, smooth_lag=a.smooth, credible=a.credible, reseed=a.reseed,
                             reseed_pitch=a.reseed_pitch, reseed_yaw_window=a.reseed_yaw_window, kld=a.kld,
                             kld_sizes=a.kld_sizes, kld_cell=a.kld_cell, kld_n_yaw=a.kld_n_yaw)
        if a.out:
            np.savetxt(a.out, np.column_stack([res['pub_idx'], res['pf_xyz'], res['fractions']]), delimiter=',',
                       header='step,x,y,z,injected_fraction')
            save_smooth(a.out, res)
        print(json.dumps(res['summary']))
        return
    params = dict(particle_count=a.particles, seed=a.seed)
    if synthetic:
        params.update(SYNTH_PARAMS)
    if a.temper_ess > 0:
        params.update(temper_ess_ratio=a.temper_ess)
    if a.estimate_drift:
        params.update(estimate_drift=True)
        if a.drift_init_std:
            params.update(drift_init_std=str([float(x) for x in a.drift_init_std]))
        if a.drift_walk_std:
            params.update(drift_walk_std=str([float(x) for x in a.drift_walk_std]))
    if a.credible > 0:
        params.update(credible_prob=a.credible)
    if a.gate_nis > 0:
        params.update(mbes_gate_nis=a.gate_nis)
    if a.information > 0:
        params.update(mbes_information_every=a.information)
    if a.match > 0:
        params.update(mbes_match_every=a.match)
    if a.swath is not None:
        params.update(mbes_swath_pings=a.swath[0], mbes_swath_every=a.swath[1] if len(a.swath) == 2 else 1)
    if a.sigma is not None:
        params.update(mbes_std=a.sigma)
    if a.regularise > 0:
        params.update(regularise_scale=a.regularise, regularise_shrink=not a.no_regularise_shrink)
    if a.fix_period > 0:
        params.update(fix_topic='/sam/external/uw_gps_odom', fix_std=a.fix_std, fix_history_depth=a.fix_history_depth,
                      fix_max_age=max(10.0, 2.0 * a.fix_latency))
    res = replay(stream, params, m2o=m2o, grid=grid, smooth_lag=a.smooth, fix_period=a.fix_period,
                 fix_latency=a.fix_latency, fix_seed=a.seed, innovation=a.innovation)
    if a.out:
        np.savetxt(a.out, np.column_stack([res['pub_idx'], res['pf_xyz']]), delimiter=',', header='step,x,y,z')
        save_smooth(a.out, res)
    print(json.dumps(res['summary']))


if __name__ == '__main__':
    main()
