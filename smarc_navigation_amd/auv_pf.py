"""Host-side mirror of the reference node class `auv_pf` (auv_particle_filter/scripts/auv_pf.py):
same class name, method names, parameter names/defaults and message fields -- the per-particle
Python loops are replaced by calls through the C ABI (libmcl_hip.so).  ROS-free core: transport
(publishers, tf) is injected; `ros_node.py` plugs in rospy when ROS is installed.

Divergences from the reference, all documented in INTEGRATION.md:
  * one owner lock around the handle (the reference's three rospy threads are unlocked);
  * the GPS gate `self.time > self.old_time` (auv_pf.py:126, only true mid-callback) is "every fix
    while not diving";
  * default resampling scheme on the GPU is systematic (resampling.py:135); pass
    resample_scheme='residual' for the node's literal behaviour (auv_pf.py:182).
"""
import bisect
import collections
import logging
import math
import threading

import numpy as np

from . import engine as _engine
from . import msgs as _msgs

_SCHEMES = {'systematic': _engine.SYSTEMATIC, 'residual': _engine.RESIDUAL,
            'stratified': _engine.STRATIFIED, 'multinomial': _engine.MULTINOMIAL}

DEFAULT_PARAMS = {
    # auv_pf.py:27-31
    'particle_count': 10, 'map_frame': 'map', 'base_frame': 'base_link', 'utm_frame': 'utm',
    'odom_frame': 'sam/odom',
    # auv_pf.py:39 (+ launch defaults auv_pf.launch:17-20 for the three strings, which have no code default)
    'measurement_std': 0.01,
    'motion_covariance': '[0.0000, 0.0000, 0.0, 0.0, 0.0, 0.000000000001]',
    'init_covariance': '[0.1, 0.1, 0.0, 0.0, 0.0, 0.0]',
    'resampling_noise_covariance': '[1., 1., 0.0, 0.0, 0.0, 0.0001]',
    # topics (auv_pf.py:64,71,101,106,110)
    'particle_poses_topic': '/particle_poses', 'odom_corrected_topic': '/average_pose',
    'aux_dive': '/dive', 'gps_odom_topic': '/gps', 'odom_topic': 'odom',
    # new, behaviour-preserving defaults
    'resample_scheme': 'systematic', 'seed': 0, 'device': 0,
    'mbes_topic': '/mbes_scan', 'mbes_std': 0.2, 'mbes_sensor_offset': '[0.0, 0.0, 0.0, 0.0, 0.0, 0.0]',
    # the bathymetric map the MBES update casts against: an .npz with `z` (nx, ny) + `origin` (2) + `res` (height
    # grid, map frame) or with `verts` (nv, 3) + `tris` (nt, 3); an ASCII .ply triangle mesh; a .mclgrid height grid
    # (save_mclgrid: the format the roscpp node reads too).  '' = no map: pings ignored
    'map_grid_file': '', 'map_mesh_file': '',
    # MBES pings as sensor_msgs/PointCloud2 (what mbes_mapper's receptor makes of a LaserScan,
    # mbes_receptor.cpp:126-165): '' = not subscribed.  `mbes_points_frame`: 'base' -- points in base_frame, as
    # transformLaserScanToPointCloud(base_frame_, ...) leaves them -- or 'sensor'
    'mbes_pointcloud_topic': '', 'mbes_points_frame': 'base', 'mbes_range_max': 100.0,
    # BASELINE config 5: landmark detections with per-particle k-NN data association.  `landmark_map_file`: the
    # feature map -- the .yaml the reference's map provider serves (auv_ekf_localization/scripts/map_provider_node.py:
    # 35-56: a list of models with position {x, y, z}, those below `rocks_depth` kept), an .npz with `landmarks`
    # (n, 3), or a text file of x y z rows; map frame.  '' = no landmark map: detections ignored.
    # `lm_detect_topic`: geometry_msgs/PoseArray of detections in base_frame, positions only, as the MBES receptors
    # publish them (mbes_toy_processor/src/toy_mbes_receptor.cpp:68-110; consumer auv_ekf_slam/src/ekf_slam.cpp:41).
    # The receptor stamps a detection message with its ping's stamp and publishes it AFTER processing the ping, so in a
    # live system it reaches the node when that ping's update and resampling are done: it is then a measurement update
    # of its own, followed by the resampling (detections and ranges are independent measurements of the same pose).  A
    # stream that delivers the detections first (a bag replayed by topic) has them wait for the ping with THEIR stamp
    # (equal within `landmark_sync_tol` seconds: the stamps are copies of one another), whose likelihood they join
    # before the resampling.  Without a bathymetric map a detection message is always an update of its own.  Detections
    # older than `landmark_max_age` seconds of the filter's clock (the latest odometry stamp) are dropped: their
    # base_frame positions describe a pose the cloud has long left.
    # NOTE (live order): a detection message that follows its ping is its OWN update + resampling, so with a receptor
    # running the filter resamples -- and adds `resampling_noise_covariance` -- TWICE per ping (once for the ranges, once
    # for the detections); choose the resampling noise for that rate.  `landmark_late` = 'drop' ignores detections that
    # arrive after their ping instead (one resampling per ping; detections then only count when they come ahead of
    # their ping and join its likelihood).
    'landmark_map_file': '', 'rocks_depth': float('inf'), 'lm_detect_topic': '/landmarks_detected',
    'landmark_std': 0.3, 'landmark_k': 1, 'landmark_gate': 11.345, 'landmark_sync_tol': 1e-3, 'landmark_max_age': 0.5,
    'landmark_late': 'update',
    # DVL bottom range (terrain-aided navigation against the bathymetric map): smarc_msgs/DVL on `dvl_topic` (the
    # reference's /sam/core/dvl, sam_dead_reckoning/scripts/dr_node.py:23,89; '' = not subscribed).  Its `altitude` is
    # one range along the DVL frame's -z axis; the frame sits at `dvl_sensor_offset` in base_frame.  Each altitude is a
    # measurement update of its own followed by the resampling, like a GPS fix.
    'dvl_topic': '', 'dvl_altitude_std': 0.2, 'dvl_range_max': 60.0,
    'dvl_sensor_offset': '[0.0, 0.0, 0.0, 0.0, 0.0, 0.0]',
    # Acoustic position fixes (underwater GPS / USBL): nav_msgs/Odometry on `fix_topic` (the reference's
    # /sam/external/uw_gps_odom, uw_gps/scripts/uw_gps_node.py:137,160-167; '' = not subscribed), position in the
    # message's header.frame_id (map_frame, or anything the transport can take to it), isotropic `fix_std` metres.  A fix
    # is OLD when it arrives.  `fix_history_depth` > 0 keeps the particle genealogy (include/mcl_history.h) in a ring of
    # that many frames, one per resampling, and weights every particle by the pose its ancestor had at the fix's stamp
    # (include/mcl_acoustic.h); a fix older than the ring or than `fix_max_age` seconds is dropped.  Depth 0: every fix is
    # applied to the cloud as it is now (right only when the latency is small against fix_std / speed).  Each fix is a
    # measurement update of its own followed by the resampling, like a GPS fix -- diving or not.
    # Frames come with the resamplings; where nothing resamples for fix_max_age / fix_history_depth seconds the node
    # records one on its own, so the ring spans fix_max_age.
    'fix_topic': '', 'fix_std': 1.0, 'fix_history_depth': 0, 'fix_max_age': 10.0,
    # ESS-targeted likelihood tempering (include/mcl_temper.h): > 0: before EVERY resampling (GPS, MBES, DVL, landmarks,
    # fix) the pending likelihood is raised to the largest power beta <= 1 of the library's lattice that leaves an
    # effective sample size of at least this fraction of the cloud; a ping that leaves more is not touched (beta = 1).
    # 0 = off: the call is never made and the node computes what it computed without the parameter.
    'temper_ess_ratio': 0.0,
    # Per-particle drift states (include/mcl_drift.h): true: every particle carries its own water current (cx, cy [m/s],
    # odom_frame) and yaw-rate bias (bw [rad/s]), drawn from N(0, drift_init_std^2), random-walking with drift_walk_std per
    # sqrt(second); every predict is preceded by drift_advance(dt), every resampling takes the drift along, and
    # `drift_mean` / `drift_cov` are refreshed with the mean pose.  The two strings hold three numbers (cx, cy, bw) and
    # are parsed like the covariance strings.  false = off: the call is never made and the node computes what it
    # computed without the parameters.
    'estimate_drift': False, 'drift_init_std': '[0.2, 0.2, 0.0]', 'drift_walk_std': '[0.005, 0.005, 0.0]',
    # Regularised resampling (include/mcl_regularise.h): > 0: right after every resampling each particle is jittered with
    # h^2 times the cloud's own sample covariance of (x, y, yaw) -- with estimate_drift, of (x, y, yaw, cx, cy, bw) jointly
    # -- h = regularise_scale x the kernel-density bandwidth for the particle count (1.0 is the textbook value);
    # regularise_shrink: shrink towards the mean first (Liu-West), so that the cloud's mean and covariance stay what they
    # were.  It comes on top of resampling_noise_covariance, which may then be zero.  0 = off: the call is never made and
    # the node computes what it computed without the parameters.
    'regularise_scale': 0.0, 'regularise_shrink': True,
    # Credible region (include/mcl_quantile.h): a probability in (0, 1]: every loc_loop also asks the cloud for the radius
    # that holds that share of the posterior about the pose it publishes, and for the heading half-width that does -- exact
    # order statistics, kept in `last_credible`.  There is no standard message for it: nothing more is published.  0 = off:
    # the call is never made and the node computes what it computed without the parameter.
    'credible_prob': 0.0,
    # Per-beam outlier gate (include/mcl_innovation.h): > 0: every MBES ping is first held against the cloud as it is -- the
    # innovation of each beam over a strided sample of 4096 particles -- and the beams whose normalised innovation squared
    # exceeds this value while under 1 % of the sample explains them (fish, a bottom-detection failure) are marked invalid
    # (range 0) before the unchanged update; 10.83 is chi^2_1 at 0.999.  When more than a quarter of the beams qualify
    # nothing is gated: the ping disagrees with the cloud as a whole (`last_innovation.inconsistent`).  The verdict of the
    # last ping is kept in `last_innovation`.  0 = off: the call is never made and the node computes what it computed
    # without the parameter.
    'mbes_gate_nis': 0.0,
    # Ping information (include/mcl_information.h): K > 0: every K-th MBES ping, before anything else is done with it, the
    # node asks how much a ping of that geometry can tell the cloud as it is -- the Cramer-Rao bounds of one ping along
    # the direction the terrain fixes best and worst, and that worst direction -- keeps the answer in `last_information`
    # and logs it (logger 'auv_pf', at most once per `information_log_period` seconds of filter time).  Nothing of the
    # filter changes.  0 = off: the call is never made and the node computes what it computed without the parameter.
    'mbes_information_every': 0,
    # Ping matching (include/mcl_match.h): K > 0: after the update (and resampling) of every K-th MBES ping the node asks
    # where that ping alone says the vehicle is -- a Levenberg-Marquardt fix of the ping on the map, started from the pose
    # the node would publish -- keeps the answer in `last_match`, appends a row to `match_log` and logs it (logger
    # 'auv_pf', at most once per `match_log_period` seconds of filter time).  Nothing is fed back into the filter: the
    # ping has been used once already.  0 = off: the call is never made and the node computes what it computed without
    # the parameter.  A call the library refuses (a ping of more than 2048 beams, say) is logged and counted in
    # `match_errors`; the callback goes on.
    'mbes_match_every': 0,
    # Swath matching (include/mcl_swath.h): `mbes_swath_pings` K > 0: the node keeps a ring of the last K MBES pings' ranges
    # with the vehicle's odometry pose at each of them, and after the update (and resampling) of every
    # `mbes_swath_every`-th ping, once the ring is full, fits those K pings to the map as one rigid set -- tied to each other
    # by the odometry, anchored at the newest, started from the pose the node would publish -- keeps the answer in
    # `last_swath`, appends a row to `swath_log` and logs it (logger 'auv_pf', at most once per `swath_log_period` seconds
    # of filter time).  One ping cannot tell the along-track position from depth; K pings can.  Nothing is fed back into
    # the filter.  K = 0 = off: no call is made and no ring is kept.  A ping whose beam count differs from the ring's
    # restarts the ring; the newest ping's beam angles stand for all K.  A call the library refuses is logged and counted
    # in `swath_errors`; the callback goes on.
    'mbes_swath_pings': 0,
    'mbes_swath_every': 1,
}


def _as_bool(v):
    """a ROS bool parameter: a bool, a number, or the strings roslaunch may leave ('true', 'False', '1')"""
    if isinstance(v, str):
        return v.strip().lower() in ('true', '1', 'yes', 'on')
    return bool(v)


def parse_cov_string(cov_string):
    """The reference's ad-hoc parser (auv_pf.py:40-44): strip brackets, split on ', '."""
    cov_string = cov_string.replace('[', '')
    cov_string = cov_string.replace(']', '')
    cov_list = list(cov_string.split(", "))
    return list(map(float, cov_list))


def quaternion_from_euler(roll, pitch, yaw):
    """tf.transformations.quaternion_from_euler, axes 'sxyz' (auv_pf.py:233)."""
    cr, sr = math.cos(roll / 2.0), math.sin(roll / 2.0)
    cp, sp = math.cos(pitch / 2.0), math.sin(pitch / 2.0)
    cy, sy = math.cos(yaw / 2.0), math.sin(yaw / 2.0)
    return [cp * (sr * cy) - sp * (cr * sy), cp * (sr * sy) + sp * (cr * cy),
            cp * (cr * sy) - sp * (sr * cy), cp * (cr * cy) + sp * (sr * sy)]


def euler_from_quaternion(q):
    """tf.transformations.euler_from_quaternion, axes 'sxyz': (roll, pitch, yaw) of a quaternion (x, y, z, w)."""
    m = matrix_from_tf((0.0, 0.0, 0.0), q)
    cy = math.sqrt(m[0, 0] * m[0, 0] + m[1, 0] * m[1, 0])
    if cy > np.finfo(float).eps * 4.0:
        return math.atan2(m[2, 1], m[2, 2]), math.atan2(-m[2, 0], cy), math.atan2(m[1, 0], m[0, 0])
    return math.atan2(-m[1, 2], m[1, 1]), math.atan2(-m[2, 0], cy), 0.0


def load_map_file(path):
    """('grid', z, origin, res) or ('mesh', verts, tris) from an .npz (keys above), an ASCII .ply triangle mesh or a
    .mclgrid height grid."""
    if path.lower().endswith('.npz'):
        with np.load(path, allow_pickle=False) as f:
            if 'z' in f.files:
                return ('grid', np.asarray(f['z'], np.float32), tuple(float(v) for v in f['origin']), float(f['res']))
            return ('mesh', np.asarray(f['verts'], np.float32), np.asarray(f['tris'], np.uint32))
    if path.lower().endswith('.ply'):
        with open(path, 'r') as f:
            if f.readline().strip() != 'ply':
                raise ValueError('%s: not a PLY file' % path)
            nv = nf = 0
            for line in f:
                t = line.split()
                if t[:2] == ['format', 'ascii']:
                    continue
                if t and t[0] == 'format':
                    raise ValueError('%s: only ASCII PLY is read' % path)
                if t[:2] == ['element', 'vertex']:
                    nv = int(t[2])
                if t[:2] == ['element', 'face']:
                    nf = int(t[2])
                if t == ['end_header']:
                    break
            verts = np.array([[float(v) for v in f.readline().split()[:3]] for _ in range(nv)], np.float32)
            tris = []
            for _ in range(nf):
                t = [int(v) for v in f.readline().split()]
                for k in range(2, t[0]):   # fan-triangulate polygons
                    tris.append((t[1], t[k], t[k + 1]))
        return ('mesh', verts, np.array(tris, np.uint32))
    if path.lower().endswith('.mclgrid'):   # text header + raw float32 (what the roscpp node reads: pf_core.hpp)
        with open(path, 'rb') as f:
            head = f.readline().split()
            if len(head) != 6 or head[0] != b'mclgrid':
                raise ValueError('%s: bad mclgrid header' % path)
            nx, ny = int(head[1]), int(head[2])
            z = np.frombuffer(f.read(4 * nx * ny), dtype='<f4')
            if z.size != nx * ny:
                raise ValueError('%s: truncated height array' % path)
        return ('grid', z.reshape(nx, ny).astype(np.float32), (float(head[3]), float(head[4])), float(head[5]))
    raise ValueError('map file %s: expected .npz, .ply or .mclgrid' % path)


def load_landmark_file(path, rocks_depth=float('inf')):
    """(n, 3) float64 landmark positions in the map frame.  .yaml / .yml: the Gazebo model list of the reference's map
    provider (map_provider_node.py:43-52: the first top-level entry is a list of models with position {x, y, z};
    models with z < rocks_depth are kept -- the provider's own filter; its default keeps the ones below -90 m, the
    default here keeps all); .npz: key `landmarks`; anything else: whitespace-separated x y z rows."""
    low = path.lower()
    if low.endswith('.npz'):
        with np.load(path, allow_pickle=False) as f:
            pts = np.asarray(f['landmarks'], np.float64).reshape(-1, 3)
    elif low.endswith('.yaml') or low.endswith('.yml'):
        import yaml
        with open(path, 'r') as f:
            data = yaml.safe_load(f)
        models = list(data.values())[0] if isinstance(data, dict) else data
        pts = np.array([[float(m['position']['x']), float(m['position']['y']), float(m['position']['z'])]
                        for m in models], np.float64).reshape(-1, 3)
    else:
        pts = np.loadtxt(path, dtype=np.float64, ndmin=2)[:, :3]
    keep = pts[:, 2] < float(rocks_depth)
    return np.ascontiguousarray(pts[keep])


def save_mclgrid(path, z, origin, res):
    """Height grid as `mclgrid nx ny origin_x origin_y res\\n` + nx * ny little-endian float32, z[ix * ny + iy]."""
    z = np.ascontiguousarray(z, dtype='<f4')
    with open(path, 'wb') as f:
        f.write(('mclgrid %d %d %r %r %r\n' % (z.shape[0], z.shape[1], float(origin[0]), float(origin[1]), float(res))).encode())
        f.write(z.tobytes())


def matrix_from_tf(translation, rotation):
    """auv_particle.py:110-125: 4x4 from a tf translation (x,y,z) and quaternion (x,y,z,w)."""
    q = np.array(rotation[:4], dtype=np.float64)
    nq = float(np.dot(q, q))
    m = np.identity(4)
    if nq >= np.finfo(float).eps * 4.0:
        q *= math.sqrt(2.0 / nq)
        o = np.outer(q, q)
        m[:3, :3] = [[1.0 - o[1, 1] - o[2, 2], o[0, 1] - o[2, 3], o[0, 2] + o[1, 3]],
                     [o[0, 1] + o[2, 3], 1.0 - o[0, 0] - o[2, 2], o[1, 2] - o[0, 3]],
                     [o[0, 2] - o[1, 3], o[1, 2] + o[0, 3], 1.0 - o[0, 0] - o[1, 1]]]
    m[:3, 3] = translation[:3]
    return m


def _rigid(tx, ty, tz, roll, pitch, yaw):
    """T(t) R(static-xyz rpy): the pose of the sensor in base_link (`mbes_sensor_offset`)."""
    cr, sr, cp, sp, cy, sy = (math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw),
                              math.sin(yaw))
    m = np.identity(4)
    m[:3, :3] = [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                 [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                 [-sp, cp * sr, cp * cr]]
    m[:3, 3] = (tx, ty, tz)
    return m


class RecordingTransport(object):
    """Default transport: keeps what the node would have published / broadcast."""

    def __init__(self, utm2map=None):
        self.utm2map = np.identity(4) if utm2map is None else np.asarray(utm2map, dtype=np.float64)
        self.particle_poses, self.odom_corrected, self.tf = [], [], []

    def transformPoint(self, frame, pt):  # tf.TransformListener.transformPoint (auv_pf.py:151)
        v = self.utm2map.dot(np.array([pt.point.x, pt.point.y, pt.point.z, 1.0]))
        out = _msgs.PointStamped()
        out.header.frame_id = frame
        out.point.x, out.point.y, out.point.z = float(v[0]), float(v[1]), float(v[2])
        return out

    def publish_poses(self, msg):
        self.particle_poses.append(msg)

    def publish_odom(self, msg):
        self.odom_corrected.append(msg)

    def sendTransform(self, trans, rot, stamp, child, parent):
        self.tf.append((list(trans), list(rot), stamp, child, parent))

    def now(self):
        return _msgs.Time(0.0)


class auv_pf(object):

    def __init__(self, params=None, m2o_mat=None, transport=None, rng_mode=_engine.RNG_NATIVE):
        p = dict(DEFAULT_PARAMS)
        p.update(params or {})
        self.params = p
        self.pc = int(p['particle_count'])
        self.map_frame, self.base_frame = p['map_frame'], p['base_frame']
        self.utm_frame, self.odom_frame = p['utm_frame'], p['odom_frame']
        meas_std = float(p['measurement_std'])
        motion_cov = parse_cov_string(p['motion_covariance'])
        init_cov = parse_cov_string(p['init_covariance'])
        self.res_noise_cov = parse_cov_string(p['resampling_noise_covariance'])
        self.mbes_std = float(p['mbes_std'])
        self.mbes_sensor_offset = parse_cov_string(p['mbes_sensor_offset'])
        self.transport = transport if transport is not None else RecordingTransport()
        self.m2o_mat = np.identity(4) if m2o_mat is None else np.asarray(m2o_mat, dtype=np.float64)
        self.lock = threading.Lock()
        # the particle list of auv_pf.py:89-94 lives in HBM
        self.particles = _engine.Engine(self.pc, init_cov=init_cov, process_cov=motion_cov,
                                        resample_cov=self.res_noise_cov, meas_std=meas_std, m2o=self.m2o_mat,
                                        seed=int(p['seed']), rng_mode=rng_mode,
                                        resample_scheme=_SCHEMES[p['resample_scheme']], device=int(p['device']))
        self._replay = None  # REPLAY mode: object with randn(n,6) / random_sample(k)
        if rng_mode == _engine.RNG_NATIVE:
            self.particles.init_particles()
        self.poses = _msgs.PoseArray()
        self.poses.header.frame_id = self.odom_frame
        self.loc_pose = _msgs.Odometry()
        self.loc_pose.header.frame_id = self.odom_frame
        self.loc_pose.child_frame_id = self.base_frame
        self.cov = np.zeros((3, 3))
        self.time = 0.0
        self.old_time = 0.0
        self.diving = True  # auv_pf.py:103
        self.odom_latest = None
        self.has_map = False
        self.mbes_range_max = float(p['mbes_range_max'])
        self.mbes_points_frame = p['mbes_points_frame']
        self.dvl_altitude_std, self.dvl_range_max = float(p['dvl_altitude_std']), float(p['dvl_range_max'])
        self.dvl_sensor_offset = parse_cov_string(p['dvl_sensor_offset'])
        for key in ('map_grid_file', 'map_mesh_file'):   # the node's own map parameters
            if p[key]:
                self.load_map(p[key])
        # landmark detections (config 5)
        self.has_landmarks = False
        self.landmark_std, self.landmark_k = float(p['landmark_std']), int(p['landmark_k'])
        self.landmark_gate, self.landmark_sync_tol = float(p['landmark_gate']), float(p['landmark_sync_tol'])
        self.landmark_max_age = float(p['landmark_max_age'])
        self.landmark_late = str(p['landmark_late'])
        if self.landmark_late not in ('update', 'drop'):
            raise ValueError("landmark_late must be 'update' or 'drop', not %r" % self.landmark_late)
        self._pending_det = None   # (stamp, (n_det, 3) detections in base_frame) that arrived AHEAD of their ping
        self._last_ping_stamp = None
        if p['landmark_map_file']:
            self.set_landmarks(load_landmark_file(p['landmark_map_file'], float(p['rocks_depth'])))
        # delayed acoustic fixes
        self.fix_std, self.fix_max_age = float(p['fix_std']), float(p['fix_max_age'])
        self.fix_history_depth = int(p['fix_history_depth'])
        self.fixes_applied = self.fixes_dropped = 0
        self.fix_lag_sum = 0.0      # summed age (filter clock - stamp) of the applied fixes
        self._zrp_log = collections.deque(maxlen=4096)   # (stamp, z, roll, pitch) of the odometry, for the fix's stamp
        self._fix_last_record = None   # stamp of the ring's newest frame (None: the ring is empty)
        if self.fix_history_depth > 0:
            self.particles.history_enable(self.fix_history_depth)
        # likelihood tempering
        self.temper_ess_ratio = float(p['temper_ess_ratio'])
        if not 0.0 <= self.temper_ess_ratio <= 1.0:
            raise ValueError('temper_ess_ratio must lie in [0, 1], not %r' % self.temper_ess_ratio)
        self.temper_last_beta = 1.0     # beta of the last resampling (1: not tempered)
        self.temper_last = None         # its TemperResult
        self.tempered_updates = 0       # resamplings whose likelihood was tempered (beta < 1)
        self.temper_betas = []          # beta of every resampling since the start, in order
        # per-particle drift states
        self.estimate_drift = _as_bool(p['estimate_drift'])
        self.drift_mean, self.drift_cov = np.zeros(3), np.zeros((3, 3))   # of (cx, cy, bw): refreshed by update_loc_pose
        if self.estimate_drift:
            self.drift_init_std = parse_cov_string(p['drift_init_std'])
            self.drift_walk_std = parse_cov_string(p['drift_walk_std'])
            if len(self.drift_init_std) != 3 or len(self.drift_walk_std) != 3:
                raise ValueError('drift_init_std and drift_walk_std hold three numbers (cx, cy, bw)')
            why = _engine.drift_config_check(self.drift_init_std, self.drift_walk_std)
            if why:
                raise ValueError('estimate_drift: ' + why)
            if rng_mode == _engine.RNG_NATIVE:
                self.particles.drift_enable(self.drift_init_std, self.drift_walk_std)
        self._drift_enabled = self.estimate_drift and rng_mode == _engine.RNG_NATIVE
        # regularised resampling
        self.regularise_scale = float(p['regularise_scale'])
        self.regularise_shrink = _as_bool(p['regularise_shrink'])
        if self.regularise_scale != 0.0:
            why = _engine.regularise_config_check(self.regularise_scale, self.regularise_shrink,
                                                  6 if self.estimate_drift else 3)
            if why:
                raise ValueError('regularise_scale: ' + why)
        self.regularise_calls = 0       # resamplings that were regularised
        # credible region about the published pose
        self.credible_prob = float(p['credible_prob'])
        if not 0.0 <= self.credible_prob <= 1.0:
            raise ValueError('credible_prob must lie in [0, 1], not %r' % self.credible_prob)
        self.last_credible = None       # dict(prob, radius, yaw_halfwidth, n_used, centre) of the last loc_loop
        self.credible_calls = 0
        self.regularise_hs = []         # the bandwidth h of each, in order (host arithmetic: regularise_bandwidth)
        # per-beam outlier gate in front of every MBES update
        self.mbes_gate_nis = float(p['mbes_gate_nis'])
        if not self.mbes_gate_nis >= 0.0 or math.isinf(self.mbes_gate_nis):
            raise ValueError('mbes_gate_nis must be finite and >= 0, not %r' % self.mbes_gate_nis)
        self.last_innovation = None     # the GateVerdict of the last ping
        self.gate_calls = 0
        self.gated_beams = 0            # beams marked invalid so far
        # ping information in front of every K-th MBES ping
        self.mbes_information_every = int(p['mbes_information_every'])
        if self.mbes_information_every < 0 or self.mbes_information_every != p['mbes_information_every']:
            raise ValueError('mbes_information_every must be an integer >= 0, not %r' % (p['mbes_information_every'],))
        self.information_log_period = 5.0
        self.last_information = None    # the PingInformation of the last ping that was asked
        self.information_calls = 0
        self.information_log = []       # (stamp, crlb_strong, crlb_weak, weak_axis, rank_pos, hit_share) of every call
        self._mbes_pings = 0
        self._information_logged = None
        # ping matching behind every K-th MBES ping
        self.mbes_match_every = int(p['mbes_match_every'])
        if self.mbes_match_every < 0 or self.mbes_match_every != p['mbes_match_every']:
            raise ValueError('mbes_match_every must be an integer >= 0, not %r' % (p['mbes_match_every'],))
        self.match_log_period = 5.0
        self.last_match = None          # dict: the start, the fix (or None), its status and rms residual
        self.match_calls = 0
        self.match_errors = 0           # calls the library refused (logged; the filter is not affected)
        self.match_log = []             # (stamp, status, x, y, yaw, rms, evaluations, start x, start y, start yaw) of every call
        self._match_pings = 0
        self._match_logged = None
        # swath matching: the last K pings as one rigid set, behind every E-th MBES ping
        # (the range first: a NaN fails every comparison, an infinity has no int())
        if not 0 <= p['mbes_swath_pings'] <= _engine.SWATH_MAX_PINGS or int(p['mbes_swath_pings']) != p['mbes_swath_pings']:
            raise ValueError('mbes_swath_pings must be an integer in 0 ... %d, not %r' % (_engine.SWATH_MAX_PINGS, p['mbes_swath_pings']))
        if not 1 <= p['mbes_swath_every'] < float('inf') or int(p['mbes_swath_every']) != p['mbes_swath_every']:
            raise ValueError('mbes_swath_every must be an integer >= 1, not %r' % (p['mbes_swath_every'],))
        self.mbes_swath_pings, self.mbes_swath_every = int(p['mbes_swath_pings']), int(p['mbes_swath_every'])
        self.swath_log_period = 5.0
        self.last_swath = None          # dict: the start, the fix (or None), its status and rms residual, the offsets
        self.swath_calls = 0
        self.swath_errors = 0           # calls the library refused (logged; the filter is not affected)
        self.swath_log = []             # rows as match_log's
        self._swath_ring = collections.deque(maxlen=self.mbes_swath_pings) if self.mbes_swath_pings > 0 else None
        self._swath_pings = 0
        self._swath_logged = None

    # ---- REPLAY-mode RNG source (parity runs): rs must offer randn(n, 6) and random_sample(k)
    def set_replay_source(self, rs):
        self._replay = rs
        self.particles.init_particles(rs.randn(self.pc, 6))
        self._fix_last_record = None   # (a re-initialisation clears the ring: include/mcl_history.h)
        if self.estimate_drift:
            # (the drift does not follow a re-initialisation on its own: include/mcl_drift.h)
            if self._drift_enabled:
                self.particles.drift_reset(rs.randn(self.pc, 3))
            else:
                self.particles.drift_enable(self.drift_init_std, self.drift_walk_std, rs.randn(self.pc, 3))
                self._drift_enabled = True

    def start_timing(self, stamp):
        """auv_pf.py:96-98: `Start timing now`."""
        self.time = float(stamp)
        self.old_time = float(stamp)

    # ---- callbacks, same names as the reference
    def dive_cb(self, dive_msg):
        self.diving = dive_msg.data

    def odom_callback(self, odom_msg):
        with self.lock:
            self.time = odom_msg.header.stamp.to_sec()
            self.odom_latest = odom_msg
            if self.fix_history_depth > 0:
                self._log_zrp(odom_msg)
            if self.old_time and self.time > self.old_time:
                self.predict(odom_msg)
            self.old_time = self.time

    def predict(self, odom_t):
        dt = self.time - self.old_time
        tw, po = odom_t.twist.twist, odom_t.pose.pose
        if self.estimate_drift:
            # the current and the rate bias move the particles before the odometry does (include/mcl_drift.h)
            self.particles.drift_advance(dt, self._replay.randn(self.pc, 3) if self._replay is not None else None)
        nz = self._replay.randn(self.pc, 6) if self._replay is not None else None
        self.particles.predict([tw.linear.x, tw.linear.y, tw.linear.z], tw.angular.z,
                               [po.orientation.x, po.orientation.y, po.orientation.z, po.orientation.w],
                               po.position.z, dt, nz, stamp=self.time)

    def gps_odom_cb(self, gps_odom):
        with self.lock:
            if self.old_time and not self.diving:
                weights = self.update(gps_odom)
                self.resample(weights)

    def update(self, gps_odom):
        goal_point = _msgs.PointStamped()
        goal_point.header.frame_id = self.utm_frame
        goal_point.point.x = gps_odom.pose.pose.position.x
        goal_point.point.y = gps_odom.pose.pose.position.y
        goal_point.point.z = 0.
        gps_map = self.transport.transformPoint(self.map_frame, goal_point)  # once, not per particle
        self.particles.update_gps(gps_map.point.x, gps_map.point.y)
        return self.particles  # the weights stay in HBM; resample() consumes them there

    def resample(self, weights):
        if self.temper_ess_ratio > 0.0:
            # the one seam every update goes through: temper what it left, then resample
            self.temper_last = self.particles.temper(self.temper_ess_ratio)
            self.temper_last_beta = self.temper_last.beta
            self.temper_betas.append(self.temper_last.beta)
            if self.temper_last.j > 0:
                self.tempered_updates += 1
        if self._replay is not None:
            need = self.particles.resample_prepare()
            u = self._replay.random_sample(need) if need != 1 else self._replay.random_sample()
            self.particles.resample(u, self._replay.randn(self.pc, 6))
        else:
            self.particles.resample()
        if self.regularise_scale > 0.0:
            # jitter from the cloud the resampling left, pose and drift jointly (include/mcl_regularise.h)
            dims = 6 if self.estimate_drift else 3
            self.particles.regularise(self.regularise_scale, self.regularise_shrink, self.estimate_drift,
                                      self._replay.randn(self.pc, dims) if self._replay is not None else None)
            self.regularise_calls += 1
            self.regularise_hs.append(_engine.regularise_bandwidth(self.pc, dims, self.regularise_scale,
                                                                   self.regularise_shrink)[0])
        if self.fix_history_depth > 0 and (self._fix_last_record is None or self.time > self._fix_last_record):
            # one frame per resampling: what a late fix is evaluated against.  The filter's clock moves with the odometry
            # alone, so a second resampling before the next odometry message (a ping and a fix, a ping and a DVL altitude,
            # two fixes) would record a second frame with the SAME stamp, which mcl_history_bracket refuses.  It is not
            # recorded: the link carries both resamplings into the next frame, and the frame of this stamp stays the cloud
            # its first resampling left.
            self.particles.history_record(self.time)
            self._fix_last_record = self.time

    def reassign_poses(self, lost, dupes):
        """Folded into resample() on the device (auv_pf.py:195-198 semantics)."""
        return None

    # ---- MBES (north_star): map + ping callback
    def set_map_grid(self, z, origin, res):
        with self.lock:
            self.particles.set_map_grid(z, origin, res)
            self.has_map = True

    def set_map_mesh(self, verts, tris):
        with self.lock:
            self.particles.set_map_mesh(verts, tris)
            self.has_map = True

    def load_map(self, path):
        m = load_map_file(path)
        if m[0] == 'grid':
            self.set_map_grid(m[1], m[2], m[3])
        else:
            self.set_map_mesh(m[1], m[2])

    # ---- landmark detections (BASELINE config 5)
    def set_landmarks(self, xyz):
        xyz = np.ascontiguousarray(np.asarray(xyz, np.float64).reshape(-1, 3))
        if xyz.shape[0] == 0:
            raise ValueError('landmark map: no landmarks (all filtered by rocks_depth?)')
        with self.lock:
            self.particles.set_landmarks(xyz)
            self.has_landmarks = True

    def lm_detect_cb(self, lm_msg):
        """geometry_msgs/PoseArray of detections in base_frame (toy_mbes_receptor.cpp:75-105: positions only, stamped
        with the ping's stamp, published after the receptor has processed the ping).  The usual order -- the ping with
        this stamp (or a later one) has already been through mbes_cb --: a measurement update of its own followed by
        the resampling, like a GPS fix.  Ahead of its ping: held until mbes_cb sees the ping with the same stamp, whose
        likelihood it joins (mcl_update_landmarks(accumulate = 1)).  Never applied to another ping's likelihood."""
        det = np.array([[p.position.x, p.position.y, p.position.z] for p in lm_msg.poses], np.float64).reshape(-1, 3)
        if det.shape[0] == 0:
            return
        with self.lock:
            if not (self.old_time and self.has_landmarks):
                return
            stamp = self._stamp_of(lm_msg)
            if self.time - stamp > self.landmark_max_age:
                return
            if self.has_map and (self._last_ping_stamp is None or stamp > self._last_ping_stamp + self.landmark_sync_tol):
                self._pending_det = (stamp, det)
                return
            if self.landmark_late == 'drop' and self.has_map:
                return   # (after its ping, and the node is asked for ONE resampling per ping)
            self.particles.update_landmarks(det, self.landmark_std, k=self.landmark_k, gate=self.landmark_gate,
                                            accumulate=False)
            self.resample(self.particles)

    def _stamp_of(self, msg):
        """header.stamp in seconds; a message without one (hand-made test messages) counts as `now`."""
        stamp = getattr(getattr(msg, 'header', None), 'stamp', None)
        return float(stamp.to_sec()) if stamp is not None else float(self.time)

    def _accumulate_pending_detections(self, ping_stamp):
        """Called under the lock right after an MBES update: detections that arrived ahead of THIS ping onto its
        likelihood; held detections of an earlier ping (which never came) are dropped, of a later one kept."""
        ping_stamp = float(ping_stamp)
        self._last_ping_stamp = ping_stamp
        if self._pending_det is None:
            return
        stamp, det = self._pending_det
        if stamp > ping_stamp + self.landmark_sync_tol:
            return   # (still ahead: its ping is yet to come)
        self._pending_det = None
        if stamp < ping_stamp - self.landmark_sync_tol:
            return   # (its ping never arrived: dropped, never applied to another ping)
        self.particles.update_landmarks(det, self.landmark_std, k=self.landmark_k, gate=self.landmark_gate,
                                        accumulate=True)

    def _information(self, angles, r_max):
        """with mbes_information_every = K > 0: what pings 0, K, 2 K, ... can tell the cloud as it stands before their update"""
        if not self.mbes_information_every > 0:
            return
        k = self._mbes_pings
        self._mbes_pings += 1
        if k % self.mbes_information_every:
            return
        inf = self.particles.ping_information(angles, self.mbes_std, r_max, self.mbes_sensor_offset)
        self.last_information = inf
        self.information_calls += 1
        self.information_log.append((self.time, inf.crlb_strong, inf.crlb_weak, inf.weak_axis, inf.rank_pos, inf.hit_share))
        if self._information_logged is None or self.time - self._information_logged >= self.information_log_period:
            self._information_logged = self.time
            logging.getLogger('auv_pf').info(
                'ping information: one ping fixes %.3g m along its strong axis, %.3g m along its weak axis (%.1f deg), '
                'rank %d, %.0f %% of the rays usable', inf.crlb_strong, inf.crlb_weak, math.degrees(inf.weak_axis),
                inf.rank_pos, 100.0 * inf.hit_share)

    def _match(self, ranges, angles, r_max):
        """with mbes_match_every = K > 0: where pings 0, K, 2 K, ... say the vehicle is, asked after their update from the pose
        the node would publish.  The filter is not told."""
        if not self.mbes_match_every > 0:
            return
        k = self._match_pings
        self._match_pings += 1
        if k % self.mbes_match_every:
            return
        mean, yaw, _ = self.particles.mean_cov()
        start = [float(mean[0]), float(mean[1]), float(mean[2]), float(mean[3]), float(mean[4]), float(yaw)]
        try:
            match, best = self.particles.match_estimate(ranges, angles, self.mbes_std, r_max, self.mbes_sensor_offset, start=start)
        except _engine.MclError as err:
            # a diagnostic that feeds nothing back must not take the callback down after the filter has been updated
            self.match_errors += 1
            logging.getLogger('auv_pf').warning('ping match refused (%s): the filter goes on without it', err)
            return
        i = 0 if best is None else best
        fix = match.pose(i)
        self.last_match = dict(start=start, converged=best is not None, match=match, **fix)
        self.match_calls += 1
        self.match_log.append((self.time, fix['status'], fix['x'], fix['y'], fix['yaw'], fix['rms'], fix['evaluations'],
                               start[0], start[1], start[5]))
        if self._match_logged is None or self.time - self._match_logged >= self.match_log_period:
            self._match_logged = self.time
            logging.getLogger('auv_pf').info(
                'ping match: %s after %d evaluations, %.3f m from the published pose, rms residual %.3g m', fix['status'],
                fix['evaluations'], math.hypot(fix['x'] - start[0], fix['y'] - start[1]), fix['rms'])

    def _swath(self, ranges, angles, r_max):
        """with mbes_swath_pings = K > 0: the ping joins the ring with the odometry pose it was taken at; behind pings 0, E,
        2 E, ... (E = mbes_swath_every), once the ring holds K pings, where those K pings together say the vehicle is at the
        newest of them.  The filter is not told."""
        ring = self._swath_ring
        if ring is None:
            return
        k = self._swath_pings
        self._swath_pings += 1
        if self.odom_latest is None:
            ring.clear()                # no pose to tie the ping to the others with
            return
        if ring and ring[-1][0].size != ranges.size:
            ring.clear()                # another sonar geometry: the pings of a swath share one beam table (the newest ping's)
        po = self.odom_latest.pose.pose
        roll, pitch, yaw = euler_from_quaternion([po.orientation.x, po.orientation.y, po.orientation.z, po.orientation.w])
        ring.append((np.array(ranges, np.float32),
                     (float(po.position.x), float(po.position.y), float(po.position.z), float(roll), float(pitch), float(yaw))))
        if k % self.mbes_swath_every or len(ring) < self.mbes_swath_pings:
            return
        mean, myaw, _ = self.particles.mean_cov()
        start = [float(mean[0]), float(mean[1]), float(mean[2]), float(mean[3]), float(mean[4]), float(myaw)]
        try:
            offsets = _engine.swath_offsets(np.array([r[1] for r in ring], np.float64).T, -1)
            match, best = self.particles.match_swath_estimate(np.stack([r[0] for r in ring]), angles, offsets, self.mbes_std, r_max,
                                                              self.mbes_sensor_offset, start=start)
        except _engine.MclError as err:
            # a diagnostic that feeds nothing back must not take the callback down after the filter has been updated
            self.swath_errors += 1
            logging.getLogger('auv_pf').warning('swath match refused (%s): the filter goes on without it', err)
            return
        i = 0 if best is None else best
        fix = match.pose(i)
        self.last_swath = dict(start=start, converged=best is not None, match=match, offsets=offsets, **fix)
        self.swath_calls += 1
        self.swath_log.append((self.time, fix['status'], fix['x'], fix['y'], fix['yaw'], fix['rms'], fix['evaluations'],
                               start[0], start[1], start[5]))
        if self._swath_logged is None or self.time - self._swath_logged >= self.swath_log_period:
            self._swath_logged = self.time
            logging.getLogger('auv_pf').info(
                'swath match of %d pings: %s after %d evaluations, %.3f m from the published pose, rms residual %.3g m',
                len(ring), fix['status'], fix['evaluations'], math.hypot(fix['x'] - start[0], fix['y'] - start[1]), fix['rms'])

    def _gate(self, ranges, angles, r_max):
        """the ping's ranges as the update takes them: with mbes_gate_nis > 0 the beams the cloud cannot explain set to 0"""
        if not self.mbes_gate_nis > 0.0:
            return ranges
        ranges, verdict = self.particles.gate_ping(ranges, angles, self.mbes_std, r_max, self.mbes_sensor_offset,
                                                   nis_gate=self.mbes_gate_nis)
        self.last_innovation = verdict
        self.gate_calls += 1
        self.gated_beams += int(verdict.n_gated)
        return ranges

    def mbes_pc_cb(self, cloud):
        """One ping as a sensor_msgs/PointCloud2 (or msgs.PointCloud2): every point is a beam's hit.  In the sensor
        frame beam b looks along (0, sin a_b, -cos a_b) (include/mcl.h), so a point gives a_b = atan2(y, -z) and the
        range |p|; points in base_frame (mbes_receptor.cpp:138: the receptor projects the scan into base_frame) are
        taken back through the sensor offset first.  The beams are handed over in ascending angle."""
        pts = _msgs.pointcloud2_xyz(cloud)
        if self.mbes_points_frame != 'sensor':
            o = self.mbes_sensor_offset
            T = _rigid(o[0], o[1], o[2], o[3], o[4], o[5])
            pts = (pts - T[:3, 3]).dot(T[:3, :3])   # R^T (p - t), row-wise
        if pts.shape[0] == 0:
            return
        ang = np.arctan2(pts[:, 1], -pts[:, 2])
        rng = np.sqrt(np.sum(pts * pts, axis=1))
        order = np.argsort(ang, kind='stable')
        with self.lock:
            if not (self.old_time and self.has_map):
                return
            ang32 = ang[order].astype(np.float32)
            rng32 = rng[order].astype(np.float32)
            self._information(ang32, self.mbes_range_max)
            self.particles.update_mbes(self._gate(rng32, ang32, self.mbes_range_max), ang32,
                                       self.mbes_std, self.mbes_range_max, self.mbes_sensor_offset)
            self._accumulate_pending_detections(self._stamp_of(cloud))
            self.resample(self.particles)
            self._match(rng32, ang32, self.mbes_range_max)
            self._swath(rng32, ang32, self.mbes_range_max)

    def mbes_cb(self, scan):
        with self.lock:
            if not (self.old_time and self.has_map):
                return
            n = len(scan.ranges)
            angles = scan.angle_min + scan.angle_increment * np.arange(n)
            ang32 = angles.astype(np.float32)
            rng32 = np.asarray(scan.ranges, dtype=np.float32)
            self._information(ang32, float(scan.range_max))
            self.particles.update_mbes(self._gate(rng32, ang32, float(scan.range_max)),
                                       ang32, self.mbes_std, float(scan.range_max), self.mbes_sensor_offset)
            self._accumulate_pending_detections(self._stamp_of(scan))
            self.resample(self.particles)
            self._match(rng32, ang32, float(scan.range_max))
            self._swath(rng32, ang32, float(scan.range_max))

    # ---- DVL bottom range
    def dvl_cb(self, msg):
        """smarc_msgs/DVL: the altitude as one range along the DVL frame's -z axis against the map, then the resampling.
        An altitude that is not finite and positive (no bottom lock) is ignored."""
        alt = float(msg.altitude)
        if not (math.isfinite(alt) and alt > 0.0):
            return
        with self.lock:
            if not (self.old_time and self.has_map):
                return
            self.particles.update_ranges([alt], [[0.0, 0.0, -1.0]], self.dvl_altitude_std, self.dvl_range_max,
                                         self.dvl_sensor_offset)
            self.resample(self.particles)

    # ---- delayed acoustic position fixes (include/mcl_acoustic.h)
    def _log_zrp(self, odom_msg):
        """Called under the lock with every odometry message, before its predict: z, roll, pitch by stamp, as long as a fix
        may be old; and the particles as they are (at old_time) as a frame of the ring when it holds none yet or when
        nothing has resampled for fix_max_age / fix_history_depth seconds -- frames come with the resamplings, and this
        keeps the ring spanning fix_max_age where they are rare (no map, no pings): a fix taken in such a stretch still
        finds the pose it belongs to."""
        o = odom_msg.pose.pose.orientation
        roll, pitch, _ = euler_from_quaternion([o.x, o.y, o.z, o.w])
        if not self._zrp_log or self.time > self._zrp_log[-1][0]:
            self._zrp_log.append((self.time, float(odom_msg.pose.pose.position.z), roll, pitch))
        while self._zrp_log and self.time - self._zrp_log[0][0] > self.fix_max_age + 1.0:
            self._zrp_log.popleft()
        if self.old_time and (self._fix_last_record is None or
                              self.old_time - self._fix_last_record >= self.fix_max_age / self.fix_history_depth):
            self.particles.history_record(self.old_time)
            self._fix_last_record = self.old_time

    def _zrp_at(self, stamp):
        """z, roll, pitch of the odometry message nearest `stamp` (None without one)"""
        log = self._zrp_log
        if not log:
            return None
        k = bisect.bisect_left(log, (stamp,))     # (the stamps were appended in order)
        if k == len(log) or (k > 0 and stamp - log[k - 1][0] <= log[k][0] - stamp):
            k -= 1
        return [log[k][1], log[k][2], log[k][3]]

    def fix_cb(self, fix_msg):
        """nav_msgs/Odometry: an acoustic position fix, stamped when it was MEASURED.  With `fix_history_depth` > 0 the
        stamp is bracketed among the recorded frames: inside the ring the update runs at that lag, with z, roll, pitch of
        the odometry nearest the stamp; newer than the newest frame: against the cloud as it is; older than the ring or
        than `fix_max_age`: dropped (fixes_dropped).  Depth 0: always against the cloud as it is.  Then the resampling."""
        pos = fix_msg.pose.pose.position
        xy = self._fix_in_map(fix_msg.header.frame_id, float(pos.x), float(pos.y), float(pos.z))
        with self.lock:
            if not self.old_time:
                return
            stamp = self._stamp_of(fix_msg)
            age = self.time - stamp
            if age > self.fix_max_age:
                self.fixes_dropped += 1
                return
            lag, frac, zrp = -1, 0.0, None
            if self.fix_history_depth > 0:
                held, _, stamps = self.particles.history_frames()
                zrp = self._zrp_at(stamp)
                if held > 0 and zrp is not None and stamp <= stamps[0]:
                    lag, frac, where = _engine.history_bracket(stamps, stamp)
                    if where < 0 and stamp < stamps[-1]:
                        self.fixes_dropped += 1
                        return
                else:
                    zrp = None   # (newer than every frame: the cloud as it is, with its own z, roll, pitch)
            self.particles.update_fix(xy, self.fix_std, zrp=zrp, lag=lag, frac=frac)
            self.fixes_applied += 1
            self.fix_lag_sum += age
            self.resample(self.particles)

    def _fix_in_map(self, frame_id, x, y, z):
        if not frame_id or frame_id == self.map_frame:
            return [x, y]
        pt = _msgs.PointStamped()
        pt.header.frame_id = frame_id
        pt.point.x, pt.point.y, pt.point.z = x, y, z
        out = self.transport.transformPoint(self.map_frame, pt)
        return [float(out.point.x), float(out.point.y)]

    # ---- publishing, auv_pf.py:218-285
    def update_loc_pose(self, pose_list=None):
        mean, yaw, cov9 = self.particles.mean_cov()
        if self.estimate_drift:
            self.drift_mean, self.drift_cov = self.particles.drift_mean_cov()
        lp = self.loc_pose
        lp.pose.pose.position.x, lp.pose.pose.position.y, lp.pose.pose.position.z = mean[0], mean[1], mean[2]
        quat_t = quaternion_from_euler(mean[3], mean[4], yaw)
        lp.pose.pose.orientation = _msgs.Quaternion(*quat_t)
        lp.header.stamp = self.transport.now()
        self.cov = np.array(cov9).reshape(3, 3)
        lp.pose.covariance = [0.] * 36
        for i in range(3):
            for j in range(3):
                lp.pose.covariance[i * 3 + j] = float(self.cov[i, j])
        self.transport.publish_odom(lp)
        self.transport.sendTransform([mean[0], mean[1], 0.], quat_t, self.transport.now(), self.base_frame,
                                     self.odom_frame)
        return mean, yaw, cov9

    def loc_loop(self, event=None):
        with self.lock:
            self.poses.data = self.particles.poses()  # (n, 7): position + quaternion_from_euler per particle
            self.poses.header.stamp = self.transport.now()
            mean, yaw, _ = self.update_loc_pose()
            if self.credible_prob > 0.0:
                # how well is that pose known: the radius and heading half-width that hold credible_prob of the cloud
                centre = (float(mean[0]), float(mean[1]), float(yaw))
                c = self.particles.credible((self.credible_prob,), centre)
                self.credible_calls += 1
                self.last_credible = dict(prob=self.credible_prob, radius=c.radius[self.credible_prob],
                                          yaw_halfwidth=c.yaw_halfwidth[self.credible_prob], n_used=c.n_used, centre=centre)
            self.transport.publish_poses(self.poses)
