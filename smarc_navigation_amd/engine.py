"""Thin Python wrapper over the C ABI handle (include/mcl.h).  numpy in / numpy out; all compute
runs in libmcl_hip.so on the GPU."""
import ctypes as C
import dataclasses
import math

import numpy as np

from . import _lib
from ._lib import Config, Odom, Timing, MclError  # noqa: F401

SYSTEMATIC, RESIDUAL, STRATIFIED, MULTINOMIAL, NAIVE = 0, 1, 2, 3, 4
RNG_NATIVE, RNG_REPLAY = 0, 1
WEIGHT_LINEAR_FLOOR, WEIGHT_LOG_SHIFT, WEIGHT_LINEAR = 0, 1, 2
FRAME_ODOM, FRAME_MAP = 0, 1


def _ptr(a):
    return None if a is None else a.ctypes.data


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


class WeightStats(object):
    """mcl_wstats as a Python object: n, n_live, argmax_gid, max_lw, sum_w, sum_w2, n_eff, log_mean_lik, map_pose (6)."""
    FIELDS = ('n', 'n_live', 'argmax_gid', 'max_lw', 'sum_w', 'sum_w2', 'n_eff', 'log_mean_lik')

    def __init__(self, c):
        for f in self.FIELDS:
            setattr(self, f, getattr(c, f))
        self.map_pose = np.array(c.map_pose[:], dtype=np.float64)

    def as_c(self):
        c = _lib.WStats()
        for f in self.FIELDS:
            setattr(c, f, getattr(self, f))
        c.map_pose[:] = [float(x) for x in self.map_pose]
        return c

    def as_dict(self):
        d = {f: getattr(self, f) for f in self.FIELDS}
        d['map_pose'] = self.map_pose.tolist()
        return d

    def __repr__(self):
        return 'WeightStats(%r)' % (self.as_dict(),)


class PoseMode(object):
    """mcl_mode as a Python object: count, score, ix, iy, iyaw, mean (6: x, y, z, roll, pitch, circular-mean yaw),
    cov_xy (xx, xy, yy), yaw_R"""

    def __init__(self, c):
        self.count, self.score = int(c.count), int(c.score)
        self.ix, self.iy, self.iyaw = int(c.ix), int(c.iy), int(c.iyaw)
        self.mean = np.array(c.mean6[:], dtype=np.float64)
        self.cov_xy = np.array(c.cov_xy[:], dtype=np.float64)
        self.yaw_R = float(c.yaw_R)

    def as_dict(self):
        return dict(count=self.count, score=self.score, ix=self.ix, iy=self.iy, iyaw=self.iyaw, mean=self.mean.tolist(),
                    cov_xy=self.cov_xy.tolist(), yaw_R=self.yaw_R)

    def __repr__(self):
        return 'PoseMode(%r)' % (self.as_dict(),)


@dataclasses.dataclass
class HistoryEstimate(object):
    """mcl_history_est as a Python object: the smoothed estimate of one recorded frame (include/mcl_history.h)"""
    lag: int
    stamp: float
    n_unique: int
    x: float
    y: float
    yaw: float
    yaw_R: float
    cov_xy: np.ndarray   # xx, xy, yy

    def as_dict(self):
        d = dataclasses.asdict(self)
        d['cov_xy'] = [float(v) for v in self.cov_xy]
        return d


@dataclasses.dataclass
class TemperResult(object):
    """mcl_temper_result as a Python object (include/mcl_temper.h): the level j of the exponent lattice, beta = 2^(-j / 64),
    the target count, whether not even the floor reached it, finite log-weights, their maximum, candidates evaluated"""
    j: int
    beta: float
    n_target: int
    floor_hit: bool
    n_live: int
    max_lw: float
    levels_evaluated: int

    @staticmethod
    def from_c(c):
        return TemperResult(int(c.j), float(c.beta), int(c.n_target), bool(c.floor_hit), int(c.n_live), float(c.max_lw),
                            int(c.levels_evaluated))

    def as_dict(self):
        return dataclasses.asdict(self)


def temper_target(ess_ratio, n_global):
    """n_target of an effective-sample-size ratio: ceil(ratio n_global), at least 1"""
    return max(1, int(math.ceil(float(ess_ratio) * int(n_global))))


Q_X, Q_Y, Q_YAW_DEV, Q_ABS_YAW_DEV, Q_RADIUS2 = 0, 1, 2, 3, 4
_QUANTITIES = {'x': Q_X, 'y': Q_Y, 'yaw_dev': Q_YAW_DEV, 'abs_yaw_dev': Q_ABS_YAW_DEV, 'radius2': Q_RADIUS2}


@dataclasses.dataclass
class Quantile(object):
    """mcl_quantile_result as a Python object (include/mcl_quantile.h): the value (NaN: no mass), its key, the mass M(key)
    at or below it, the total mass S and the particles whose value is not NaN -- Python integers"""
    value: float
    key: int
    mass: int
    total: int
    n_used: int

    @staticmethod
    def from_c(c):
        return Quantile(float(c.value), int(c.key), int(c.mass), int(c.total), int(c.n_used))


@dataclasses.dataclass
class Credible(object):
    """what Engine.credible returns: the component-wise median pose (x, y, yaw), the radius that holds a share p of the
    posterior about `centre` (radius[p], metres) and the heading bound (yaw_halfwidth[p], radians), the particles used"""
    median: tuple
    radius: dict
    yaw_halfwidth: dict
    n_used: int
    centre: tuple


INNOVATION_BEAM = np.dtype(_lib.INNOVATION_BEAM_FIELDS)
INNOVATION_DERIVED = np.dtype(_lib.INNOVATION_DERIVED_FIELDS)
INNOVATION_QUANTUM = 2.0 ** -12          # metres per unit of the quantised residual
INNOVATION_DEFAULT_SAMPLES = 4096


def innovation_derived(beams, sigma):
    """the Python mirror of the derived quantities of include/mcl_innovation.h, in Python integers and one rounding per IEEE
    operation: (nu, var, nis, support) as float64 arrays over the records `beams` (zeros where n = 0)"""
    b = np.asarray(beams, dtype=INNOVATION_BEAM).reshape(-1)
    out = np.zeros((4, b.size))
    s2g = float(sigma) * float(sigma)
    nf = b['n'].astype(np.float64)
    if b.size and np.all(b['n'] >= 0) and float(np.max(nf * b['s2'].astype(np.float64))) < 2.0 ** 62:
        # every numerator fits 64 bits (the usual case: residuals of metres, thousands of samples): the same roundings in numpy
        live = b['n'] > 0
        n, s1 = b['n'][live], b['s1'][live]
        num = n * b['s2'][live].astype(np.int64) - s1 * s1
        nl = nf[live]
        nu = s1.astype(np.float64) / (nl * 4096.0)
        var = num.astype(np.float64) / (nl * nl) * (1.0 / 16777216.0)
        out[0, live], out[1, live] = nu, var
        out[2, live], out[3, live] = (nu * nu) / (var + s2g), b['n_within'][live].astype(np.float64) / nl
        return out[0], out[1], out[2], out[3]
    for k in range(b.size):
        n, s1, s2, nw = int(b['n'][k]), int(b['s1'][k]), int(b['s2'][k]), int(b['n_within'][k])
        if n <= 0:
            continue
        nf = float(n)
        nu = float(s1) / (nf * 4096.0)
        var = float(n * s2 - s1 * s1) / (nf * nf) * (1.0 / 16777216.0)
        out[:, k] = (nu, var, (nu * nu) / (var + s2g), float(nw) / nf)
    return out[0], out[1], out[2], out[3]


class PingInnovation(object):
    """what Engine.ping_innovation returns: the integer records of include/mcl_innovation.h (`beams`, a record array with the
    fields n, n_miss, n_within, s1, s2, one per beam), the sampled particles (n_sampled), the sigma they are held against,
    the derived nu (m), var (m^2), nis and support per beam (zeros where n = 0), and with dump=True `expected`, the
    (n_sampled, B) expected ranges (entries of invalid beams are NaN)"""

    def __init__(self, beams, n_sampled, sigma, expected=None):
        self.beams = beams
        self.n_sampled = int(n_sampled)
        self.sigma = float(sigma)
        self.expected = expected
        self.nu, self.var, self.nis, self.support = innovation_derived(beams, sigma)

    n = property(lambda self: self.beams['n'])
    n_miss = property(lambda self: self.beams['n_miss'])
    n_within = property(lambda self: self.beams['n_within'])
    s1 = property(lambda self: self.beams['s1'])
    s2 = property(lambda self: self.beams['s2'])

    @property
    def valid(self):
        return self.beams['n'] > 0

    def mean_nis(self):
        """mean NIS per valid beam (about 1 on a consistent run; NaN without a valid beam)"""
        v = self.valid
        return float(self.nis[v].sum() / v.sum()) if v.any() else math.nan


@dataclasses.dataclass
class GateVerdict(object):
    """mcl_innovation_verdict and the per-beam output of mcl_innovation_gate as a Python object: mask (bool per beam: gate
    it), n_gated, inconsistent, n_valid, n_candidates, nis_sum (its degrees of freedom: n_valid), mean_nu, and the derived
    nu, var, nis, support per beam as the library computed them"""
    mask: np.ndarray
    n_gated: int
    inconsistent: bool
    n_valid: int
    n_candidates: int
    nis_sum: float
    mean_nu: float
    nu: np.ndarray
    var: np.ndarray
    nis: np.ndarray
    support: np.ndarray

    def mean_nis(self):
        return self.nis_sum / self.n_valid if self.n_valid else math.nan


INFORMATION_SUMS = np.dtype(_lib.INFORMATION_SUMS_FIELDS)
INFORMATION_RESULT = np.dtype(_lib.INFORMATION_RESULT_FIELDS)
INFORMATION_DEFAULT_SAMPLES = 4096
INFORMATION_MAX_JUMP = 2048.0


def make_information_steps(r_max, delta_xy=0.5, delta_yaw=0.01, jump_max=None):
    """mcl_information_steps; jump_max=None: min(r_max, 2048).  The defaults are policy, not tolerances."""
    s = _lib.InformationSteps()
    s.delta_xy, s.delta_yaw = float(delta_xy), float(delta_yaw)
    s.jump_max = min(float(r_max), INFORMATION_MAX_JUMP) if jump_max is None else float(jump_max)
    return s


def _matrix3(J):
    """the packed xx, xy, xw, yy, yw, ww as the symmetric 3 x 3 (the last axis of J holds the six)"""
    J = np.asarray(J, np.float64)
    return np.stack([J[..., [0, 1, 2]], J[..., [1, 3, 4]], J[..., [2, 4, 5]]], axis=-2)


class PingInformation(object):
    """what Engine.ping_information returns: the integer records of include/mcl_information.h per beam (`beams`, a record
    array with the fields n, n_miss, n_jump, sxx, syy, sww, sxy, sxw, syw), the sampled particles (n_sampled), and the
    quantities mcl_information_matrix derives from them: `matrix` (3 x 3 over x, y, yaw: the sample mean of the ping's
    Fisher information), lambda_max / lambda_min of the position information with yaw marginalised, crlb_strong and
    crlb_weak (metres; inf where the ping fixes nothing), weak_axis (radians in [0, pi), state coordinates), rank_pos and
    hit_share.  With dump=True `ranges` holds the six ranges of every pair, shaped (n_sampled, 6, B)."""

    def __init__(self, beams, n_sampled, sigma, delta_xy, delta_yaw, ranges=None):
        self.beams = beams
        self.n_sampled = int(n_sampled)
        self.sigma, self.delta_xy, self.delta_yaw = float(sigma), float(delta_xy), float(delta_yaw)
        self.ranges = ranges
        r = information_matrix(beams, sigma, delta_xy, delta_yaw)
        self.result = r
        self.J = r['J'].copy()
        self.matrix = _matrix3(self.J)
        self.lambda_max, self.lambda_min = float(r['lambda_max']), float(r['lambda_min'])
        self.crlb_strong, self.crlb_weak = float(r['crlb_strong']), float(r['crlb_weak'])
        self.weak_axis, self.rank_pos, self.hit_share = float(r['weak_axis']), int(r['rank_pos']), float(r['hit_share'])

    def as_dict(self):
        return dict(n_sampled=self.n_sampled, crlb_strong=self.crlb_strong, crlb_weak=self.crlb_weak,
                    weak_axis=self.weak_axis, rank_pos=self.rank_pos, hit_share=self.hit_share)


class PoseInformation(object):
    """what Engine.pose_information returns: one integer record per pose (`poses`, fields as PingInformation.beams) and
    arrays of the derived quantities, one entry per pose: J (M x 6, packed xx, xy, xw, yy, yw, ww), matrix (M x 3 x 3),
    lambda_max, lambda_min, crlb_strong, crlb_weak, weak_axis, rank_pos, hit_share"""

    def __init__(self, records, sigma, delta_xy, delta_yaw):
        self.poses = records
        self.sigma, self.delta_xy, self.delta_yaw = float(sigma), float(delta_xy), float(delta_yaw)
        r = information_matrix(records, sigma, delta_xy, delta_yaw, per_pose=True)
        self.result = r
        self.J = r['J'].copy()
        self.matrix = _matrix3(self.J)
        for f in ('lambda_max', 'lambda_min', 'crlb_strong', 'crlb_weak', 'weak_axis', 'rank_pos', 'hit_share'):
            setattr(self, f, r[f].copy())


MATCH_SUMS = np.dtype(_lib.MATCH_SUMS_FIELDS)
MATCH_RESULT = np.dtype(_lib.MATCH_RESULT_FIELDS)
MATCH_TRACE = np.dtype(_lib.MATCH_TRACE_FIELDS)
MATCH_DERIVED = np.dtype(_lib.MATCH_DERIVED_FIELDS)
MATCH_CONVERGED, MATCH_MAX_ITER, MATCH_STALLED, MATCH_NO_OVERLAP = 0, 1, 2, 3
MATCH_STATUS_NAMES = ('CONVERGED', 'MAX_ITER', 'STALLED', 'NO_OVERLAP')
MATCH_MAX_DUMP = 1 << 26
SwathOffset = np.dtype(_lib.SWATH_OFFSET_FIELDS)
SWATH_MAX_PINGS, SWATH_MAX_BEAMS = 64, 16384
ReseedComponent = np.dtype(_lib.RESEED_COMPONENT_FIELDS)
RESEED_MAX_COMPONENTS = 256
RESEED_MAX_STARTS = 65536          # MCL_MATCH_MAX_POSES: what one match call takes


def make_match_config(r_max, fit_z=False, max_iter=12, min_beams=8, grad_floor_q=2, step_max_xy=2.0, step_max_yaw=0.1,
                      tol_xy=1e-3, tol_yaw=1e-4, delta_xy=0.5, delta_yaw=0.01, jump_max=None):
    """mcl_match_config (include/mcl_match.h); the steps as make_information_steps.  The defaults are policy."""
    c = _lib.MatchConfig()
    c.dims, c.max_iter, c.min_beams, c.grad_floor_q = (4 if fit_z else 3), int(max_iter), int(min_beams), int(grad_floor_q)
    c.step_max_xy, c.step_max_yaw, c.tol_xy, c.tol_yaw = float(step_max_xy), float(step_max_yaw), float(tol_xy), float(tol_yaw)
    c.steps = make_information_steps(r_max, delta_xy, delta_yaw, jump_max)
    return c


class PingMatch(object):
    """what Engine.match_ping returns: `results` (a record array of MATCH_RESULT, one per start pose: x, y, yaw, z, status,
    evaluations, accepted, j, dead, start, final), per pose the contributing beams m and -- the arithmetic of
    mcl_match_derived, operation by operation -- rms, mean (metres), chi2 (per contributing beam) of the final record and
    start_rms of the start's, the config, and with trace=True `trace` (M x (max_iter + 1) records of MATCH_TRACE), with
    dump=True `ranges` (M x (max_iter + 1) x (1 + 2 D) x B, NaN where nothing was cast)."""

    def __init__(self, results, cfg, sigma, trace=None, ranges=None, derive=None):
        self.results, self.cfg, self.sigma, self.trace, self.ranges = results, cfg, float(sigma), trace, ranges
        self._derive = derive if derive is not None else match_derived   # (Engine.match_swath: swath_derived)
        self.status = results['status'].copy()
        self.m, self.rms, self.mean = self._residuals(results['final'])
        self.start_rms = self._residuals(results['start'])[1]
        z = self.rms / self.sigma
        self.chi2 = z * z

    @staticmethod
    def _residuals(rec):
        m = rec['n'] - rec['n_miss'] - rec['n_jump']
        some = m > 0
        mf = np.where(some, m, 1).astype(np.float64)
        rms = np.where(some, np.sqrt(rec['s_rho2'].astype(np.float64) / mf) / 4096.0, 0.0)
        return m, rms, np.where(some, (rec['s_rho'].astype(np.float64) / mf) / 4096.0, 0.0)

    def __len__(self):
        return self.results.size

    def best(self):
        """the index of the CONVERGED pose with the lowest rms residual, or None"""
        ok = np.flatnonzero(self.status == MATCH_CONVERGED)
        return int(ok[np.argmin(self.rms[ok])]) if ok.size else None

    def pose(self, i):
        r = self.results[i]
        return dict(x=float(r['x']), y=float(r['y']), yaw=float(r['yaw']), z=float(r['z']),
                    status=MATCH_STATUS_NAMES[int(r['status'])], rms=float(self.rms[i]), evaluations=int(r['evaluations']))

    def derived(self, i):
        """mcl_match_derived (a swath's fix: mcl_swath_derived) of fix i's final record"""
        return self._derive(self.results['final'][i], self.cfg, self.sigma)

    def cov(self, i):
        """the covariance of fix i over (x, y, yaw[, z]): sigma^2 A^-1, D x D; inf on the diagonal of a dead dimension"""
        return self._symmetric(self.derived(i)['cov'])

    def information(self, i):
        """J = A / sigma^2 of fix i, without damping, D x D"""
        return self._symmetric(self.derived(i)['J'])

    def _symmetric(self, packed):
        """the packed lower triangle over (x, y, yaw, z) as the full symmetric D x D matrix"""
        low = _unpack_lower(packed, 4)
        return (low + np.tril(low, -1).T)[:self.cfg.dims, :self.cfg.dims]


def make_gate_config(nis_gate=10.83, min_support=0.01, max_gated_fraction=0.25):
    c = _lib.InnovationGateConfig()
    c.nis_gate, c.min_support, c.max_gated_fraction = float(nis_gate), float(min_support), float(max_gated_fraction)
    return c


def make_quantile_query(quantity, centre=None, weighted=False):
    q = _lib.QuantileQuery()
    q.quantity = int(_QUANTITIES.get(quantity, quantity)) if isinstance(quantity, str) else int(quantity)
    if isinstance(quantity, str) and quantity not in _QUANTITIES:
        raise ValueError('quantity: one of %s' % ', '.join(sorted(_QUANTITIES)))
    q.weighted = 1 if weighted else 0
    c = (0.0, 0.0, 0.0) if centre is None else tuple(float(v) for v in centre)
    if len(c) != 3:
        raise ValueError('centre: (x, y, yaw)')
    q.centre[:] = c
    return q


def make_mode_grid(x0, y0, cell, nx, ny, n_yaw):
    g = _lib.ModeGrid()
    g.x0, g.y0, g.cell = float(x0), float(y0), float(cell)
    g.nx, g.ny, g.n_yaw, g.reserved = int(nx), int(ny), int(n_yaw), 0
    return g


def make_box(xy, yaw=(-math.pi, math.pi), frame='map'):
    """mcl_box from (x_min, x_max, y_min, y_max), a yaw interval and 'map' / 'odom' (or FRAME_MAP / FRAME_ODOM)"""
    b = _lib.Box()
    b.x_min, b.x_max, b.y_min, b.y_max = [float(v) for v in xy]
    b.yaw_min, b.yaw_max = float(yaw[0]), float(yaw[1])
    b.frame = {'odom': FRAME_ODOM, 'map': FRAME_MAP}.get(frame, frame)
    return b


def make_odom(v, wz, q, z, stamp=0.0):
    o = Odom()
    o.stamp = float(stamp)
    o.v[:] = [float(x) for x in v]
    o.w_z = float(wz)
    o.q[:] = [float(x) for x in q]
    o.z = float(z)
    return o


class Engine(object):
    """One shard of the particle filter on one GPU."""

    def __init__(self, n_particles, init_cov=(0,) * 6, process_cov=(0,) * 6, resample_cov=(0,) * 6,
                 meas_std=1.0, m2o=None, seed=0, rng_mode=RNG_NATIVE, resample_scheme=SYSTEMATIC,
                 device=0, rank=0, world=1, n_global=0, global_offset=0):
        self.lib = _lib.load()
        cfg = Config()
        cfg.n_particles = int(n_particles)
        cfg.n_global = int(n_global)
        cfg.global_offset = int(global_offset)
        cfg.device, cfg.rank, cfg.world = int(device), int(rank), int(world)
        cfg.resample_scheme, cfg.rng_mode, cfg.comm_mode = int(resample_scheme), int(rng_mode), 0
        cfg.seed = int(seed)
        cfg.init_cov[:] = [float(x) for x in init_cov]
        cfg.process_cov[:] = [float(x) for x in process_cov]
        cfg.resample_cov[:] = [float(x) for x in resample_cov]
        cfg.meas_std = float(meas_std)
        m = np.identity(4) if m2o is None else np.asarray(m2o, dtype=np.float64)
        cfg.m2o[:] = [float(x) for x in m.reshape(-1)]
        self.m2o = m.reshape(4, 4).copy()
        self.n = int(n_particles)
        self.n_global = int(n_global) if n_global else self.n
        self.h = C.c_void_p()
        _lib.check(self.lib.mcl_create(C.byref(cfg), C.byref(self.h)))

    def close(self):
        if getattr(self, 'h', None) is not None and self.h.value:
            self.lib.mcl_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st):
        _lib.check(st, self.h)

    # ---- particle lifecycle
    def init_particles(self, normals=None):
        nz = _f64(normals)
        self._ck(self.lib.mcl_init_particles(self.h, _ptr(nz)))

    # ---- global localisation and kidnap recovery (include/mcl_recovery.h)
    def map_bounds(self):
        """(x_min, x_max, y_min, y_max) of the map set by set_map_grid / set_map_mesh, map frame"""
        b = np.zeros(4)
        self._ck(self.lib.mcl_map_bounds(self.h, _ptr(b)))
        return tuple(float(v) for v in b)

    def _box(self, box, frame, yaw):
        if isinstance(box, _lib.Box):
            return box
        if box is None:   # the map's footprint: map-frame numbers whatever `frame` says
            return make_box(self.map_bounds(), yaw, 'map')
        return make_box(box, yaw, frame)

    def init_particles_uniform(self, box=None, frame='map', yaw=(-math.pi, math.pi), uniforms=None):
        """x, y, yaw uniform in the box (x_min, x_max, y_min, y_max) x yaw; box=None: the map's footprint.
        uniforms: n x 3 in [0, 1) (REPLAY mode)."""
        b, u = self._box(box, frame, yaw), _f64(uniforms)
        self._ck(self.lib.mcl_init_particles_uniform(self.h, C.byref(b), _ptr(u)))

    def weight_stats(self):
        """statistics of the log-weights the last update left (before they are resampled away): a WeightStats"""
        c = _lib.WStats()
        self._ck(self.lib.mcl_weight_stats(self.h, C.byref(c)))
        return WeightStats(c)

    def inject_uniform(self, fraction, box=None, frame='map', yaw=(-math.pi, math.pi), uniforms=None, count=True):
        """replace the particles whose selection draw is < fraction by uniform draws from the box (box=None: the map's
        footprint); returns the number replaced, or None with count=False (the call then does not wait for the GPU).
        uniforms: n x 4 in [0, 1) (REPLAY mode)."""
        b, u = self._box(box, frame, yaw), _f64(uniforms)
        k = C.c_int64(0)
        self._ck(self.lib.mcl_inject_uniform(self.h, float(fraction), C.byref(b), _ptr(u), C.byref(k) if count else None))
        return int(k.value) if count else None

    # ---- sensor resetting (include/mcl_reseed.h)
    def inject_gaussian(self, fraction, components, normals=None, count=True):
        """replace the particles whose selection draw is < fraction by draws from the mixture `components` (records of
        ReseedComponent: mean (x, y, yaw), the packed factor of the covariance, an integer mass; reseed_select makes
        them from a match); returns the number replaced, or None with count=False (the call then does not wait for the
        GPU).  normals: n x 5 (u_select, u_comp, xi_0, xi_1, xi_2; REPLAY mode)."""
        comps = np.ascontiguousarray(components, dtype=ReseedComponent).reshape(-1)
        u = _f64(normals)
        k = C.c_int64(0)
        self._ck(self.lib.mcl_inject_gaussian(self.h, float(fraction), _ptr(comps), comps.size, _ptr(u),
                                              C.byref(k) if count else None))
        return int(k.value) if count else None

    def reseed_starts(self, box=None, pitch=4.0, yaw=(-math.pi, math.pi), n_yaw=8, z=0.0, roll=0.0, pitch_angle=0.0):
        """reseed_starts over `box` (ODOM frame), or with box=None over the map's footprint carried into the odom frame"""
        if box is None:
            return reseed_starts(None, pitch, yaw, n_yaw, z, roll, pitch_angle, bounds=self.map_bounds(), m2o=self.m2o)
        return reseed_starts(box, pitch, yaw, n_yaw, z, roll, pitch_angle)

    # ---- dominant modes of the cloud (include/mcl_modes.h)
    def mode_grid(self, cell, n_yaw=36, box=None):
        """the lattice of pose_modes: box = (x_min, x_max, y_min, y_max) in the ODOM frame, or None: the bounding box of the
        map footprint's four corners carried through the inverse of m2o (the rule of mcl_recovery.h; m2o must turn about z
        alone); nx = ceil(extent / cell)"""
        cell = float(cell)
        if box is None:
            m = self.m2o
            if (abs(m[0, 2]) > 1e-12 or abs(m[1, 2]) > 1e-12 or abs(m[2, 0]) > 1e-12 or abs(m[2, 1]) > 1e-12 or
                    abs(m[2, 2] - 1.0) > 1e-12):
                raise MclError(-4, 'pose_modes: the map footprint needs an m2o that turns about z alone')
            x_min, x_max, y_min, y_max = self.map_bounds()
            xs, ys = [], []
            for x, y in ((x_min, y_min), (x_min, y_max), (x_max, y_min), (x_max, y_max)):
                dx, dy = x - m[0, 3], y - m[1, 3]
                xs.append(m[0, 0] * dx + m[1, 0] * dy)
                ys.append(m[0, 1] * dx + m[1, 1] * dy)
            box = (min(xs), max(xs), min(ys), max(ys))
        x_min, x_max, y_min, y_max = [float(v) for v in box]
        if not (cell > 0.0 and np.isfinite(cell) and x_max >= x_min and y_max >= y_min):
            raise MclError(-1, 'pose_modes: bad cell or box')
        nx = max(1, int(math.ceil((x_max - x_min) / cell)))
        ny = max(1, int(math.ceil((y_max - y_min) / cell)))
        return make_mode_grid(x_min, y_min, cell, nx, ny, n_yaw)

    def pose_modes(self, cell, n_yaw=36, k=4, box=None, grid=None):
        """the up to k densest places of the cloud on a lattice of `cell` metres and n_yaw yaw bins (mcl_pose_modes):
        returns (list of PoseMode, densest first; n_outside).  grid: a ModeGrid instead of cell / n_yaw / box."""
        g = grid if grid is not None else self.mode_grid(cell, n_yaw, box)
        k = int(k)
        out = (_lib.Mode * max(k, 1))()
        nm, no = C.c_int32(0), C.c_int64(0)
        self._ck(self.lib.mcl_pose_modes(self.h, C.byref(g), k, out, C.byref(nm), C.byref(no)))
        return [PoseMode(out[j]) for j in range(nm.value)], int(no.value)

    # ---- KLD-sampling across handles (include/mcl_kld.h)
    def kld_grid(self, cell, n_yaw=36, box=None):
        """the lattice of kld_bins: the box rule of mode_grid; the limits are those of kld_grid_check (2^27 cells)"""
        return self.mode_grid(cell, n_yaw, box)

    def kld_bins(self, cell=None, n_yaw=36, box=None, grid=None):
        """(k, n_outside): the number of cells of a lattice of `cell` metres and n_yaw yaw bins that hold at least one
        particle, and the particles that belong to no cell (mcl_kld_bins).  box, grid: as in pose_modes."""
        g = grid if grid is not None else self.kld_grid(cell, n_yaw, box)
        k, ni, no = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._ck(self.lib.mcl_kld_bins(self.h, C.byref(g), C.byref(k), C.byref(ni), C.byref(no)))
        return int(k.value), int(no.value)

    def resample_into(self, dst, uniform=None):
        """dst's particles := dst.n systematic draws from this handle's weighted cloud, without noise (mcl_resample_into);
        this handle is left as it was.  uniform: one number in [0, 1), or None: dst's own Philox draw."""
        u = None if uniform is None else _f64(np.atleast_1d(uniform))
        _lib.check(self.lib.mcl_resample_into(self.h, dst.h, _ptr(u)), dst.h)

    def transfer_indices(self):
        """the ancestors (slots of the source) of the last resample_into with this handle as dst"""
        idx = np.zeros(self.n, np.int32)
        self._ck(self.lib.mcl_transfer_last_indices(self.h, _ptr(idx)))
        return idx

    # ---- exact order statistics of the cloud (include/mcl_quantile.h)
    def cloud_quantiles(self, quantity, probs, centre=None, weighted=False):
        """the quantiles of a quantity ('x', 'y', 'yaw_dev', 'abs_yaw_dev', 'radius2', or MCL_Q_*) about centre =
        (x, y, yaw) (odom frame; None: zeros) at up to eight probabilities in [2^-32, 1], all found in the same passes
        (mcl_cloud_quantiles): a list of Quantile, one per probability.  weighted: by the pending log-weights."""
        q = make_quantile_query(quantity, centre, weighted)
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        out = (_lib.QuantileResult * max(p.size, 1))()
        self._ck(self.lib.mcl_cloud_quantiles(self.h, C.byref(q), _ptr(p), p.size, out))
        return [Quantile.from_c(out[k]) for k in range(p.size)]

    def cloud_mass(self, quantity, values, centre=None, weighted=False, max_lw=None):
        """the inverse question (mcl_cloud_mass): dict(mass = M(key(v)) per value, total = S, n_used, fraction = mass / total
        per value (NaN: no mass)) of THIS shard; integers are Python integers.  weighted: max_lw is the cloud's largest finite
        log-weight (None: this handle's own, from weight_stats)."""
        q = make_quantile_query(quantity, centre, weighted)
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        if weighted and max_lw is None:
            ws = self.weight_stats()
            max_lw = ws.max_lw if ws.argmax_gid >= 0 else -math.inf
        mass, total, used = np.zeros(max(v.size, 1), np.uint64), C.c_uint64(0), C.c_int64(0)
        self._ck(self.lib.mcl_cloud_mass(self.h, C.byref(q), float(max_lw) if weighted else 0.0, _ptr(v), v.size, _ptr(mass),
                                         C.byref(total), C.byref(used)))
        m, t = [int(x) for x in mass[:v.size]], int(total.value)
        return dict(mass=m, total=t, n_used=int(used.value), fraction=[x / t if t else math.nan for x in m])

    def cloud_key_hist(self, quantity, prefix, prefix_bits, centre=None, weighted=False, max_lw=0.0):
        """this shard's masses by the next 8 key bits among the keys whose leading prefix_bits bits equal prefix
        (mcl_cloud_key_hist): 256 Python integers"""
        q = make_quantile_query(quantity, centre, weighted)
        hist = np.zeros(256, np.uint64)
        self._ck(self.lib.mcl_cloud_key_hist(self.h, C.byref(q), float(max_lw), int(prefix), int(prefix_bits), _ptr(hist)))
        return [int(x) for x in hist]

    def credible(self, probs=(0.5, 0.95), centre='mean', weighted=False):
        """a Credible: about centre = 'mean' (mean_cov's x, y, yaw), 'median' (the component-wise median, x and y first) or
        (x, y, yaw), the radius that holds each share p of the posterior (the correctly rounded square root of the exact
        quantile of the squared distance) and the half-width of the heading interval that does, and the median pose."""
        probs = tuple(float(p) for p in probs)
        if isinstance(centre, str):
            if centre == 'mean':
                mean, yaw, _ = self.mean_cov()
                c = (float(mean[0]), float(mean[1]), float(yaw))
            elif centre == 'median':
                mx = self.cloud_quantiles(Q_X, [0.5], None, weighted)[0].value
                my = self.cloud_quantiles(Q_Y, [0.5], None, weighted)[0].value
                # (a lower median is a particle's own yaw: a centre inside the cloud wherever the cut at +-pi falls)
                c = (mx, my, self.cloud_quantiles(Q_YAW_DEV, [0.5], None, weighted)[0].value)
            else:
                raise ValueError("credible: centre is 'mean', 'median' or (x, y, yaw)")
            med_xy = (mx, my) if centre == 'median' else None
        else:
            c, med_xy = tuple(float(v) for v in centre), None
        if med_xy is None:
            med_xy = (self.cloud_quantiles(Q_X, [0.5], c, weighted)[0].value,
                      self.cloud_quantiles(Q_Y, [0.5], c, weighted)[0].value)
        dyaw = self.cloud_quantiles(Q_YAW_DEV, [0.5], c, weighted)[0].value
        r2 = self.cloud_quantiles(Q_RADIUS2, probs, c, weighted)
        ay = self.cloud_quantiles(Q_ABS_YAW_DEV, probs, c, weighted)
        return Credible(median=(med_xy[0], med_xy[1], c[2] + dyaw),
                        radius={p: math.sqrt(r.value) for p, r in zip(probs, r2)},
                        yaw_halfwidth={p: r.value for p, r in zip(probs, ay)}, n_used=r2[0].n_used, centre=c)

    # ---- particle genealogy and the fixed-lag smoother (include/mcl_history.h)
    def history_bytes(self, depth):
        """device bytes history_enable(depth) allocates on this handle (mcl_history_bytes: host arithmetic)"""
        b = C.c_int64(0)
        self._ck(self.lib.mcl_history_bytes(self.n, int(depth), C.byref(b)))
        return int(b.value)

    def history_enable(self, depth):
        """keep the ancestor link of every resample and a ring of `depth` recorded frames"""
        self._ck(self.lib.mcl_history_enable(self.h, int(depth)))

    def history_disable(self):
        self._ck(self.lib.mcl_history_disable(self.h))

    def history_reset(self):
        """forget the frames, link = identity (a clean cut, e.g. after inject_uniform)"""
        self._ck(self.lib.mcl_history_reset(self.h))

    def history_record(self, stamp=0.0):
        """append a frame: the link since the last record and x, y, yaw of every slot as they are now (asynchronous)"""
        self._ck(self.lib.mcl_history_record(self.h, float(stamp)))

    def history_frames(self):
        """(held, recorded, stamps of the held frames, newest first)"""
        held, rec = C.c_int32(0), C.c_int64(0)
        self._ck(self.lib.mcl_history_frames(self.h, C.byref(held), C.byref(rec), None))
        stamps = np.zeros(max(int(held.value), 1))
        self._ck(self.lib.mcl_history_frames(self.h, None, None, _ptr(stamps)))
        return int(held.value), int(rec.value), stamps[:held.value].copy()

    def history_ancestors(self, lag=0):
        """slots[i] = the slot of the frame at `lag` (0: the newest) that current slot i descends from (uint32)"""
        out = np.zeros(self.n, np.uint32)
        self._ck(self.lib.mcl_history_ancestors(self.h, int(lag), _ptr(out)))
        return out

    def history_smooth(self, lags):
        """the smoothed estimates of the frames at lags 0 ... lags - 1: a list of HistoryEstimate"""
        lags = int(lags)
        out = (_lib.HistoryEst * max(lags, 1))()
        self._ck(self.lib.mcl_history_smooth(self.h, lags, out))
        return [HistoryEstimate(k, float(o.stamp), int(o.n_unique), float(o.x), float(o.y), float(o.yaw), float(o.yaw_R),
                                np.array(o.cov_xy[:], dtype=np.float64)) for k, o in enumerate(out[:lags])]

    def history_path(self, slot, lags):
        """(xyyaw (lags, 3), slots (lags,)): the trajectory of current slot `slot` through the frames at lags 0 ... lags - 1
        (a descendant of the best particle of weight_stats() gives the MAP path)"""
        lags = int(lags)
        xyw, sl = np.zeros((max(lags, 1), 3)), np.zeros(max(lags, 1), np.uint32)
        self._ck(self.lib.mcl_history_path(self.h, int(slot), lags, _ptr(xyw), _ptr(sl)))
        return xyw[:lags], sl[:lags]

    # ---- delayed acoustic position fixes and beacon ranges (include/mcl_acoustic.h)
    @staticmethod
    def _cov3(cov):
        """xx, xy, yy from a scalar std, three numbers (xx, xy, yy) or a 2 x 2 matrix"""
        c = np.asarray(cov, dtype=np.float64)
        if c.ndim == 0:
            return np.array([float(c) ** 2, 0.0, float(c) ** 2])
        if c.shape == (3,):
            return np.ascontiguousarray(c)
        if c.shape == (2, 2):
            if c[0, 1] != c[1, 0]:
                raise ValueError('update_fix: the covariance matrix is not symmetric')
            return np.array([c[0, 0], c[0, 1], c[1, 1]])
        raise ValueError('update_fix: cov is a scalar std, (xx, xy, yy) or a 2 x 2 matrix')

    @staticmethod
    def _vec3(a, name):
        if a is None:
            return None
        v = _f64(a).reshape(-1)
        if v.size != 3:
            raise ValueError('%s: three numbers' % name)
        return v

    def update_fix(self, xy, cov, offset=None, zrp=None, lag=-1, frac=0.0, accumulate=False):
        """position fix xy (map frame) with covariance `cov` (a scalar std, xx xy yy, or a 2 x 2 matrix), evaluated at the
        pose each particle's ancestor had in the recorded frame at `lag` (moved `frac` of the way to the frame before it);
        lag=-1: at the particle's pose now.  offset: the transponder in base_link; zrp: z, roll, pitch of the vehicle when
        measured (needed with lag >= 0; None with lag=-1: the particles' own).  mcl_update_fix."""
        p, c = _f64(xy).reshape(-1), self._cov3(cov)
        if p.size != 2:
            raise ValueError('update_fix: xy is two numbers')
        off, z = self._vec3(offset, 'offset'), self._vec3(zrp, 'zrp')
        self._ck(self.lib.mcl_update_fix(self.h, _ptr(p), _ptr(c), _ptr(off), _ptr(z), int(lag), float(frac),
                                         1 if accumulate else 0))

    def update_beacon_ranges(self, beacons, ranges, sigma, offset=None, zrp=None, lag=-1, frac=0.0, accumulate=False):
        """slant ranges to fixed transponders at beacons (n_b x 3, map frame; n_b <= 8); a range <= 0 or NaN is skipped;
        pose, offset, zrp, lag, frac, accumulate as in update_fix.  mcl_update_beacon_ranges."""
        b, r = _f64(beacons).reshape(-1, 3), _f64(ranges).reshape(-1)
        if r.size != b.shape[0]:
            raise ValueError('update_beacon_ranges: %d ranges for %d beacons' % (r.size, b.shape[0]))
        off, z = self._vec3(offset, 'offset'), self._vec3(zrp, 'zrp')
        self._ck(self.lib.mcl_update_beacon_ranges(self.h, _ptr(b), _ptr(r), b.shape[0], float(sigma), _ptr(off), _ptr(z),
                                                   int(lag), float(frac), 1 if accumulate else 0))

    def history_bracket(self, stamp):
        """(lag, frac, where) of `stamp` among the held frames' stamps (mcl_history_bracket over history_frames()): where 0:
        between two frames, +1: not older than the newest, -1: not newer than the oldest.  MclError without a frame."""
        return history_bracket(self.history_frames()[2], stamp)

    # ---- ESS-targeted likelihood tempering (include/mcl_temper.h)
    def temper(self, ess_ratio=0.5, apply=True, n_target=None, wait=True):
        """raise the pending likelihood to the largest power beta = 2^(-j / 64) <= 1 that leaves an effective sample size of
        at least n_target = ceil(ess_ratio n_global) (or n_target itself when given); apply=True scales the log-weights.
        Returns a TemperResult, or None with wait=False (the call then does not wait for the GPU).  mcl_temper."""
        nt = temper_target(ess_ratio, self.n_global) if n_target is None else int(n_target)
        c = _lib.TemperRes()
        self._ck(self.lib.mcl_temper(self.h, nt, 1 if apply else 0, C.byref(c) if wait else None))
        return TemperResult.from_c(c) if wait else None

    def temper_sums(self, max_lw, levels):
        """(S1, S2): this shard's integer sums at the levels (at most 17) relative to the CLOUD's maximum max_lw, as lists of
        Python integers (mcl_temper_sums)"""
        lv = np.ascontiguousarray(levels, dtype=np.int32).reshape(-1)
        s1, s2 = np.zeros(max(lv.size, 1), np.uint64), np.zeros(max(lv.size, 1), np.uint64)
        self._ck(self.lib.mcl_temper_sums(self.h, float(max_lw), _ptr(lv), lv.size, _ptr(s1), _ptr(s2)))
        return [int(v) for v in s1[:lv.size]], [int(v) for v in s2[:lv.size]]

    def temper_apply(self, j):
        """lw <- beta_j lw on this shard (mcl_temper_apply); j = 0 changes nothing"""
        self._ck(self.lib.mcl_temper_apply(self.h, int(j)))

    # ---- per-particle drift states: water current and yaw-rate bias (include/mcl_drift.h)
    def drift_bytes(self):
        """device bytes drift_enable allocates on this handle (mcl_drift_bytes: host arithmetic)"""
        return drift_bytes(self.n)

    def _normals3(self, normals):
        nz = _f64(normals)
        if nz is not None and nz.size != 3 * self.n:
            raise ValueError('drift: normals are n x 3, particle-major')
        return nz

    def drift_enable(self, init_std, walk_std, normals=None):
        """give every particle its own (cx, cy [m/s, odom frame], bw [rad/s]) drawn from N(0, init_std^2), random-walking
        with walk_std per sqrt(second); it follows its particle through every resample.  normals: n x 3 (REPLAY mode)."""
        cfg, nz = make_drift_config(init_std, walk_std), self._normals3(normals)
        self._ck(self.lib.mcl_drift_enable(self.h, C.byref(cfg), _ptr(nz)))

    def drift_reset(self, normals=None):
        """redraw the prior and restart the advance count (after re-initialising the filter)"""
        nz = self._normals3(normals)
        self._ck(self.lib.mcl_drift_reset(self.h, _ptr(nz)))

    def drift_disable(self):
        self._ck(self.lib.mcl_drift_disable(self.h))

    def drift_advance(self, dt, normals=None):
        """x, y += current dt, yaw += bias dt, then the drift's random walk: call it BEFORE the predict (or fused step) of
        the same dt; dt <= 0 does nothing (asynchronous)"""
        nz = self._normals3(normals)
        self._ck(self.lib.mcl_drift_advance(self.h, float(dt), _ptr(nz)))

    def drift_get(self):
        """the drift, (3, n): rows cx, cy, bw"""
        out = np.zeros((3, self.n))
        self._ck(self.lib.mcl_drift_get(self.h, _ptr(out)))
        return out

    def drift_set(self, soa):
        s = _f64(soa)
        if s.shape != (3, self.n):
            raise ValueError('drift_set: a (3, n) array')
        self._ck(self.lib.mcl_drift_set(self.h, _ptr(s)))

    def drift_mean_cov(self):
        """(mean (3,), cov (3, 3)) of (cx, cy, bw) over the slots, every slot counting once: read it after a resample"""
        mean, c = np.zeros(3), np.zeros(6)
        self._ck(self.lib.mcl_drift_mean_cov(self.h, _ptr(mean), _ptr(c)))
        return mean, np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])

    # ---- regularised resampling: jitter from the cloud's own covariance (include/mcl_regularise.h)
    def regularise(self, scale=1.0, shrink=True, with_drift=False, normals=None):
        """call it right after a resample: every particle is jittered with h^2 times the cloud's own covariance of
        (x, y, yaw) -- with_drift: of (x, y, yaw, cx, cy, bw), jointly -- h = scale x the kernel-density bandwidth;
        shrink: towards the mean first, so that mean and covariance stay what they were.  normals: n x 3 or n x 6
        (REPLAY mode).  Asynchronous."""
        cfg = make_regularise_config(scale, shrink, 6 if with_drift else 3)
        nz = _f64(normals)
        if nz is not None and nz.size != cfg.dims * self.n:
            raise ValueError('regularise: normals are n x %d, particle-major' % cfg.dims)
        self._ck(self.lib.mcl_regularise(self.h, C.byref(cfg), _ptr(nz)))

    def regularise_last(self):
        """what the last regularise measured and used: dict(n, dims, dead, h, a, shift (D,), dmean (D,), mean (D,),
        cov (D, D), chol (D, D) lower-triangular)"""
        r = _lib.RegulariseResult()
        self._ck(self.lib.mcl_regularise_last(self.h, C.byref(r)))
        d = int(r.dims)
        shift, dmean = np.array(r.shift[:d]), np.array(r.dmean[:d])
        chol = _unpack_lower(r.chol, d)
        cov = _unpack_lower(r.cov, d)
        cov = cov + np.tril(cov, -1).T
        return dict(n=int(r.n), dims=d, dead=int(r.dead), h=float(r.h), a=float(r.a), shift=shift, dmean=dmean,
                    mean=shift + dmean, cov=cov, chol=chol)

    def predict(self, v, wz, q, z, dt, normals=None, stamp=0.0):
        nz = _f64(normals)
        od = make_odom(v, wz, q, z, stamp)
        self._ck(self.lib.mcl_predict(self.h, C.byref(od), float(dt), _ptr(nz)))

    def update_gps(self, gx, gy):
        self._ck(self.lib.mcl_update_gps(self.h, float(gx), float(gy)))

    def set_map_grid(self, z, origin, res):
        z = _f32(z)
        self._ck(self.lib.mcl_set_map_grid(self.h, _ptr(z), z.shape[0], z.shape[1], float(origin[0]),
                                           float(origin[1]), float(res)))

    def set_map_mesh(self, verts, tris, heightfield=False, general=False, unstructured=False):
        v = _f32(verts)
        t = np.ascontiguousarray(tris, dtype=np.uint32)
        self._ck(self.lib.mcl_set_map_mesh_ex(self.h, _ptr(v), v.shape[0], _ptr(t), t.shape[0],
                                              (1 if heightfield else 0) | (2 if general else 0) |
                                              (4 if unstructured else 0)))

    def update_mbes(self, ranges, beam_angles, sigma, r_max, sensor_offset=None):
        r, a, so = _f32(ranges), _f32(beam_angles), _f64(sensor_offset)
        self._ck(self.lib.mcl_update_mbes(self.h, _ptr(r), _ptr(a), a.size, float(sigma), float(r_max), _ptr(so)))

    def mbes_expected(self, first, count, beam_angles, r_max, sensor_offset=None):
        a, so = _f32(beam_angles), _f64(sensor_offset)
        out = np.zeros((count, a.size), np.float32)
        self._ck(self.lib.mcl_mbes_expected(self.h, int(first), int(count), _ptr(a), a.size, float(r_max),
                                            _ptr(so), _ptr(out)))
        return out

    def update_ranges(self, ranges, dirs, sigma, r_max, sensor_offset=None, accumulate=False):
        """DVL / altimeter ranges: beam b looks along dirs[b] (sensor frame, any length > 0); ranges <= 0 or NaN are
        skipped; accumulate=True adds onto the log-likelihood an earlier update left (mcl_update_ranges)."""
        r, d, so = _f32(ranges).reshape(-1), _f32(dirs).reshape(-1, 3), _f64(sensor_offset)
        if r.size != d.shape[0]:
            raise ValueError('update_ranges: %d ranges for %d directions' % (r.size, d.shape[0]))
        self._ck(self.lib.mcl_update_ranges(self.h, _ptr(r), _ptr(d), d.shape[0], float(sigma), float(r_max), _ptr(so),
                                            1 if accumulate else 0))

    def ranges_expected(self, first, count, dirs, r_max, sensor_offset=None):
        """expected ranges (count, n_beams) of particles [first, first + count) along dirs (mcl_ranges_expected)"""
        d, so = _f32(dirs).reshape(-1, 3), _f64(sensor_offset)
        out = np.zeros((int(count), d.shape[0]), np.float32)
        self._ck(self.lib.mcl_ranges_expected(self.h, int(first), int(count), _ptr(d), d.shape[0], float(r_max), _ptr(so),
                                              _ptr(out)))
        return out

    # ---- ping innovation statistics and the per-beam gate (include/mcl_innovation.h)
    def ping_innovation(self, ranges, beam_angles, sigma, r_max, sensor_offset=None, max_samples=INNOVATION_DEFAULT_SAMPLES,
                        support_k=3.0, dump=False):
        """hold a ping against the cloud as it is (after predict, before the update): per beam the integer sums of the
        quantised residual over a strided sample of at most max_samples particles (mcl_ping_innovation) -- a PingInnovation
        of THIS shard's sampled particles.  Nothing of the filter changes."""
        r, a, so = _f32(ranges).reshape(-1), _f32(beam_angles).reshape(-1), _f64(sensor_offset)
        if r.size != a.size:
            raise ValueError('ping_innovation: %d ranges for %d beam angles' % (r.size, a.size))
        beams = np.zeros(max(a.size, 1), INNOVATION_BEAM)
        exp = None
        if dump:
            stride, _ = innovation_sample(self.n_global, max_samples)
            exp = np.full(((self.n + stride - 1) // stride, a.size), np.nan, np.float32)
        ns = C.c_int64(0)
        self._ck(self.lib.mcl_ping_innovation(self.h, _ptr(r), _ptr(a), a.size, float(sigma), float(support_k), float(r_max),
                                              _ptr(so), int(max_samples), _ptr(beams), _ptr(exp), C.byref(ns)))
        if exp is not None:
            exp = exp[:ns.value]
            exp[:, ~(r > 0)] = np.nan   # (the library leaves the entries of invalid beams unwritten)
        return PingInnovation(beams[:a.size], ns.value, sigma, exp)

    def gate_ping(self, ranges, beam_angles, sigma, r_max, sensor_offset=None, max_samples=INNOVATION_DEFAULT_SAMPLES,
                  support_k=3.0, nis_gate=10.83, min_support=0.01, max_gated_fraction=0.25):
        """(ranges_masked, verdict): ping_innovation, then innovation_gate; the gated beams' ranges are set to 0 -- the mark
        update_mbes skips -- in a float32 copy.  verdict.innovation is the PingInnovation."""
        inn = self.ping_innovation(ranges, beam_angles, sigma, r_max, sensor_offset, max_samples, support_k)
        verdict = innovation_gate(inn.beams, sigma, nis_gate, min_support, max_gated_fraction)
        verdict.innovation = inn
        masked = np.array(_f32(ranges).reshape(-1), copy=True)
        masked[verdict.mask] = 0.0
        return masked, verdict

    # ---- ping information: what the terrain can fix (include/mcl_information.h)
    def ping_information(self, beam_angles, sigma, r_max, sensor_offset=None, max_samples=INFORMATION_DEFAULT_SAMPLES,
                         delta_xy=0.5, delta_yaw=0.01, jump_max=None, dump=False):
        """how much a ping of this geometry can tell the cloud as it is: per beam the integer sums of the quantised central
        differences of the expected range in x, y and yaw over a strided sample of at most max_samples particles
        (mcl_ping_information) -- a PingInformation of THIS shard's sampled particles.  Nothing of the filter changes."""
        a, so = _f32(beam_angles).reshape(-1), _f64(sensor_offset)
        steps = make_information_steps(r_max, delta_xy, delta_yaw, jump_max)
        beams = np.zeros(max(a.size, 1), INFORMATION_SUMS)
        rng = None
        if dump:
            stride, _ = innovation_sample(self.n_global, max_samples)
            rng = np.full(((self.n + stride - 1) // stride, 6, max(a.size, 1)), np.nan, np.float32)
        ns = C.c_int64(0)
        self._ck(self.lib.mcl_ping_information(self.h, _ptr(a), a.size, float(r_max), _ptr(so), int(max_samples),
                                               C.byref(steps), _ptr(beams), _ptr(rng), C.byref(ns)))
        if rng is not None:
            rng = rng.reshape(-1)[:ns.value * 6 * a.size].reshape(ns.value, 6, a.size)
        return PingInformation(beams[:a.size], ns.value, sigma, delta_xy, delta_yaw, rng)

    def pose_information(self, poses, beam_angles, sigma, r_max, sensor_offset=None, delta_xy=0.5, delta_yaw=0.01,
                         jump_max=None):
        """how much a ping of this geometry can tell at each of M given poses (6 x M: x, y, z, roll, pitch, yaw in the
        coordinates the particle state is stored in; mcl_pose_information) -- a PoseInformation.  Needs a map, no
        particles; the cloud is neither read nor written."""
        p = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(6, -1))
        a, so = _f32(beam_angles).reshape(-1), _f64(sensor_offset)
        steps = make_information_steps(r_max, delta_xy, delta_yaw, jump_max)
        out = np.zeros(max(p.shape[1], 1), INFORMATION_SUMS)
        self._ck(self.lib.mcl_pose_information(self.h, _ptr(p), p.shape[1], _ptr(a), a.size, float(r_max), _ptr(so),
                                               C.byref(steps), _ptr(out)))
        return PoseInformation(out[:p.shape[1]], sigma, delta_xy, delta_yaw)

    # ---- ping matching: where the ping says the vehicle is (include/mcl_match.h)
    def match_ping(self, poses, ranges, beam_angles, sigma, r_max, sensor_offset=None, fit_z=False, max_iter=12, trace=False,
                   dump=False, cfg=None, **config):
        """the Levenberg-Marquardt pose fix of one ping from each of M start poses (6 x M: x, y, z, roll, pitch, yaw in the
        coordinates the particle state is stored in; mcl_match_ping) -- a PingMatch.  Needs a map, no particles; nothing of
        the filter is read or written.  cfg: a MatchConfig instead of fit_z / max_iter / the keywords of make_match_config."""
        p = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(6, -1))
        r, a, so = _f32(ranges).reshape(-1), _f32(beam_angles).reshape(-1), _f64(sensor_offset)
        if r.size != a.size:
            raise ValueError('match_ping: %d ranges for %d beam angles' % (r.size, a.size))
        c = cfg if cfg is not None else make_match_config(r_max, fit_z, max_iter, **config)
        M, T, nv = p.shape[1], max(int(c.max_iter), 0) + 1, 1 + 2 * int(c.dims)
        res = np.zeros(max(M, 1), MATCH_RESULT)
        tr = np.zeros((max(M, 1), T), MATCH_TRACE) if trace else None
        floats = max(M, 1) * T * max(nv, 1) * max(a.size, 1)
        # (a dump beyond the limit: the library refuses it before it writes; one float stands in for the buffer)
        rng = np.full(floats if floats <= MATCH_MAX_DUMP else 1, np.nan, np.float32) if dump else None
        self._ck(self.lib.mcl_match_ping(self.h, _ptr(p), M, _ptr(r), _ptr(a), a.size, float(sigma), float(r_max), _ptr(so),
                                         C.byref(c), _ptr(res), _ptr(tr), _ptr(rng)))
        if rng is not None:
            rng = rng.reshape(M, T, nv, a.size)
        return PingMatch(res[:M], c, sigma, tr, rng)

    def match_estimate(self, ranges, beam_angles, sigma, r_max, sensor_offset=None, modes=0, mode_cell=2.0, mode_n_yaw=36,
                       start=None, **kw):
        """match_ping from the cloud's mean pose (start: a pose of 6 instead), plus up to `modes` peaks of pose_modes: returns
        (PingMatch, index of its best fix or None)"""
        if start is None:
            mean, yaw, _ = self.mean_cov()
            start = np.array(mean, np.float64)
            start[5] = yaw
        starts = [np.asarray(start, np.float64).reshape(6)]
        if modes > 0:
            starts += [m.mean for m in self.pose_modes(mode_cell, mode_n_yaw, int(modes))[0]]
        match = self.match_ping(np.stack(starts, axis=1), ranges, beam_angles, sigma, r_max, sensor_offset, **kw)
        return match, match.best()

    # ---- swath matching: where the last K pings, rigidly tied by dead reckoning, say the vehicle is (include/mcl_swath.h)
    def match_swath(self, poses, ranges, beam_angles, offsets, sigma, r_max, sensor_offset=None, fit_z=False, max_iter=12,
                    trace=False, dump=False, cfg=None, **config):
        """the Levenberg-Marquardt fix of the ANCHOR of a swath from each of M start poses (6 x M as for match_ping; their
        roll and pitch are not read): ranges K x B, offsets K records of SwathOffset (swath_offsets makes them) -- a
        PingMatch whose derived quantities go through mcl_swath_derived and whose dump is M x (max_iter + 1) x K x
        (1 + 2 D) x B.  Needs a map, no particles; nothing of the filter is read or written."""
        p = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(6, -1))
        a, so = _f32(beam_angles).reshape(-1), _f64(sensor_offset)
        off = np.ascontiguousarray(offsets, dtype=SwathOffset).reshape(-1)
        K = off.size
        r = _f32(ranges).reshape(-1)
        if r.size != K * a.size:
            raise ValueError('match_swath: %d ranges for %d pings of %d beam angles' % (r.size, K, a.size))
        c = cfg if cfg is not None else make_match_config(r_max, fit_z, max_iter, **config)
        M, T, nv = p.shape[1], max(int(c.max_iter), 0) + 1, 1 + 2 * int(c.dims)
        res = np.zeros(max(M, 1), MATCH_RESULT)
        tr = np.zeros((max(M, 1), T), MATCH_TRACE) if trace else None
        floats = max(M, 1) * T * max(K, 1) * max(nv, 1) * max(a.size, 1)
        # (a dump beyond the limit: the library refuses it before it writes; one float stands in for the buffer)
        rng = np.full(floats if floats <= MATCH_MAX_DUMP else 1, np.nan, np.float32) if dump else None
        self._ck(self.lib.mcl_match_swath(self.h, _ptr(p), M, _ptr(r), _ptr(a), a.size, _ptr(off), K, float(sigma), float(r_max),
                                          _ptr(so), C.byref(c), _ptr(res), _ptr(tr), _ptr(rng)))
        if rng is not None:
            rng = rng.reshape(M, T, K, nv, a.size)
        return PingMatch(res[:M], c, sigma, tr, rng, derive=swath_derived)

    def match_swath_estimate(self, ranges, beam_angles, offsets, sigma, r_max, sensor_offset=None, modes=0, mode_cell=2.0,
                             mode_n_yaw=36, start=None, **kw):
        """match_swath from the cloud's mean pose (start: a pose of 6 instead), plus up to `modes` peaks of pose_modes:
        returns (PingMatch, index of its best fix or None)"""
        if start is None:
            mean, yaw, _ = self.mean_cov()
            start = np.array(mean, np.float64)
            start[5] = yaw
        starts = [np.asarray(start, np.float64).reshape(6)]
        if modes > 0:
            starts += [m.mean for m in self.pose_modes(mode_cell, mode_n_yaw, int(modes))[0]]
        match = self.match_swath(np.stack(starts, axis=1), ranges, beam_angles, offsets, sigma, r_max, sensor_offset, **kw)
        return match, match.best()

    def set_landmarks(self, xyz):
        a = _f64(xyz)
        self._ck(self.lib.mcl_set_landmarks(self.h, _ptr(a), a.shape[0]))

    def set_landmark_noise(self, cov6=None, Q6=None):
        """Mahalanobis association: per-landmark covariance (n x 6: xx xy xz yy yz zz, map frame) and / or the
        sensor-frame measurement covariance Q (6); both None = isotropic sigma again."""
        c, q = _f64(cov6), _f64(Q6)
        self._ck(self.lib.mcl_set_landmark_noise(self.h, _ptr(c), _ptr(q)))

    def update_landmarks(self, det_xyz, sigma, k=1, gate=11.345, sensor_offset=None, accumulate=False):
        d, so = _f64(det_xyz), _f64(sensor_offset)
        self._ck(self.lib.mcl_update_landmarks(self.h, _ptr(d), d.shape[0], float(sigma), int(k), float(gate),
                                               _ptr(so), 1 if accumulate else 0))

    def update_landmarks_assign(self, det_xyz, sigma, k_cand=8, gate=11.345, new_mh_dist=11.345, sensor_offset=None,
                                accumulate=False, n_keep=0):
        """Landmark update with a global (Hungarian) assignment per particle; returns the assignment of
        the first n_keep particles (n_keep x n_det int32) or None."""
        d, so = _f64(det_xyz), _f64(sensor_offset)
        out = np.zeros((int(n_keep), d.shape[0]), dtype=np.int32) if n_keep else None
        self._ck(self.lib.mcl_update_landmarks_assign(self.h, _ptr(d), d.shape[0], float(sigma), int(k_cand), float(gate),
                                                      float(new_mh_dist), _ptr(so), 1 if accumulate else 0,
                                                      out.ctypes.data if out is not None else None, int(n_keep)))
        return out

    def resample(self, uniforms=None, normals=None):
        u = None if uniforms is None else _f64(np.atleast_1d(uniforms))
        nz = _f64(normals)
        self._ck(self.lib.mcl_resample(self.h, _ptr(u), 0 if u is None else u.size, _ptr(nz)))

    def resample_prepare(self):
        k = C.c_int64(0)
        self._ck(self.lib.mcl_resample_prepare(self.h, C.byref(k)))
        return int(k.value)

    def mean_cov(self):
        mean, yaw, cov = np.zeros(6), np.zeros(1), np.zeros(9)
        self._ck(self.lib.mcl_mean_cov(self.h, _ptr(mean), _ptr(yaw), _ptr(cov)))
        return mean, float(yaw[0]), cov

    def mean_cov_async(self):
        """queue mean/cov on the stream without waiting; read it later with last_mean_cov / mean_history"""
        self._ck(self.lib.mcl_mean_cov_async(self.h))

    def last_mean_cov(self):
        mean, yaw, cov = np.zeros(6), np.zeros(1), np.zeros(9)
        self._ck(self.lib.mcl_last_mean_cov(self.h, _ptr(mean), _ptr(yaw), _ptr(cov)))
        return mean, float(yaw[0]), cov

    def mean_history(self, last_k):
        out = np.zeros((int(last_k), 6))
        self._ck(self.lib.mcl_mean_history(self.h, int(last_k), _ptr(out)))
        return out

    def poses(self):
        out = np.zeros((self.n, 7))
        self._ck(self.lib.mcl_get_poses(self.h, _ptr(out)))
        return out

    # ---- state access
    def get_particles(self, weights=False):
        soa = np.zeros((6, self.n))
        w = np.zeros(self.n) if weights else None
        self._ck(self.lib.mcl_get_particles(self.h, _ptr(soa), _ptr(w)))
        return (soa, w) if weights else soa

    def set_particles(self, soa):
        s = _f64(soa)
        assert s.shape == (6, self.n)
        self._ck(self.lib.mcl_set_particles(self.h, _ptr(s)))

    def get_log_weights(self):
        lw = np.zeros(self.n)
        self._ck(self.lib.mcl_get_log_weights(self.h, _ptr(lw)))
        return lw

    def set_log_weights(self, lw, mode=WEIGHT_LOG_SHIFT):
        a = _f64(lw)
        self._ck(self.lib.mcl_set_log_weights(self.h, _ptr(a), int(mode)))

    def last_indices(self):
        idx = np.zeros(self.n, np.int32)
        self._ck(self.lib.mcl_get_last_indices(self.h, _ptr(idx)))
        return idx

    def last_offspring_cdf(self):
        c = np.zeros(self.n_global, np.uint32)
        self._ck(self.lib.mcl_get_last_offspring_cdf(self.h, _ptr(c)))
        return c

    def fixed_weights(self):
        q = np.zeros(self.n, np.uint64)
        t = C.c_uint64(0)
        self._ck(self.lib.mcl_get_fixed_weights(self.h, _ptr(q), C.addressof(t)))
        return q, int(t.value)

    # ---- fused asynchronous step
    def step_mbes(self, v, wz, q, z, dt, ranges, beam_angles, sigma, r_max, sensor_offset=None):
        od = make_odom(v, wz, q, z)
        r, a, so = _f32(ranges), _f32(beam_angles), _f64(sensor_offset)
        self._ck(self.lib.mcl_step_mbes(self.h, C.byref(od), float(dt), _ptr(r), _ptr(a), a.size, float(sigma),
                                        float(r_max), _ptr(so)))

    def step_mbes_landmarks(self, v, wz, q, z, dt, ranges, beam_angles, sigma, r_max, det_xyz, lm_sigma, k=1, gate=11.345,
                            sensor_offset=None, lm_sensor_offset=None):
        """step_mbes with the landmark observation of the ping accumulated onto the MBES log-likelihood (BASELINE
        config 5): mcl_step_mbes_landmarks"""
        od = make_odom(v, wz, q, z)
        r, a, so = _f32(ranges), _f32(beam_angles), _f64(sensor_offset)
        d, lso = _f64(det_xyz), _f64(lm_sensor_offset)
        self._ck(self.lib.mcl_step_mbes_landmarks(self.h, C.byref(od), float(dt), _ptr(r), _ptr(a), a.size, float(sigma),
                                                  float(r_max), _ptr(so), _ptr(d), d.shape[0], float(lm_sigma), int(k),
                                                  float(gate), _ptr(lso)))

    def sync(self):
        self._ck(self.lib.mcl_sync(self.h))

    # ---- multi-GPU
    def comm_init(self, uid_bytes, overlap=True):
        self._ck(self.lib.mcl_comm_init_ex(self.h, uid_bytes, 0 if overlap else 1))

    def comm_ranks(self):
        """(ranks RCCL connected = all-reduce(sum) of 1, overlapped-gather communicator present)"""
        r, o = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.mcl_comm_ranks(self.h, C.byref(r), C.byref(o)))
        return int(r.value), bool(o.value)

    def comm_selftest(self, timeout_ms=20000):
        self._ck(self.lib.mcl_comm_selftest(self.h, int(timeout_ms)))

    def comm_shutdown(self, abort=False):
        self._ck(self.lib.mcl_comm_shutdown(self.h, 1 if abort else 0))

    def exchange_stats(self, reset=False):
        """(particle states sent to peers, lost slots filled) by the sharded resamples since the last reset"""
        a, b = C.c_int64(0), C.c_int64(0)
        self._ck(self.lib.mcl_exchange_stats(self.h, C.byref(a), C.byref(b), 1 if reset else 0))
        return int(a.value), int(b.value)

    def exchange_ops(self, reset=False):
        """(point-to-point operations issued, exchanges) by the sharded resamples since the last reset"""
        a, b = C.c_int64(0), C.c_int64(0)
        self._ck(self.lib.mcl_exchange_ops(self.h, C.byref(a), C.byref(b), 1 if reset else 0))
        return int(a.value), int(b.value)

    # ---- instrumentation
    def timing_enable(self, on=True):
        self._ck(self.lib.mcl_timing_enable(self.h, 1 if on else 0))

    def mbes_last_path(self):
        """(path, handed_over, deferred_groups) of the last MBES update: path 1 = fan sweep, 0 = ray traversal."""
        p, ho, dg = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._ck(self.lib.mcl_mbes_last_path(self.h, C.byref(p), C.byref(ho), C.byref(dg)))
        return int(p.value), int(ho.value), int(dg.value)

    def mbes_last_handover(self):
        """(by_slice, by_traversal): who cast the particles the last update's sweep handed over (TIN with holes: the fan slice first)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._ck(self.lib.mcl_mbes_last_handover(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def mbes_visit_order(self):
        """(slots, sorted): slots[p] = state slot of the particle the last fused step's sweep visited at position p."""
        slots = np.empty(self.n, dtype=np.uint32)
        srt = C.c_int32(0)
        self._ck(self.lib.mcl_mbes_visit_order(self.h, _ptr(slots), C.byref(srt)))
        return slots, bool(srt.value)

    def timing_get(self):
        t = Timing()
        self._ck(self.lib.mcl_timing_get(self.h, C.byref(t)))
        return {name: (t.ms[k], t.launches[k]) for k, name in enumerate(_lib.MCL_K_NAMES)}


def comm_unique_id():
    lib = _lib.load()
    buf = C.create_string_buffer(128)
    _lib.check(lib.mcl_comm_unique_id(buf))
    return buf.raw


def history_bracket(stamps_newest_first, stamp):
    """(lag, frac, where) of `stamp` among frame stamps, newest first (mcl_history_bracket: host arithmetic, no handle)"""
    lib = _lib.load()
    s = _f64(stamps_newest_first).reshape(-1)
    lag, frac, where = C.c_int32(0), C.c_double(0.0), C.c_int32(0)
    _lib.check(lib.mcl_history_bracket(_ptr(s), s.size, float(stamp), C.byref(lag), C.byref(frac), C.byref(where)))
    return int(lag.value), float(frac.value), int(where.value)


def make_drift_config(init_std, walk_std):
    cfg = _lib.DriftConfig()
    for name, v in (('init_std', init_std), ('walk_std', walk_std)):
        a = _f64(v).reshape(-1)
        if a.size != 3:
            raise ValueError('drift: %s is three numbers (cx, cy, bw)' % name)
        getattr(cfg, name)[:] = [float(x) for x in a]
    return cfg


def drift_config_check(init_std, walk_std):
    """None, or the sentence saying which std is negative or not finite (mcl_drift_config_check: no device)"""
    cfg, why = make_drift_config(init_std, walk_std), C.c_char_p()
    st = _lib.load().mcl_drift_config_check(C.byref(cfg), C.byref(why))
    return None if st == 0 else (why.value or b'').decode()


def drift_bytes(n):
    """device bytes mcl_drift_enable allocates on a handle of n particles (mcl_drift_bytes: no device)"""
    b = C.c_int64(0)
    _lib.check(_lib.load().mcl_drift_bytes(int(n), C.byref(b)))
    return int(b.value)


def _unpack_lower(packed, d):
    """(d, d) lower-triangular from the packed order (0,0), (1,0), (1,1), (2,0), ..."""
    m = np.zeros((d, d))
    m[np.tril_indices(d)] = np.array(packed[:d * (d + 1) // 2])
    return m


def _pack_lower(m):
    m = _f64(m)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError('regularise: a square matrix')
    return np.ascontiguousarray(m[np.tril_indices(m.shape[0])])


def make_regularise_config(scale, shrink, dims):
    cfg = _lib.RegulariseConfig()
    cfg.scale, cfg.shrink, cfg.dims = float(scale), 1 if shrink else 0, int(dims)
    return cfg


def regularise_config_check(scale, shrink=True, dims=3):
    """None, or the sentence saying what mcl_regularise refuses about (scale, dims) (mcl_regularise_config_check: no device)"""
    cfg, why = make_regularise_config(scale, shrink, dims), C.c_char_p()
    st = _lib.load().mcl_regularise_config_check(C.byref(cfg), C.byref(why))
    return None if st == 0 else (why.value or b'').decode()


def regularise_bandwidth(n, dims, scale=1.0, shrink=True):
    """(h, a): h0 = scale (4 / ((dims + 2) n))^(1 / (dims + 4)); shrink: h = min(h0, 1), a = sqrt(1 - h^2), else h = h0,
    a = 1 (mcl_regularise_bandwidth: host arithmetic)"""
    h, a = C.c_double(0.0), C.c_double(0.0)
    _lib.check(_lib.load().mcl_regularise_bandwidth(int(n), int(dims), float(scale), 1 if shrink else 0, C.byref(h),
                                                    C.byref(a)))
    return float(h.value), float(a.value)


def regularise_factor(cov):
    """(chol, dead): the lower-triangular factor of a (3, 3) or (6, 6) covariance (its lower triangle is read) by the rule
    of include/mcl_regularise.h, and the mask of the columns it left zero (mcl_regularise_factor: the very function the
    device runs)"""
    c = _pack_lower(cov)
    d = np.asarray(cov).shape[0]
    out, dead = np.zeros(c.size), C.c_int32(0)
    _lib.check(_lib.load().mcl_regularise_factor(_ptr(c), int(d), _ptr(out), C.byref(dead)))
    return _unpack_lower(out, d), int(dead.value)


def temper_beta(j):
    """beta_j = 2^(-j / 64) of the tempering lattice, 0 <= j <= 2048 (mcl_temper_beta: host arithmetic)"""
    b = C.c_double(0.0)
    _lib.check(_lib.load().mcl_temper_beta(int(j), C.byref(b)))
    return float(b.value)


def temper_pass(s1, s2, n_target):
    """s1^2 >= n_target s2 2^32 in 128-bit integers (mcl_temper_pass: host arithmetic)"""
    p = C.c_int32(0)
    _lib.check(_lib.load().mcl_temper_pass(int(s1), int(s2), int(n_target), C.byref(p)))
    return bool(p.value)


def temper_candidates(round_, j_prev=0):
    """the candidate levels of a round of the search, ascending (mcl_temper_candidates: host arithmetic)"""
    cand, nc = (C.c_int32 * 17)(), C.c_int32(0)
    _lib.check(_lib.load().mcl_temper_candidates(int(round_), int(j_prev), cand, C.byref(nc)))
    return [int(cand[k]) for k in range(nc.value)]


def group_temper(engines, ess_ratio=0.5, apply=True, n_target=None):
    """Engine.temper over shards that together hold the cloud (mcl_group_temper): n_global = the sum of their sizes; level
    and log-weights equal the unsharded call's bit for bit.  Returns a TemperResult."""
    lib = _lib.load()
    ns = len(engines)
    hs = (C.c_void_p * ns)(*[e.h for e in engines])
    nt = temper_target(ess_ratio, sum(e.n for e in engines)) if n_target is None else int(n_target)
    c = _lib.TemperRes()
    _lib.check(lib.mcl_group_temper(hs, ns, nt, 1 if apply else 0, C.byref(c)), engines[0].h)
    return TemperResult.from_c(c)


def quantile_key(v):
    """the order-preserving 64-bit key of v + 0.0 (mcl_quantile_key: host arithmetic); NaN is refused"""
    k = C.c_uint64(0)
    _lib.check(_lib.load().mcl_quantile_key(float(v), C.byref(k)))
    return int(k.value)


def quantile_value(key):
    """the double a key stands for (mcl_quantile_value: host arithmetic)"""
    v = C.c_double(0.0)
    _lib.check(_lib.load().mcl_quantile_value(int(key), C.byref(v)))
    return float(v.value)


def quantile_threshold(p):
    """P = floor(p 2^32), 2^-32 <= p <= 1 (mcl_quantile_threshold: host arithmetic)"""
    t = C.c_uint64(0)
    _lib.check(_lib.load().mcl_quantile_threshold(float(p), C.byref(t)))
    return int(t.value)


def quantile_reached(mass, total, P):
    """2^32 mass >= P total in 128-bit integers (mcl_quantile_reached: host arithmetic)"""
    r = C.c_int32(0)
    _lib.check(_lib.load().mcl_quantile_reached(int(mass), int(total), int(P), C.byref(r)))
    return bool(r.value)


def group_cloud_quantiles(engines, quantity, probs, centre=None, weighted=False):
    """Engine.cloud_quantiles over shards that together hold the cloud (mcl_group_cloud_quantiles): the unsharded call's
    result bit for bit, for any split.  A list of Quantile."""
    lib = _lib.load()
    ns = len(engines)
    hs = (C.c_void_p * ns)(*[e.h for e in engines])
    q = make_quantile_query(quantity, centre, weighted)
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    out = (_lib.QuantileResult * max(p.size, 1))()
    _lib.check(lib.mcl_group_cloud_quantiles(hs, ns, C.byref(q), _ptr(p), p.size, out), engines[0].h)
    return [Quantile.from_c(out[k]) for k in range(p.size)]


def innovation_sample(n_global, max_samples=INNOVATION_DEFAULT_SAMPLES):
    """(stride, count) of the strided sample (mcl_innovation_sample: host arithmetic)"""
    st, ct = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.load().mcl_innovation_sample(int(n_global), int(max_samples), C.byref(st), C.byref(ct)))
    return int(st.value), int(ct.value)


def innovation_dirs(beam_angles):
    """(B, 3) float32: the unit directions the innovation kernel casts along (mcl_innovation_dirs: host arithmetic)"""
    a = _f32(beam_angles).reshape(-1)
    out = np.zeros((max(a.size, 1), 3), np.float32)
    _lib.check(_lib.load().mcl_innovation_dirs(_ptr(a), a.size, _ptr(out)))
    return out[:a.size]


def _innovation_records(beams):
    if isinstance(beams, PingInnovation):
        beams = beams.beams
    return np.ascontiguousarray(beams, dtype=INNOVATION_BEAM).reshape(-1)


def merge_innovation(parts):
    """the records of the union of several shards' samples (mcl_innovation_merge: host arithmetic): parts are
    PingInnovation objects or record arrays of equal length; returns a record array"""
    recs = [_innovation_records(p) for p in parts]
    B = recs[0].size if recs else 0
    if any(r.size != B for r in recs):
        raise ValueError('merge_innovation: the parts differ in their beam count')
    stack = np.ascontiguousarray(np.stack(recs)) if recs else np.zeros((0, 0), INNOVATION_BEAM)
    out = np.zeros(max(B, 1), INNOVATION_BEAM)
    _lib.check(_lib.load().mcl_innovation_merge(_ptr(stack), len(recs), B, _ptr(out)))
    return out[:B]


def innovation_gate(beams, sigma, nis_gate=10.83, min_support=0.01, max_gated_fraction=0.25):
    """the derived quantities and the gate of include/mcl_innovation.h over the records `beams` (a PingInnovation or a
    record array): a GateVerdict (mcl_innovation_gate: host arithmetic)"""
    rec = _innovation_records(beams)
    cfg = make_gate_config(nis_gate, min_support, max_gated_fraction)
    per = np.zeros(max(rec.size, 1), INNOVATION_DERIVED)
    v = _lib.InnovationVerdict()
    _lib.check(_lib.load().mcl_innovation_gate(_ptr(rec), rec.size, float(sigma), C.byref(cfg), _ptr(per), C.byref(v)))
    per = per[:rec.size]
    return GateVerdict(mask=per['gated'] != 0, n_gated=int(v.n_gated), inconsistent=bool(v.inconsistent),
                       n_valid=int(v.n_valid), n_candidates=int(v.n_candidates), nis_sum=float(v.nis_sum),
                       mean_nu=float(v.mean_nu), nu=per['nu'].copy(), var=per['var'].copy(), nis=per['nis'].copy(),
                       support=per['support'].copy())


def group_ping_innovation(engines, ranges, beam_angles, sigma, r_max, sensor_offset=None,
                          max_samples=INNOVATION_DEFAULT_SAMPLES, support_k=3.0):
    """Engine.ping_innovation over shards that together hold the cloud (mcl_group_ping_innovation): the unsharded call's
    records bit for bit, for any split.  A PingInnovation (no dump)."""
    lib = _lib.load()
    ns = len(engines)
    hs = (C.c_void_p * ns)(*[e.h for e in engines])
    r, a, so = _f32(ranges).reshape(-1), _f32(beam_angles).reshape(-1), _f64(sensor_offset)
    if r.size != a.size:
        raise ValueError('group_ping_innovation: %d ranges for %d beam angles' % (r.size, a.size))
    beams = np.zeros(max(a.size, 1), INNOVATION_BEAM)
    n = C.c_int64(0)
    _lib.check(lib.mcl_group_ping_innovation(hs, ns, _ptr(r), _ptr(a), a.size, float(sigma), float(support_k), float(r_max),
                                             _ptr(so), int(max_samples), _ptr(beams), C.byref(n)), engines[0].h)
    return PingInnovation(beams[:a.size], n.value, sigma)


def _information_records(recs):
    if isinstance(recs, PingInformation):
        recs = recs.beams
    elif isinstance(recs, PoseInformation):
        recs = recs.poses
    return np.ascontiguousarray(recs, dtype=INFORMATION_SUMS).reshape(-1)


def information_matrix(records, sigma, delta_xy=0.5, delta_yaw=0.01, per_pose=False):
    """the derived quantities of include/mcl_information.h (mcl_information_matrix: host arithmetic) as records of
    INFORMATION_RESULT: one for the beams of a cloud sample, or with per_pose=True an array, one per record"""
    rec = _information_records(records)
    out = np.zeros(max(rec.size, 1) if per_pose else 1, INFORMATION_RESULT)
    _lib.check(_lib.load().mcl_information_matrix(_ptr(rec), rec.size, 1 if per_pose else 0, float(sigma), float(delta_xy),
                                                  float(delta_yaw), _ptr(out)))
    return out[:rec.size] if per_pose else out[0]


def merge_information(parts):
    """the records of the union of several shards' samples (mcl_information_merge: host arithmetic): parts are
    PingInformation objects or record arrays of equal length; returns a record array"""
    recs = [_information_records(p) for p in parts]
    B = recs[0].size if recs else 0
    if any(r.size != B for r in recs):
        raise ValueError('merge_information: the parts differ in their beam count')
    stack = np.ascontiguousarray(np.stack(recs)) if recs else np.zeros((0, 0), INFORMATION_SUMS)
    out = np.zeros(max(B, 1), INFORMATION_SUMS)
    _lib.check(_lib.load().mcl_information_merge(_ptr(stack), len(recs), B, _ptr(out)))
    return out[:B]


def group_ping_information(engines, beam_angles, sigma, r_max, sensor_offset=None, max_samples=INFORMATION_DEFAULT_SAMPLES,
                           delta_xy=0.5, delta_yaw=0.01, jump_max=None):
    """Engine.ping_information over shards that together hold the cloud (mcl_group_ping_information): the unsharded call's
    records bit for bit, for any split.  A PingInformation (no dump)."""
    lib = _lib.load()
    ns = len(engines)
    hs = (C.c_void_p * ns)(*[e.h for e in engines])
    a, so = _f32(beam_angles).reshape(-1), _f64(sensor_offset)
    steps = make_information_steps(r_max, delta_xy, delta_yaw, jump_max)
    beams = np.zeros(max(a.size, 1), INFORMATION_SUMS)
    n = C.c_int64(0)
    _lib.check(lib.mcl_group_ping_information(hs, ns, _ptr(a), a.size, float(r_max), _ptr(so), int(max_samples),
                                              C.byref(steps), _ptr(beams), C.byref(n)), engines[0].h)
    return PingInformation(beams[:a.size], n.value, sigma, delta_xy, delta_yaw)


def _match_record(rec):
    return np.ascontiguousarray(rec, dtype=MATCH_SUMS).reshape(-1)[:1].copy()


def match_config_check(cfg, r_max):
    """None when mcl_match_ping would accept the config for this r_max, else the rule that is broken (host arithmetic)"""
    why = C.c_char_p()
    rc = _lib.load().mcl_match_config_check(C.byref(cfg) if cfg is not None else None, float(r_max), C.byref(why))
    return None if rc == 0 else (why.value or b'').decode()


def match_solve(rec, cfg, j):
    """SOLVE of include/mcl_match.h (mcl_match_solve: host arithmetic): (delta over x, y, yaw, z; the dead mask)"""
    r, d, dead = _match_record(rec), np.zeros(4), C.c_int32(0)
    _lib.check(_lib.load().mcl_match_solve(_ptr(r), C.byref(cfg), int(j), _ptr(d), C.byref(dead)))
    return d, int(dead.value)


def match_better(q, p, min_beams):
    """is the pose with the record q better than the one with the record p (mcl_match_better: 128-bit integers)"""
    a, b, out = _match_record(q), _match_record(p), C.c_int32(0)
    _lib.check(_lib.load().mcl_match_better(_ptr(a), _ptr(b), int(min_beams), C.byref(out)))
    return bool(out.value)


def match_derived(rec, cfg, sigma):
    """the derived quantities of a record (mcl_match_derived: host arithmetic) as one record of MATCH_DERIVED"""
    r, out = _match_record(rec), np.zeros(1, MATCH_DERIVED)
    _lib.check(_lib.load().mcl_match_derived(_ptr(r), C.byref(cfg), float(sigma), _ptr(out)))
    return out[0]


def swath_offsets(poses6, anchor=-1):
    """mcl_swath_offsets (host arithmetic): the K records of SwathOffset of the vehicle's poses at the K pings (6 x K: x, y,
    z, roll, pitch, yaw; dead reckoning will do) relative to column `anchor` (-1: the last)"""
    p = np.ascontiguousarray(np.asarray(poses6, np.float64).reshape(6, -1))
    out = np.zeros(max(p.shape[1], 1), SwathOffset)
    _lib.check(_lib.load().mcl_swath_offsets(_ptr(p), p.shape[1], int(anchor), _ptr(out)))
    return out[:p.shape[1]]


def swath_check(K, B, offsets):
    """None when mcl_match_swath would accept the swath's shape and offsets, else the rule that is broken"""
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=SwathOffset).reshape(-1)
    why = C.c_char_p()
    rc = _lib.load().mcl_swath_check(int(K), int(B), _ptr(off), C.byref(why))
    return None if rc == 0 else (why.value or b'').decode()


def swath_solve(rec, cfg, j):
    """match_solve for the record of a swath (mcl_swath_solve: n up to 16384)"""
    r, d, dead = _match_record(rec), np.zeros(4), C.c_int32(0)
    _lib.check(_lib.load().mcl_swath_solve(_ptr(r), C.byref(cfg), int(j), _ptr(d), C.byref(dead)))
    return d, int(dead.value)


def swath_better(q, p, min_beams):
    """match_better for the records of a swath (mcl_swath_better)"""
    a, b, out = _match_record(q), _match_record(p), C.c_int32(0)
    _lib.check(_lib.load().mcl_swath_better(_ptr(a), _ptr(b), int(min_beams), C.byref(out)))
    return bool(out.value)


def swath_derived(rec, cfg, sigma):
    """match_derived for the record of a swath (mcl_swath_derived) as one record of MATCH_DERIVED"""
    r, out = _match_record(rec), np.zeros(1, MATCH_DERIVED)
    _lib.check(_lib.load().mcl_swath_derived(_ptr(r), C.byref(cfg), float(sigma), _ptr(out)))
    return out[0]


def make_reseed_select_config(max_components=16, min_beams=32, max_rms=0.5, sep_xy=1.0, sep_yaw=0.1, cov_scale=1.0,
                              add_std_xy=0.25, add_std_yaw=0.02, dead_std_xy=4.0, dead_std_yaw=0.2):
    """mcl_reseed_select_config (include/mcl_reseed.h).  The defaults are policy."""
    c = _lib.ReseedSelectConfig()
    c.max_components, c.min_beams = int(max_components), int(min_beams)
    c.max_rms, c.sep_xy, c.sep_yaw, c.cov_scale = float(max_rms), float(sep_xy), float(sep_yaw), float(cov_scale)
    c.add_std_xy, c.add_std_yaw, c.dead_std_xy, c.dead_std_yaw = (float(add_std_xy), float(add_std_yaw), float(dead_std_xy),
                                                                  float(dead_std_yaw))
    return c


def reseed_select_check(cfg=None, **config):
    """None when mcl_reseed_select would accept the config (a ReseedSelectConfig, or the keywords of
    make_reseed_select_config), else the rule that is broken (host arithmetic)"""
    c = cfg if cfg is not None else make_reseed_select_config(**config)
    why = C.c_char_p()
    rc = _lib.load().mcl_reseed_select_check(C.byref(c), C.byref(why))
    return None if rc == 0 else (why.value or b'').decode()


def reseed_components_check(components):
    """None when mcl_inject_gaussian would accept the table of components, else the rule that is broken"""
    comps = None if components is None else np.ascontiguousarray(components, dtype=ReseedComponent).reshape(-1)
    why = C.c_char_p()
    rc = _lib.load().mcl_reseed_components_check(_ptr(comps), 0 if comps is None else comps.size, C.byref(why))
    return None if rc == 0 else (why.value or b'').decode()


def reseed_select(match, sigma=None, cfg=None, **config):
    """mcl_reseed_select (host arithmetic): the mixture of a PingMatch's converged fixes -- (components, a record array of
    ReseedComponent, lowest rms first; indices, the result each came from).  sigma: the match's own when None.  cfg: a
    ReseedSelectConfig instead of the keywords of make_reseed_select_config.  No candidate gives two empty arrays."""
    c = cfg if cfg is not None else make_reseed_select_config(**config)
    res = np.ascontiguousarray(match.results, dtype=MATCH_RESULT).reshape(-1)
    room = max(int(c.max_components), 1) if 1 <= int(c.max_components) <= RESEED_MAX_COMPONENTS else 1
    comps, idx, n = np.zeros(room, ReseedComponent), np.zeros(room, np.int64), C.c_int32(0)
    _lib.check(_lib.load().mcl_reseed_select(_ptr(res), res.size, C.byref(match.cfg), float(match.sigma if sigma is None else sigma),
                                             C.byref(c), _ptr(comps), _ptr(idx), C.byref(n)))
    return comps[:n.value].copy(), idx[:n.value].copy()


KLD_Z_99 = 2.3263478740408408     # the upper 0.99 quantile of the standard normal (delta = 0.01)
KLD_MAX_CELLS = 1 << 27
KLD_MAX_YAW = 1024


def kld_bound(k, epsilon=0.05, z=KLD_Z_99, n_min=1, n_max=2 ** 31):
    """mcl_kld_bound (host arithmetic): the particle count Fox's bound asks for when k cells are occupied, the KL error
    of the sampled posterior staying below epsilon with probability 1 - delta (z: the normal's upper 1 - delta quantile)"""
    n = C.c_int64(0)
    _lib.check(_lib.load().mcl_kld_bound(int(k), float(epsilon), float(z), int(n_min), int(n_max), C.byref(n)))
    return int(n.value)


def kld_grid_check(grid):
    """the cell count of the lattice when mcl_kld_bins would accept it (up to 2^27 cells, n_yaw up to 1024), else None"""
    n = C.c_int64(0)
    rc = _lib.load().mcl_kld_grid_check(C.byref(grid) if grid is not None else None, C.byref(n))
    return int(n.value) if rc == 0 else None


def footprint_odom(bounds, m2o):
    """the bounding box, in the odom frame, of the map footprint's four corners carried through the inverse of m2o (the rule
    of Engine.mode_grid and of mcl_recovery.h; m2o must turn about z alone): (x_min, x_max, y_min, y_max)"""
    m = np.identity(4) if m2o is None else np.asarray(m2o, np.float64).reshape(4, 4)
    if (abs(m[0, 2]) > 1e-12 or abs(m[1, 2]) > 1e-12 or abs(m[2, 0]) > 1e-12 or abs(m[2, 1]) > 1e-12 or
            abs(m[2, 2] - 1.0) > 1e-12):
        raise MclError(-4, 'the map footprint needs an m2o that turns about z alone')
    x_min, x_max, y_min, y_max = [float(v) for v in bounds]
    xs, ys = [], []
    for x, y in ((x_min, y_min), (x_min, y_max), (x_max, y_min), (x_max, y_max)):
        dx, dy = x - m[0, 3], y - m[1, 3]
        xs.append(m[0, 0] * dx + m[1, 0] * dy)
        ys.append(m[0, 1] * dx + m[1, 1] * dy)
    return (min(xs), max(xs), min(ys), max(ys))


def reseed_starts(box, pitch, yaw=(-math.pi, math.pi), n_yaw=8, z=0.0, roll=0.0, pitch_angle=0.0, bounds=None, m2o=None):
    """a lattice of start poses for match_ping / match_swath, 6 x M (x, y, z, roll, pitch, yaw): the box (x_min, x_max,
    y_min, y_max; ODOM frame) cut into nx x ny equal cells no wider than `pitch` (nx = ceil(extent / pitch), at least 1),
    the yaw interval into n_yaw equal cells, one start at every cell's CENTRE, column (iy nx + ix) n_yaw + k; yaw wrapped
    into [-pi, pi).  box=None: the map footprint `bounds` (map frame) carried into the odom frame through the inverse of
    m2o by the rule Engine.mode_grid uses (footprint_odom).  ValueError when M would exceed 65 536, what one match call
    takes."""
    if box is None:
        if bounds is None:
            raise ValueError('reseed_starts: a box, or the bounds of the map')
        box = footprint_odom(bounds, m2o)
    x_min, x_max, y_min, y_max = [float(v) for v in box]
    pitch, n_yaw = float(pitch), int(n_yaw)
    y0, y1 = float(yaw[0]), float(yaw[1])
    if not (pitch > 0.0 and np.isfinite(pitch) and x_max >= x_min and y_max >= y_min and n_yaw >= 1 and y1 >= y0 and
            np.all(np.isfinite([x_min, x_max, y_min, y_max, y0, y1]))):
        raise ValueError('reseed_starts: bad pitch, box, yaw interval or n_yaw')
    nx = max(1, int(math.ceil((x_max - x_min) / pitch)))
    ny = max(1, int(math.ceil((y_max - y_min) / pitch)))
    M = nx * ny * n_yaw
    if M > RESEED_MAX_STARTS:
        raise ValueError('reseed_starts: %d x %d x %d = %d starts, above the %d one match call takes (a coarser pitch, fewer '
                         'yaws or a smaller box)' % (nx, ny, n_yaw, M, RESEED_MAX_STARTS))
    xs = x_min + (np.arange(nx) + 0.5) * ((x_max - x_min) / nx)
    ys = y_min + (np.arange(ny) + 0.5) * ((y_max - y_min) / ny)
    ws = y0 + (np.arange(n_yaw) + 0.5) * ((y1 - y0) / n_yaw)
    ws = np.mod(ws + math.pi, 2.0 * math.pi) - math.pi
    out = np.zeros((6, M))
    gy, gx, gw = np.meshgrid(ys, xs, ws, indexing='ij')
    out[0], out[1], out[5] = gx.reshape(-1), gy.reshape(-1), gw.reshape(-1)
    out[2], out[3], out[4] = float(z), float(roll), float(pitch_angle)
    return out


def localisability_map(engine, cell, z, yaws, beam_angles, sigma, r_max, sensor_offset=None, roll=0.0, pitch=0.0,
                       delta_xy=0.5, delta_yaw=0.01, jump_max=None, margin=0.0):
    """Where on the engine's map can a vehicle localise?  A lattice of poses over map_bounds() -- cell centres `cell`
    metres apart, in map coordinates, at height z and each heading of `yaws` -- through Engine.pose_information.  Returns a
    dict of (ny, nx) rasters crlb_strong, crlb_weak, weak_axis, hit_share (row = y, column = x) and the lattice's x, y.
    With several yaws a cell reports the heading with the worst (largest) crlb_weak: its other rasters belong to that
    heading.  margin > 0 lets the lattice run that many metres past the map's edge on every side (cells from which no ray
    finds the map have hit_share 0 and infinite bounds).  The map frame is the state's frame only for an identity m2o;
    otherwise the lattice is carried into it."""
    x0, x1, y0, y1 = engine.map_bounds()
    x0, x1, y0, y1 = x0 - float(margin), x1 + float(margin), y0 - float(margin), y1 + float(margin)
    cell = float(cell)
    if not cell > 0.0:
        raise ValueError('localisability_map: cell must be positive')
    nx, ny = max(int(math.floor((x1 - x0) / cell)), 1), max(int(math.floor((y1 - y0) / cell)), 1)
    xs, ys = x0 + cell * (np.arange(nx) + 0.5), y0 + cell * (np.arange(ny) + 0.5)
    gx, gy = np.meshgrid(xs, ys)                      # (ny, nx)
    yaws = np.atleast_1d(np.asarray(yaws, np.float64))
    # map -> state coordinates (the inverse of m2o: a rigid motion about z for every configuration the node builds)
    m2o = np.asarray(engine.m2o, np.float64).reshape(-1)
    T = np.identity(4)
    T[:3, :] = m2o[:12].reshape(3, 4)
    Ti = np.linalg.inv(T)
    pts = Ti @ np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, float(z)), np.ones(gx.size)])
    dyaw = math.atan2(Ti[1, 0], Ti[0, 0])
    best = None
    for yaw in yaws:
        poses = np.stack([pts[0], pts[1], pts[2], np.full(gx.size, float(roll)), np.full(gx.size, float(pitch)),
                          np.full(gx.size, float(yaw) + dyaw)])
        r = engine.pose_information(poses, beam_angles, sigma, r_max, sensor_offset, delta_xy, delta_yaw, jump_max)
        cur = dict(crlb_strong=r.crlb_strong, crlb_weak=r.crlb_weak, weak_axis=r.weak_axis, hit_share=r.hit_share)
        if best is None:
            best = cur
        else:
            worse = cur['crlb_weak'] > best['crlb_weak']
            for k in best:
                best[k] = np.where(worse, cur[k], best[k])
    out = dict((k, v.reshape(ny, nx)) for k, v in best.items())
    out['x'], out['y'] = xs, ys
    return out


def merge_weight_stats(parts):
    """statistics of the union of several shards' WeightStats, in the order given (mcl_weight_stats_merge: host only)"""
    lib = _lib.load()
    arr = (_lib.WStats * len(parts))(*[p.as_c() if isinstance(p, WeightStats) else p for p in parts])
    out = _lib.WStats()
    _lib.check(lib.mcl_weight_stats_merge(arr, len(parts), C.byref(out)))
    return WeightStats(out)


def group_resample(engines, uniforms=None, normals_per_shard=None):
    lib = _lib.load()
    ns = len(engines)
    hs = (C.c_void_p * ns)(*[e.h for e in engines])
    u = None if uniforms is None else _f64(np.atleast_1d(uniforms))
    keep = None
    nzp = None
    if normals_per_shard is not None:
        keep = [_f64(a) for a in normals_per_shard]
        nzp = (C.c_void_p * ns)(*[a.ctypes.data for a in keep])
    _lib.check(lib.mcl_group_resample(hs, ns, _ptr(u), 0 if u is None else u.size, nzp), engines[0].h)


def group_step_mbes(engines, v, wz, q, z, dt, ranges, beam_angles, sigma, r_max, sensor_offset=None):
    """one fused step of a LOCAL group of shards (mcl_group_step_mbes); read the result with
    engines[0].last_mean_cov()"""
    lib = _lib.load()
    ns = len(engines)
    hs = (C.c_void_p * ns)(*[e.h for e in engines])
    od = make_odom(v, wz, q, z)
    r, a, so = _f32(ranges), _f32(beam_angles), _f64(sensor_offset)
    _lib.check(lib.mcl_group_step_mbes(hs, ns, C.byref(od), float(dt), _ptr(r), _ptr(a), a.size, float(sigma),
                                       float(r_max), _ptr(so)), engines[0].h)


def group_step_mbes_landmarks(engines, v, wz, q, z, dt, ranges, beam_angles, sigma, r_max, det_xyz, lm_sigma, k=1,
                              gate=11.345, sensor_offset=None, lm_sensor_offset=None):
    """group_step_mbes with the landmark observation of the ping on top (mcl_group_step_mbes_landmarks)"""
    lib = _lib.load()
    ns = len(engines)
    hs = (C.c_void_p * ns)(*[e.h for e in engines])
    od = make_odom(v, wz, q, z)
    r, a, so = _f32(ranges), _f32(beam_angles), _f64(sensor_offset)
    d, lso = _f64(det_xyz), _f64(lm_sensor_offset)
    _lib.check(lib.mcl_group_step_mbes_landmarks(hs, ns, C.byref(od), float(dt), _ptr(r), _ptr(a), a.size, float(sigma),
                                                 float(r_max), _ptr(so), _ptr(d), d.shape[0], float(lm_sigma), int(k),
                                                 float(gate), _ptr(lso)), engines[0].h)


def group_mean_cov(engines):
    lib = _lib.load()
    ns = len(engines)
    hs = (C.c_void_p * ns)(*[e.h for e in engines])
    mean, yaw, cov = np.zeros(6), np.zeros(1), np.zeros(9)
    _lib.check(lib.mcl_group_mean_cov(hs, ns, _ptr(mean), _ptr(yaw), _ptr(cov)), engines[0].h)
    return mean, float(yaw[0]), cov


def resample_indices(weights, uniforms, scheme=SYSTEMATIC, device=0):
    """resampling.py free-function form on the GPU (fixed-point CDF)."""
    lib = _lib.load()
    w = _f64(weights)
    u = _f64(np.atleast_1d(uniforms))
    out = np.zeros(w.size, np.int32)
    _lib.check(lib.mcl_resample_indices(int(scheme), _ptr(w), w.size, _ptr(u), u.size, int(device), _ptr(out)))
    return out
