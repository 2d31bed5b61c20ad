"""GPU tests of the delayed acoustic updates (include/mcl_acoustic.h; csrc/mcl_acoustic.h): a position fix and slant
ranges to fixed transponders, evaluated at the pose each particle's ancestor had when the measurement was taken.

The reference has no symbol for any of this.  The oracle is a numpy restatement of the header's definition, in this file:
the lineage as tests/test_gpu_history.py restates it (resampling.slot_ancestors(engine.last_indices()) composed across
resamples and records), the frames as get_particles() gave them at each record, the pose rule (lag, frac, the wrapped yaw
interpolation), the transponder position and the two likelihoods.  It shares nothing with the device code.  Tolerances:
rtol 1e-10 (what tests/test_gpu_parity.py asks of the GPS weights) plus atol 1e-9."""
import math

import numpy as np
import pytest

from smarc_navigation_amd import resampling, synth

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -5
RTOL, ATOL = 1e-10, 1e-9
N = 1000        # neither a multiple of 64 nor of the 256-thread block; four blocks
COV = dict(init_cov=[4.0, 4.0, 0.0, 0.0, 0.0, 0.04], process_cov=[1e-2, 1e-2, 0.0, 0.0, 0.0, 1e-4],
           resample_cov=[1e-2, 1e-2, 0.0, 0.0, 0.0, 1e-4])
M2O = synth.rigid_matrix(5.0, -3.0, 2.0, 0.1, -0.2, 0.7)      # a rotation about every axis: the z column is not zero
OFFSET = [0.4, -0.25, 0.6]
Q0 = [0.0, 0.0, 0.0, 1.0]


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


# ------------------------------------------------------------------ the definition, restated
def wrap(d):
    return d - 2.0 * np.pi * np.ceil((d - np.pi) / (2.0 * np.pi))


class Lineage(object):
    """link, frames and a_k of include/mcl_history.h and the pose rule of include/mcl_acoustic.h in numpy"""

    def __init__(self, n, depth):
        self.n, self.depth = n, depth
        self.link = np.arange(n, dtype=np.int64)
        self.frames = []        # (parent, xyw (3, n), stamp), oldest first, at most depth

    def resample(self, indices):
        self.link = self.link[resampling.slot_ancestors(indices).astype(np.int64)]

    def record(self, soa, stamp):
        self.frames.append((self.link.copy(), soa[[0, 1, 5]].copy(), float(stamp)))
        self.frames = self.frames[-self.depth:]
        self.link = np.arange(self.n, dtype=np.int64)

    def ancestors(self, lag):
        a = self.link
        for j in range(lag):
            a = self.frames[-1 - j][0][a]
        return a

    def pose(self, soa_now, lag, frac=0.0):
        """x, y, yaw (n each) the measurement is evaluated at"""
        if lag < 0:
            return soa_now[0], soa_now[1], soa_now[5]
        a = self.ancestors(lag)
        x, y, yaw = self.frames[-1 - lag][1][:, a]
        if frac > 0.0:
            a1 = self.frames[-1 - lag][0][a]
            x1, y1, yaw1 = self.frames[-2 - lag][1][:, a1]
            x, y, yaw = x + frac * (x1 - x), y + frac * (y1 - y), yaw + frac * wrap(yaw1 - yaw)
        return x, y, yaw


def transponder(m2o, x, y, yaw, z, roll, pitch, offset=None):
    """p (3, n) = m2o [x y z 1]' + Rm R(roll, pitch, yaw) offset; z, roll, pitch scalars or arrays"""
    n = len(x)
    z, roll, pitch = [np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in (z, roll, pitch)]
    p = m2o[:3, :3].dot(np.stack([x, y, z])) + m2o[:3, 3:4]
    if offset is not None:
        cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
        R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                      [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                      [-sp, cp * sr, cp * cr]])                       # (3, 3, n): rot_rpy
        p = p + m2o[:3, :3].dot(np.einsum('ijn,j->in', R, np.asarray(offset, dtype=np.float64)))
    return p


def fix_term(p, xy, cov3):
    xx, xy_, yy = cov3
    S = np.array([[xx, xy_], [xy_, yy]])
    d = np.asarray(xy, dtype=np.float64)[:, None] - p[:2]
    return -0.5 * np.einsum('in,ij,jn->n', d, np.linalg.inv(S), d) - 0.5 * math.log((2.0 * math.pi) ** 2 * np.linalg.det(S))


def beacon_term(p, beacons, ranges, sigma):
    out, n_valid = np.zeros(p.shape[1]), 0
    for b, r in zip(np.asarray(beacons, dtype=np.float64).reshape(-1, 3), ranges):
        if not r > 0.0:      # (NaN fails the test)
            continue
        out += ((r - np.sqrt(np.sum((p - b[:, None]) ** 2, axis=0))) / sigma) ** 2
        n_valid += 1
    return -0.5 * out - n_valid * math.log(sigma * math.sqrt(2.0 * math.pi))


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def cloud(n, seed, yaw_centre=0.0, spread=6.0):
    rs = np.random.RandomState(seed)
    soa = np.zeros((6, n))
    soa[0], soa[1] = 40.0 + spread * rs.randn(n), -25.0 + spread * rs.randn(n)
    soa[2], soa[3], soa[4] = -3.0 + 0.5 * rs.randn(n), 0.1 * rs.randn(n), 0.1 * rs.randn(n)
    soa[5] = synth.wrap_pi(yaw_centre + 0.4 * rs.randn(n))
    return soa


# ------------------------------------------------------------------ 1: the fix at the current state
def test_isotropic_fix_at_the_current_state_is_the_gps_update(eng):
    for m2o in (None, M2O):
        e = eng.Engine(N, seed=3, meas_std=0.5, m2o=m2o, **COV)
        e.set_particles(cloud(N, 1))
        e.update_gps(43.5, -21.25)
        want = e.get_log_weights()
        e.update_fix([43.5, -21.25], 0.5)
        got = e.get_log_weights()
        assert np.std(want) > 1.0
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=0.0)
        # the three ways to say the same covariance
        for cov in ([0.25, 0.0, 0.25], [[0.25, 0.0], [0.0, 0.25]]):
            e.update_fix([43.5, -21.25], cov)
            assert np.array_equal(e.get_log_weights(), got)
        e.close()


@pytest.mark.parametrize('own_zrp', [True, False])
@pytest.mark.parametrize('offset', [None, OFFSET])
def test_general_covariance_and_m2o_against_numpy(offset, own_zrp, eng):
    e = eng.Engine(N, seed=4, m2o=M2O, **COV)
    soa = cloud(N, 2)
    e.set_particles(soa)
    cov3, xy = [2.5, -0.9, 0.8], [38.0, -20.0]
    zrp = None if own_zrp else [-2.75, 0.15, -0.1]
    e.update_fix(xy, cov3, offset=offset, zrp=zrp)
    z, roll, pitch = (soa[2], soa[3], soa[4]) if own_zrp else zrp
    want = fix_term(transponder(M2O, soa[0], soa[1], soa[5], z, roll, pitch, offset), xy, cov3)
    assert np.std(want) > 1.0
    close(e.get_log_weights(), want)
    e.update_fix(xy, np.array([[2.5, -0.9], [-0.9, 0.8]]), offset=offset, zrp=zrp)
    close(e.get_log_weights(), want)
    with pytest.raises(ValueError):
        e.update_fix(xy, [[2.5, -0.9], [0.9, 0.8]])
    e.close()


# ------------------------------------------------------------------ 2: the lagged fix across a ring that wraps
def resample_round(e, ref, rs, scale=2.0):
    e.set_log_weights(scale * rs.randn(ref.n))
    e.resample()
    ref.resample(e.last_indices())


def record_round(e, ref, stamp):
    ref.record(e.get_particles(), stamp)
    e.history_record(stamp)


def check_every_lag(e, ref, zrp, offset, xy, cov3):
    held = e.history_frames()[0]
    assert held == len(ref.frames)
    crossed = 0
    for lag in range(held):
        for frac in (0.0, 0.37):
            if frac > 0.0 and lag + 1 >= held:
                continue
            x, y, yaw = ref.pose(None, lag, frac)
            want = fix_term(transponder(M2O, x, y, yaw, zrp[0], zrp[1], zrp[2], offset), xy, cov3)
            e.update_fix(xy, cov3, offset=offset, zrp=zrp, lag=lag, frac=frac)
            close(e.get_log_weights(), want)
            if frac > 0.0:
                a = ref.ancestors(lag)
                d = ref.frames[-2 - lag][1][2][ref.frames[-1 - lag][0][a]] - ref.frames[-1 - lag][1][2][a]
                crossed += int(np.count_nonzero(np.abs(d) > np.pi))
    return crossed


@pytest.mark.parametrize('scheme', ['SYSTEMATIC', 'RESIDUAL'])
def test_lagged_fix_across_a_wrapping_ring(scheme, eng):
    """depth 4, 7 records, 0 / 1 / 3 resamples and a predict between records; after each record, and again after one more
    resample (a link that is not the identity), every valid lag with frac 0 and 0.37.  The yaws straddle +-pi and the
    vehicle turns, so lineages cross the branch cut between frames; lever arm, roll and pitch are not zero."""
    e = eng.Engine(N, seed=5, m2o=M2O, resample_scheme=getattr(eng, scheme), **COV)
    e.set_particles(cloud(N, 3, yaw_centre=np.pi))
    e.history_enable(4)
    ref = Lineage(N, 4)
    rs = np.random.RandomState(6)
    zrp, cov3 = [-2.5, 0.12, -0.08], [1.5, 0.6, 2.0]
    crossed = 0
    for r, between in enumerate([0, 1, 3, 0, 1, 3, 1]):
        for _ in range(between):
            resample_round(e, ref, rs)
        e.predict([1.5, 0.1, 0.0], 0.25 if r % 2 else -0.3, Q0, -2.5, 0.8)
        record_round(e, ref, 10.0 + r)
        xy = M2O[:2, :2].dot([40.0 + r, -25.0]) + M2O[:2, 3]
        crossed += check_every_lag(e, ref, zrp, OFFSET, xy, cov3)
        resample_round(e, ref, rs)
        assert np.any(ref.link != np.arange(N))
        crossed += check_every_lag(e, ref, zrp, OFFSET if r % 2 else None, xy, cov3)
    assert e.history_frames()[:2] == (4, 7)
    assert crossed > 0          # the wrapped interpolation was exercised
    e.close()


# ------------------------------------------------------------------ 3: beacon ranges
BEACONS = np.array([[60.0, -10.0, -30.0], [10.0, -40.0, -28.0], [45.0, 5.0, -31.0], [80.0, -60.0, -25.0], [20.0, 20.0, -29.0],
                    [55.0, -45.0, -33.0], [30.0, -5.0, -27.0], [70.0, -30.0, -26.0]])


def true_ranges(n_b, at=(50.0, -30.0, -1.0)):
    return np.sqrt(np.sum((BEACONS[:n_b] - np.asarray(at)) ** 2, axis=1)) + 0.3


@pytest.mark.parametrize('n_b', [1, 3, 8])
def test_beacon_ranges_at_the_particles_own_pose(n_b, eng):
    """lag = -1, zrp = None: per-particle z, roll, pitch after set_particles; the odometry's on every particle after a
    predict; one NaN and one negative range are skipped"""
    e = eng.Engine(N, seed=7, m2o=M2O, **COV)
    soa = cloud(N, 4)
    e.set_particles(soa)
    r = true_ranges(n_b)
    if n_b >= 3:
        r[1] = np.nan
    if n_b == 8:
        r[6] = -4.0
    for offset in (None, OFFSET):
        e.update_beacon_ranges(BEACONS[:n_b], r, 0.8, offset=offset)
        want = beacon_term(transponder(M2O, soa[0], soa[1], soa[5], soa[2], soa[3], soa[4], offset), BEACONS[:n_b], r, 0.8)
        assert np.std(want) > 1.0
        close(e.get_log_weights(), want)
    e.predict([1.0, 0.0, 0.0], 0.1, [0.05, -0.03, 0.0, 0.998], -4.5, 0.5)
    now = e.get_particles()
    assert np.all(now[2] == -4.5) and np.ptp(now[3]) == 0.0 and now[3][0] != 0.0
    e.update_beacon_ranges(BEACONS[:n_b], r, 0.8, offset=OFFSET)
    close(e.get_log_weights(), beacon_term(transponder(M2O, now[0], now[1], now[5], now[2], now[3], now[4], OFFSET),
                                           BEACONS[:n_b], r, 0.8))
    # zrp given: the same three numbers on every particle instead of its own
    e.set_particles(soa)
    e.update_beacon_ranges(BEACONS[:n_b], r, 0.8, offset=OFFSET, zrp=[-2.0, 0.2, 0.1])
    close(e.get_log_weights(), beacon_term(transponder(M2O, soa[0], soa[1], soa[5], -2.0, 0.2, 0.1, OFFSET), BEACONS[:n_b], r, 0.8))
    e.close()


def test_all_ranges_invalid_in_both_modes(eng):
    e = eng.Engine(N, seed=8, **COV)
    e.set_particles(cloud(N, 5))
    before = np.random.RandomState(1).randn(N)
    e.set_log_weights(before)
    e.update_beacon_ranges(BEACONS[:3], [np.nan, -1.0, 0.0], 0.5, accumulate=True)
    assert np.array_equal(e.get_log_weights(), before)
    e.update_beacon_ranges(BEACONS[:3], [np.nan, -1.0, 0.0], 0.5, accumulate=False)
    assert np.array_equal(e.get_log_weights(), np.zeros(N))
    e.close()


def test_lagged_beacon_ranges(eng):
    e = eng.Engine(N, seed=9, m2o=M2O, **COV)
    e.set_particles(cloud(N, 6, yaw_centre=-np.pi))
    e.history_enable(3)
    ref = Lineage(N, 3)
    rs = np.random.RandomState(7)
    for r in range(3):
        resample_round(e, ref, rs)
        e.predict([1.2, 0.0, 0.0], 0.2, Q0, -3.0, 1.0)
        record_round(e, ref, float(r))
    resample_round(e, ref, rs)
    rng = true_ranges(4)
    rng[2] = np.nan
    zrp = [-3.0, 0.05, 0.1]
    for lag, frac, offset in ((0, 0.0, None), (1, 0.37, OFFSET), (2, 0.0, OFFSET), (0, 0.6, None)):
        x, y, yaw = ref.pose(None, lag, frac)
        e.update_beacon_ranges(BEACONS[:4], rng, 1.1, offset=offset, zrp=zrp, lag=lag, frac=frac)
        close(e.get_log_weights(), beacon_term(transponder(M2O, x, y, yaw, zrp[0], zrp[1], zrp[2], offset), BEACONS[:4], rng, 1.1))
    e.close()


# ------------------------------------------------------------------ 4: accumulate and bookkeeping
def test_accumulate_adds_and_replace_replaces(eng):
    e = eng.Engine(N, seed=10, **COV)
    soa = cloud(N, 7)
    e.set_particles(soa)
    term = fix_term(transponder(np.identity(4), soa[0], soa[1], soa[5], soa[2], soa[3], soa[4]), [41.0, -24.0], [1.0, 0.0, 1.0])
    before = 3.0 * np.random.RandomState(2).randn(N)
    e.set_log_weights(before)
    e.update_fix([41.0, -24.0], 1.0, accumulate=True)
    close(e.get_log_weights(), before + term)
    e.update_beacon_ranges(BEACONS[:2], true_ranges(2), 2.0, accumulate=True)
    close(e.get_log_weights(), before + term + beacon_term(transponder(np.identity(4), soa[0], soa[1], soa[5], soa[2], soa[3], soa[4]),
                                                           BEACONS[:2], true_ranges(2), 2.0))
    e.update_fix([41.0, -24.0], 1.0, accumulate=False)
    close(e.get_log_weights(), term)
    e.close()


def test_resample_after_a_fix_only_update_is_the_fixed_point_systematic(eng, orc):
    """the update must say that the maximum of the weights before it is stale (weights_written): a larger maximum is
    left behind by weight_stats on purpose"""
    e = eng.Engine(N, seed=11, **COV)
    e.init_particles()
    e.set_log_weights(50.0 + np.random.RandomState(3).randn(N))
    assert e.weight_stats().max_lw > 45.0
    e.update_fix([0.5, -0.25], 0.6)
    lw = e.get_log_weights()
    assert np.isfinite(lw).all() and np.std(lw) > 1.0 and lw.max() < 45.0
    e.resample()
    ref, _, _ = orc.systematic_fixed(lw, 1, orc.native_u53(11, 0))
    assert np.array_equal(e.last_indices(), ref)
    e.close()


def lagged_run(eng):
    e = eng.Engine(N, seed=12, m2o=M2O, **COV)
    e.init_particles()
    e.history_enable(3)
    out = []
    for r in range(4):
        e.predict([1.5, 0.0, 0.0], 0.1, Q0, -2.0, 1.0)
        e.update_fix([6.0 + r, -2.0], [0.8, 0.1, 0.5], zrp=None)
        e.resample()
        e.history_record(float(r))
        if r >= 2:
            e.update_fix([5.5 + r, -2.5], [0.8, 0.1, 0.5], offset=OFFSET, zrp=[-2.0, 0.02, 0.01], lag=1, frac=0.25)
            out.append(e.get_log_weights())
            e.update_beacon_ranges(BEACONS[:3], [70.0, 55.0, 60.0], 1.5, zrp=[-2.0, 0.02, 0.01], lag=0, accumulate=True)
            out.append(e.get_log_weights())
            e.resample()
    out.append(e.get_particles())
    return e, out


def test_two_identical_runs_agree_bit_for_bit(eng):
    a, x = lagged_run(eng)
    b, y = lagged_run(eng)
    assert len(x) == 5
    for k, (p, q) in enumerate(zip(x, y)):
        assert np.array_equal(p.view(np.uint64), q.view(np.uint64)), k
    a.close()
    b.close()


def test_the_updates_write_the_weights_and_nothing_else(eng):
    e, _ = lagged_run(eng)
    e.timing_enable(True)
    e.timing_get()
    state, frames = e.get_particles(), e.history_frames()
    anc = [e.history_ancestors(k) for k in range(frames[0])]
    path = e.history_path(N - 1, frames[0])
    e.update_fix([9.0, -2.0], 0.7, offset=OFFSET, zrp=[-2.0, 0.0, 0.1], lag=2)
    e.update_fix([9.0, -2.0], 0.7, zrp=[-2.0, 0.0, 0.1], lag=1, frac=0.9, accumulate=True)
    e.update_beacon_ranges(BEACONS, true_ranges(8), 0.9, lag=-1, accumulate=True)
    e.update_beacon_ranges(BEACONS, true_ranges(8), 0.9, offset=OFFSET, zrp=[-2.0, 0.0, 0.1], lag=0, frac=0.5)
    assert np.array_equal(e.get_particles().view(np.uint64), state.view(np.uint64))
    after = e.history_frames()
    assert after[:2] == frames[:2] and np.array_equal(after[2], frames[2])
    for k in range(frames[0]):
        assert np.array_equal(e.history_ancestors(k), anc[k])
    again = e.history_path(N - 1, frames[0])
    assert np.array_equal(again[0], path[0]) and np.array_equal(again[1], path[1])
    # one timed region per update, under the GPS update's counter; nothing else was launched on their behalf
    t = e.timing_get()
    assert t['update_gps'][1] == 4
    assert sum(v[1] for k, v in t.items()) == 4
    e.close()


# ------------------------------------------------------------------ 5: errors
def raises(eng, status, call):
    with pytest.raises(eng.MclError) as ei:
        call()
    assert ei.value.status == status, ei.value


def test_every_refusal_and_the_call_after_it(eng):
    e = eng.Engine(N, seed=13, **COV)
    soa = cloud(N, 8)
    e.set_particles(soa)
    zrp, nan, inf = [-2.0, 0.0, 0.0], float('nan'), float('inf')
    want = fix_term(transponder(np.identity(4), soa[0], soa[1], soa[5], soa[2], soa[3], soa[4]), [40.0, -25.0], [1.0, 0.0, 1.0])

    def still_works():
        e.update_fix([40.0, -25.0], 1.0)
        close(e.get_log_weights(), want)

    def refused(status, call):
        raises(eng, status, call)
        still_works()

    # nothing to accumulate onto (no update has written weights since the particles were set)
    fresh = eng.Engine(64, seed=1, **COV)
    fresh.init_particles()
    raises(eng, ERR_STATE, lambda: fresh.update_fix([0.0, 0.0], 1.0, accumulate=True))
    raises(eng, ERR_STATE, lambda: fresh.update_beacon_ranges(BEACONS[:1], [50.0], 1.0, accumulate=True))
    fresh.update_fix([0.0, 0.0], 1.0)
    fresh.update_fix([0.0, 0.0], 1.0, accumulate=True)
    fresh.close()
    # history is off
    refused(ERR_STATE, lambda: e.update_fix([40.0, -25.0], 1.0, zrp=zrp, lag=0))
    refused(ERR_STATE, lambda: e.update_beacon_ranges(BEACONS[:2], [50.0, 60.0], 1.0, zrp=zrp, lag=0))
    # the pose arguments
    refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], 1.0, lag=-2))
    refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], 1.0, frac=-0.1))
    refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], 1.0, frac=1.0))
    refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], 1.0, frac=nan))
    refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], 1.0, frac=0.5))          # nothing to move towards at lag -1
    refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], 1.0, zrp=[nan, 0.0, 0.0]))
    refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], 1.0, offset=[0.0, inf, 0.0]))
    e.history_enable(4)
    refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], 1.0, zrp=zrp, lag=0))    # enabled, but no frame held yet
    e.history_record(0.0)
    e.history_record(1.0)
    e.update_fix([40.0, -25.0], 1.0, zrp=zrp, lag=1)
    e.update_fix([40.0, -25.0], 1.0, zrp=zrp, lag=0, frac=0.5)
    refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], 1.0, zrp=zrp, lag=2))
    refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], 1.0, zrp=zrp, lag=1, frac=0.5))    # lag + 1 is not held
    refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], 1.0, zrp=None, lag=0))             # frames hold no z, roll, pitch
    refused(ERR_INVALID, lambda: e.update_beacon_ranges(BEACONS[:2], [50.0, 60.0], 1.0, zrp=zrp, lag=2))
    refused(ERR_INVALID, lambda: e.update_beacon_ranges(BEACONS[:2], [50.0, 60.0], 1.0, zrp=zrp, lag=1, frac=0.5))
    refused(ERR_INVALID, lambda: e.update_beacon_ranges(BEACONS[:2], [50.0, 60.0], 1.0, zrp=None, lag=1))
    # the fix
    for cov in ([0.0, 0.0, 1.0], [-1.0, 0.0, -1.0], [1.0, 1.0, 1.0], [1.0, 2.0, 1.0], [nan, 0.0, 1.0], [1.0, 0.0, inf], 0.0):
        refused(ERR_INVALID, lambda: e.update_fix([40.0, -25.0], cov))
    refused(ERR_INVALID, lambda: e.update_fix([nan, -25.0], 1.0))
    refused(ERR_INVALID, lambda: e.update_fix([40.0, inf], 1.0))
    # the ranges
    refused(ERR_INVALID, lambda: e.update_beacon_ranges(np.zeros((0, 3)), [], 1.0))
    refused(ERR_INVALID, lambda: e.update_beacon_ranges(np.zeros((9, 3)), np.ones(9), 1.0))
    refused(ERR_INVALID, lambda: e.update_beacon_ranges(BEACONS[:2], [50.0, 60.0], 0.0))
    refused(ERR_INVALID, lambda: e.update_beacon_ranges(BEACONS[:2], [50.0, 60.0], nan))
    refused(ERR_INVALID, lambda: e.update_beacon_ranges([[nan, 0.0, 0.0]], [50.0], 1.0))
    refused(ERR_INVALID, lambda: e.update_beacon_ranges(BEACONS[:2], [50.0, inf], 1.0))
    e.update_beacon_ranges(BEACONS[:2], [50.0, 60.0], 1.0, zrp=zrp, lag=1)
    # after history is switched off the lagged form is a state error again, the current-state form still works
    e.history_disable()
    refused(ERR_STATE, lambda: e.update_fix([40.0, -25.0], 1.0, zrp=zrp, lag=0))
    e.close()


def test_a_shard_takes_the_current_state_form(eng):
    """lag = -1 is a function of the particle alone: a handle of a sharded cloud takes it; lag >= 0 needs history, which
    such a handle cannot enable"""
    shard = eng.Engine(256, rank=1, world=2, n_global=512, global_offset=256, **COV)
    soa = cloud(256, 9)
    shard.set_particles(soa)
    shard.update_fix([40.0, -25.0], [1.5, 0.3, 0.9], offset=OFFSET)
    close(shard.get_log_weights(), fix_term(transponder(np.identity(4), soa[0], soa[1], soa[5], soa[2], soa[3], soa[4], OFFSET),
                                            [40.0, -25.0], [1.5, 0.3, 0.9]))
    raises(eng, ERR_STATE, lambda: shard.update_fix([40.0, -25.0], 1.0, zrp=[0.0, 0.0, 0.0], lag=0))
    shard.close()


# ------------------------------------------------------------------ 6: it does what it is for
def test_a_late_fix_is_applied_where_the_vehicle_was(eng):
    """the cloud is recorded, moves d = 6 m (four 1 s predicts at 1.5 m/s, no process noise: exact), then a fix of the
    RECORDED-TIME truth arrives (std 0.5).  Evaluated at lag 0 the weighted mean of the CURRENT particles lands within
    sigma / 2 = 0.25 m of truth + d; evaluated against the current cloud it lands more than d / 2 = 3 m away.  (A numpy
    simulation of this setup over 20 seeds gave at most 0.072 m for the former and at least 5.78 m for the latter.)"""
    n, d, sigma = 4096, 6.0, 0.5
    truth = np.array([12.0, -7.0])
    rs = np.random.RandomState(14)
    soa = np.zeros((6, n))
    soa[0], soa[1] = truth[0] + 3.0 * rs.randn(n), truth[1] + 3.0 * rs.randn(n)
    soa[2] = -2.0
    e = eng.Engine(n, seed=14, process_cov=[0.0] * 6, resample_cov=[0.0] * 6)
    e.set_particles(soa)
    e.history_enable(2)
    e.history_record(100.0)
    for _ in range(4):
        e.predict([1.5, 0.0, 0.0], 0.0, Q0, -2.0, 1.0)
    now = e.get_particles()
    np.testing.assert_allclose(now[0] - soa[0], d, rtol=0, atol=1e-9)

    def weighted_mean():
        lw = e.get_log_weights()
        w = np.exp(lw - lw.max())
        return np.array([np.sum(w * now[0]), np.sum(w * now[1])]) / np.sum(w)

    e.update_fix(truth, sigma, zrp=[-2.0, 0.0, 0.0], lag=0)
    lagged = np.linalg.norm(weighted_mean() - (truth + [d, 0.0]))
    e.update_fix(truth, sigma, lag=-1)
    naive = np.linalg.norm(weighted_mean() - (truth + [d, 0.0]))
    print('late fix: lagged %.3f m, naive %.3f m from truth + d' % (lagged, naive))
    assert lagged <= sigma / 2.0
    assert naive > d / 2.0
    e.close()


# ------------------------------------------------------------------ 7: node and replay
def straight_stream(steps=240, dt=0.125, speed=1.5, t0=100.0):
    """constant velocity along x, level, with truth: what the odometry integrates to, exactly"""
    k = np.arange(steps)
    stamp = t0 + (k + 1) * dt
    truth = np.stack([speed * (k + 1) * dt, np.zeros(steps), np.full(steps, -2.0)], axis=1)
    return dict(stamp=stamp, t0=t0, v=np.tile([speed, 0.0, 0.0], (steps, 1)), wz=np.zeros(steps), q=np.tile(Q0, (steps, 1)),
                z=np.full(steps, -2.0), truth_xyz=truth)


NODE = dict(particle_count=2048, seed=15, init_covariance='[0.25, 0.25, 0.0, 0.0, 0.0, 0.0]',
            motion_covariance='[0.0004, 0.0004, 0.0, 0.0, 0.0, 0.0]',
            resampling_noise_covariance='[0.01, 0.01, 0.0, 0.0, 0.0, 0.0]', fix_topic='/sam/external/uw_gps_odom', fix_std=0.5)


def test_replay_with_late_fixes_needs_the_history(eng):
    """latency 4 s at 1.5 m/s = 6 m = 12 sigma: applied to the past the fixes keep the track, applied to the present they
    drag it back"""
    from smarc_navigation_amd import replay
    st = straight_stream()
    runs = {}
    for depth in (8, 0):
        out = replay.replay(st, dict(NODE, fix_history_depth=depth), fix_period=1.0, fix_latency=4.0, fix_seed=1)
        runs[depth] = out['summary']
        print(depth, out['summary'])
    with_history, without = runs[8], runs[0]
    assert with_history['fixes_applied'] > 0 and with_history['fixes_dropped'] == 0
    assert without['fixes_applied'] == with_history['fixes_applied']
    assert with_history['fix_mean_lag'] == 4.0                    # (every time of this stream is a multiple of 1 / 8 s)
    assert with_history['pf_rmse_vs_truth'] < without['pf_rmse_vs_truth']
    with pytest.raises(ValueError):
        replay.replay(st, dict(NODE, fix_history_depth=8), fix_period=1.0, fix_latency=4.0, smooth_lag=4)


def test_the_node_drops_what_is_older_than_the_ring_or_too_old(eng):
    from smarc_navigation_amd import auv_pf, msgs
    st = straight_stream(steps=130)
    pf = auv_pf.auv_pf(dict(NODE, fix_history_depth=2, fix_max_age=10.0))
    pf.start_timing(st['t0'])

    def fix(stamp, x):
        m = msgs.Odometry()
        m.header = msgs.Header('map', msgs.Time(stamp))
        m.pose.pose.position.x = x
        pf.fix_cb(m)

    for k in range(60):
        pf.odom_callback(msgs.odometry_from_stream(st, k))
    # 107.5 s; frames so far: the keep-alive ones, fix_max_age / depth = 5 s apart
    assert pf.particles.history_frames()[2].tolist() == [105.0, 100.0]
    fix(103.0, 4.5)                                    # inside the ring: applied, resampled, recorded
    assert (pf.fixes_applied, pf.fixes_dropped) == (1, 0)
    assert pf.particles.history_frames()[2].tolist() == [107.5, 105.0]
    fix(104.0, 6.0)                                    # older than the ring's oldest frame now
    assert (pf.fixes_applied, pf.fixes_dropped) == (1, 1)
    for k in range(60, 130):
        pf.odom_callback(msgs.odometry_from_stream(st, k))
    assert pf.time == 116.25 and pf.particles.history_frames()[2].tolist() == [112.5, 107.5]
    fix(102.0, 3.0)                                    # older than fix_max_age
    assert (pf.fixes_applied, pf.fixes_dropped) == (1, 2)
    fix(114.0, 1.5 * 14.0)                             # newer than the newest frame: the cloud as it is
    assert (pf.fixes_applied, pf.fixes_dropped) == (2, 2)
    assert pf.fix_lag_sum == 4.5 + 2.25
    pf.particles.close()


def test_two_resamplings_between_two_odometry_messages_leave_one_frame_of_that_stamp(eng):
    """the filter's clock moves with the odometry alone: two fixes in a row are two resamplings at ONE stamp.  The ring
    keeps strictly decreasing stamps (what mcl_history_bracket asks for) and the fixes after them are still applied."""
    from smarc_navigation_amd import auv_pf, msgs
    st = straight_stream(steps=40)
    pf = auv_pf.auv_pf(dict(NODE, fix_history_depth=4, fix_max_age=10.0))
    pf.start_timing(st['t0'])

    def fix(stamp):
        m = msgs.Odometry()
        m.header = msgs.Header('map', msgs.Time(stamp))
        m.pose.pose.position.x = 1.5 * (stamp - st['t0'])
        pf.fix_cb(m)

    for k in range(16):
        pf.odom_callback(msgs.odometry_from_stream(st, k))
    assert pf.time == 102.0
    fix(101.0)
    fix(101.5)                                   # a second resampling at 102.0: no second frame of that stamp
    stamps = pf.particles.history_frames()[2]
    assert stamps.tolist() == [102.0, 100.0]
    for k in range(16, 24):
        pf.odom_callback(msgs.odometry_from_stream(st, k))
    fix(101.75)                                  # bracketed between 102.0 and 100.0: the link carried both resamplings
    fix(102.5)
    assert (pf.fixes_applied, pf.fixes_dropped) == (4, 0)
    assert np.all(np.diff(pf.particles.history_frames()[2]) < 0)
    pf.particles.close()


def test_replay_with_a_map_pings_and_fixes_arriving_with_a_ping(eng):
    """the configuration the node is meant for: a map, a resampling on every ping, and late fixes that arrive in the same
    step as a ping (ping and fix resample at one stamp).  Every fix is applied, none raises, none is dropped."""
    from smarc_navigation_amd import replay
    st = straight_stream(steps=160)
    origin = (-32.0, -64.0)
    z = synth.bathymetry_grid(128, 128, 1.0, origin, seed=1)
    ba = synth.beam_angles(16)
    one = eng.Engine(1)
    one.set_map_grid(z, origin, 1.0)
    idx, ranges = np.arange(0, 160, 2), []
    for k in idx:
        soa = np.zeros((6, 1))
        soa[:3, 0] = st['truth_xyz'][k]
        one.set_particles(soa)
        ranges.append(one.mbes_expected(0, 1, ba, 60.0)[0])
    one.close()
    st.update(mbes_idx=idx, mbes_ranges=np.array(ranges), mbes_angles=ba, mbes_range_max=60.0)
    # fixes are taken at samples 8, 16, ... and arrive 2 s = 16 samples later: always with a ping (even samples)
    out = replay.replay(st, dict(NODE, fix_history_depth=16, mbes_std=0.5), grid=dict(z=z, origin=origin, res=1.0),
                        fix_period=1.0, fix_latency=2.0, fix_seed=2)
    s = out['summary']
    print(s)
    assert (s['fixes_applied'], s['fixes_dropped'], s['fix_mean_lag']) == (17, 0, 2.0)
    assert s['pf_rmse_vs_truth'] < 1.0
