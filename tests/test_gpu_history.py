"""GPU tests of the particle genealogy and the fixed-lag smoother (include/mcl_history.h; csrc/mcl_history.h).

The reference is numpy alone: resampling.slot_ancestors(engine.last_indices()) -- the slot map A of every resample, from
the ancestor vector the library has always reported -- composed across resamples and records exactly as the header
defines link, parent and a_k.  It shares nothing with the new device code.  Every link comparison is EXACT.  The
smoother's counts and n_unique are exact; its moments are compared with math.fsum sums within SURVEY 8(d)'s parity
tolerances, as tests/test_gpu_modes.py does: means and yaw_R 1e-9 absolute, cov_xy 1e-9 relative + 1e-12 absolute, the yaw
as a wrapped difference and only where the resultant is not zero."""
import math
import os
import re

import numpy as np
import pytest

from smarc_navigation_amd import resampling, synth

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV = dict(init_cov=[1.0, 1.0, 0.0, 0.0, 0.0, 0.01], process_cov=[1e-4, 1e-4, 0.0, 0.0, 0.0, 1e-6],
           resample_cov=[1e-3, 1e-3, 0.0, 0.0, 0.0, 1e-5])


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def rs_tile():
    """the particles one k_cdf_expand workgroup expands: RS_BLOCK * RS_ITEMS (csrc/mcl_resample.h, mcl_kernels.h)"""
    src = open(os.path.join(ROOT, 'smarc_navigation_amd', 'csrc', 'mcl_resample.h')).read()
    ker = open(os.path.join(ROOT, 'smarc_navigation_amd', 'csrc', 'mcl_kernels.h')).read()
    block = int(re.search(r'#define\s+RS_BLOCK\s+(\d+)', src).group(1))
    assert re.search(r'#define\s+RS_ITEMS\s+MCL_SCAN_ITEMS\b', src)
    return block * int(re.search(r'#define\s+MCL_SCAN_ITEMS\s+(\d+)', ker).group(1))


# ------------------------------------------------------------------ the definition, restated
class Lineage(object):
    """link, frames and a_k of include/mcl_history.h in numpy"""

    def __init__(self, n, depth):
        self.n, self.depth = n, depth
        self.link = np.arange(n, dtype=np.int64)
        self.frames = []        # (parent, xyw (3, n), stamp), oldest first, at most depth
        self.recorded = 0

    def resample(self, indices):
        a = resampling.slot_ancestors(indices).astype(np.int64)
        self.link = self.link[a]
        return a

    def record(self, soa, stamp):
        self.frames.append((self.link.copy(), soa[[0, 1, 5]].copy(), float(stamp)))
        self.frames = self.frames[-self.depth:]
        self.link = np.arange(self.n, dtype=np.int64)
        self.recorded += 1

    def ancestors(self, lag):
        a = self.link
        for j in range(lag):
            a = self.frames[-1 - j][0][a]
        return a

    def smooth(self, lag):
        c = np.bincount(self.ancestors(lag), minlength=self.n)
        x, y, yaw = self.frames[-1 - lag][1]
        n, w = float(self.n), c.astype(np.float64)
        dx, dy = x - x[0], y - y[0]
        mdx, mdy = math.fsum(w * dx) / n, math.fsum(w * dy) / n
        ss, sc = math.fsum(w * np.sin(yaw)), math.fsum(w * np.cos(yaw))
        return dict(counts=c, n_unique=int(np.count_nonzero(c)), x=x[0] + mdx, y=y[0] + mdy, yaw=math.atan2(ss, sc),
                    yaw_R=math.hypot(ss, sc) / n, resultant=math.hypot(ss, sc), stamp=self.frames[-1 - lag][2],
                    cov_xy=np.array([math.fsum(w * dx * dx) / n - mdx * mdx, math.fsum(w * dx * dy) / n - mdx * mdy,
                                     math.fsum(w * dy * dy) / n - mdy * mdy]))


def check_lineage(e, ref, slots=None):
    """frames, every valid lag's ancestors and a handful of paths against the numpy lineage; exact"""
    held, recorded, stamps = e.history_frames()
    assert held == len(ref.frames) and recorded == ref.recorded
    assert stamps.tolist() == [f[2] for f in reversed(ref.frames)]
    for k in range(held):
        got = e.history_ancestors(k)
        assert got.dtype == np.uint32
        assert np.array_equal(got, ref.ancestors(k)), 'lag %d of %d' % (k, held)
    n = ref.n
    for s in sorted(set([0, n - 1, n // 2, n // 3, (7 * n) // 8]) if slots is None else slots):
        xyw, sl = e.history_path(s, held)
        for k in range(held):
            a = int(ref.ancestors(k)[s])
            assert int(sl[k]) == a, (s, k)
            want = ref.frames[-1 - k][1][:, a]
            assert xyw[k].view(np.uint64).tolist() == want.view(np.uint64).tolist(), (s, k)    # the bits get_particles gave


def resample_round(e, ref, rs, scale=2.0):
    e.set_log_weights(scale * rs.randn(ref.n))
    e.resample()
    return ref.resample(e.last_indices())


def record_round(e, ref, stamp):
    ref.record(e.get_particles(), stamp)
    e.history_record(stamp)


def make(eng, n, depth, seed=7, **kw):
    e = eng.Engine(n, seed=seed, **dict(COV, **kw))
    e.init_particles()
    e.history_enable(depth)
    return e, Lineage(n, depth)


# ------------------------------------------------------------------ 1, 2: lineage of the systematic pipeline
@pytest.mark.parametrize('n', [1000, 1, 63, 64, 65, 'tile+1'])
def test_lineage_of_six_systematic_resamples(n, eng):
    n = rs_tile() + 1 if n == 'tile+1' else n
    e, ref = make(eng, n, 8)
    rs = np.random.RandomState(n)
    lost = 0
    for r in range(6):
        a = resample_round(e, ref, rs)
        lost += int(np.count_nonzero(a != np.arange(n)))
        record_round(e, ref, 10.0 + r)
        check_lineage(e, ref)
    assert n < 3 or lost > 0            # the resamples did move particles
    e.close()


# ------------------------------------------------------------------ 3: extremes
def test_one_heavy_particle_takes_every_slot(eng):
    """one log-weight 0, the rest -1e3: the whole-workgroup expansion of one ancestor (k_cdf_expand)"""
    n = rs_tile() + 300
    e, ref = make(eng, n, 4)
    record_round(e, ref, 0.0)
    heavy = 777
    lw = np.full(n, -1e3)
    lw[heavy] = 0.0
    e.set_log_weights(lw)
    e.resample()
    a = ref.resample(e.last_indices())
    assert np.all(a == heavy)
    record_round(e, ref, 1.0)
    resample_round(e, ref, np.random.RandomState(2))
    record_round(e, ref, 2.0)
    check_lineage(e, ref)
    assert np.all(e.history_ancestors(2) == heavy)
    est = e.history_smooth(3)
    assert [s.n_unique for s in est[1:]] == [ref.smooth(1)['n_unique'], 1]
    assert est[2].n_unique == 1 and est[0].n_unique == n
    # the smoothed pose at the oldest frame is that one particle's
    x, y, yaw = ref.frames[0][1][:, heavy]
    assert abs(est[2].x - x) <= 1e-9 and abs(est[2].y - y) <= 1e-9 and abs(est[2].yaw_R - 1.0) <= 1e-9
    assert abs(math.remainder(est[2].yaw - yaw, 2 * math.pi)) <= 1e-9
    e.close()


def test_equal_weights_keep_every_lineage(eng):
    n = 1000
    e, ref = make(eng, n, 4)
    record_round(e, ref, 0.0)
    for r in range(2):
        e.set_log_weights(np.zeros(n))
        e.resample()
        a = ref.resample(e.last_indices())
        assert np.array_equal(a, np.arange(n))
        record_round(e, ref, 1.0 + r)
    check_lineage(e, ref)
    for k in range(3):
        assert np.array_equal(e.history_ancestors(k), np.arange(n, dtype=np.uint32))
    assert [s.n_unique for s in e.history_smooth(3)] == [n, n, n]
    e.close()


# ------------------------------------------------------------------ 4: zero and several resamples between two records
def test_zero_and_three_resamples_between_records(eng):
    n = 1000
    e, ref = make(eng, n, 8)
    rs = np.random.RandomState(3)
    record_round(e, ref, 0.0)
    record_round(e, ref, 1.0)                  # nothing in between: parent = identity
    assert np.array_equal(ref.frames[-1][0], np.arange(n))
    check_lineage(e, ref)
    for _ in range(3):
        resample_round(e, ref, rs)
        check_lineage(e, ref)                  # the link between records is visible at lag 0
    record_round(e, ref, 2.0)
    check_lineage(e, ref)
    resample_round(e, ref, rs)
    e.predict([1.0, 0.0, 0.0], 0.1, [0.0, 0.0, 0.0, 1.0], -2.0, 0.02)     # predicts and updates do not touch the link
    e.update_gps(0.3, -0.2)
    check_lineage(e, ref)
    e.resample()
    ref.resample(e.last_indices())
    record_round(e, ref, 3.0)
    check_lineage(e, ref)
    assert len(set(ref.ancestors(3).tolist())) < len(set(ref.ancestors(1).tolist())) < n
    e.close()


# ------------------------------------------------------------------ 5: ring wrap
def test_ring_of_three_frames_after_eight_records(eng):
    n = 500
    e, ref = make(eng, n, 3)
    rs = np.random.RandomState(4)
    for r in range(8):
        resample_round(e, ref, rs, scale=1.0)
        record_round(e, ref, 100.0 + r)
    held, recorded, stamps = e.history_frames()
    assert (held, recorded) == (3, 8) and stamps.tolist() == [107.0, 106.0, 105.0]
    check_lineage(e, ref)
    for call in (lambda: e.history_ancestors(3), lambda: e.history_smooth(4), lambda: e.history_path(0, 4),
                 lambda: e.history_ancestors(-1), lambda: e.history_smooth(0), lambda: e.history_path(n, 1),
                 lambda: e.history_path(-1, 1)):
        with pytest.raises(eng.MclError) as ei:
            call()
        assert ei.value.status == ERR_INVALID
    e.close()


# ------------------------------------------------------------------ 6: the explicit-index schemes
@pytest.mark.parametrize('scheme', ['RESIDUAL', 'STRATIFIED', 'MULTINOMIAL', 'NAIVE'])
def test_lineage_of_the_other_schemes(scheme, eng):
    n = 1000
    e, ref = make(eng, n, 8, resample_scheme=getattr(eng, scheme))
    rs = np.random.RandomState(5)
    unordered = False
    for r in range(4):
        resample_round(e, ref, rs)
        unordered |= bool(np.any(np.diff(e.last_indices()) < 0))
        if r != 1:                              # (one pair of resamples without a record between them)
            record_round(e, ref, float(r))
        check_lineage(e, ref)
    if scheme in ('STRATIFIED', 'NAIVE'):
        assert not unordered                    # one ascending sweep of the CDF
    if scheme == 'MULTINOMIAL':
        assert unordered                        # independent draws: the slot map of an UNORDERED ancestor vector
    est = e.history_smooth(3)
    assert [s.n_unique for s in est] == [ref.smooth(k)['n_unique'] for k in range(3)]
    e.close()


# ------------------------------------------------------------------ 7: the fused step
GRID_ORIGIN = (-32.0, -32.0)


@pytest.fixture(scope='module')
def small_grid():
    return synth.bathymetry_grid(64, 64, 1.0, GRID_ORIGIN, seed=1)


def _ping16():
    ba = synth.beam_angles(16)
    return ba, (18.0 / np.cos(ba)).astype(np.float32)


@pytest.mark.parametrize('visit', [False, True])
def test_fused_step_lineage(visit, eng, small_grid, monkeypatch):
    if visit:
        monkeypatch.setenv('MCL_SWEEP', '1')
        monkeypatch.setenv('MCL_VISIT', '1')
    n = 4096
    e = eng.Engine(n, seed=9, **COV)
    e.set_map_grid(small_grid, GRID_ORIGIN, 1.0)
    e.init_particles()
    e.history_enable(4)
    ref = Lineage(n, 4)
    ba, ranges = _ping16()
    st = synth.odom_stream(10)
    sorted_steps = 0
    for k in range(10):
        e.step_mbes(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], st['dt'], ranges, ba, 0.5, 60.0)
        sorted_steps += int(e.mbes_visit_order()[1])
        ref.resample(e.last_indices())
        record_round(e, ref, st['stamp'][k])
        check_lineage(e, ref, slots=(0, n - 1, 1234))
    assert sorted_steps == (9 if visit else 0)      # (the first step has no gather behind it)
    assert ref.smooth(3)['n_unique'] < n
    e.close()


@pytest.mark.parametrize('visit', [False, True])
def test_fused_step_of_a_static_vehicle_copies_the_ancestors_bits(visit, eng, small_grid, monkeypatch):
    """zero process and resample covariance, zero twist: slot i of the new state IS the old state's slot A(i), so the link
    is checked against the particle states alone (mcl_get_last_indices is not involved)"""
    if visit:
        monkeypatch.setenv('MCL_SWEEP', '1')
        monkeypatch.setenv('MCL_VISIT', '1')
    n = 4096
    zero = [0.0] * 6
    e = eng.Engine(n, seed=10, init_cov=[1.0, 1.0, 0.0, 0.0, 0.0, 0.01], process_cov=zero, resample_cov=zero)
    e.set_map_grid(small_grid, GRID_ORIGIN, 1.0)
    e.init_particles()
    ba, ranges = _ping16()
    q = [0.0, 0.0, 0.0, 1.0]
    # (the first predict rounds yaw + pi - pi once; from then on every yaw is a fixed point of it)
    e.predict([0.0, 0.0, 0.0], 0.0, q, -2.0, 0.02)
    e.history_enable(2)
    e.history_record(0.0)
    moved = 0
    for k in range(10):
        prev = e.get_particles()[[0, 1, 5]]
        e.step_mbes([0.0, 0.0, 0.0], 0.0, q, -2.0, 0.02, ranges, ba, 2.0, 60.0)
        a = e.history_ancestors(0).astype(np.int64)          # link = A: the record before it reset the link
        cur = e.get_particles()[[0, 1, 5]]
        assert np.array_equal(cur.view(np.uint64), prev[:, a].view(np.uint64)), k
        moved += int(np.count_nonzero(a != np.arange(n)))
        e.history_record(1.0 + k)
    assert moved > 0
    e.close()


# ------------------------------------------------------------------ 8: the filter does not notice
def test_filter_is_bitwise_the_same_with_history_and_launches_return_after_disable(eng, small_grid):
    n = 4096
    ba, ranges = _ping16()
    st = synth.odom_stream(12)

    def step(e, k):
        e.step_mbes(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], st['dt'], ranges, ba, 0.5, 60.0)

    def run(history):
        e = eng.Engine(n, seed=11, **COV)
        e.set_map_grid(small_grid, GRID_ORIGIN, 1.0)
        e.init_particles()
        if history:
            e.history_enable(4)
        out = []
        for k in range(10):
            step(e, k)
            if history:
                e.history_record(float(k))
                held = e.history_frames()[0]
                e.history_ancestors(held - 1)
                e.history_smooth(held)
                e.history_path(n - 1, held)
            mean, yaw, cov = e.last_mean_cov()
            out.append(dict(st=e.get_particles(), lw=e.get_log_weights(), idx=e.last_indices(), mean=mean, yaw=yaw, cov=cov))
        return e, out

    a, with_history = run(True)
    b, without = run(False)
    for k, (x, y) in enumerate(zip(with_history, without)):
        for key in ('st', 'lw', 'idx', 'mean', 'cov'):
            assert np.array_equal(x[key], y[key]), (k, key)
        assert x['yaw'] == y['yaw'], k
    # history on: one more timed region (the compose) per step; disabled again: a never-enabled handle's launches
    # (mcl_timing.launches counts TIMED REGIONS: what is compared is the regions a step opens, not every kernel in them)
    for e in (a, b):
        e.timing_enable(True)
        e.timing_get()
    step(a, 10)
    step(b, 10)
    on, off = a.timing_get(), b.timing_get()
    assert {k: v[1] for k, v in on.items()} == dict({k: v[1] for k, v in off.items()}, resample=off['resample'][1] + 1)
    a.history_disable()
    step(a, 11)
    step(b, 11)
    on, off = a.timing_get(), b.timing_get()
    assert {k: v[1] for k, v in on.items()} == {k: v[1] for k, v in off.items()}
    assert np.array_equal(a.get_particles(), b.get_particles())
    with pytest.raises(eng.MclError) as ei:
        a.history_frames()
    assert ei.value.status == ERR_STATE
    a.close()
    b.close()


# ------------------------------------------------------------------ 9: smoothing
def wrapped(a, b):
    return abs(math.remainder(a - b, 2 * math.pi))


@pytest.mark.parametrize('n', [1000, 4097])
def test_smoothed_estimates_against_numpy(n, eng):
    e, ref = make(eng, n, 8, init_cov=[4.0, 9.0, 0.0, 0.0, 0.0, 0.5])
    rs = np.random.RandomState(6)
    e.predict([1.0, 0.0, 0.0], 0.1, [0.0, 0.0, 0.0, 1.0], -2.0, 400.0)      # away from the origin: x ~ 400 m
    for r in range(6):
        resample_round(e, ref, rs, scale=1.5)
        if r == 3:
            resample_round(e, ref, rs, scale=1.5)
        record_round(e, ref, 50.0 + r)
    # lag 0 right after a record is the cloud's mean
    est = e.history_smooth(6)
    mean = e.mean_cov()[0]
    assert abs(est[0].x - mean[0]) <= 1e-9 and abs(est[0].y - mean[1]) <= 1e-9
    assert est[0].n_unique == n
    # ... and after one more resample (link != identity) every lag against numpy
    resample_round(e, ref, rs, scale=1.5)
    est = e.history_smooth(6)
    again = e.history_smooth(6)
    uniq = []
    for k in range(6):
        want, got = ref.smooth(k), est[k]
        counts = np.bincount(e.history_ancestors(k), minlength=n)
        assert np.array_equal(counts, want['counts']) and int(counts.sum()) == n
        assert got.lag == k and got.stamp == want['stamp']
        assert got.n_unique == want['n_unique']
        assert abs(got.x - want['x']) <= 1e-9 and abs(got.y - want['y']) <= 1e-9, (k, got, want)
        assert np.all(np.abs(got.cov_xy - want['cov_xy']) <= 1e-9 * np.abs(want['cov_xy']) + 1e-12), (k, got.cov_xy, want['cov_xy'])
        assert abs(got.yaw_R - want['yaw_R']) <= 1e-9
        if want['resultant'] > 0.0:
            assert wrapped(got.yaw, want['yaw']) <= 1e-9
        assert got.as_dict() == again[k].as_dict() and got.cov_xy.tobytes() == again[k].cov_xy.tobytes()   # bit for bit
        uniq.append(got.n_unique)
    assert uniq == sorted(uniq, reverse=True) and uniq[-1] < uniq[0] < n     # lineages coalesce going back
    # a prefix of the lags is the same walk
    short = e.history_smooth(2)
    assert [s.as_dict() for s in short] == [s.as_dict() for s in est[:2]]
    e.close()


# ------------------------------------------------------------------ 10: status codes
def test_status_codes(eng, small_grid):
    n = 256
    e = eng.Engine(n, seed=1, **COV)
    for call in (e.history_frames, lambda: e.history_ancestors(0), lambda: e.history_smooth(1), lambda: e.history_path(0, 1),
                 e.history_reset, lambda: e.history_record(0.0)):
        with pytest.raises(eng.MclError) as ei:
            call()
        assert ei.value.status == ERR_STATE                  # not enabled
    e.history_disable()                                      # (nothing to do: fine)
    for depth in (0, -1, 1025):
        with pytest.raises(eng.MclError) as ei:
            e.history_enable(depth)
        assert ei.value.status == ERR_INVALID
    e.history_enable(4)
    assert e.history_bytes(4) == 28 * n * 4 + 16 * n + 80 * 4 + 131072
    with pytest.raises(eng.MclError) as ei:
        e.history_record(0.0)                                # no particles yet
    assert ei.value.status == ERR_STATE
    assert e.history_frames()[:2] == (0, 0)
    with pytest.raises(eng.MclError) as ei:
        e.history_ancestors(0)                               # no frame yet
    assert ei.value.status == ERR_INVALID
    e.init_particles()
    ref = Lineage(n, 4)
    rs = np.random.RandomState(8)
    for r in range(3):
        resample_round(e, ref, rs)
        record_round(e, ref, float(r))
    check_lineage(e, ref)
    # injection keeps the lineage: a replaced particle inherits its slot's past
    e.set_map_grid(small_grid, GRID_ORIGIN, 1.0)
    assert e.inject_uniform(0.5) > 0
    check_lineage(e, ref)
    resample_round(e, ref, rs)
    record_round(e, ref, 3.0)
    check_lineage(e, ref)
    # reset: a clean cut
    e.history_reset()
    assert e.history_frames()[:2] == (0, 0)
    ref = Lineage(n, 4)
    resample_round(e, ref, rs)          # composed onto the identity
    record_round(e, ref, 4.0)
    check_lineage(e, ref)
    # every re-initialisation clears the frames and the link, history stays enabled
    for reinit in (e.init_particles, lambda: e.init_particles_uniform(), lambda: e.set_particles(np.zeros((6, n)))):
        resample_round(e, ref, rs)
        reinit()
        assert e.history_frames()[:2] == (0, 0)
        ref = Lineage(n, 4)
        record_round(e, ref, 5.0)
        assert np.array_equal(e.history_ancestors(0), np.arange(n, dtype=np.uint32))
        check_lineage(e, ref)
    # enable on an enabled handle starts over with the new depth
    e.history_enable(2)
    assert e.history_frames()[:2] == (0, 0)
    e.close()
    shard = eng.Engine(256, rank=1, world=2, n_global=512, global_offset=256)
    with pytest.raises(eng.MclError) as ei:
        shard.history_enable(4)
    assert ei.value.status == ERR_UNSUPPORTED
    shard.close()


def test_comm_local_handle_is_refused(eng):
    """a handle created for a LOCAL group (comm_mode = MCL_COMM_LOCAL, world 2), through the C ABI"""
    import ctypes
    from smarc_navigation_amd import _lib
    lib = _lib.load()
    cfg = _lib.Config()
    cfg.n_particles, cfg.n_global, cfg.global_offset = 256, 512, 0
    cfg.device, cfg.rank, cfg.world, cfg.comm_mode = 0, 0, 2, 2
    cfg.m2o[:] = [float(v) for v in np.identity(4).reshape(-1)]
    h = ctypes.c_void_p()
    assert lib.mcl_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    assert lib.mcl_history_enable(h, 4) == ERR_UNSUPPORTED
    assert lib.mcl_history_frames(h, None, None, None) == ERR_STATE
    assert lib.mcl_history_enable(None, 4) == ERR_INVALID
    lib.mcl_destroy(h)


# ------------------------------------------------------------------ 11: replay
def test_replay_emits_a_smoothed_track_and_is_unchanged_without_it(small_grid):
    from smarc_navigation_amd import replay
    s = synth.odom_stream(90)
    st = dict(stamp=s['stamp'], v=s['v'], wz=s['wz'], q=s['q'], z=s['z'], t0=s['t0'], truth_xyz=s['truth'][:, :3])
    ang = synth.beam_angles(16)
    st['mbes_idx'] = np.arange(5, 90, 8)                      # 11 pings
    st['mbes_angles'] = ang
    st['mbes_ranges'] = (18.0 / np.cos(ang))[None, :].repeat(len(st['mbes_idx']), axis=0).astype(np.float32)
    st['mbes_range_max'] = 60.0
    grid = dict(z=small_grid, origin=GRID_ORIGIN, res=1.0)
    params = dict(particle_count=512, seed=4, init_covariance='[0.5, 0.5, 0.0, 0.0, 0.0, 0.01]',
                  motion_covariance='[0.001, 0.001, 0.0, 0.0, 0.0, 0.00001]', mbes_std=1.0)
    plain = replay.replay(st, params, grid=grid)
    zero = replay.replay(st, params, grid=grid, smooth_lag=0)
    lag4 = replay.replay(st, params, grid=grid, smooth_lag=4)
    assert 'smooth' not in plain and 'smooth' not in zero
    assert np.array_equal(plain['pf_xyz'], zero['pf_xyz']) and plain['summary'] == zero['summary']
    assert np.array_equal(plain['pf_xyz'], lag4['pf_xyz'])    # the filter does not notice
    tr = lag4['smooth']
    m = len(st['mbes_idx'])
    assert tr['idx'].tolist() == st['mbes_idx'].tolist() and tr['lag'] == 4
    assert tr['filtered_xyyaw'].shape == (m, 3) and tr['smoothed_xyyaw'].shape == (m, 3) and tr['n_unique'].shape == (m,)
    assert np.isfinite(tr['filtered_xyyaw']).all() and np.isfinite(tr['smoothed_xyyaw']).all()
    assert np.all(tr['n_unique'] >= 1) and np.all(tr['n_unique'] <= 512)
    # the newest ping has nothing after it: smoothed = filtered there; an entry finalised at lag 4 has lost lineages
    assert np.array_equal(tr['smoothed_xyyaw'][-1], tr['filtered_xyyaw'][-1]) and tr['n_unique'][-1] == 512
    assert tr['n_unique'][0] < 512
    for key in ('smooth_lag', 'smooth_pings', 'smooth_n_unique_min', 'filtered_rmse_vs_truth', 'smoothed_rmse_vs_truth'):
        assert key in lag4['summary'], key
    assert lag4['summary']['smooth_pings'] == m


def test_smooth_track_marks_the_pings_a_reinitialisation_cut_off(eng):
    """replay's SmoothTrack over an engine whose particles are re-initialised in mid-stream: the ring is cleared, the pings
    that were still in the window keep their filtered pose (n_unique = -1) and the two tracks stay aligned"""
    from smarc_navigation_amd import replay
    n = 256
    e = eng.Engine(n, seed=3, **COV)
    e.init_particles()
    tr = replay.SmoothTrack(e, 2)
    rs = np.random.RandomState(9)

    def ping(k):
        e.set_log_weights(2.0 * rs.randn(n))
        e.resample()
        tr.record(k, 10.0 + k)

    for k in range(3):
        ping(k)                    # the third record fills the window: ping 0 is final
    e.init_particles()
    for k in range(3, 5):
        ping(k)
    out = tr.finish()
    e.close()
    assert out['idx'].tolist() == [0, 1, 2, 3, 4]
    assert out['filtered_xyyaw'].shape == out['smoothed_xyyaw'].shape == (5, 3) and np.isfinite(out['smoothed_xyyaw']).all()
    nu = out['n_unique'].tolist()
    assert 1 <= nu[0] <= n and nu[1:3] == [-1, -1] and 1 <= nu[3] <= n and nu[4] == n
    assert np.array_equal(out['smoothed_xyyaw'][1:3], out['filtered_xyyaw'][1:3])
    assert np.array_equal(out['smoothed_xyyaw'][4], out['filtered_xyyaw'][4])
