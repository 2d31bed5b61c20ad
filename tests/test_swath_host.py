"""CPU tests of the swath matching (include/mcl_swath.h): every symbol of the header exported and bound in a table of its
own, the offset record, mcl_swath_offsets against a numpy restatement, the device-free solve / better / derived bit for bit
against the restatement of tests/test_match_host.py (imported, not edited) up to n = 16384 and the largest legal sums, the
restated loop over K pings on the fp64 oracle's casts rounded to fp32 -- the along-track scene where one ping slides along
its valley and two do not, a flat seabed, a ridge along the track, a turning track on rough terrain -- and the stand-alone
sanitizer driver.  The restatement here (compose, SwathEval) is what tests/test_gpu_swath.py compares the kernel with.

The compositions of a ping's pose use Python's sin and cos; the device uses its own.  So nothing here is compared with the
device's poses bit for bit: the integers are, over the ranges the device cast (tests/test_gpu_swath.py)."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from smarc_navigation_amd import synth
from tests.test_innovation_host import SIGMA, scene, scene_map
from tests.test_match_host import (BC_RMAX, CONVERGED, D_MAX, ERR_INVALID, GRID_N, GRID_ORIGIN, J0, J_MAX, J_MIN, RHO_MAX, TRUTH,
                                   OracleEval, _bits, better_ref, c_cfg, default_cfg, derived_ref, flat_grid, loop_ref, m_of,
                                   packed, random_record, rec_array, record_of, ridge_grid, solve_ref, starts_of, sums_ref,
                                   variants)
from tests.test_innovation_host import M2O, OFF, R_MAX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mcl_swath_offsets', 'mcl_swath_check', 'mcl_swath_solve', 'mcl_swath_better', 'mcl_swath_derived', 'mcl_match_swath')
MAX_PINGS, MAX_BEAMS = 64, 16384


# ------------------------------------------------------------------ the restatement of include/mcl_swath.h
def offsets_ref(poses6, anchor=-1):
    """mcl_swath_offsets in numpy: one operation at a time"""
    p = np.asarray(poses6, np.float64).reshape(6, -1)
    K = p.shape[1]
    a = K - 1 if anchor < 0 else anchor
    s, c = math.sin(p[5, a]), math.cos(p[5, a])
    out = []
    for k in range(K):
        u, w = p[0, k] - p[0, a], p[1, k] - p[1, a]
        t = p[5, k] - p[5, a]
        if not -math.pi <= t < math.pi:
            t = math.fmod(t + math.pi, 2.0 * math.pi)
            t = (t + 2.0 * math.pi if t < 0.0 else t) - math.pi
        out.append((c * u + s * w, c * w - s * u, p[2, k] - p[2, a], p[3, k], p[4, k], t) if k != a else (0.0, 0.0, 0.0, p[3, k], p[4, k], 0.0))
    return out


def compose(v6, off):
    """the pose of a ping from a variant of the anchor (6: x, y, z, -, -, yaw) and its offset (dx, dy, dz, roll, pitch, dyaw):
    the definition's four lines; an exactly zero offset keeps the variant's bits"""
    x, y, z, yaw = float(v6[0]), float(v6[1]), float(v6[2]), float(v6[5])
    dx, dy, dz, roll, pitch, dyaw = [float(v) for v in off]
    if dx != 0.0 or dy != 0.0:
        s, c = math.sin(yaw), math.cos(yaw)
        x, y = x + (c * dx - s * dy), y + (s * dx + c * dy)
    if dz != 0.0:
        z = z + dz
    if dyaw != 0.0:
        yaw = yaw + dyaw
    return [x, y, z, roll, pitch, yaw]


def ping_poses(anchor6, offsets, cfg):
    """6 x (K NV): the poses the K pings are cast from at the 1 + 2 D variants of the anchor, ping-major"""
    v = variants(anchor6, cfg)
    return np.array([compose(v[:, i], off) for off in offsets for i in range(v.shape[1])]).T


def add_records(recs):
    recs = list(recs)
    return (sum(r[0] for r in recs), sum(r[1] for r in recs), sum(r[2] for r in recs),
            tuple(sum(r[3][e] for r in recs) for e in range(10)), tuple(sum(r[4][e] for r in recs) for e in range(4)),
            sum(r[5] for r in recs), sum(r[6] for r in recs))


def swath_sums_ref(meas, rng, cfg, r_max):
    """the record of a swath from its K x B ranges and the K x NV x B ranges of one evaluation: sums_ref per ping, added"""
    meas = np.asarray(meas, np.float32)
    return add_records(sums_ref(meas[k], rng[k], cfg, r_max) for k in range(meas.shape[0]))


class SwathEval(object):
    """evaluate(anchor pose6) over the fp64 oracle: its ranges at the composed poses rounded to float32, then the sums"""

    def __init__(self, omap, ba, meas, offsets, cfg, m2o, off, r_max):
        from oracle import oracle as orc
        self.orc, self.omap, self.ba, self.meas, self.offsets, self.cfg = orc, omap, ba, np.asarray(meas, np.float32), list(offsets), cfg
        self.m2o, self.off, self.r_max, self.seen = m2o, off, r_max, {}

    def __call__(self, pose6):
        key = tuple(float(v) for v in pose6)
        if key not in self.seen:
            K, nv = len(self.offsets), 1 + 2 * self.cfg['dims']
            p = np.ascontiguousarray(ping_poses(pose6, self.offsets, self.cfg))
            e = self.orc.mbes_update(p, self.m2o, self.off, self.omap, self.ba, None, SIGMA, self.r_max)[1].astype(np.float32)
            self.seen[key] = swath_sums_ref(self.meas, e.reshape(K, nv, -1), self.cfg, self.r_max)
        return self.seen[key]


def swath_pings(omap, anchor6, offsets, ba, m2o, off, r_max):
    """the K x B ranges the vehicle measures with its anchor at anchor6 (fp64 oracle, rounded to float32)"""
    from oracle import oracle as orc
    p = np.array([compose(anchor6, o) for o in offsets]).T
    return orc.mbes_update(np.ascontiguousarray(p), m2o, off, omap, ba, None, SIGMA, r_max)[1].astype(np.float32)


def swath_rules():
    """(solve, better) with the signatures of solve_ref / better_ref, decided by mcl_swath_solve / mcl_swath_better"""
    from smarc_navigation_amd import engine

    def solve(rec, cfg, j):
        delta, dead = engine.swath_solve(rec_array(rec), c_cfg(cfg), j)
        return [float(v) for v in delta], dead

    def better(q, p, min_beams):
        return engine.swath_better(rec_array(q), rec_array(p), min_beams)
    return solve, better


def loop_both(evaluate, pose6, cfg):
    """the restated loop, and once more with the library's mcl_swath_* deciding every step: the same bits"""
    mine = loop_ref(evaluate, pose6, cfg)
    theirs = loop_ref(evaluate, pose6, cfg, *swath_rules())
    assert repr(mine) == repr(theirs)
    return mine


def straight_offsets(K, spacing=2.0, roll=0.0, pitch=0.0):
    """K pings `spacing` apart along the anchor's heading, the newest (the anchor) last"""
    return [(-spacing * (K - 1 - k), 0.0, 0.0, roll, pitch, 0.0) for k in range(K)]


# ------------------------------------------------------------------ the scenes (1 m grids, identity m2o, no sensor offset)
TRACK_TRUTH = np.array([3.125, -2.25, -2.0, 0.0, 0.0, 0.0])
TRACK_START = TRACK_TRUTH + np.array([1.5, 0.0, 0.4, 0.0, 0.0, 0.0])
IDENT, NO_OFF = np.identity(4), [0.0] * 6


def track_grid():
    """heights that depend on x only: what a ping across the track cannot tell from depth"""
    ix = np.arange(GRID_N, dtype=np.float64) + GRID_ORIGIN[0]
    return np.repeat((-20.0 + 3.0 * np.sin(ix / 6.0) + 0.05 * ix)[:, None], GRID_N, axis=1).astype(np.float32)


_CACHE = {}


def track_reference(K, dims=4):
    """the restated loop on the along-track scene with K pings 2 m apart -- computed once, shared with the GPU tests"""
    if ('track', K, dims) not in _CACHE:
        from oracle import oracle as orc
        omap = orc.Grid(track_grid(), GRID_ORIGIN, 1.0)
        ba = synth.beam_angles(64)
        cfg = default_cfg(dims=dims, jump_max=BC_RMAX)
        offsets = straight_offsets(K)
        meas = swath_pings(omap, TRACK_TRUTH, offsets, ba, IDENT, NO_OFF, BC_RMAX)
        ev = SwathEval(omap, ba, meas, offsets, cfg, IDENT, NO_OFF, BC_RMAX)
        _CACHE[('track', K, dims)] = dict(cfg=cfg, ba=ba, meas=meas, offsets=offsets, omap=omap, run=loop_both(ev, TRACK_START, cfg))
    return _CACHE[('track', K, dims)]


TURN_K = 4


def turning_offsets():
    """a turning track: four pings on an arc, each with its own roll and pitch, anchored at the newest"""
    from smarc_navigation_amd import engine
    k = np.arange(TURN_K, dtype=np.float64)
    yaw = TRUTH[5] - 0.12 * (TURN_K - 1 - k)
    p = np.stack([TRUTH[0] - 2.5 * (TURN_K - 1 - k) * np.cos(yaw), TRUTH[1] - 2.5 * (TURN_K - 1 - k) * np.sin(yaw),
                  TRUTH[2] + 0.15 * (TURN_K - 1 - k), 0.01 + 0.02 * np.sin(k), -0.02 + 0.015 * np.cos(2.0 * k), yaw])
    return [tuple(float(v) for v in o) for o in engine.swath_offsets(p)]


def turning_reference(dims, kind='grid'):
    """the restated loop from every start of starts_of(dims) on the rough scene of tests/test_match_host.py with the
    turning track -- computed once, shared with the GPU tests"""
    if ('turn', dims, kind) not in _CACHE:
        z, origin, _ = scene()
        _, omap = scene_map(kind, z, origin)
        ba = synth.beam_angles(64, 1.0)
        cfg = default_cfg(dims=dims)
        offsets = turning_offsets()
        meas = swath_pings(omap, TRUTH, offsets, ba, M2O, OFF, R_MAX)
        ev = SwathEval(omap, ba, meas, offsets, cfg, M2O, OFF, R_MAX)
        starts = starts_of(dims)
        _CACHE[('turn', dims, kind)] = dict(cfg=cfg, ba=ba, meas=meas, offsets=offsets, omap=omap, starts=starts,
                                            runs=[loop_both(ev, starts[:, k], cfg) for k in range(starts.shape[1])])
    return _CACHE[('turn', dims, kind)]


# ------------------------------------------------------------------ the ABI
@pytest.fixture(scope='module')
def lib():
    from smarc_navigation_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def test_every_symbol_of_the_header_is_exported_and_bound_in_a_table_of_its_own(lib):
    from smarc_navigation_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'mcl_swath.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(NAMES) == sorted(_lib.SWATH_SYMBOLS)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    assert not set(_lib.MATCH_SYMBOLS) & set(NAMES) and not set(_lib.SYMBOLS) & set(NAMES)
    assert lib.mcl_abi_version() == 4
    assert ctypes.sizeof(_lib.Timing) == 15 * 16                 # no timing slot was added
    for other in ('mcl.h', 'mcl_match.h'):
        assert 'swath' not in open(os.path.join(ROOT, 'include', other)).read()          # the existing headers are what they were


def test_the_offset_record_has_the_declared_size_and_offsets(eng):
    o = eng.SwathOffset
    assert o.itemsize == 48 and [o.fields[f][1] for f in ('dx', 'dy', 'dz', 'roll', 'pitch', 'dyaw')] == [0, 8, 16, 24, 32, 40]
    src = open(os.path.join(ROOT, 'include', 'mcl_swath.h')).read()
    assert re.search(r'typedef struct mcl_swath_offset \{', src)
    assert '#define MCL_SWATH_MAX_PINGS 64' in src and '#define MCL_SWATH_MAX_BEAMS 16384' in src
    assert eng.SWATH_MAX_PINGS == MAX_PINGS and eng.SWATH_MAX_BEAMS == MAX_BEAMS


# ------------------------------------------------------------------ the offsets
def test_offsets_equal_the_numpy_restatement_and_compose_back_to_the_poses(eng):
    rs = np.random.RandomState(3)
    for K in (1, 2, 3, 9, 64):
        p = np.stack([rs.uniform(-300, 300, K), rs.uniform(-300, 300, K), rs.uniform(-20, 0, K), rs.uniform(-0.2, 0.2, K),
                      rs.uniform(-0.2, 0.2, K), rs.uniform(-math.pi, math.pi, K)])
        for anchor in sorted({-1, 0, K // 2, K - 1}):
            got = eng.swath_offsets(p, anchor)
            want = offsets_ref(p, anchor)
            a = K - 1 if anchor < 0 else anchor
            assert [tuple(_bits(v) for v in g) for g in got.tolist()] == [tuple(_bits(v) for v in w) for w in want], (K, anchor)
            assert got[a].tolist() == (0.0, 0.0, 0.0, p[3, a], p[4, a], 0.0)
            assert [_bits(v) for v in got[a].tolist()[:3]] == [_bits(0.0)] * 3 and _bits(got[a]['dyaw']) == _bits(0.0)     # +0.0, not -0.0
            for k in range(K):
                back = compose(p[:, a], got[k].tolist())
                assert abs(back[0] - p[0, k]) < 1e-12 and abs(back[1] - p[1, k]) < 1e-12 and abs(back[2] - p[2, k]) < 1e-12
                assert back[3] == p[3, k] and back[4] == p[4, k]
                assert abs(math.remainder(back[5] - p[5, k], 2.0 * math.pi)) < 1e-12
            assert eng.swath_check(K, 8, got) is None


def test_offsets_of_a_yaw_pair_across_pi_are_the_short_way_round(eng):
    p = np.zeros((6, 2))
    p[5] = [3.1, -3.1]
    fwd, back = eng.swath_offsets(p, 0), eng.swath_offsets(p, 1)
    assert abs(fwd[1]['dyaw'] - (2.0 * math.pi - 6.2)) < 1e-14 and abs(back[0]['dyaw'] - (6.2 - 2.0 * math.pi)) < 1e-14
    assert -math.pi <= fwd[1]['dyaw'] < math.pi and -math.pi <= back[0]['dyaw'] < math.pi


def test_bad_offsets_and_swaths_are_refused(eng, lib):
    p = np.zeros((6, 3))
    for anchor in (3, -2):
        with pytest.raises(eng.MclError):
            eng.swath_offsets(p, anchor)
    for bad in (math.inf, math.nan):
        q = p.copy()
        q[4, 1] = bad
        with pytest.raises(eng.MclError):
            eng.swath_offsets(q)
    with pytest.raises(eng.MclError):
        eng.swath_offsets(np.zeros((6, 65)))
    with pytest.raises(eng.MclError):
        eng.swath_offsets(np.zeros((6, 0)))
    off = np.zeros(64, eng.SwathOffset)
    assert eng.swath_check(64, 256, off) is None and eng.swath_check(8, 2048, off) is None and eng.swath_check(1, 1, off) is None
    assert 'K outside' in eng.swath_check(0, 8, off) and 'K outside' in eng.swath_check(65, 8, off)
    assert 'B outside' in eng.swath_check(1, 0, off) and 'B outside' in eng.swath_check(1, 2049, off)
    assert 'K B' in eng.swath_check(64, 257, off) and 'K B' in eng.swath_check(9, 2048, off)
    assert eng.swath_check(2, 8, None)
    for f in off.dtype.names:
        for bad in (math.inf, -math.inf, math.nan):
            o = off.copy()
            o[f][2] = bad
            assert 'not finite' in eng.swath_check(3, 8, o) and eng.swath_check(2, 8, o) is None
    assert lib.mcl_swath_offsets(None, 1, 0, off.ctypes.data) == ERR_INVALID and lib.mcl_swath_offsets(p.ctypes.data, 3, 0, None) == ERR_INVALID
    assert lib.mcl_swath_check(1, 1, off.ctypes.data, None) == 0


# ------------------------------------------------------------------ solve, better, derived: bit for bit, up to 16384 beams
def _check_solve(eng, rec, cfg, j):
    got, dead = eng.swath_solve(rec_array(rec), c_cfg(cfg), j)
    want, wdead = solve_ref(rec, cfg, j)
    assert [_bits(v) for v in got] == [_bits(v) for v in want] and dead == wdead, (rec, cfg, j, list(got), want, dead, wdead)


def _check_derived(eng, rec, cfg, sigma):
    got = eng.swath_derived(rec_array(rec), c_cfg(cfg), sigma)
    want = derived_ref(rec, cfg, sigma)
    for f in ('rms', 'mean', 'chi2'):
        assert _bits(got[f]) == _bits(want[f]), (f, rec)
    assert [_bits(v) for v in got['J']] == [_bits(v) for v in want['J']], rec
    assert [_bits(v) for v in got['cov']] == [_bits(v) for v in want['cov']], rec
    assert int(got['dead']) == want['dead'] and int(got['m']) == want['m']


def test_solve_better_and_derived_equal_the_restatement_bit_for_bit_up_to_16384_beams(eng):
    rs = np.random.RandomState(6)
    recs = []
    for trial in range(120):
        D = 3 + trial % 2
        cfg = default_cfg(dims=D, delta_xy=float(rs.choice([0.5, 0.25, 0.3])), delta_yaw=float(rs.choice([0.01, 0.003, 0.05])),
                          grad_floor_q=int(rs.choice([0, 2, 9])), step_max_xy=float(rs.choice([2.0, 0.3, 1e-3])),
                          step_max_yaw=float(rs.choice([0.1, 1e-3])))
        rec = random_record(rs, D, n=int(rs.choice([1, 64, 2049, 5000, 16380])))         # (with up to four misses and jumps: <= 16384)
        _check_solve(eng, rec, cfg, int(rs.randint(J_MIN, J_MAX + 3)))
        _check_derived(eng, rec, cfg, float(rs.choice([0.05, 0.2, 3.7])))
        recs.append(rec)
    seen = set()
    for q, p in zip(recs, recs[1:] + recs[:1]):
        for min_beams in (1, 8, 2049, 16384):
            want = better_ref(q, p, min_beams)
            assert eng.swath_better(rec_array(q), rec_array(p), min_beams) == want
            seen.add(want)
    assert seen == {True, False}


def test_the_largest_legal_sums_and_the_records_the_bounds_forbid(eng):
    top = record_of([(D_MAX, -D_MAX, D_MAX, D_MAX, RHO_MAX)] * MAX_BEAMS, D=4)
    assert top[0] == 1 << 14 and top[6] == 1 << 62 and top[3][0] == 1 << 60 and top[4][0] == 1 << 61 and top[5] == 1 << 38
    less = top[:6] + (top[6] - 1,)
    fewer = record_of([(D_MAX, -D_MAX, D_MAX, D_MAX, RHO_MAX)] * (MAX_BEAMS - 1), D=4, n_miss=1)
    for q, p in [(top, top), (less, top), (top, less), (fewer, top), (top, fewer), (less, fewer), (fewer, less)]:
        for min_beams in (1, 8, 16384):
            assert eng.swath_better(rec_array(q), rec_array(p), min_beams) == better_ref(q, p, min_beams), (min_beams,)
    assert eng.swath_better(rec_array(less), rec_array(top), 8) and not eng.swath_better(rec_array(top), rec_array(less), 8)
    for D in (3, 4):
        cfg = default_cfg(dims=D)
        for j in (J_MIN, J0, J_MAX + 2):
            _check_solve(eng, top, cfg, j)
        _check_derived(eng, top, cfg, SIGMA)
    cfg = default_cfg(dims=4)
    m = 1 << 14
    bad = [(m + 1,) + top[1:], top[:3] + (((m << 46) + 1,) + top[3][1:],) + top[4:], top[:4] + (((m << 47) + 1,) + top[4][1:],) + top[5:],
           top[:5] + ((m << 24) + 1, top[6]), top[:6] + ((m << 48) + 1,), top[:6] + (-1,), (-1,) + top[1:], (m, m, 1) + top[3:]]
    for r in bad:
        with pytest.raises(eng.MclError) as ei:
            eng.swath_solve(rec_array(r), c_cfg(cfg), J0)
        assert ei.value.status == ERR_INVALID
        with pytest.raises(eng.MclError):
            eng.swath_derived(rec_array(r), c_cfg(cfg), SIGMA)
        with pytest.raises(eng.MclError):
            eng.swath_better(rec_array(r), rec_array(top), 8)
    for j in (J_MIN - 1, J_MAX + 3):
        with pytest.raises(eng.MclError):
            eng.swath_solve(rec_array(top), c_cfg(cfg), j)


def test_the_ping_entry_points_keep_refusing_more_than_2048_beams(eng):
    ok = record_of([(100, 50, 3, 7)] * 10)
    many = (2049,) + ok[1:]
    cfg = c_cfg(default_cfg())
    eng.swath_solve(rec_array(many), cfg, J0)
    eng.swath_derived(rec_array(many), cfg, SIGMA)
    eng.swath_better(rec_array(many), rec_array(ok), 8)
    with pytest.raises(eng.MclError):
        eng.match_solve(rec_array(many), cfg, J0)
    with pytest.raises(eng.MclError):
        eng.match_derived(rec_array(many), cfg, SIGMA)
    with pytest.raises(eng.MclError):
        eng.match_better(rec_array(many), rec_array(ok), 8)
    eng.match_solve(rec_array(ok), cfg, J0)


# ------------------------------------------------------------------ the restated loop on the oracle's casts
def _variances(run, cfg):
    d = derived_ref(run['final'], cfg, SIGMA)
    return d['cov'][packed(0, 0)], d['cov'][packed(3, 3)]


def test_one_ping_slides_along_its_valley_and_two_do_not():
    """the table of the issue that asked for the swath: x / z errors of the fix and var(x), var(z) of its final record"""
    rows = {}
    for K in (1, 2, 8):
        ref = track_reference(K)
        run = ref['run']
        ex, ez = abs(run['pose'][0] - TRACK_TRUTH[0]), abs(run['pose'][3] - TRACK_TRUTH[2])
        vx, vz = _variances(run, ref['cfg'])
        rows[K] = (run['status'], ex, ez, vx, vz)
        print('K = %d: status %d after %d evaluations, rms %.2f quanta, x error %.3g m, z error %.3g m, var(x) %.3g m^2, var(z) %.3g m^2' % (
            K, run['status'], run['evaluations'], math.sqrt(run['final'][6] / max(m_of(run['final']), 1)), ex, ez, vx, vz))
        assert run['status'] == CONVERGED
        assert m_of(run['final']) == 64 * K
    assert rows[1][1] > 0.5                                   # one ping: CONVERGED, more than half a metre off along the track
    for K in (2, 8):
        assert rows[K][1] < 2e-3 and rows[K][2] < 2e-3        # the bound test_the_restated_loop_recovers_the_truth_on_rough_terrain uses
    assert rows[1][3] > 1000.0 * rows[8][3] and rows[2][3] > rows[8][3] and rows[1][4] > 1000.0 * rows[8][4]


def test_a_swath_of_one_ping_with_a_zero_offset_is_the_ping_match_of_the_restatement():
    ref = track_reference(1)
    cfg = ref['cfg']
    ev = OracleEval(ref['omap'], ref['ba'], ref['meas'][0], cfg, IDENT, NO_OFF, BC_RMAX)
    assert repr(loop_ref(ev, TRACK_START, cfg)) == repr(ref['run'])


def test_the_yaw_variance_falls_with_the_lever_arm():
    v = {}
    for K in (1, 8):
        ref = track_reference(K, dims=3)
        # the record at the truth: what the terrain can fix there
        ev = SwathEval(ref['omap'], ref['ba'], ref['meas'], ref['offsets'], ref['cfg'], IDENT, NO_OFF, BC_RMAX)
        v[K] = derived_ref(ev(TRACK_TRUTH), ref['cfg'], SIGMA)['cov'][packed(2, 2)]
        print('K = %d, D = 3: var(yaw) %.3g rad^2' % (K, v[K]))
    assert v[8] < 0.5 * v[1]


def _grid_swath(z, truth, cfg, offsets, B=64):
    from oracle import oracle as orc
    omap = orc.Grid(z, GRID_ORIGIN, 1.0)
    ba = synth.beam_angles(B)
    meas = swath_pings(omap, truth, offsets, ba, IDENT, NO_OFF, BC_RMAX)
    return SwathEval(omap, ba, meas, offsets, cfg, IDENT, NO_OFF, BC_RMAX)


FLAT_START = np.array([3.125, -2.25, -2.4, 0.0, 0.0, 0.7])
RIDGE_TRUTH = np.array([3.125, -2.25, -2.0, 0.0, 0.0, 0.0])          # the track along x, the ridge along x
RIDGE_START = np.array([3.5, -1.0, -2.0, 0.0, 0.0, 0.0])


def test_flat_seabed_x_y_and_yaw_keep_their_bits_and_z_is_recovered():
    cfg = default_cfg(dims=4, jump_max=BC_RMAX)
    truth = FLAT_START.copy()
    truth[2] = -2.0
    run = loop_both(_grid_swath(flat_grid(), truth, cfg, straight_offsets(8)), FLAT_START, cfg)
    print('flat: status %d, %d evaluations, z %.6f, dead %d' % (run['status'], run['evaluations'], run['pose'][3], run['dead']))
    assert run['status'] == CONVERGED and run['dead'] == 1 | 2 | 4
    assert [_bits(v) for v in run['pose'][:3]] == [_bits(FLAT_START[0]), _bits(FLAT_START[1]), _bits(FLAT_START[5])]
    assert abs(run['pose'][3] - truth[2]) < 1e-3


def test_ridge_along_the_track_keeps_the_bits_of_x():
    """a swath does not invent information: eight pings along a ridge that runs along the track say nothing about x"""
    cfg = default_cfg(dims=3, jump_max=BC_RMAX)
    run = loop_both(_grid_swath(ridge_grid(), RIDGE_TRUTH, cfg, straight_offsets(8)), RIDGE_START, cfg)
    print('ridge: status %d, %d evaluations, y %.6f (truth %.6f), dead %d' % (run['status'], run['evaluations'], run['pose'][1],
                                                                              RIDGE_TRUTH[1], run['dead']))
    assert run['status'] == CONVERGED and run['dead'] & 1
    assert _bits(run['pose'][0]) == _bits(RIDGE_START[0])
    assert abs(run['pose'][1] - RIDGE_TRUTH[1]) < 2e-3


@pytest.mark.parametrize('dims', [3, 4])
def test_a_turning_track_recovers_the_truth_on_rough_terrain(dims):
    ref = turning_reference(dims)
    assert all(o[5] != 0.0 and o[3] != 0.0 and o[4] != 0.0 for o in ref['offsets'][:-1]) and ref['offsets'][-1][:3] == (0.0, 0.0, 0.0)
    for k, run in enumerate(ref['runs']):
        start = ref['starts'][:, k]
        err = math.hypot(run['pose'][0] - TRUTH[0], run['pose'][1] - TRUTH[1])
        print('dims %d start %d: %.2f m off -> status %d after %d evaluations, %.2e m off, yaw %.2e rad off' % (
            dims, k, math.hypot(start[0] - TRUTH[0], start[1] - TRUTH[1]), run['status'], run['evaluations'], err, abs(run['pose'][2] - TRUTH[5])))
        assert run['status'] == CONVERGED
        assert err < 2e-3 and abs(run['pose'][2] - TRUTH[5]) < 1e-3
        if dims == 4:
            assert abs(run['pose'][3] - TRUTH[2]) < 2e-3
        else:
            assert _bits(run['pose'][3]) == _bits(start[2])
    assert len(ref['runs']) == 8


# ------------------------------------------------------------------ the sanitizer driver
def test_the_host_arithmetic_runs_clean_under_the_sanitizers_as_a_program(tmp_path):
    """tests/host_san/swath_driver.cpp: its own main over the device-free functions, g++ -fsanitize=address,undefined, run as
    a program (nothing loaded into Python runs under a sanitizer)"""
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no g++ / make')
    san = str(tmp_path / 'host_san')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'smarc_navigation_amd', 'csrc'), 'host-asan-swath', 'SAN_DIR=' + san],
                          stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(san, 'swath_asan')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                       timeout=300, cwd=ROOT)
    for marker in ('AddressSanitizer', 'runtime error', 'LeakSanitizer'):
        assert marker not in p.stdout, p.stdout[-2000:]
    assert p.returncode == 0 and 'swath_driver: ok' in p.stdout, p.stdout[-2000:]
