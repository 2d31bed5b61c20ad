"""Host tests of the sensor resetting (include/mcl_reseed.h; no GPU): the ABI, mcl_reseed_select bit for bit against the
numpy restatement of tests/reseed_ref.py on random result sets and at its edges, every rule of the two checks, the
component rule in Python integers, the start lattice, the policy recovery.SensorResetting over a recording engine, the
summary of replay_recover with and without --reseed, and the sanitizer driver tests/host_san/reseed_driver.cpp."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import reseed_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1
NAMES = ('mcl_reseed_select_check', 'mcl_reseed_components_check', 'mcl_reseed_select', 'mcl_inject_gaussian')
CONVERGED, MAX_ITER, STALLED, NO_OVERLAP = 0, 1, 2, 3
SIGMA, R_MAX = 0.2, 80.0


@pytest.fixture(scope='module')
def lib():
    from smarc_navigation_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


# ------------------------------------------------------------------ synthetic match results
def record(eng, rs, n, D, flat=0, rho=400):
    """the record of n contributing beams with random differences (zero in the dimensions of `flat`) and the residual rho
    quanta on every beam: rms = rho / 4096 m"""
    d = rs.randint(-3000, 3001, (n, 4)).astype(np.int64)
    for k in range(4):
        if k >= D or (flat >> k) & 1:
            d[:, k] = 0
    r = np.zeros(1, eng.MATCH_SUMS)[0]
    r['n'] = n
    for j in range(4):
        for k in range(j + 1):
            r['S'][j * (j + 1) // 2 + k] = int(np.sum(d[:, j] * d[:, k]))
        r['C'][j] = int(np.sum(d[:, j])) * rho
    r['s_rho'], r['s_rho2'] = n * rho, n * rho * rho
    return r


def results_of(eng, poses, finals, status=None):
    res = np.zeros(len(poses), eng.MATCH_RESULT)
    for i, (p, f) in enumerate(zip(poses, finals)):
        res[i]['x'], res[i]['y'], res[i]['yaw'] = p
        res[i]['final'] = f
        res[i]['start'] = f
        res[i]['status'] = CONVERGED if status is None else status[i]
    return res


def match_of(eng, res, D=3):
    cfg = eng.make_match_config(R_MAX, fit_z=(D == 4))
    return eng.PingMatch(res, cfg, SIGMA, derive=eng.swath_derived)


def same_components(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_select(eng, res, D, **kw):
    m = match_of(eng, res, D)
    cfg = eng.make_reseed_select_config(**kw)
    comps, idx = eng.reseed_select(m, cfg=cfg)
    rc, ri = ref.select_ref(eng, res, m.cfg, SIGMA, cfg)
    assert np.array_equal(idx, ri), (idx, ri)
    assert same_components(comps, rc)
    assert eng.reseed_components_check(comps) is None if len(comps) else True
    return comps, idx


# ------------------------------------------------------------------ the ABI
def test_every_symbol_of_the_header_is_exported_and_bound_in_a_table_of_its_own(lib):
    from smarc_navigation_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'mcl_reseed.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(NAMES) == sorted(_lib.RESEED_SYMBOLS)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    for table in (_lib.SYMBOLS, _lib.RECOVERY_SYMBOLS, _lib.MATCH_SYMBOLS, _lib.SWATH_SYMBOLS):
        assert not set(table) & set(NAMES)
    assert lib.mcl_abi_version() == 4
    assert ctypes.sizeof(_lib.Timing) == 15 * 16                 # no timing slot was added
    for other in ('mcl.h', 'mcl_recovery.h', 'mcl_match.h', 'mcl_swath.h', 'mcl_regularise.h'):
        assert 'reseed' not in open(os.path.join(ROOT, 'include', other)).read()   # the existing headers are what they were


def test_the_records_have_the_declared_sizes_and_offsets(eng):
    from smarc_navigation_amd import _lib
    c = eng.ReseedComponent
    assert c.itemsize == 80 and [c.fields[f][1] for f in ('mean', 'chol', 'mass', 'reserved')] == [0, 24, 72, 76]
    s = _lib.ReseedSelectConfig
    assert ctypes.sizeof(s) == 72 and s.max_rms.offset == 8 and s.dead_std_yaw.offset == 64
    src = open(os.path.join(ROOT, 'include', 'mcl_reseed.h')).read()
    assert '#define MCL_RESEED_MAX_COMPONENTS 256' in src and eng.RESEED_MAX_COMPONENTS == 256
    assert re.search(r'typedef struct mcl_reseed_component \{', src)


# ------------------------------------------------------------------ the selection against the restatement
@pytest.mark.parametrize('D', [3, 4])
def test_select_equals_the_restatement_on_random_result_sets(eng, D):
    rs = np.random.RandomState(100 + D)
    taken = 0
    for round_ in range(12):
        M = int(rs.randint(1, 50))
        poses = [(40.0 * rs.randn(), 40.0 * rs.randn(), rs.uniform(-math.pi, math.pi)) for _ in range(M)]
        for i in range(1, M):
            if rs.rand() < 0.3:   # a near twin of the fix before it
                poses[i] = (poses[i - 1][0] + 0.3 * rs.randn(), poses[i - 1][1] + 0.3 * rs.randn(), poses[i - 1][2] + 0.03 * rs.randn())
        finals = [record(eng, rs, int(rs.randint(8, 200)), D, flat=int(rs.randint(0, 8)) if rs.rand() < 0.2 else 0,
                         rho=int(rs.randint(0, 3000))) for _ in range(M)]
        status = [int(rs.randint(0, 4)) if rs.rand() < 0.2 else CONVERGED for _ in range(M)]
        res = results_of(eng, poses, finals, status)
        for maxc in (1, 4, 256):
            comps, idx = check_select(eng, res, D, max_components=maxc, min_beams=32, max_rms=0.5)
            taken += len(idx)
            assert all(status[i] == CONVERGED for i in idx)
    assert taken > 50


def test_equal_rms_goes_to_the_lower_index_and_the_order_is_by_rms(eng):
    rs = np.random.RandomState(1)
    f = record(eng, rs, 64, 3, rho=300)
    g = record(eng, rs, 64, 3, rho=100)
    res = results_of(eng, [(0.0, 0.0, 0.0), (50.0, 0.0, 0.0), (0.0, 50.0, 0.0), (50.0, 50.0, 0.0)], [f, g, f, f])
    comps, idx = check_select(eng, res, 3, max_components=3)
    assert list(idx) == [1, 0, 2]                      # the lowest rms first, then the equal ones by index; 3 is cut off
    assert np.all(comps['mass'] == 1) and np.all(comps['reserved'] == 0)
    assert np.array_equal(comps['mean'][:, :2], [[50.0, 0.0], [0.0, 0.0], [0.0, 50.0]])


def test_two_fixes_exactly_sep_apart_are_one_hypothesis_and_a_hair_more_are_two(eng):
    rs = np.random.RandomState(2)
    f, g = record(eng, rs, 64, 3, rho=100), record(eng, rs, 64, 3, rho=200)
    for dx, dyaw, n in ((1.0, 0.0, 1), (np.nextafter(1.0, 2.0), 0.0, 2), (0.6, 0.125, 1), (0.6, np.nextafter(0.125, 1.0), 2),
                        (3.0, 0.0, 2), (0.0, 0.0, 1)):
        res = results_of(eng, [(0.0, 0.0, 0.0), (dx, 0.0, dyaw)], [f, g])      # (from zero: the hair survives the subtraction)
        comps, idx = check_select(eng, res, 3, sep_xy=1.0, sep_yaw=0.125)
        assert len(idx) == n and idx[0] == 0, (dx, dyaw, idx)
    # near in position but not in heading (and the other way round): two hypotheses
    res = results_of(eng, [(0.0, 0.0, 0.0), (0.1, 0.0, 1.0), (30.0, 0.0, 0.0)], [f, g, g])
    assert list(check_select(eng, res, 3, sep_xy=1.0, sep_yaw=0.125)[1]) == [0, 1, 2]


def test_a_yaw_pair_across_pi_is_one_hypothesis(eng):
    rs = np.random.RandomState(3)
    f, g = record(eng, rs, 64, 3, rho=100), record(eng, rs, 64, 3, rho=200)
    res = results_of(eng, [(0.0, 0.0, math.pi - 0.01), (0.2, 0.0, -math.pi + 0.01)], [f, g])
    assert list(check_select(eng, res, 3, sep_xy=1.0, sep_yaw=0.05)[1]) == [0]
    assert list(check_select(eng, res, 3, sep_xy=1.0, sep_yaw=0.01)[1]) == [0, 1]


@pytest.mark.parametrize('D', [3, 4])
def test_dead_masks_zero_to_seven(eng, D):
    rs = np.random.RandomState(4)
    for flat in range(8):
        res = results_of(eng, [(1.0, 2.0, 0.5)], [record(eng, rs, 100, D, flat=flat, rho=50)])
        comps, idx = check_select(eng, res, D, cov_scale=2.0, add_std_xy=0.25, add_std_yaw=0.02, dead_std_xy=4.0, dead_std_yaw=0.2)
        assert len(idx) == 1
        L = np.zeros((3, 3))
        L[np.tril_indices(3)] = comps[0]['chol']
        cov = L.dot(L.T)
        d = eng.swath_derived(res[0]['final'], match_of(eng, res, D).cfg, SIGMA)
        assert int(d['dead']) & 7 == flat
        for k in range(3):
            if (flat >> k) & 1:   # dead: its own spread, no correlation
                want = (0.2 ** 2 + 0.02 ** 2) if k == 2 else (4.0 ** 2 + 0.25 ** 2)
                assert abs(cov[k, k] - want) < 1e-12 * want
                assert all(cov[k, j] == 0.0 for j in range(3) if j != k)
            else:
                assert cov[k, k] > (0.02 ** 2 if k == 2 else 0.25 ** 2)
        assert np.all(np.isfinite(comps[0]['chol']))


def test_no_candidate_is_ok_and_other_statuses_are_never_taken(eng, lib):
    rs = np.random.RandomState(5)
    f = record(eng, rs, 64, 3, rho=100)
    res = results_of(eng, [(0.0, 0.0, 0.0), (20.0, 0.0, 0.0), (40.0, 0.0, 0.0)], [f, f, f], [MAX_ITER, STALLED, NO_OVERLAP])
    comps, idx = check_select(eng, res, 3)
    assert len(comps) == 0 and len(idx) == 0
    res = results_of(eng, [(0.0, 0.0, 0.0), (20.0, 0.0, 0.0), (40.0, 0.0, 0.0), (60.0, 0.0, 0.0)], [f, f, f, f],
                     [MAX_ITER, CONVERGED, STALLED, NO_OVERLAP])
    assert list(check_select(eng, res, 3)[1]) == [1]
    # too few beams, too large a residual
    res = results_of(eng, [(0.0, 0.0, 0.0), (20.0, 0.0, 0.0)], [record(eng, rs, 31, 3, rho=10), record(eng, rs, 64, 3, rho=2100)])
    assert len(check_select(eng, res, 3, min_beams=32, max_rms=0.5)[1]) == 0
    assert list(check_select(eng, res, 3, min_beams=31, max_rms=0.5)[1]) == [0]
    assert list(check_select(eng, res, 3, min_beams=32, max_rms=2100 / 4096.0)[1]) == [1]      # rms <= max_rms
    # what the entry point refuses
    m = match_of(eng, res)
    cfg = eng.make_reseed_select_config()
    comps, idx, n = np.zeros(16, eng.ReseedComponent), np.zeros(16, np.int64), ctypes.c_int32(7)
    args = [res.ctypes.data, 2, ctypes.byref(m.cfg), SIGMA, ctypes.byref(cfg), comps.ctypes.data, idx.ctypes.data, ctypes.byref(n)]
    assert lib.mcl_reseed_select(*args) == 0
    for k in (0, 2, 4, 5, 6, 7):
        bad = list(args)
        bad[k] = None
        assert lib.mcl_reseed_select(*bad) == ERR_INVALID, k
    for M in (0, -1, 65537):
        assert lib.mcl_reseed_select(*(args[:1] + [M] + args[2:])) == ERR_INVALID
    for s in (0.0, -1.0, math.nan, math.inf):
        assert lib.mcl_reseed_select(*(args[:3] + [s] + args[4:])) == ERR_INVALID
    broken = res.copy()
    broken[0]['final']['n_miss'] = 1000                # a CONVERGED record that cannot be a sum
    assert lib.mcl_reseed_select(*([broken.ctypes.data] + args[1:])) == ERR_INVALID
    broken = res.copy()
    broken[1]['x'] = math.nan
    assert lib.mcl_reseed_select(*([broken.ctypes.data] + args[1:])) == ERR_INVALID
    broken[1]['status'] = STALLED                      # ... but what is not CONVERGED is not looked at
    assert lib.mcl_reseed_select(*([broken.ctypes.data] + args[1:])) == 0


# ------------------------------------------------------------------ the checks
def test_every_rule_of_the_select_check(eng, lib):
    assert eng.reseed_select_check() is None
    assert lib.mcl_reseed_select_check(None, None) == ERR_INVALID
    why = ctypes.c_char_p()
    assert lib.mcl_reseed_select_check(None, ctypes.byref(why)) == ERR_INVALID and why.value == b'null config'
    for v in (0, -3, 257):
        assert 'max_components' in eng.reseed_select_check(max_components=v)
    for v in (1, 256):
        assert eng.reseed_select_check(max_components=v) is None
    assert 'min_beams' in eng.reseed_select_check(min_beams=0) and eng.reseed_select_check(min_beams=1) is None
    zero_ok = dict(max_rms=True, sep_xy=True, sep_yaw=True, cov_scale=False, add_std_xy=True, add_std_yaw=True, dead_std_xy=False,
                   dead_std_yaw=False)
    for name, ok in zero_ok.items():
        for v in (-1e-9, math.nan, math.inf, -math.inf):
            assert name.split('_std')[0].split('_xy')[0].split('_yaw')[0] in eng.reseed_select_check(**{name: v}), (name, v)
        assert (eng.reseed_select_check(**{name: 0.0}) is None) == ok, name
        assert eng.reseed_select_check(**{name: 1e-9}) is None


def test_every_rule_of_the_components_check(eng, lib):
    c = np.zeros(3, eng.ReseedComponent)
    c['mass'] = (1, 0, 2)
    c['chol'][:, (0, 2, 5)] = 1.0
    assert eng.reseed_components_check(c) is None
    assert lib.mcl_reseed_components_check(None, 1, None) == ERR_INVALID
    assert 'n_comp' in eng.reseed_components_check(np.zeros(0, eng.ReseedComponent))
    big = np.zeros(257, eng.ReseedComponent)
    big['mass'] = 1
    assert 'n_comp' in eng.reseed_components_check(big) and eng.reseed_components_check(big[:256]) is None
    for field, n in (('mean', 3), ('chol', 6)):
        for k in range(n):
            for v in (math.nan, math.inf, -math.inf):
                b = c.copy()
                b[field][1, k] = v                        # (a component of mass 0 is checked too)
                assert 'not finite' in eng.reseed_components_check(b)
    for k in (0, 2, 5):
        b = c.copy()
        b['chol'][2, k] = -1e-300
        assert 'negative' in eng.reseed_components_check(b)
    b = c.copy()
    b['chol'][:, (1, 3, 4)] = -9.0                        # the off-diagonal may be
    assert eng.reseed_components_check(b) is None
    b = c.copy()
    b['mass'] = 0
    assert 'add up to 0' in eng.reseed_components_check(b)
    b['mass'] = (1 << 31, 0, 0)
    assert eng.reseed_components_check(b) is None
    b['mass'] = (1 << 31, 0, 1)
    assert '2^31' in eng.reseed_components_check(b)
    b['mass'] = (0xffffffff, 0xffffffff, 2)              # the sum does not wrap
    assert '2^31' in eng.reseed_components_check(b)


# ------------------------------------------------------------------ the component rule in Python integers
def test_the_component_rule_at_its_edges():
    T = (1 << 53) - 1
    for masses in ([1], [1 << 31], [0, 5, 0, 0, 3, 0], [0, 0, 1], [7, 0, 0], [1] * 256, [3, 1, 4, 1, 5, 9, 2, 6], [1 << 30, 0, 1 << 30],
                   [0, 1, 0, (1 << 31) - 1]):
        W = sum(masses)
        positive = [c for c, m in enumerate(masses) if m > 0]
        assert ref.rank_int(0, W) == 0 and ref.rank_int(T, W) == W - 1
        assert ref.component_int(0, masses) == positive[0] and ref.component_int(T, masses) == positive[-1]
        # every boundary: the smallest t with rank r is ceil(r 2^53 / W); r = cum - 1 still picks the component, r = cum the next
        ts, want = [0, T], [positive[0], positive[-1]]
        cum = 0
        for c, m in enumerate(masses[:64]):
            cum += m
            for r in (cum - 1, cum):
                if m == 0 or not 0 <= r < W:
                    continue
                t = -((-r << 53) // W)
                assert ref.rank_int(t, W) == r and (t == 0 or ref.rank_int(t - 1, W) == r - 1)
                nxt = [p for p in positive if p > c]
                ts += [t, max(t - 1, 0)]
                want += [c if r == cum - 1 else nxt[0], ref.component_int(max(t - 1, 0), masses)]
        got = ref.components_of(np.array(ts, np.uint64), masses)
        assert list(got) == want == [ref.component_int(t, masses) for t in ts]
        assert all(masses[c] > 0 for c in got)            # a component of mass 0 is never drawn
    rs = np.random.RandomState(6)
    masses = [int(v) for v in rs.randint(0, 1 << 23, 256)]
    t = (rs.randint(0, 1 << 31, 4000).astype(np.uint64) << np.uint64(22)) | rs.randint(0, 1 << 22, 4000).astype(np.uint64)
    assert list(ref.components_of(t, masses)) == [ref.component_int(int(v), masses) for v in t]


def test_the_apply_rule_keeps_the_means_bits_on_a_row_of_zeros():
    mean = np.array([[-0.0], [3.5], [math.pi - 1e-3]])
    chol = np.array([[0.0], [0.0], [0.0], [0.0], [0.0], [0.5]])
    with np.errstate(invalid='ignore'):
        x, y, yaw = ref.apply_rule(mean, chol, np.array([[math.inf], [math.nan], [1.0]]))
    assert np.signbit(x[0]) and x[0] == 0.0 and y[0] == 3.5              # the mean's bits, whatever the normals are
    x, y, yaw = ref.apply_rule(mean, chol, np.array([[2.0], [-3.0], [1.0]]))
    assert np.signbit(x[0]) and y[0] == 3.5                              # (-0.0 + 0.0 would be +0.0)
    assert yaw[0] == ref.wrap_yaw(np.float64(math.pi - 1e-3) + 0.5) and -math.pi <= yaw[0] < 0.0


# ------------------------------------------------------------------ the start lattice
def test_reseed_starts_counts_cell_centres_and_the_limit(eng):
    s = eng.reseed_starts((0.0, 10.0, -3.0, 3.0), 4.0, yaw=(-0.4, 0.4), n_yaw=4, z=-2.0, roll=0.01, pitch_angle=-0.02)
    assert s.shape == (6, 3 * 2 * 4)                                   # ceil(10 / 4) x ceil(6 / 4) x 4
    assert np.allclose(np.unique(s[0]), [10.0 / 6, 5.0, 50.0 / 6]) and np.allclose(np.unique(s[1]), [-1.5, 1.5])
    assert np.allclose(np.unique(s[5]), [-0.3, -0.1, 0.1, 0.3])
    assert np.all(s[2] == -2.0) and np.all(s[3] == 0.01) and np.all(s[4] == -0.02)
    assert np.allclose(s[:, 0][[0, 1, 5]], [10.0 / 6, -1.5, -0.3]) and np.allclose(s[:, 1][[0, 1, 5]], [10.0 / 6, -1.5, -0.1])   # yaw fastest
    assert np.allclose(s[:, 4][[0, 1, 5]], [5.0, -1.5, -0.3]) and np.allclose(s[:, 12][[0, 1, 5]], [10.0 / 6, 1.5, -0.3])      # then x, then y
    # every point of the box is within half a cell of a start; a box thinner than the pitch gets one cell
    assert np.diff(np.unique(s[0])).max() <= 4.0 and eng.reseed_starts((0.0, 1.0, 5.0, 5.0), 4.0, n_yaw=1).shape == (6, 1)
    full = eng.reseed_starts((0.0, 8.0, 0.0, 8.0), 4.0, n_yaw=8)
    assert full.shape == (6, 32) and np.all((full[5] >= -math.pi) & (full[5] < math.pi))
    assert np.allclose(np.unique(full[5]), -math.pi + (np.arange(8) + 0.5) * math.pi / 4)
    window = eng.reseed_starts((0.0, 4.0, 0.0, 4.0), 4.0, yaw=(3.0, 3.4), n_yaw=2)      # a window across +pi is wrapped
    assert np.allclose(window[5], [3.1, 3.3 - 2.0 * math.pi])
    assert eng.reseed_starts((0.0, 256.0, 0.0, 256.0), 1.0, n_yaw=1).shape == (6, 65536)
    for box, pitch, n_yaw in (((0.0, 257.0, 0.0, 256.0), 1.0, 1), ((0.0, 256.0, 0.0, 256.0), 1.0, 2), ((0.0, 192.0, 0.0, 192.0), 2.0, 36)):
        with pytest.raises(ValueError, match='starts'):
            eng.reseed_starts(box, pitch, n_yaw=n_yaw)
    for bad in (dict(pitch=0.0), dict(pitch=math.nan), dict(n_yaw=0), dict(box=(1.0, 0.0, 0.0, 1.0)), dict(yaw=(1.0, 0.0))):
        kw = dict(dict(box=(0.0, 1.0, 0.0, 1.0), pitch=1.0), **bad)
        with pytest.raises(ValueError):
            eng.reseed_starts(**kw)
    with pytest.raises(ValueError):
        eng.reseed_starts(None, 4.0)                                   # neither a box nor the map's bounds


def test_reseed_starts_over_the_footprint_follow_the_frame_rule_with_a_turned_m2o(eng):
    from smarc_navigation_amd import synth
    bounds = (-96.0, 95.0, -40.0, 23.0)
    m2o = synth.rigid_matrix(12.0, -7.0, 0.0, 0.0, 0.0, 0.7)
    box = eng.footprint_odom(bounds, m2o)
    # the rule of Engine.mode_grid and mcl_recovery.h: d = p - t;  x_o = R00 dx + R10 dy;  y_o = R01 dx + R11 dy
    xs, ys = [], []
    for x, y in ((-96.0, -40.0), (-96.0, 23.0), (95.0, -40.0), (95.0, 23.0)):
        dx, dy = x - 12.0, y + 7.0
        xs.append(math.cos(0.7) * dx + math.sin(0.7) * dy)
        ys.append(-math.sin(0.7) * dx + math.cos(0.7) * dy)
    assert np.allclose(box, (min(xs), max(xs), min(ys), max(ys)), rtol=0, atol=1e-12)
    s = eng.reseed_starts(None, 8.0, n_yaw=2, bounds=bounds, m2o=m2o)
    t = eng.reseed_starts(box, 8.0, n_yaw=2)
    assert np.array_equal(s, t) and s.shape[1] == math.ceil((box[1] - box[0]) / 8.0) * math.ceil((box[3] - box[2]) / 8.0) * 2
    # carried back into the map frame, every corner of the footprint is within a cell of a start
    back = m2o[:2, :2].dot(s[:2]) + m2o[:2, 3:4]
    for x, y in ((-96.0, -40.0), (-96.0, 23.0), (95.0, -40.0), (95.0, 23.0)):
        assert np.min(np.hypot(back[0] - x, back[1] - y)) <= 8.0 * math.sqrt(0.5) + 1e-9
    assert np.array_equal(eng.reseed_starts(None, 8.0, n_yaw=2, bounds=bounds), eng.reseed_starts(bounds, 8.0, n_yaw=2))   # identity m2o
    with pytest.raises(eng.MclError):
        eng.footprint_odom(bounds, synth.rigid_matrix(0.0, 0.0, 0.0, 0.1, 0.0, 0.0))    # m2o must turn about z alone


# ------------------------------------------------------------------ the policy over a recording engine
class Aug(object):
    def __init__(self, frac):
        self.frac, self.n_injected = frac, 0

    def fraction(self):
        return self.frac

    def injected(self):
        self.n_injected += 1


class Mode(object):
    def __init__(self, mean):
        self.mean = np.asarray(mean, np.float64)


class RecordingEngine(object):
    """the engine-shaped object SensorResetting drives: records the calls, answers match_swath with prepared results"""

    def __init__(self, eng, results, peaks=()):
        self.eng, self.results, self.peaks, self.calls = eng, results, list(peaks), []

    def reseed_starts(self, box, pitch, yaw, n_yaw, z=0.0, roll=0.0, pitch_angle=0.0):
        self.calls.append(('reseed_starts', box, pitch, tuple(yaw), n_yaw, z, roll, pitch_angle))
        return self.eng.reseed_starts((0.0, 8.0, 0.0, 8.0) if box is None else box, pitch, yaw, n_yaw, z, roll, pitch_angle)

    def pose_modes(self, cell, n_yaw, k):
        self.calls.append(('pose_modes', cell, n_yaw, k))
        return [Mode(p) for p in self.peaks[:k]], 0

    def match_swath(self, starts, ranges, beam_angles, offsets, sigma, r_max, sensor_offset=None, **kw):
        self.calls.append(('match_swath', np.array(starts), np.array(ranges), np.array(offsets), sigma, r_max, kw))
        return match_of(self.eng, self.results)

    def inject_gaussian(self, fraction, components, normals=None, count=True):
        self.calls.append(('inject_gaussian', fraction, np.array(components)))
        return 100

    def inject_uniform(self, fraction, box=None, frame='map', yaw=(-math.pi, math.pi), uniforms=None, count=True):
        self.calls.append(('inject_uniform', fraction, box, frame, tuple(yaw)))
        return 10

    def names(self):
        return [c[0] for c in self.calls]


def _policy_results(eng):
    rs = np.random.RandomState(9)
    return results_of(eng, [(1.0, 2.0, 0.5), (40.0, 2.0, 0.5), (1.2, 2.1, 0.5)],
                      [record(eng, rs, 64, 3, rho=100), record(eng, rs, 64, 3, rho=150), record(eng, rs, 64, 3, rho=200)])


def _push(sr, k, B=16):
    sr.push(np.full(B, 20.0 + k, np.float32), (float(k), 0.5 * k, -2.0, 0.01, -0.02, 0.5))


def test_sensor_resetting_calls_nothing_while_the_fraction_is_zero(eng):
    from smarc_navigation_amd.recovery import SensorResetting
    aug, e = Aug(0.0), RecordingEngine(eng, _policy_results(eng))
    sr = SensorResetting(aug, eng.make_reseed_select_config(), 4.0, 2, pings=3)
    for k in range(5):
        _push(sr, k)
        assert sr.step(e, np.zeros(16, np.float32), SIGMA, R_MAX) == 0
    assert e.calls == [] and aug.n_injected == 0 and (sr.calls, sr.fallbacks, sr.components, sr.injected) == (0, 0, 0, 0) and sr.last is None


def test_sensor_resetting_matches_selects_and_injects(eng):
    from smarc_navigation_amd.recovery import SensorResetting
    peak = [5.0, 6.0, -2.0, 0.0, 0.0, 0.4]
    aug, e = Aug(0.08), RecordingEngine(eng, _policy_results(eng), peaks=[peak])
    cfg = eng.make_reseed_select_config(min_beams=32)
    sr = SensorResetting(aug, cfg, 4.0, 2, yaw_window=0.4, modes=4, pings=3, match_kw=dict(max_iter=8))
    for k in range(5):
        _push(sr, k)
    assert sr.ring_full() and sr.step(e, np.zeros(16, np.float32), SIGMA, R_MAX) == 100
    assert e.names() == ['reseed_starts', 'pose_modes', 'match_swath', 'inject_gaussian']
    starts_call, match_call, inject_call = e.calls[0], e.calls[2], e.calls[3]
    assert starts_call[1:] == (None, 4.0, (0.5 - 0.4, 0.5 + 0.4), 2, -2.0, 0.01, -0.02)      # about the newest dead-reckoned heading
    starts, ranges, offsets = match_call[1], match_call[2], match_call[3]
    assert starts.shape == (6, 1 + 2 * 2 * 2) and np.array_equal(starts[:, 0], peak)         # the peaks, then the lattice
    assert np.array_equal(starts[:, 1:], eng.reseed_starts((0.0, 8.0, 0.0, 8.0), 4.0, (0.1, 0.9), 2, -2.0, 0.01, -0.02))
    assert ranges.shape == (3, 16) and np.array_equal(ranges[:, 0], [22.0, 23.0, 24.0])      # the newest three pings
    want = eng.swath_offsets(np.array([[float(k), 0.5 * k, -2.0, 0.01, -0.02, 0.5] for k in (2, 3, 4)]).T, -1)
    assert offsets.tobytes() == want.tobytes() and offsets[-1]['dx'] == 0.0
    assert match_call[4:] == (SIGMA, R_MAX, dict(max_iter=8))
    comps, idx = eng.reseed_select(match_of(eng, e.results), cfg=cfg)
    assert list(idx) == [0, 1] and inject_call[1] == 0.08 and same_components(inject_call[2], comps)
    assert aug.n_injected == 1
    assert (sr.calls, sr.fallbacks, sr.components, sr.injected) == (1, 0, 2, 100)
    assert sr.last['fallback'] is False and sr.last['components'] == 2 and sr.last['starts'] == 9 and sr.last['injected'] == 100
    assert list(sr.last['indices']) == [0, 1]


def test_sensor_resetting_leaves_out_the_peaks_that_would_exceed_one_match_call(eng):
    from smarc_navigation_amd.recovery import SensorResetting
    peaks = [[float(k), 0.0, -2.0, 0.0, 0.0, 0.0] for k in range(4)]
    aug, e = Aug(0.1), RecordingEngine(eng, _policy_results(eng), peaks=peaks)
    sr = SensorResetting(aug, eng.make_reseed_select_config(), 1.0, 1, pings=1, box=(0.0, 256.0, 0.0, 255.5))      # 256 x 256 starts:
    _push(sr, 0)
    sr.step(e, np.zeros(16, np.float32), SIGMA, R_MAX)                                                              # no room for a peak
    assert [c for c in e.calls if c[0] == 'match_swath'][0][1].shape == (6, 65536) and sr.last['starts'] == 65536
    sr.box = (0.0, 256.0, 0.0, 254.5)                                                                               # 256 x 255: room for all four
    sr.step(e, np.zeros(16, np.float32), SIGMA, R_MAX)
    starts = [c for c in e.calls if c[0] == 'match_swath'][1][1]
    assert starts.shape == (6, 256 * 255 + 4) and np.array_equal(starts[0, :4], [0.0, 1.0, 2.0, 3.0])


def test_sensor_resetting_splits_by_the_uniform_share(eng):
    from smarc_navigation_amd.recovery import SensorResetting
    aug, e = Aug(0.1), RecordingEngine(eng, _policy_results(eng))
    sr = SensorResetting(aug, eng.make_reseed_select_config(), 4.0, 2, uniform_share=0.25, modes=0, pings=2, box=(0.0, 4.0, 0.0, 4.0))
    _push(sr, 0)
    _push(sr, 1)
    assert sr.step(e, np.zeros(16, np.float32), SIGMA, R_MAX) == 110
    assert e.names() == ['reseed_starts', 'match_swath', 'inject_gaussian', 'inject_uniform']      # modes=0: no pose_modes
    assert e.calls[2][1] == 0.1 * 0.75 and e.calls[3][1:] == (0.1 * 0.25, (0.0, 4.0, 0.0, 4.0), 'odom', (-math.pi, math.pi))
    assert aug.n_injected == 1 and sr.injected == 110 and sr.fallbacks == 0
    with pytest.raises(ValueError):
        SensorResetting(aug, None, 4.0, 2, uniform_share=1.5)


def test_sensor_resetting_falls_back_to_the_uniform_injection(eng):
    from smarc_navigation_amd.recovery import SensorResetting
    none = _policy_results(eng)
    none['status'] = STALLED
    aug, e = Aug(0.1), RecordingEngine(eng, none)
    sr = SensorResetting(aug, eng.make_reseed_select_config(), 4.0, 2, yaw_window=0.3, modes=0, pings=2)
    _push(sr, 0)
    # the ring is not yet full: today's call, nothing else
    assert not sr.ring_full() and sr.step(e, np.zeros(16, np.float32), SIGMA, R_MAX) == 10
    assert e.names() == ['inject_uniform'] and e.calls[0][1:] == (0.1, None, 'odom', (0.5 - 0.3, 0.5 + 0.3))
    assert (sr.calls, sr.fallbacks, sr.components, aug.n_injected) == (1, 1, 0, 1) and sr.last['fallback'] is True
    # full, but no fix is a candidate: the same call after the match
    _push(sr, 1)
    assert sr.step(e, np.zeros(16, np.float32), SIGMA, R_MAX) == 10
    assert e.names()[1:] == ['reseed_starts', 'match_swath', 'inject_uniform'] and e.calls[-1][1] == 0.1
    assert (sr.calls, sr.fallbacks, sr.components, sr.injected, aug.n_injected) == (2, 2, 0, 20, 2)
    assert sr.last['fallback'] is True and sr.last['components'] == 0 and sr.last['starts'] == 8


# ------------------------------------------------------------------ replay_recover's summary
class _Stats(object):
    def __init__(self, lml):
        self.log_mean_lik, self.n_eff = lml, 100.0


class FakeEngine(RecordingEngine):
    """what replay_recover drives, without a device: the likelihood drops at ping 12 (so that injections follow)"""
    instances = []

    def __init__(self, n, **kw):
        from smarc_navigation_amd import engine
        RecordingEngine.__init__(self, engine, _policy_results(engine))
        self.pings, self.m2o = 0, np.identity(4)
        FakeEngine.instances.append(self)

    def set_map_grid(self, z, origin, res):
        pass

    def init_particles_uniform(self, box=None, frame='map', yaw=(-math.pi, math.pi), uniforms=None):
        pass

    def predict(self, *a, **kw):
        pass

    def update_mbes(self, ranges, angles, sigma, r_max):
        self.pings += 1

    def weight_stats(self):
        return _Stats(-16.0 if self.pings < 12 else -64.0)

    def resample(self):
        pass

    def mean_cov(self):
        return np.array([1.0, 2.0, -2.0, 0.0, 0.0, 0.0]), 0.5, np.zeros(9)

    def close(self):
        pass


def _recover_stream():
    from smarc_navigation_amd import synth
    st = synth.odom_stream(n_steps=40, dt=0.5)
    st['mbes_idx'] = np.arange(1, 40, 2)
    st['mbes_angles'] = synth.beam_angles(16)
    st['mbes_ranges'] = np.full((20, 16), 20.0, np.float32)
    st['truth_xyz'] = st['truth'][:, :3]
    return st


def test_replay_recover_summary_is_unchanged_without_reseed_and_gains_its_keys_with_it(eng, monkeypatch):
    from smarc_navigation_amd import replay
    monkeypatch.setattr(eng, 'Engine', FakeEngine)
    grid = dict(z=np.zeros((8, 8), np.float32), origin=(0.0, 0.0), res=1.0)
    FakeEngine.instances = []
    plain = replay.replay_recover(_recover_stream(), grid=grid, particles=64)
    assert sorted(plain['summary']) == ['final_error_vs_truth', 'injected_total', 'pf_distance', 'pf_final', 'pings']
    names = set(FakeEngine.instances[-1].names())
    assert names == {'inject_uniform'} and plain['summary']['injected_total'] > 0          # today's code path
    uniform_calls = [c for c in FakeEngine.instances[-1].calls]
    assert all(c[2:] == (None, 'map', (-math.pi, math.pi)) for c in uniform_calls)
    res = replay.replay_recover(_recover_stream(), grid=grid, particles=64, reseed=4, reseed_pitch=4.0, reseed_n_yaw=2,
                                reseed_yaw_window=0.4, reseed_select=dict(min_beams=32))
    s = res['summary']
    assert sorted(s) == sorted(list(plain['summary']) + ['reseed_calls', 'reseed_fallbacks', 'reseed_components_median',
                                                         'first_ping_within_1m_after_kidnap'])
    assert s['reseed_calls'] == int(np.count_nonzero(res['fractions'])) > 0 and s['reseed_fallbacks'] == 0
    assert s['reseed_components_median'] == 2.0 and s['first_ping_within_1m_after_kidnap'] is None      # (the fake pose never moves)
    e = FakeEngine.instances[-1]
    assert 'inject_gaussian' in e.names() and 'inject_uniform' not in e.names()
    m = [c for c in e.calls if c[0] == 'match_swath'][0]
    assert m[2].shape == (4, 16) and m[3].size == 4 and m[3][-1]['dx'] == 0.0 and m[3][0]['dx'] < 0.0      # a ring of 4 pings behind the anchor
    with pytest.raises(ValueError):
        replay.replay_recover(_recover_stream(), grid=grid, particles=64, reseed=65)


def test_the_command_line_takes_reseed_only_with_recover():
    from smarc_navigation_amd import replay
    with pytest.raises(SystemExit):
        replay.main(['synth:100', '--reseed', '4'])
    with pytest.raises(SystemExit):
        replay.main(['x.npz', '--recover', '--reseed', '65'])
    with pytest.raises(SystemExit):
        replay.main(['x.npz', '--recover', '--reseed', '4', '--reseed-pitch', '0'])


# ------------------------------------------------------------------ the sanitizer driver
def test_the_host_arithmetic_runs_clean_under_the_sanitizers_as_a_program(tmp_path):
    """tests/host_san/reseed_driver.cpp: its own main over the device-free functions, g++ -fsanitize=address,undefined, run
    as a program (nothing loaded into Python runs under a sanitizer)"""
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no g++ / make')
    san = str(tmp_path / 'host_san')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'smarc_navigation_amd', 'csrc'), 'host-asan-reseed', 'SAN_DIR=' + san],
                          stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(san, 'reseed_asan')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                       timeout=300, cwd=ROOT)
    for marker in ('AddressSanitizer', 'runtime error', 'LeakSanitizer'):
        assert marker not in p.stdout, p.stdout[-2000:]
    assert p.returncode == 0 and 'reseed_driver: ok' in p.stdout, p.stdout[-2000:]
