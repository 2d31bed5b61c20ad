"""CPU tests of the ping information (include/mcl_information.h): every symbol of the header exported and bound in a table
of its own, the device-free entry points -- matrix and merge -- against Python integers and numpy.linalg.eigh, the
stand-alone sanitizer driver of the host arithmetic, the node mirror over a recording engine, and the checks that the scene
of tests/test_gpu_information.py is well conditioned for the fp64 oracle alone at the six perturbed pose sets.  Also the
restatement of the header's definition in numpy and Python integers that the GPU tests compare the kernel with."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from smarc_navigation_amd import msgs, synth
from tests.test_innovation_host import (M2O, MAX_SAMPLES, N, OFF, OUTLIER_CAP, R_MAX, SIGMA, sample_ref, sampled_slots, scene,
                                        scene_map)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mcl_information_merge', 'mcl_information_matrix', 'mcl_ping_information', 'mcl_group_ping_information',
         'mcl_pose_information')
ERR_INVALID = -1
MAX_N = 32768
D_MAX = 1 << 23                 # the largest |d| of a contributing pair (jump_max <= 2048 m)
FIELDS = ('n', 'n_miss', 'n_jump', 'sxx', 'syy', 'sww', 'sxy', 'sxw', 'syw')
DELTA_XY, DELTA_YAW = 0.5, 0.01
VARIANTS = ((0, DELTA_XY), (0, -DELTA_XY), (1, DELTA_XY), (1, -DELTA_XY), (5, DELTA_YAW), (5, -DELTA_YAW))   # (state row, step)


# ------------------------------------------------------------------ the restatement of include/mcl_information.h
def perturbed(soa, v):
    """the state of variant v: one fp64 addition (or subtraction) on the stored number"""
    row, step = VARIANTS[v]
    s = np.array(soa, np.float64, copy=True)
    s[row] = s[row] + step if step > 0 else s[row] - (-step)
    return s


def pairs_ref(ranges6, r_max, jump_max):
    """from the six ranges of every pair (poses x 6 x B, float32): (miss, jump, dx, dy, dw) as bool / int64 arrays (poses x B)"""
    e = np.asarray(ranges6, np.float32)
    miss = np.any(e == np.float32(r_max), axis=1)
    d = [np.rint((e[:, 2 * k].astype(np.float64) - e[:, 2 * k + 1].astype(np.float64)) * 4096.0).astype(np.int64) for k in range(3)]
    jq = int(math.floor(jump_max * 4096.0))
    jump = ~miss & ((np.abs(d[0]) > jq) | (np.abs(d[1]) > jq) | (np.abs(d[2]) > jq))
    return miss, jump, d[0], d[1], d[2]


def _record(miss, jump, dx, dy, dw):
    use = ~miss & ~jump
    if int(use.sum()) << 48 < 1 << 62:      # |d| <= 2^24: the products of so few pairs add up inside an int64
        x, y, w = dx[use], dy[use], dw[use]
        return (int(miss.size), int(miss.sum()), int(jump.sum()), int(np.sum(x * x)), int(np.sum(y * y)), int(np.sum(w * w)),
                int(np.sum(x * y)), int(np.sum(x * w)), int(np.sum(y * w)))
    x, y, w = ([int(v) for v in a[use]] for a in (dx, dy, dw))
    return (int(miss.size), int(miss.sum()), int(jump.sum()), sum(v * v for v in x), sum(v * v for v in y), sum(v * v for v in w),
            sum(a * b for a, b in zip(x, y)), sum(a * b for a, b in zip(x, w)), sum(a * b for a, b in zip(y, w)))


def records_ref(ranges6, r_max, jump_max, per_pose=False):
    """the nine integers per beam (or per pose) from the dumped ranges and the definition, as Python integers"""
    miss, jump, dx, dy, dw = pairs_ref(ranges6, r_max, jump_max)
    if per_pose:
        return [_record(miss[k], jump[k], dx[k], dy[k], dw[k]) for k in range(miss.shape[0])]
    return [_record(miss[:, b], jump[:, b], dx[:, b], dy[:, b], dw[:, b]) for b in range(miss.shape[1])]


def matrix_ref(recs, sigma, delta_xy=DELTA_XY, delta_yaw=DELTA_YAW, per_pose=False):
    """J (packed xx, xy, xw, yy, yw, ww) and hit_share from Python integers, one rounding per IEEE operation (int -> float is
    the nearest double); per_pose: a list, one per record"""
    dl = (delta_xy, delta_xy, delta_yaw)
    q = [(4.0 * dl[j]) * dl[k] for j, k in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    s2 = sigma * sigma

    def six(r):
        return [float(int(r[i])) for i in (3, 6, 7, 4, 8, 5)]
    if per_pose:
        out = []
        for r in recs:
            n, m = int(r[0]), int(r[0]) - int(r[1]) - int(r[2])
            out.append(([s / ((16777216.0 * qq) * s2) for s, qq in zip(six(r), q)], float(m) / float(n) if n > 0 else 0.0))
        return out
    J = [0.0] * 6
    sum_m = sum_n = 0
    for r in recs:
        m = int(r[0]) - int(r[1]) - int(r[2])
        sum_n += int(r[0])
        if m <= 0:
            continue
        sum_m += m
        mm = float(m) * 16777216.0
        J = [acc + s / (mm * qq) for acc, s, qq in zip(J, six(r), q)]
    return [v / s2 for v in J], (float(sum_m) / float(sum_n) if sum_n > 0 else 0.0)


def schur_ref(J):
    """the 2 x 2 position information with yaw marginalised, the header's operations in the header's order"""
    a, b, c = J[0], J[1], J[3]
    if J[5] != 0.0:
        a = J[0] - (J[2] * J[2]) / J[5]
        b = J[1] - (J[2] * J[4]) / J[5]
        c = J[3] - (J[4] * J[4]) / J[5]
        if a + c <= (J[0] + J[3]) * 2.0 ** -40:
            a = b = c = 0.0
    return a, b, c


def records_array(recs):
    from smarc_navigation_amd import engine as eng
    a = np.zeros(len(recs), eng.INFORMATION_SUMS)
    for k, r in enumerate(recs):
        a[k] = tuple(int(v) for v in r)
    return a


def record_of(triples, n_miss=0, n_jump=0):
    t = [(int(x), int(y), int(w)) for x, y, w in triples]
    return (len(t) + n_miss + n_jump, n_miss, n_jump, sum(x * x for x, _, _ in t), sum(y * y for _, y, _ in t),
            sum(w * w for _, _, w in t), sum(x * y for x, y, _ in t), sum(x * w for x, _, w in t), sum(y * w for _, y, w in t))


def ints(rec):
    return [tuple(int(rec[f][k]) for f in FIELDS) for k in range(rec.size)]


def random_record(rs, n=None, scale=None):
    n = int(rs.choice([0, 1, 2, 7, 100, 820, 4096])) if n is None else n
    scale = int(rs.choice([1, 50, 4096, 1 << 16, D_MAX])) if scale is None else scale
    t = np.clip((rs.randn(n, 3) * scale * np.array([1.0, 0.3, 0.1]) + rs.randn(3) * scale).round().astype(np.int64), -D_MAX, D_MAX)
    return record_of(t, int(rs.randint(0, 5)), int(rs.randint(0, 5)))


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
    from smarc_navigation_amd import _lib, engine
    src = open(os.path.join(ROOT, 'include', 'mcl_information.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(NAMES) == sorted(_lib.INFORMATION_SYMBOLS)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    others = [_lib.SYMBOLS, _lib.RECOVERY_SYMBOLS, _lib.MODES_SYMBOLS, _lib.HISTORY_SYMBOLS, _lib.ACOUSTIC_SYMBOLS,
              _lib.TEMPER_SYMBOLS, _lib.DRIFT_SYMBOLS, _lib.REGULARISE_SYMBOLS, _lib.QUANTILE_SYMBOLS, _lib.INNOVATION_SYMBOLS]
    for t in others:
        assert not set(t) & set(NAMES)
    assert lib.mcl_abi_version() == 4
    assert engine.INFORMATION_SUMS.itemsize == 72 and engine.INFORMATION_RESULT.itemsize == 104
    assert ctypes.sizeof(_lib.InformationSteps) == 24
    assert ctypes.sizeof(_lib.Timing) == 15 * 16                 # no timing slot was added
    hdr = open(os.path.join(ROOT, 'include', 'mcl.h')).read()
    assert 'mcl_information' not in hdr and 'ping_information' not in hdr   # mcl.h is what it was


# ------------------------------------------------------------------ the matrix
def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def test_matrix_J_against_python_integers_bit_for_bit_on_random_records(eng):
    rs = np.random.RandomState(2)
    for trial in range(60):
        B = int(rs.randint(1, 40))
        sigma = float(rs.choice([0.05, 0.2, 1.0, 3.7]))
        dxy, dyaw = float(rs.choice([0.5, 0.25, 0.3, 1.7])), float(rs.choice([0.01, 0.003, 0.05]))
        recs = [random_record(rs) for _ in range(B)]
        got = eng.information_matrix(records_array(recs), sigma, dxy, dyaw)
        J, share = matrix_ref(recs, sigma, dxy, dyaw)
        assert all(_same(g, w) for g, w in zip(got['J'], J)), (trial, list(got['J']), J)
        assert _same(got['hit_share'], share)
        per = eng.information_matrix(records_array(recs), sigma, dxy, dyaw, per_pose=True)
        for k, (Jk, sk) in enumerate(matrix_ref(recs, sigma, dxy, dyaw, per_pose=True)):
            assert all(_same(g, w) for g, w in zip(per['J'][k], Jk)) and _same(per['hit_share'][k], sk), (trial, k)


def _check_eigen(res):
    """one result of the library against numpy.linalg.eigh of the restated Schur complement, at fp64 round-off"""
    a, b, c = schur_ref([float(v) for v in res['J']])
    lam, vec = np.linalg.eigh(np.array([[a, b], [b, c]]))
    lmin, lmax = float(lam[0]), float(lam[1])
    if not lmax > 0.0:
        assert res['rank_pos'] == 0 and res['lambda_max'] == 0.0 and np.isinf(res['crlb_strong']) and np.isinf(res['crlb_weak'])
        return
    assert abs(res['lambda_max'] - lmax) <= 1e-12 * lmax
    assert abs(res['lambda_min'] - max(lmin, 0.0)) <= 1e-12 * lmax
    assert res['lambda_max'] >= res['lambda_min'] >= 0.0 and 0.0 <= res['weak_axis'] < math.pi
    if lmax - lmin > 1e-3 * lmax:
        axis = math.atan2(vec[1, 0], vec[0, 0]) % math.pi       # the eigenvector of lambda_min
        diff = abs(res['weak_axis'] - axis)
        assert min(diff, math.pi - diff) <= 1e-9, (res['weak_axis'], axis)
    assert res['crlb_strong'] == 1.0 / math.sqrt(res['lambda_max'])
    if res['lambda_min'] <= 2.0 ** -40 * res['lambda_max']:
        assert res['rank_pos'] == 1 and np.isinf(res['crlb_weak'])
    else:
        assert res['rank_pos'] == 2 and res['crlb_weak'] == 1.0 / math.sqrt(res['lambda_min'])


def test_eigen_quantities_against_numpy_eigh(eng):
    rs = np.random.RandomState(3)
    seen = set()
    for trial in range(200):
        B = int(rs.randint(1, 12))
        recs = [random_record(rs, n=int(rs.choice([3, 50, 700])), scale=int(rs.choice([50, 4096, 1 << 16]))) for _ in range(B)]
        if trial % 3 == 0:      # no yaw information at all: J_ww == 0, the position block itself
            recs = [r[:5] + (0,) + r[6:7] + (0, 0) for r in recs]
        arr = records_array(recs)
        one = eng.information_matrix(arr, 0.2)
        _check_eigen(one)
        seen.add(int(one['rank_pos']))
        for r in eng.information_matrix(arr, 0.2, per_pose=True):
            _check_eigen(r)
    assert 2 in seen


def test_matrix_edges(eng):
    sigma = 0.2
    zero = (0,) * 9
    # the all-zero record: nothing is known
    r = eng.information_matrix(records_array([zero]), sigma)
    assert r['rank_pos'] == 0 and np.isinf(r['crlb_strong']) and np.isinf(r['crlb_weak']) and r['hit_share'] == 0.0
    assert not r['J'].any() and r['lambda_max'] == 0.0 and r['weak_axis'] == 0.0
    # rank 0 with information about yaw only (a flat seabed under a tilted fan)
    r = eng.information_matrix(records_array([record_of([(0, 0, 40)] * 10)]), sigma)
    assert r['rank_pos'] == 0 and np.isinf(r['crlb_weak']) and r['J'][5] > 0 and r['hit_share'] == 1.0
    # J_ww == 0: the position block itself; a ridge across x is rank 1, and y is the weak axis
    ridge = record_of([(4096, 0, 0)] * 100, 3, 2)
    r = eng.information_matrix(records_array([ridge]), sigma)
    assert r['J'][5] == 0.0 and r['rank_pos'] == 1 and r['weak_axis'] == math.pi / 2 and np.isinf(r['crlb_weak'])
    assert r['J'][0] == 1.0 / (sigma * sigma) and r['crlb_strong'] == 1.0 / math.sqrt(r['J'][0]) and r['hit_share'] == 100.0 / 105.0
    # ... across y: x is the weak axis; across the diagonal: the other diagonal
    assert eng.information_matrix(records_array([record_of([(0, 7, 0)] * 9)]), sigma)['weak_axis'] == 0.0
    r = eng.information_matrix(records_array([record_of([(500, 500, 0)] * 9)]), sigma)
    assert r['rank_pos'] == 1 and abs(r['weak_axis'] - 3 * math.pi / 4) < 1e-15
    # yaw explains everything (d_x = 2 d_w in every pair): what the Schur complement leaves is rounding -- rank 0
    r = eng.information_matrix(records_array([record_of([(74 * k, 0, 37 * k) for k in range(1, 51)])]), sigma)
    assert r['J'][0] > 0 and r['rank_pos'] == 0 and np.isinf(r['crlb_strong'])
    # beams with m == 0 are skipped, in J; they count in the hit share
    rs = np.random.RandomState(5)
    full = random_record(rs, n=64, scale=4096)
    a = eng.information_matrix(records_array([full]), sigma)
    b = eng.information_matrix(records_array([zero, full, (7, 7, 0, 0, 0, 0, 0, 0, 0), (4, 1, 3, 0, 0, 0, 0, 0, 0)]), sigma)
    assert a['J'].tobytes() == b['J'].tobytes() and a['rank_pos'] == b['rank_pos'] == 2
    m = full[0] - full[1] - full[2]
    assert b['hit_share'] == float(m) / float(full[0] + 11)
    # the largest legal sums stay finite
    top = record_of([(D_MAX, -D_MAX, D_MAX)] * MAX_N)
    assert top[3] == 1 << 61 and top[6] == -(1 << 61)
    assert np.isfinite(eng.information_matrix(records_array([top]), sigma)['J']).all()


def test_merge_adds_field_wise_is_associative_and_refuses_overflow(eng):
    rs = np.random.RandomState(4)
    B = 9
    parts = [records_array([random_record(rs, n=int(rs.randint(0, 3000))) for _ in range(B)]) for _ in range(4)]
    whole = eng.merge_information(parts)
    for f in FIELDS:
        assert [int(v) for v in whole[f]] == [sum(int(p[f][b]) for p in parts) for b in range(B)]
    left = eng.merge_information([eng.merge_information(parts[:2]), eng.merge_information(parts[2:])])
    right = eng.merge_information([parts[3], eng.merge_information([parts[1], eng.merge_information([parts[2], parts[0]])])])
    assert whole.tobytes() == left.tobytes() == right.tobytes()
    assert eng.merge_information([parts[0]]).tobytes() == parts[0].tobytes()
    full = records_array([record_of([(D_MAX, D_MAX, -D_MAX)] * MAX_N)])
    one = records_array([record_of([(1, 1, 1)])])
    assert int(eng.merge_information([full])['sxx'][0]) == 1 << 61
    for over in ([full, one], [full, full], [records_array([(20000, 20000, 0, 0, 0, 0, 0, 0, 0)])] * 2):
        with pytest.raises(eng.MclError) as ei:
            eng.merge_information(over)
        assert ei.value.status == ERR_INVALID
    with pytest.raises(eng.MclError):
        eng.merge_information([records_array([(5, 6, 0, 0, 0, 0, 0, 0, 0)]), one])      # a part that is no record


def test_impossible_records_and_arguments_are_refused(eng):
    bad = [(-1, 0, 0, 0, 0, 0, 0, 0, 0), (MAX_N + 1, 0, 0, 0, 0, 0, 0, 0, 0), (10, 11, 0, 0, 0, 0, 0, 0, 0),
           (10, 6, 5, 0, 0, 0, 0, 0, 0), (10, -1, 0, 0, 0, 0, 0, 0, 0), (10, 0, -1, 0, 0, 0, 0, 0, 0),
           (10, 0, 0, (10 << 46) + 1, 0, 0, 0, 0, 0), (10, 5, 5, 1, 0, 0, 0, 0, 0), (10, 0, 0, 100, 100, 0, 101, 0, 0),
           (10, 0, 0, 100, 0, 100, 0, -101, 0), (10, 0, 0, 0, 100, 100, 0, 0, 101), (10, 0, 0, 0, 0, 0, 1, 0, 0),
           (10, 0, 0, 1, 1, 1, -(1 << 63), 0, 0)]
    for r in bad:
        for per_pose in (False, True):
            with pytest.raises(eng.MclError) as ei:
                eng.information_matrix(records_array([r]), 0.2, per_pose=per_pose)
            assert ei.value.status == ERR_INVALID, r
    ok = records_array([(10, 0, 0, 100, 100, 100, 100, -100, 100)])
    assert eng.information_matrix(ok, 0.2)['rank_pos'] in (0, 1, 2)
    for v in (0.0, -1.0, math.nan, math.inf):
        for args in ((v, 0.5, 0.01), (0.2, v, 0.01), (0.2, 0.5, v)):
            with pytest.raises(eng.MclError):
                eng.information_matrix(ok, *args)


def test_null_pointers_are_refused(lib):
    from smarc_navigation_amd import _lib
    i = ctypes.c_int64(0)
    buf = (ctypes.c_uint64 * 32)()
    f = (ctypes.c_float * 4)()
    d = (ctypes.c_double * 6)()
    st = _lib.InformationSteps(0.5, 0.01, 50.0)
    assert lib.mcl_information_merge(None, 1, 1, buf) == ERR_INVALID and lib.mcl_information_merge(buf, 1, 1, None) == ERR_INVALID
    assert lib.mcl_information_merge(buf, 0, 1, buf) == ERR_INVALID and lib.mcl_information_merge(buf, 1, 0, buf) == ERR_INVALID
    assert lib.mcl_information_matrix(None, 1, 0, 0.2, 0.5, 0.01, buf) == ERR_INVALID
    assert lib.mcl_information_matrix(buf, 1, 0, 0.2, 0.5, 0.01, None) == ERR_INVALID
    assert lib.mcl_information_matrix(buf, 0, 0, 0.2, 0.5, 0.01, buf) == ERR_INVALID
    assert lib.mcl_information_matrix(buf, 1, 0, 0.2, 0.5, 0.01, buf) == 0
    assert lib.mcl_ping_information(None, f, 1, 50.0, None, 4096, ctypes.byref(st), buf, None, ctypes.byref(i)) == ERR_INVALID
    assert lib.mcl_pose_information(None, d, 1, f, 1, 50.0, None, ctypes.byref(st), buf) == ERR_INVALID
    none = (ctypes.c_void_p * 1)(None)
    assert lib.mcl_group_ping_information(None, 1, f, 1, 50.0, None, 4096, ctypes.byref(st), buf, ctypes.byref(i)) == ERR_INVALID
    assert lib.mcl_group_ping_information(none, 1, f, 1, 50.0, None, 4096, ctypes.byref(st), buf, ctypes.byref(i)) == ERR_INVALID


def test_steps_object_defaults_are_the_policy(eng):
    s = eng.make_information_steps(80.0)
    assert (s.delta_xy, s.delta_yaw, s.jump_max) == (0.5, 0.01, 80.0)
    assert eng.make_information_steps(4096.0).jump_max == 2048.0 and eng.make_information_steps(80.0, jump_max=1.0).jump_max == 1.0


def test_the_host_arithmetic_runs_clean_under_the_sanitizers_as_a_program(tmp_path):
    """tests/host_san/information_driver.cpp: its own main over the device-free functions, g++ -fsanitize=address,undefined,
    run as a program (nothing loaded into Python runs under a sanitizer)"""
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no g++ / make')
    san = str(tmp_path / 'host_san')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'smarc_navigation_amd', 'csrc'), 'host-asan-information',
                           'SAN_DIR=' + san], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(san, 'information_asan')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=300, cwd=ROOT)
    for marker in ('AddressSanitizer', 'runtime error', 'LeakSanitizer'):
        assert marker not in p.stdout, p.stdout[-2000:]
    assert p.returncode == 0 and 'information_driver: ok' in p.stdout, p.stdout[-2000:]


# ------------------------------------------------------------------ the scene of the GPU tests, for the oracle alone
@pytest.fixture(scope='module')
def oracle_ranges():
    """per map kind: the oracle's fp64 ranges of the scene's sample at the six perturbed pose sets (6 x 586 x 300), cast once"""
    from oracle import oracle as orc
    z, origin, soa = scene()
    stride, _ = sample_ref(N, MAX_SAMPLES)
    sub = np.ascontiguousarray(soa[:, sampled_slots(N, stride)])
    ba = synth.beam_angles(300)
    out = {}

    def get(kind):
        if kind not in out:
            _, omap = scene_map(kind, z, origin)
            out[kind] = (omap, sub, ba, np.stack([orc.mbes_update(perturbed(sub, v), M2O, OFF, omap, ba, None, SIGMA, R_MAX)[1]
                                                  for v in range(6)]))
        return out[kind]
    return get


@pytest.mark.parametrize('kind', ['grid', 'tin'])
def test_the_oracle_alone_keeps_the_gpu_scene_within_the_outlier_cap_at_the_six_pose_sets(oracle_ranges, kind):
    """the rays whose fp64 answer jumps when the sensor moves by 1 mm are the ones a fp32 cast may miss by more than 1e-3 m
    (helpers.outliers_explained excuses exactly those): at each of the six perturbed pose sets of the scene of
    test_gpu_information.py their share stays under the cap"""
    from oracle import oracle as orc
    omap, sub, ba, ref = oracle_ranges(kind)
    assert sub.shape[1] == 586
    moved = np.zeros(ref.shape, bool)
    for v in range(6):
        base = perturbed(sub, v)
        for axis in range(3):
            for sgn in (1.0, -1.0):
                s = base.copy()
                s[axis] += sgn * 1e-3
                _, ex = orc.mbes_update(s, M2O, OFF, omap, ba, None, SIGMA, R_MAX)
                moved[v] |= np.abs(ex - ref[v]) > 0.1
    hit = np.all(ref < R_MAX, axis=0)
    diff = np.abs(ref[0::2] - ref[1::2])[:, hit]
    print('%s: %d of %d rays jump under a 1 mm shift; all six rays hit for %.1f %% of the pairs; largest |e+ - e-| %.2f m'
          % (kind, int(moved.sum()), moved.size, 100.0 * hit.mean(), diff.max()))
    assert moved.mean() < OUTLIER_CAP
    assert 0.9 < hit.mean() < 1.0       # the 21 samples past the edge miss; almost every other pair contributes


@pytest.mark.parametrize('kind', ['grid', 'tin'])
def test_on_the_oracle_a_jump_limit_of_one_metre_excludes_some_pairs_and_not_all(oracle_ranges, kind):
    _, _, _, ref = oracle_ranges(kind)
    e = np.ascontiguousarray(np.transpose(ref, (1, 0, 2))).astype(np.float32)       # poses x 6 x B
    miss, jump, _, _, _ = pairs_ref(e, R_MAX, 1.0)
    none = pairs_ref(e, R_MAX, R_MAX)[1]
    print('%s: %d misses, %d jumps at 1 m, %d at r_max, of %d pairs' % (kind, miss.sum(), jump.sum(), none.sum(), miss.size))
    assert 0 < jump.sum() < (~miss).sum() and none.sum() == 0


# ------------------------------------------------------------------ the node mirror over a recording engine
class RecordingEngine(object):
    calls = []

    def __init__(self, n, **kw):
        self.n = n
        RecordingEngine.calls.append(('create', (n,), kw))

    def __getattr__(self, name):
        def f(*a, **k):
            RecordingEngine.calls.append((name, a, k))
            if name == 'mean_cov':
                return np.zeros(6), 0.0, np.zeros(9)
            if name == 'resample_prepare':
                return 1
            if name == 'ping_information':
                class Info(object):
                    crlb_strong, crlb_weak, weak_axis, rank_pos, hit_share = 0.25, math.inf, math.pi / 2, 1, 0.9
                return Info()
            return None
        return f


@pytest.fixture
def node(monkeypatch):
    from smarc_navigation_amd import auv_pf, engine as e
    monkeypatch.setattr(e, 'Engine', RecordingEngine)
    RecordingEngine.calls = []
    return auv_pf


def _drive(pf, pings=7):
    pf.start_timing(100.0)
    pf.set_map_grid(np.full((8, 8), -20.0, np.float32), (-4.0, -4.0), 1.0)
    ranges = np.array([18.0, 18.5, 19.0, 18.2], np.float32)
    scan = msgs.LaserScan(ranges, -0.3, 0.2, 60.0)
    a = -0.3 + 0.2 * np.arange(4)
    pc = msgs.pointcloud2_from_xyz(np.stack([np.zeros(4), ranges * np.sin(a), -ranges * np.cos(a)], axis=1), 'base')
    for k in range(pings):
        m = msgs.Odometry()
        m.header.stamp = msgs.Time(100.02 + 0.02 * k)
        m.twist.twist.linear.x = 1.0
        m.pose.pose.orientation = msgs.Quaternion(0.0, 0.0, 0.0, 1.0)
        pf.odom_callback(m)
        pf.mbes_cb(scan) if k % 3 < 2 else pf.mbes_pc_cb(pc)


def test_node_off_the_call_sequence_is_todays_and_on_one_call_before_every_kth_update(node, caplog):
    import logging
    assert node.DEFAULT_PARAMS['mbes_information_every'] == 0
    pf = node.auv_pf({'particle_count': 16})
    _drive(pf)
    plain = list(RecordingEngine.calls)
    names = [c[0] for c in plain]
    assert names.count('update_mbes') == 7 and 'ping_information' not in names
    assert pf.last_information is None and pf.information_calls == 0
    RecordingEngine.calls = []
    pf = node.auv_pf({'particle_count': 16, 'mbes_information_every': 0})
    _drive(pf)
    assert repr(RecordingEngine.calls) == repr(plain)
    RecordingEngine.calls = []
    with caplog.at_level(logging.INFO, logger='auv_pf'):
        pf = node.auv_pf({'particle_count': 16, 'mbes_information_every': 3})
        _drive(pf)
    on = list(RecordingEngine.calls)
    assert repr([c for c in on if c[0] != 'ping_information']) == repr(plain)       # everything else: today's sequence
    names = [c[0] for c in on]
    assert names.count('ping_information') == 3 and names.count('update_mbes') == 7     # pings 0, 3, 6
    ups = [i for i, c in enumerate(on) if c[0] == 'update_mbes']
    for i, c in enumerate(on):
        if c[0] != 'ping_information':
            continue
        u = on[i + 1]
        assert u[0] == 'update_mbes' and ups.index(i + 1) % 3 == 0            # right in front of the update of every 3rd ping
        assert np.array_equal(c[1][0], u[1][1]) and repr(c[1][1:]) == repr(u[1][2:]) and c[2] == {}   # its angles, sigma, r_max, offset
    assert pf.information_calls == 3 and len(pf.information_log) == 3 and pf.last_information.rank_pos == 1
    said = [r for r in caplog.records if 'ping information' in r.getMessage()]
    assert len(said) == 1                                                     # throttled: the pings are 20 ms apart


@pytest.mark.parametrize('bad', [-1, 2.5, float('nan')])
def test_node_refuses_a_period_that_means_nothing(node, bad):
    with pytest.raises(ValueError):
        node.auv_pf({'particle_count': 8, 'mbes_information_every': bad})


def test_launch_file_passes_the_parameter():
    import xml.etree.ElementTree as ET
    from smarc_navigation_amd import auv_pf
    root = ET.parse(os.path.join(ROOT, 'ros', 'auv_particle_filter_hip', 'launch', 'auv_pf.launch')).getroot()
    args = {a.get('name'): a.get('default') for a in root.iter('arg')}
    params = {p.get('name'): p for p in next(root.iter('node')).iter('param')}
    assert int(args['mbes_information_every']) == auv_pf.DEFAULT_PARAMS['mbes_information_every'] == 0
    assert params['mbes_information_every'].get('type') == 'int'
    assert params['mbes_information_every'].get('value') == '$(arg mbes_information_every)'
