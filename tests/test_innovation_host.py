"""CPU tests of the ping innovation statistics (include/mcl_innovation.h): every symbol of the header exported and bound in
a table of its own, the device-free entry points -- sample, gate, merge, direction table -- against Python integers, the
stand-alone sanitizer driver of the host arithmetic, the node mirror over a recording engine, and the check that the scene
of tests/test_gpu_innovation.py is well conditioned for the fp64 oracle alone.  Also the restatement of the header's
definition in numpy and Python integers that the GPU tests compare the kernel with."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from smarc_navigation_amd import msgs, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mcl_innovation_dirs', 'mcl_innovation_sample', 'mcl_innovation_merge', 'mcl_innovation_gate',
         'mcl_ping_innovation', 'mcl_group_ping_innovation')
ERR_INVALID = -1
Q_MAX, MAX_N = 1 << 24, 32768
OUTLIER_CAP = 2e-3      # share of rays beyond the tolerance the MBES tests allow (tests/test_gpu_mbes.py: rough terrain)


# ------------------------------------------------------------------ the restatement of include/mcl_innovation.h
def sample_ref(n_global, max_samples):
    stride = -(-n_global // max_samples)
    return stride, -(-n_global // stride)


def sampled_slots(n, stride, global_offset=0):
    g = np.arange(global_offset, global_offset + n)
    return np.nonzero(g % stride == 0)[0]


def quantise_ref(r, e):
    """q of one float32 range against float32 expected ranges, as int64"""
    x = (np.float64(np.float32(r)) - np.asarray(e, np.float32).astype(np.float64)) * 4096.0
    return np.rint(np.clip(x, -float(Q_MAX), float(Q_MAX))).astype(np.int64)


def records_ref(ranges, expected, sigma, support_k, r_max):
    """the five integers per beam from the dumped e (samples x B, float32) and the definition, as Python integers"""
    ranges = np.asarray(ranges, np.float32)
    q_support = min(int(math.floor(support_k * sigma * 4096.0)), Q_MAX)
    out = []
    for b in range(ranges.size):
        if not ranges[b] > 0:                      # zero, negative, NaN
            out.append((0, 0, 0, 0, 0))
            continue
        e = expected[:, b]
        q = quantise_ref(ranges[b], e)
        out.append((int(q.size), int(np.sum(e == np.float32(r_max))), int(np.sum(np.abs(q) <= q_support)),
                    sum(int(v) for v in q), sum(int(v) * int(v) for v in q)))
    return out


def derive_ref(rec, sigma):
    n, _, n_within, s1, s2 = [int(v) for v in rec]
    if n <= 0:
        return 0.0, 0.0, 0.0, 0.0
    nf = float(n)
    nu = float(s1) / (nf * 4096.0)
    var = float(n * s2 - s1 * s1) / (nf * nf) * 2.0 ** -24      # (int -> float: the nearest double, ties to even)
    return nu, var, (nu * nu) / (var + sigma * sigma), float(n_within) / nf


def gate_ref(recs, sigma, nis_gate=10.83, min_support=0.01, max_gated_fraction=0.25):
    d = [derive_ref(r, sigma) for r in recs]
    valid = [int(r[0]) > 0 for r in recs]
    cand = [v and x[2] > nis_gate and x[3] < min_support for v, x in zip(valid, d)]
    n_valid, n_cand = sum(valid), sum(cand)
    inconsistent = float(n_cand) > max_gated_fraction * float(n_valid)
    nis_sum = nu_sum = 0.0
    for v, x in zip(valid, d):
        if v:
            nis_sum += x[2]
            nu_sum += x[0]
    return dict(d=d, mask=[c and not inconsistent for c in cand], n_valid=n_valid, n_candidates=n_cand,
                n_gated=0 if inconsistent else n_cand, inconsistent=inconsistent, nis_sum=nis_sum,
                mean_nu=nu_sum / n_valid if n_valid else 0.0)


def records_array(recs):
    from smarc_navigation_amd import engine as eng
    a = np.zeros(len(recs), eng.INNOVATION_BEAM)
    for k, r in enumerate(recs):
        a[k] = tuple(int(v) for v in r)
    return a


def record_of(q, n_within=None):
    q = [int(v) for v in q]
    return (len(q), 0, len(q) if n_within is None else n_within, sum(q), sum(v * v for v in q))


# ------------------------------------------------------------------ the scene the GPU tests share
SIGMA, R_MAX, N = 0.2, 80.0, 4096
M2O = synth.rigid_matrix(1.0, -2.0, 0.0, 0.0, 0.0, 0.2)
OFF = [0.3, -0.1, -0.2, 0.01, -0.02, 0.05]
MAX_SAMPLES = 600       # stride 7 does not divide 4096; 586 samples are no multiple of 4, 7 or 64


def scene(n=N, seed=5):
    """(z, origin, soa): a height grid of 160 x 192 nodes and a cloud of n particles over it; the particles of every
    203rd slot -- sampled ones at stride 7 -- stand past the map's edge, where every ray misses"""
    origin = (-60.0, -110.0)
    z = synth.bathymetry_grid(160, 192, 1.0, origin, seed=seed)
    rs = np.random.RandomState(seed)
    soa = rs.randn(6, n) * np.array([3.0, 3.0, 0.3, 0.05, 0.05, 3.0])[:, None]
    soa[0] += 20.0
    soa[1] += -10.0
    soa[2] += -2.0
    soa[0, ::203] += 200.0
    return z, origin, soa


def scene_map(kind, z, origin):
    """(what Engine.set_map_* takes, the oracle's map) for 'grid', 'mesh' (a regular mesh) and 'tin' (triangle records)"""
    from oracle import oracle as orc
    if kind == 'grid':
        return ('grid', (z, origin, 1.0)), orc.Grid(z, origin, 1.0)
    verts, tris = synth.mesh_from_grid(z, 1.0, origin) if kind == 'mesh' else synth.mesh_tin(z, 1.0, origin, seed=3)
    return ('mesh', (verts, tris)), orc.Mesh(verts, tris)


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
    src = open(os.path.join(ROOT, 'include', 'mcl_innovation.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(NAMES) == sorted(_lib.INNOVATION_SYMBOLS)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    others = [_lib.SYMBOLS, _lib.RECOVERY_SYMBOLS, _lib.MODES_SYMBOLS, _lib.HISTORY_SYMBOLS, _lib.ACOUSTIC_SYMBOLS,
              _lib.TEMPER_SYMBOLS, _lib.DRIFT_SYMBOLS, _lib.REGULARISE_SYMBOLS, _lib.QUANTILE_SYMBOLS]
    for t in others:
        assert not set(t) & set(NAMES)
    assert lib.mcl_abi_version() == 4
    from smarc_navigation_amd import engine
    assert engine.INNOVATION_BEAM.itemsize == 40 and engine.INNOVATION_DERIVED.itemsize == 40
    assert ctypes.sizeof(_lib.InnovationGateConfig) == 24 and ctypes.sizeof(_lib.InnovationVerdict) == 32
    assert ctypes.sizeof(_lib.Timing) == 15 * 16                 # no timing slot was added
    hdr = open(os.path.join(ROOT, 'include', 'mcl.h')).read()
    assert 'mcl_innovation' not in hdr and 'ping_innovation' not in hdr   # mcl.h, its config and its timing table are what they were


def test_sample_against_the_restatement_and_its_refusals(eng):
    rs = np.random.RandomState(1)
    pairs = [(1, 1), (1, 32768), (10, 4096), (4096, 4096), (4097, 4096), (4096, 1000), (1 << 20, 4096), (1 << 20, 32768),
             ((1 << 32) - 1, 32768), (32768, 32768), (32769, 32768), (5, 1)]
    pairs += [(int(rs.randint(1, 1 << 22)), int(rs.randint(1, 32769))) for _ in range(500)]
    pairs += [(int(rs.randint(1, 3000)), int(rs.randint(2000, 32769))) for _ in range(100)]      # n_global < max_samples
    for ng, ms in pairs:
        stride, count = eng.innovation_sample(ng, ms)
        assert (stride, count) == sample_ref(ng, ms), (ng, ms)
        assert 1 <= count <= ms
        if ng <= 5000:
            assert count == sampled_slots(ng, stride).size
    for ng, ms in [(0, 1), (-5, 4096), (100, 0), (100, -1), (100, 32769)]:
        with pytest.raises(eng.MclError) as ei:
            eng.innovation_sample(ng, ms)
        assert ei.value.status == ERR_INVALID


def test_dirs_are_the_normalised_float_triples(eng):
    a = np.array([0.0, 0.5, -1.0, 1.4835, -3.0, 1e-8], np.float32)
    d = eng.innovation_dirs(a)
    raw = np.stack([np.zeros(a.size), np.sin(a.astype(np.float64)), -np.cos(a.astype(np.float64))], axis=1).astype(np.float32)
    want = (raw.astype(np.float64) / np.linalg.norm(raw.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    assert np.abs(d - want).max() <= 2.0 ** -23 and np.all(d[:, 0] == 0.0)
    assert np.array_equal(d[0], [0.0, 0.0, -1.0])
    for bad in ([math.nan], [math.inf], []):
        with pytest.raises(eng.MclError):
            eng.innovation_dirs(np.array(bad, np.float32))


def _same_float(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _check_gate(eng, recs, sigma, **cfg):
    got = eng.innovation_gate(records_array(recs), sigma, **cfg)
    ref = gate_ref(recs, sigma, **cfg)
    assert [bool(m) for m in got.mask] == ref['mask']
    assert (got.n_valid, got.n_candidates, got.n_gated, got.inconsistent) == (
        ref['n_valid'], ref['n_candidates'], ref['n_gated'], ref['inconsistent'])
    for b, d in enumerate(ref['d']):
        assert _same_float(got.nu[b], d[0]) and _same_float(got.var[b], d[1]) and _same_float(got.nis[b], d[2]) and \
            _same_float(got.support[b], d[3]), (b, recs[b], d, got.nu[b], got.var[b], got.nis[b])
    assert _same_float(got.nis_sum, ref['nis_sum']) and _same_float(got.mean_nu, ref['mean_nu'])
    # the Python mirror the result objects use says the same
    nu, var, nis, sup = eng.innovation_derived(records_array(recs), sigma)
    for b, d in enumerate(ref['d']):
        assert _same_float(nu[b], d[0]) and _same_float(var[b], d[1]) and _same_float(nis[b], d[2]) and _same_float(sup[b], d[3])
    return got


def test_gate_against_python_integers_bit_for_bit_on_random_records(eng):
    rs = np.random.RandomState(2)
    for trial in range(40):
        B = int(rs.randint(1, 40))
        sigma = float(rs.choice([0.05, 0.2, 1.0, 3.7]))
        recs = []
        for b in range(B):
            n = int(rs.choice([0, 1, 2, 7, 100, 820, 4096, MAX_N]))
            scale = int(rs.choice([1, 50, 4096, 1 << 16, Q_MAX]))
            q = np.clip((rs.randn(n) * scale + rs.randn() * scale).round().astype(np.int64), -Q_MAX, Q_MAX)
            nw = int(np.sum(np.abs(q) <= int(3 * sigma * 4096)))
            recs.append((n, int(rs.randint(0, n + 1)), nw, int(q.sum()), int((q * q).astype(np.uint64).sum())))
        _check_gate(eng, recs, sigma)
        _check_gate(eng, recs, sigma, nis_gate=float(rs.rand() * 5), min_support=float(rs.rand()), max_gated_fraction=float(rs.rand()))


def test_gate_edges(eng):
    sigma = 0.2
    q20 = int(round(20 * sigma * 4096))
    cand, clean = record_of([-q20] * 100, 0), record_of([0] * 100)
    # n = 0: not valid, nothing derived, never gated; alone: no valid beam at all
    g = _check_gate(eng, [(0, 0, 0, 0, 0)], sigma)
    assert g.n_valid == 0 and not g.inconsistent and g.mean_nu == 0.0 and g.nis_sum == 0.0
    g = _check_gate(eng, [(0, 0, 0, 0, 0), cand, clean, clean, clean, clean], sigma)
    assert g.n_valid == 5 and list(g.mask) == [False, True, False, False, False, False]
    # V = 0 exactly: every residual the same
    g = _check_gate(eng, [record_of([12345] * 77), record_of([-Q_MAX] * MAX_N), record_of([Q_MAX] * MAX_N)], sigma)
    assert np.all(g.var == 0.0) and g.nu[1] == -4096.0 and g.nu[2] == 4096.0
    # the largest legal s2: 2^63, with s1 = 0 (V = 2^24 m^2) and with s1 = 2^39 (V = 0)
    half = record_of([Q_MAX] * (MAX_N // 2) + [-Q_MAX] * (MAX_N // 2))
    assert half[4] == 1 << 63 and half[3] == 0
    g = _check_gate(eng, [half], sigma)
    assert g.var[0] == 2.0 ** 24 and g.nu[0] == 0.0
    odd = record_of([Q_MAX] * (MAX_N - 1) + [Q_MAX - 1])         # a numerator that needs more than 53 bits
    _check_gate(eng, [odd, record_of([Q_MAX] * (MAX_N - 3) + [-Q_MAX, 1, -7])], sigma)
    # the max_gated_fraction boundary over 64 valid beams: 16 candidates are gated, 17 are a ping that disagrees
    g = _check_gate(eng, [cand] * 16 + [clean] * 48, sigma)
    assert g.n_gated == 16 and not g.inconsistent and list(g.mask) == [True] * 16 + [False] * 48
    g = _check_gate(eng, [cand] * 17 + [clean] * 47, sigma)
    assert g.n_gated == 0 and g.inconsistent and g.n_candidates == 17 and not g.mask.any()
    # a candidate needs BOTH: a large NIS with support, and no support with a small NIS, pass
    spread = record_of([-q20] * 50 + [0] * 50, 50)
    g = _check_gate(eng, [spread, record_of([3] * 100, 0)] + [clean] * 8, sigma)
    assert not g.mask.any() and g.nis[0] < 10.83 < 400 and g.support[1] == 0.0


def test_gate_refuses_what_cannot_be_a_record(eng):
    bad = [(-1, 0, 0, 0, 0), (MAX_N + 1, 0, 0, 0, 0), (10, 11, 0, 0, 0), (10, 0, 11, 0, 0), (10, 0, 0, 10 * Q_MAX + 1, 10 << 48),
           (10, 0, 0, 0, (10 << 48) + 1), (10, 0, 0, 100, 999), (0, 0, 0, 1, 1), (10, -1, 0, 0, 0), (1, 0, 0, -(1 << 63), 1 << 48)]
    for r in bad:
        with pytest.raises(eng.MclError) as ei:
            eng.innovation_gate(records_array([r]), 0.2)
        assert ei.value.status == ERR_INVALID, r
    ok = records_array([(10, 0, 0, 100, 1000)])
    for sigma in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(eng.MclError):
            eng.innovation_gate(ok, sigma)
    for cfg in (dict(nis_gate=-1.0), dict(nis_gate=math.nan), dict(min_support=1.5), dict(max_gated_fraction=-0.1)):
        with pytest.raises(eng.MclError):
            eng.innovation_gate(ok, 0.2, **cfg)


def test_merge_adds_field_wise_is_associative_and_refuses_overflow(eng):
    rs = np.random.RandomState(3)
    B = 9
    parts = []
    for p in range(4):
        recs = []
        for b in range(B):
            n = int(rs.randint(0, 3000))
            q = rs.randint(-Q_MAX, Q_MAX + 1, n).astype(np.int64)
            recs.append((n, int(rs.randint(0, n + 1)), int(rs.randint(0, n + 1)), int(q.sum()), sum(int(v) * int(v) for v in q)))
        parts.append(records_array(recs))
    whole = eng.merge_innovation(parts)
    for f in ('n', 'n_miss', 'n_within', 's1', 's2'):
        assert [int(v) for v in whole[f]] == [sum(int(p[f][b]) for p in parts) for b in range(B)]
    left = eng.merge_innovation([eng.merge_innovation(parts[:2]), eng.merge_innovation(parts[2:])])
    right = eng.merge_innovation([parts[3], eng.merge_innovation([parts[1], eng.merge_innovation([parts[2], parts[0]])])])
    assert whole.tobytes() == left.tobytes() == right.tobytes()
    assert eng.merge_innovation([parts[0]]).tobytes() == parts[0].tobytes()
    full = records_array([record_of([Q_MAX] * MAX_N)])
    one = records_array([record_of([1])])
    assert int(eng.merge_innovation([full])['s2'][0]) == 1 << 63
    for over in ([full, one], [full, full], [records_array([(20000, 0, 0, 0, 0)])] * 2):
        with pytest.raises(eng.MclError) as ei:
            eng.merge_innovation(over)
        assert ei.value.status == ERR_INVALID
    with pytest.raises(eng.MclError):
        eng.merge_innovation([records_array([(5, 6, 0, 0, 0)]), one])      # a part that is no record


def test_null_pointers_are_refused(lib):
    from smarc_navigation_amd import _lib
    i = ctypes.c_int64(0)
    v = _lib.InnovationVerdict()
    buf = (ctypes.c_uint64 * 16)()
    f = (ctypes.c_float * 4)()
    assert lib.mcl_innovation_sample(10, 5, None, ctypes.byref(i)) == ERR_INVALID
    assert lib.mcl_innovation_dirs(None, 1, f) == ERR_INVALID and lib.mcl_innovation_dirs(f, 1, None) == ERR_INVALID
    assert lib.mcl_innovation_merge(None, 1, 1, buf) == ERR_INVALID and lib.mcl_innovation_merge(buf, 1, 1, None) == ERR_INVALID
    assert lib.mcl_innovation_merge(buf, 0, 1, buf) == ERR_INVALID
    assert lib.mcl_innovation_gate(None, 1, 0.2, None, None, ctypes.byref(v)) == ERR_INVALID
    assert lib.mcl_innovation_gate(buf, 1, 0.2, None, None, None) == ERR_INVALID
    assert lib.mcl_innovation_gate(buf, 1, 0.2, None, None, ctypes.byref(v)) == 0 and v.n_valid == 0   # defaults, no per-beam array
    assert lib.mcl_ping_innovation(None, f, f, 1, 0.2, 3.0, 50.0, None, 4096, buf, None, ctypes.byref(i)) == ERR_INVALID
    none = (ctypes.c_void_p * 1)(None)
    assert lib.mcl_group_ping_innovation(None, 1, f, f, 1, 0.2, 3.0, 50.0, None, 4096, buf, ctypes.byref(i)) == ERR_INVALID
    assert lib.mcl_group_ping_innovation(none, 1, f, f, 1, 0.2, 3.0, 50.0, None, 4096, buf, ctypes.byref(i)) == ERR_INVALID


def test_the_host_arithmetic_runs_clean_under_the_sanitizers_as_a_program(tmp_path):
    """tests/host_san/innovation_driver.cpp: its own main over the device-free functions, g++ -fsanitize=address,undefined,
    run as a program (nothing loaded into Python runs under a sanitizer)"""
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no g++ / make')
    san = str(tmp_path / 'host_san')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'smarc_navigation_amd', 'csrc'), 'host-asan-innovation',
                           'SAN_DIR=' + san], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(san, 'innovation_asan')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=300, cwd=ROOT)
    for marker in ('AddressSanitizer', 'runtime error', 'LeakSanitizer'):
        assert marker not in p.stdout, p.stdout[-2000:]
    assert p.returncode == 0 and 'innovation_driver: ok' in p.stdout, p.stdout[-2000:]


# ------------------------------------------------------------------ the scene of the GPU tests, for the oracle alone
@pytest.mark.parametrize('kind', ['grid', 'mesh', 'tin'])
def test_the_oracle_alone_keeps_the_gpu_scene_within_the_outlier_cap(kind):
    """the rays whose fp64 answer jumps when the sensor moves by 1 mm are the ones a fp32 cast may miss by more than 1e-3 m
    (helpers.outliers_explained excuses exactly those): in the scene of test_gpu_innovation.py they stay under the cap"""
    from oracle import oracle as orc
    z, origin, soa = scene()
    _, omap = scene_map(kind, z, origin)
    stride, _ = sample_ref(N, MAX_SAMPLES)
    sub = np.ascontiguousarray(soa[:, sampled_slots(N, stride)])
    ba = synth.beam_angles(300)
    _, ref = orc.mbes_update(sub, M2O, OFF, omap, ba, None, SIGMA, R_MAX)
    assert (ref >= R_MAX).any() and (ref < R_MAX).mean() > 0.9       # misses past the edge, hits elsewhere
    moved = np.zeros(ref.shape, bool)
    for axis in range(3):
        for sgn in (1.0, -1.0):
            s = sub.copy()
            s[axis] += sgn * 1e-3
            _, ex = orc.mbes_update(s, M2O, OFF, omap, ba, None, SIGMA, R_MAX)
            moved |= np.abs(ex - ref) > 0.1
    print('%s: %d of %d rays jump under a 1 mm shift' % (kind, int(moved.sum()), moved.size))
    assert moved.mean() < OUTLIER_CAP


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
            if name == 'gate_ping':
                from smarc_navigation_amd import engine as e
                masked = np.array(a[0], np.float32, copy=True)
                masked[1] = 0.0
                mask = np.zeros(masked.size, bool)
                mask[1] = True
                zeros = np.zeros(masked.size)
                return masked, e.GateVerdict(mask, 1, False, masked.size, 1, 0.0, 0.0, zeros, zeros, zeros, zeros)
            return None
        return f


@pytest.fixture
def node(monkeypatch):
    from smarc_navigation_amd import auv_pf, engine as e
    monkeypatch.setattr(e, 'Engine', RecordingEngine)
    RecordingEngine.calls = []
    return auv_pf


def _drive(pf):
    pf.start_timing(100.0)
    pf.set_map_grid(np.full((8, 8), -20.0, np.float32), (-4.0, -4.0), 1.0)
    ranges = np.array([18.0, 18.5, 19.0, 18.2], np.float32)
    scan = msgs.LaserScan(ranges, -0.3, 0.2, 60.0)
    a = -0.3 + 0.2 * np.arange(4)
    pc = msgs.pointcloud2_from_xyz(np.stack([np.zeros(4), ranges * np.sin(a), -ranges * np.cos(a)], axis=1), 'base')
    for k in range(3):
        m = msgs.Odometry()
        m.header.stamp = msgs.Time(100.02 + 0.02 * k)
        m.twist.twist.linear.x = 1.0
        m.pose.pose.orientation = msgs.Quaternion(0.0, 0.0, 0.0, 1.0)
        pf.odom_callback(m)
        pf.mbes_cb(scan) if k < 2 else pf.mbes_pc_cb(pc)


def test_node_off_the_call_sequence_is_todays_and_on_one_gate_before_each_update(node):
    assert node.DEFAULT_PARAMS['mbes_gate_nis'] == 0.0
    pf = node.auv_pf({'particle_count': 16})
    _drive(pf)
    plain = list(RecordingEngine.calls)
    names = [c[0] for c in plain]
    assert names.count('update_mbes') == 3 and 'gate_ping' not in names and 'ping_innovation' not in names
    assert pf.last_innovation is None and pf.gate_calls == 0
    RecordingEngine.calls = []
    pf = node.auv_pf({'particle_count': 16, 'mbes_gate_nis': 0.0})
    _drive(pf)
    assert repr(RecordingEngine.calls) == repr(plain)
    RecordingEngine.calls = []
    pf = node.auv_pf({'particle_count': 16, 'mbes_gate_nis': 10.83})
    _drive(pf)
    on = list(RecordingEngine.calls)
    assert repr([c for c in on if c[0] != 'gate_ping' and c[0] != 'update_mbes']) == \
        repr([c for c in plain if c[0] != 'update_mbes'])
    names = [c[0] for c in on]
    assert names.count('gate_ping') == names.count('update_mbes') == 3
    ups = [c for c in plain if c[0] == 'update_mbes']
    for i, c in enumerate(on):
        if c[0] != 'update_mbes':
            continue
        g, raw = on[i - 1], ups.pop(0)
        assert g[0] == 'gate_ping'                                       # right in front of the update it serves
        assert np.array_equal(g[1][0], raw[1][0]) and np.array_equal(g[1][1], raw[1][1])   # the ping as it came
        assert repr(g[1][2:]) == repr(raw[1][2:]) and g[2] == dict(nis_gate=10.83)   # sigma, r_max, offset: the update's own
        want = np.array(raw[1][0], copy=True)
        want[1] = 0.0
        assert np.array_equal(c[1][0], want) and np.array_equal(c[1][1], raw[1][1]) and repr(c[1][2:]) == repr(raw[1][2:])
        assert c[2] == raw[2]
    assert pf.gate_calls == 3 and pf.gated_beams == 3 and pf.last_innovation.n_gated == 1


@pytest.mark.parametrize('bad', [-1.0, float('nan'), float('inf')])
def test_node_refuses_a_gate_that_means_nothing(node, bad):
    with pytest.raises(ValueError) as ei:
        node.auv_pf({'particle_count': 8, 'mbes_gate_nis': bad})
    assert 'mbes_gate_nis' in str(ei.value)


def test_launch_file_passes_the_parameter():
    import xml.etree.ElementTree as ET
    from smarc_navigation_amd import auv_pf
    root = ET.parse(os.path.join(ROOT, 'ros', 'auv_particle_filter_hip', 'launch', 'auv_pf.launch')).getroot()
    args = {a.get('name'): a.get('default') for a in root.iter('arg')}
    params = {p.get('name'): p for p in next(root.iter('node')).iter('param')}
    assert float(args['mbes_gate_nis']) == auv_pf.DEFAULT_PARAMS['mbes_gate_nis'] == 0.0
    assert params['mbes_gate_nis'].get('type') == 'double' and params['mbes_gate_nis'].get('value') == '$(arg mbes_gate_nis)'
