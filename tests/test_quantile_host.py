"""CPU tests of the exact order statistics (include/mcl_quantile.h): every symbol of the header exported and bound, the
device-free entry points -- key / value, threshold, the 128-bit predicate -- against Python integers, the null-pointer
refusals, and the stand-alone sanitizer driver of the host arithmetic.  Also the restatement of the header's definition in
numpy and Python integers that tests/test_gpu_quantile.py compares the GPU with."""
import bisect
import ctypes
import itertools
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mcl_quantile_key', 'mcl_quantile_value', 'mcl_quantile_threshold', 'mcl_quantile_reached', 'mcl_cloud_quantiles',
         'mcl_cloud_mass', 'mcl_cloud_key_hist', 'mcl_group_cloud_quantiles')
ERR_INVALID = -1
TWO32, TWO64, TOP = 1 << 32, 1 << 64, 1 << 63
Q_X, Q_Y, Q_YAW_DEV, Q_ABS_YAW_DEV, Q_RADIUS2 = range(5)


# ------------------------------------------------------------------ the restatement of include/mcl_quantile.h
def key_ref(v):
    """key(v + 0.0) of one double, in Python integers"""
    b = struct.unpack('<Q', struct.pack('<d', float(v) + 0.0))[0]
    return (~b) & (TWO64 - 1) if b >> 63 else b | TOP


def value_ref(k):
    b = k & (TOP - 1) if k >> 63 else (~k) & (TWO64 - 1)
    return struct.unpack('<d', struct.pack('<Q', b))[0]


def keys_ref(v):
    """the keys of an array of doubles (no NaN), as uint64"""
    b = (np.asarray(v, dtype=np.float64) + 0.0).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(TOP))


def threshold_ref(p):
    return int(math.floor(p * 4294967296.0))


def reached_ref(mass, total, P):
    return (mass << 32) >= P * total


def quantity_ref(soa, quantity, centre=(0.0, 0.0, 0.0)):
    """the quantity of every particle, each IEEE operation on its own (numpy never fuses)"""
    x, y, yaw = soa[0], soa[1], soa[5]
    cx, cy, cyaw = [np.float64(c) for c in centre]
    with np.errstate(all='ignore'):
        if quantity == Q_X:
            return x.copy()
        if quantity == Q_Y:
            return y.copy()
        if quantity == Q_RADIUS2:
            dx, dy = x - cx, y - cy
            return dx * dx + dy * dy
        d = ((yaw - cyaw) + np.pi) % (2.0 * np.pi) - np.pi
        return np.abs(d) if quantity == Q_ABS_YAW_DEV else d


def masses_ref(lw, m=None):
    """(q_i as Python integers, m): floor(det_exp(lw_i - m) 2^32), 0 for a log-weight that is not finite"""
    from oracle import oracle
    lw = np.asarray(lw, dtype=np.float64)
    fin = np.isfinite(lw)
    if m is None:
        m = float(lw[fin].max()) if fin.any() else -math.inf
    q = [0] * lw.size
    if m > -math.inf:
        for i in np.nonzero(fin)[0]:
            d = min(float(lw[i] - m), 0.0)
            q[i] = int(oracle.det_exp(d) * 4294967296.0) if d >= -700.0 else 0
    return q, m


class Selection(object):
    """the used particles of a query, sorted: the distinct keys ascending with the cumulative mass at each"""

    def __init__(self, values, masses=None):
        values = np.asarray(values, dtype=np.float64)
        used = ~np.isnan(values)
        self.n_used = int(used.sum())
        keys = keys_ref(values[used])
        q = [1] * self.n_used if masses is None else [masses[i] for i in np.nonzero(used)[0]]
        order = np.argsort(keys, kind='stable')
        skeys = keys[order]
        cum = list(itertools.accumulate(q[i] for i in order))
        last = np.nonzero(np.append(skeys[1:] != skeys[:-1], True))[0] if self.n_used else np.zeros(0, int)
        self.keys = [int(skeys[i]) for i in last]
        self.cum = [cum[i] for i in last]
        self.total = cum[-1] if cum else 0

    def mass_at(self, key):
        """M(key)"""
        i = bisect.bisect_right(self.keys, key)
        return self.cum[i - 1] if i else 0

    def quantile(self, p):
        """(value, key, mass): the smallest key with 2^32 M(K) >= P S; (nan, 0, 0) when S = 0"""
        P = threshold_ref(p)
        if self.total == 0:
            return math.nan, 0, 0
        need = (P * self.total + TWO32 - 1) >> 32          # the least integer mass that reaches: a search aid only ...
        i = bisect.bisect_left(self.cum, need)
        assert reached_ref(self.cum[i], self.total, P)      # ... the rule itself, in unbounded integers
        assert i == 0 or not reached_ref(self.cum[i - 1], self.total, P)
        return value_ref(self.keys[i]), self.keys[i], self.cum[i]


def test_restatement_on_a_worked_example():
    s = Selection([3.0, -0.0, 0.0, math.nan, -2.0, math.inf])
    assert s.n_used == 5 and s.total == 5 and len(s.keys) == 4
    assert s.quantile(0.5)[0] == 0.0 and s.quantile(0.5)[2] == 3            # the lower median of -2, 0, 0, 3, inf
    assert s.quantile(2.0 ** -32)[0] == -2.0 and s.quantile(1.0)[0] == math.inf
    assert s.quantile(0.2)[0] == -2.0 and s.quantile(0.2 + 2.0 ** -30)[0] == 0.0
    w = Selection([1.0, 2.0, 3.0], [TWO32, 0, TWO32])
    assert w.quantile(0.5)[:1] == (1.0,) and w.quantile(0.75) == (3.0, key_ref(3.0), 2 * TWO32)
    assert math.isnan(Selection([1.0], [0]).quantile(0.5)[0])


# ------------------------------------------------------------------ the ABI
@pytest.fixture(scope='module')
def lib():
    from smarc_navigation_amd import _lib
    return _lib.load()


def test_every_symbol_of_the_header_is_exported_and_bound_in_a_table_of_its_own(lib):
    from smarc_navigation_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'mcl_quantile.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(NAMES) == sorted(_lib.QUANTILE_SYMBOLS)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    others = [_lib.SYMBOLS, _lib.RECOVERY_SYMBOLS, _lib.MODES_SYMBOLS, _lib.HISTORY_SYMBOLS, _lib.ACOUSTIC_SYMBOLS,
              _lib.TEMPER_SYMBOLS, _lib.DRIFT_SYMBOLS, _lib.REGULARISE_SYMBOLS]
    for t in others:
        assert not set(t) & set(NAMES)
    assert lib.mcl_abi_version() == 4
    assert ctypes.sizeof(_lib.QuantileQuery) == 32 and ctypes.sizeof(_lib.QuantileResult) == 40
    hdr = open(os.path.join(ROOT, 'include', 'mcl.h')).read()
    assert 'quantile' not in hdr.lower()                       # mcl.h, its config and its timing table are what they were


EDGE = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, -1.0, 512.3, -87.1,
        1.7976931348623157e308, -1.7976931348623157e308, math.inf, -math.inf, 1e300, math.pi, -math.pi]


def test_key_and_value_round_trip_and_keep_the_order():
    from smarc_navigation_amd import engine as eng
    for v in EDGE:
        k = eng.quantile_key(v)
        assert k == key_ref(v), v
        back = eng.quantile_value(k)
        assert back == v and (v != 0.0 or math.copysign(1.0, back) == 1.0), v   # (-0 comes back as +0)
    assert eng.quantile_key(-0.0) == eng.quantile_key(0.0) == TOP
    asc = sorted(set(EDGE))
    ks = [eng.quantile_key(v) for v in asc]
    assert ks == sorted(ks) and len(set(ks)) == len(ks)
    # neighbours one ulp apart keep their order, and their keys are neighbours (the key -0 would have had stays unused: the
    # step from the largest negative denormal up to zero is 2)
    for v in EDGE:
        if v == math.inf:
            continue
        with np.errstate(over='ignore'):
            up = float(np.nextafter(v, math.inf))
        assert up > v and eng.quantile_key(up) == eng.quantile_key(v) + (2 if up == 0.0 else 1), v
    rs = np.random.RandomState(1)
    raw = rs.randint(0, 2 ** 32, 2000).astype(np.uint64) << np.uint64(32) | rs.randint(0, 2 ** 32, 2000).astype(np.uint64)
    v = raw.view(np.float64)
    v = v[~np.isnan(v)]
    k = np.array([eng.quantile_key(x) for x in v], dtype=np.uint64)
    assert np.array_equal(k, keys_ref(v))
    o = np.argsort(v, kind='stable')
    assert np.all(k[o][1:] >= k[o][:-1])
    for kk in (0, 1, TWO64 - 1, key_ref(-math.inf) - 1, key_ref(math.inf) + 1):   # no key of a value: a NaN
        assert math.isnan(eng.quantile_value(kk))
    with pytest.raises(eng.MclError) as ei:
        eng.quantile_key(math.nan)
    assert ei.value.status == ERR_INVALID


def test_threshold_at_its_ends_and_its_refusals():
    from smarc_navigation_amd import engine as eng
    assert eng.quantile_threshold(2.0 ** -32) == 1
    assert eng.quantile_threshold(0.5) == 1 << 31
    assert eng.quantile_threshold(1.0) == TWO32
    assert eng.quantile_threshold(1.0 - 2.0 ** -32) == TWO32 - 1
    assert eng.quantile_threshold(0.95) == threshold_ref(0.95) == int(0.95 * 4294967296.0)
    for bad in (float(np.nextafter(2.0 ** -32, 0.0)), 0.0, -0.5, float(np.nextafter(1.0, 2.0)), 2.0, math.nan, math.inf,
                -math.inf):
        with pytest.raises(eng.MclError) as ei:
            eng.quantile_threshold(bad)
        assert ei.value.status == ERR_INVALID, bad


def test_reached_is_exact_for_every_uint64():
    from smarc_navigation_amd import engine as eng
    top = TWO64 - 1
    triples = [(top, top, top), (top, top, TWO32), (top, top, TWO32 + 1), (0, 0, 0), (0, 0, top), (0, 1, 1), (1, TWO32, 1),
               (1, TWO32 + 1, 1), (1 << 31, top, 1 << 31), ((1 << 31) - 1, top, 1 << 31), (1, top, 1), (TWO32, top, top)]
    rs = np.random.RandomState(2)
    for _ in range(3000):
        a, b, c = [int(rs.randint(0, 2 ** 32)) << 32 | int(rs.randint(0, 2 ** 32)) for _ in range(3)]
        sh = rs.randint(0, 64, 3)
        triples.append((a >> int(sh[0]), b >> int(sh[1]), c >> int(sh[2])))
    for _ in range(1000):                                   # on and next to the boundary
        total, P = int(rs.randint(1, 2 ** 31)) << int(rs.randint(0, 25)), int(rs.randint(1, 2 ** 32)) + 1
        need = (P * total + TWO32 - 1) >> 32
        triples += [(need, total, P), (max(need - 1, 0), total, P)]
    for mass, total, P in triples:
        assert eng.quantile_reached(mass, total, P) == reached_ref(mass, total, P), (mass, total, P)


def test_null_pointers_are_refused(lib):
    from smarc_navigation_amd import _lib
    q = _lib.QuantileQuery()
    one, out = (ctypes.c_double * 1)(0.5), (_lib.QuantileResult * 1)()
    u, i = ctypes.c_uint64(0), ctypes.c_int64(0)
    hist = (ctypes.c_uint64 * 256)()
    assert lib.mcl_quantile_key(1.0, None) == ERR_INVALID
    assert lib.mcl_quantile_value(1, None) == ERR_INVALID
    assert lib.mcl_quantile_threshold(0.5, None) == ERR_INVALID
    assert lib.mcl_quantile_reached(1, 1, 1, None) == ERR_INVALID
    assert lib.mcl_cloud_quantiles(None, ctypes.byref(q), one, 1, out) == ERR_INVALID
    assert lib.mcl_cloud_mass(None, ctypes.byref(q), 0.0, one, 1, ctypes.addressof(u), ctypes.byref(u), ctypes.byref(i)) == ERR_INVALID
    assert lib.mcl_cloud_key_hist(None, ctypes.byref(q), 0.0, 0, 0, hist) == ERR_INVALID
    assert lib.mcl_group_cloud_quantiles(None, 1, ctypes.byref(q), one, 1, out) == ERR_INVALID
    none = (ctypes.c_void_p * 1)(None)
    assert lib.mcl_group_cloud_quantiles(none, 1, ctypes.byref(q), one, 1, out) == ERR_INVALID
    assert lib.mcl_group_cloud_quantiles(none, 0, ctypes.byref(q), one, 1, out) == ERR_INVALID


def test_the_host_arithmetic_runs_clean_under_the_sanitizers_as_a_program(tmp_path):
    """tests/host_san/quantile_driver.cpp: its own main over the device-free functions, g++ -fsanitize=address,undefined,
    run as a program (nothing loaded into Python runs under a sanitizer)"""
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no g++ / make')
    san = str(tmp_path / 'host_san')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'smarc_navigation_amd', 'csrc'), 'host-asan-quantile',
                           'SAN_DIR=' + san], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(san, 'quantile_asan')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=300, cwd=ROOT)
    for marker in ('AddressSanitizer', 'runtime error', 'LeakSanitizer'):
        assert marker not in p.stdout, p.stdout[-2000:]
    assert p.returncode == 0 and 'quantile_driver: ok' in p.stdout, p.stdout[-2000:]
