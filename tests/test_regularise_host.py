"""CPU tests of the regularised resampling (include/mcl_regularise.h): every symbol of the header is exported and bound at
ABI version 4 in a table of its own, mcl_regularise_bandwidth agrees with Python's math, mcl_regularise_factor -- the
function the device runs -- gives the bits of the header's rule restated in numpy (host sqrt and / are correctly rounded, and
the restatement rounds every product, difference and quotient separately, as the function does), every refused
configuration gives its sentence, and the stand-alone driver of the same arithmetic is clean under ASan + UBSan."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mcl_regularise_config_check', 'mcl_regularise_bandwidth', 'mcl_regularise_factor', 'mcl_regularise',
         'mcl_regularise_last')
ERR_INVALID = -1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _declared():
    src = open(os.path.join(ROOT, 'include', 'mcl_regularise.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src)))


def test_regularise_symbols_declared_exported_and_bound_at_abi_4():
    from smarc_navigation_amd import _lib
    assert _declared() == sorted(NAMES)
    assert sorted(_lib.REGULARISE_SYMBOLS) == sorted(NAMES)
    others = (set(_lib.SYMBOLS) | set(_lib.RECOVERY_SYMBOLS) | set(_lib.MODES_SYMBOLS) | set(_lib.HISTORY_SYMBOLS) |
              set(_lib.ACOUSTIC_SYMBOLS) | set(_lib.TEMPER_SYMBOLS) | set(_lib.DRIFT_SYMBOLS))
    assert not set(NAMES) & others
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), 'libmcl_hip.so does not export %s' % n
    lib = _lib.load()
    assert lib.mcl_abi_version() == 4
    counts = dict(mcl_regularise_config_check=2, mcl_regularise_bandwidth=6, mcl_regularise_factor=4, mcl_regularise=3,
                  mcl_regularise_last=2)
    for n in NAMES:
        assert getattr(lib, n).argtypes is not None, n
        assert len(_lib.REGULARISE_SYMBOLS[n][1]) == counts[n], n


def test_abi_version_timing_table_and_struct_layouts():
    from smarc_navigation_amd import _lib
    assert re.search(r'#define\s+MCL_ABI_VERSION\s+4\b', open(os.path.join(ROOT, 'include', 'mcl.h')).read())
    assert ctypes.sizeof(_lib.Timing) == 15 * 16          # MCL_K_COUNT entries of (double ms, int64 launches)
    assert ctypes.sizeof(_lib.RegulariseConfig) == 16
    assert (_lib.RegulariseConfig.scale.offset, _lib.RegulariseConfig.shrink.offset, _lib.RegulariseConfig.dims.offset) == (0, 8, 12)
    R = _lib.RegulariseResult
    assert ctypes.sizeof(R) == 464
    assert [getattr(R, f).offset for f in ('n', 'dims', 'dead', 'h', 'a', 'shift', 'dmean', 'cov', 'chol')] == \
        [0, 8, 12, 16, 24, 32, 80, 128, 296]


# ------------------------------------------------------------------ bandwidth
def bandwidth_ref(n, dims, scale, shrink):
    h0 = scale * (4.0 / ((dims + 2.0) * n)) ** (1.0 / (dims + 4.0))
    if not shrink:
        return h0, 1.0
    h = min(h0, 1.0)
    return h, math.sqrt(1.0 - h * h)


@pytest.mark.parametrize('dims', [3, 6])
def test_bandwidth_agrees_with_pythons_math(dims):
    from smarc_navigation_amd import engine
    for n in (1, 2, 63, 1000, 65536, 1 << 20, (1 << 31) - 1):
        for scale in (0.05, 0.5, 1.0, 1.5):
            for shrink in (False, True):
                h, a = engine.regularise_bandwidth(n, dims, scale, shrink)
                wh, wa = bandwidth_ref(n, dims, scale, shrink)
                assert abs(h - wh) <= 1e-14 * wh, (n, scale, shrink, h, wh)
                assert abs(a - wa) <= 1e-14 * wa, (n, scale, shrink, a, wa)
                if not shrink:
                    assert a == 1.0


@pytest.mark.parametrize('dims', [3, 6])
def test_bandwidth_clamps_at_one_with_a_zero(dims):
    from smarc_navigation_amd import engine
    # one particle: h0 = (4 / (D + 2))^(1 / (D + 4)) < 1; a scale that lifts it over 1 is clamped when shrinking
    h1, a1 = engine.regularise_bandwidth(1, dims, 1.0, True)
    want = (4.0 / (dims + 2.0)) ** (1.0 / (dims + 4.0))
    assert abs(h1 - want) <= 1e-14 * want and 0.0 < a1 < 1.0
    assert engine.regularise_bandwidth(1, dims, 5.0, True) == (1.0, 0.0)
    assert engine.regularise_bandwidth(100, dims, 50.0, True) == (1.0, 0.0)
    h, a = engine.regularise_bandwidth(1, dims, 5.0, False)                   # not clamped without the shrink
    assert abs(h - 5.0 * want) <= 1e-14 * 5.0 * want and a == 1.0


@pytest.mark.parametrize('args', [(0, 3, 1.0), (-5, 3, 1.0), (100, 2, 1.0), (100, 4, 1.0), (100, 0, 1.0), (100, 3, 0.0),
                                  (100, 6, -1.0), (100, 3, float('nan')), (100, 6, float('inf'))])
def test_bandwidth_refusals(args):
    from smarc_navigation_amd import _lib
    lib = _lib.load()
    h, a = ctypes.c_double(-7.0), ctypes.c_double(-7.0)
    assert lib.mcl_regularise_bandwidth(args[0], args[1], args[2], 1, ctypes.byref(h), ctypes.byref(a)) == ERR_INVALID
    assert (h.value, a.value) == (-7.0, -7.0)             # nothing is written on a refusal
    assert lib.mcl_regularise_bandwidth(100, 3, 1.0, 1, None, ctypes.byref(a)) == ERR_INVALID
    assert lib.mcl_regularise_bandwidth(100, 3, 1.0, 1, ctypes.byref(h), None) == ERR_INVALID


# ------------------------------------------------------------------ the factor
def factor_ref(C):
    """the header's rule, one numpy double operation per product, difference, quotient and root; C: (D, D), lower triangle"""
    C = np.asarray(C, dtype=np.float64)
    D = C.shape[0]
    L, dead = np.zeros((D, D)), 0
    with np.errstate(all='ignore'):
        for j in range(D):
            p = C[j, j]
            for k in range(j):
                p = p - L[j, k] * L[j, k]
            if p > C[j, j] * np.float64(2.0 ** -26):
                L[j, j] = np.sqrt(p)
                for i in range(j + 1, D):
                    t = C[i, j]
                    for k in range(j):
                        t = t - L[i, k] * L[j, k]
                    L[i, j] = t / L[j, j]
            else:
                dead |= 1 << j
    return L, dead


def _spd(d, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(500, d) * (10.0 ** rs.uniform(-3, 2, d))
    x[:, 1] += 0.7 * x[:, 0]
    return np.cov(x.T, bias=True)


@pytest.mark.parametrize('d', [3, 6])
@pytest.mark.parametrize('seed', range(8))
def test_factor_of_a_random_spd_matrix_is_the_numpy_restatement_bit_for_bit(d, seed):
    from smarc_navigation_amd import engine
    C = _spd(d, 10 * d + seed)
    L, dead = engine.regularise_factor(C)
    wL, wdead = factor_ref(C)
    assert dead == wdead == 0
    assert np.array_equal(bits(L), bits(wL))
    assert np.all(np.diag(L) > 0) and not np.any(np.triu(L, 1))
    assert np.max(np.abs(L @ L.T - C)) <= 1e-13 * np.abs(C).max()
    # only the lower triangle is read
    junk = C.copy()
    junk[np.triu_indices(d, 1)] = 1e30
    assert np.array_equal(bits(engine.regularise_factor(junk)[0]), bits(L))


@pytest.mark.parametrize('d,const', [(3, 2), (3, 0), (6, 2), (6, 4)])
def test_a_constant_dimension_gives_a_zero_row_and_column_and_its_dead_bit(d, const):
    from smarc_navigation_amd import engine
    C = _spd(d, 77 + d)
    C[const, :] = 0.0
    C[:, const] = 0.0
    L, dead = engine.regularise_factor(C)
    wL, wdead = factor_ref(C)
    assert dead == wdead == 1 << const
    assert np.array_equal(bits(L), bits(wL))
    assert not np.any(L[const, :]) and not np.any(L[:, const])
    assert np.array_equal(bits(L[const, :]), bits(np.zeros(d)))       # +0.0, every bit
    keep = [i for i in range(d) if i != const]
    sub = L[np.ix_(keep, keep)]
    assert np.max(np.abs(sub @ sub.T - C[np.ix_(keep, keep)])) <= 1e-13 * np.abs(C).max()


@pytest.mark.parametrize('d,src,dup', [(3, 0, 2), (3, 0, 1), (6, 1, 4), (6, 2, 5)])
def test_an_exact_copy_of_an_earlier_dimension_is_a_dead_column_whose_row_is_kept(d, src, dup):
    from smarc_navigation_amd import engine
    rs = np.random.RandomState(d * 10 + dup)
    x = rs.randn(400, d) * np.linspace(0.5, 3.0, d)
    x[:, dup] = x[:, src]
    C = np.cov(x.T, bias=True)
    assert np.array_equal(bits(C[dup, :]), bits(C[src, :]))
    L, dead = engine.regularise_factor(C)
    wL, wdead = factor_ref(C)
    assert dead == wdead == 1 << dup
    assert np.array_equal(bits(L), bits(wL))
    assert not np.any(L[:, dup])                                      # the column is zero ...
    assert L[dup, src] != 0.0                                         # ... the row is kept: the copy moves with its source
    assert np.max(np.abs(L[dup, :dup] - L[src, :dup])) <= 1e-7 * np.abs(L).max()
    assert np.max(np.abs(L @ L.T - C)) <= 2e-4 * np.abs(C).max()      # (2^-13: what a dead column may leave out)


@pytest.mark.parametrize('d', [3, 6])
def test_nan_and_non_positive_variances_are_dead_columns(d):
    from smarc_navigation_amd import engine
    C = _spd(d, 5)
    C[1, 1] = float('nan')
    L, dead = engine.regularise_factor(C)
    wL, wdead = factor_ref(C)
    assert dead == wdead and dead & 2
    assert np.array_equal(np.isnan(L), np.isnan(wL))
    ok = ~np.isnan(wL)
    assert np.array_equal(bits(L[ok]), bits(wL[ok]))
    assert not np.any(L[:, 1])
    allnan = np.full((d, d), float('nan'))
    L, dead = engine.regularise_factor(allnan)
    assert dead == (1 << d) - 1 and np.array_equal(bits(L), bits(np.zeros((d, d))))
    for bad in (0.0, -1.0, -0.0):
        C = _spd(d, 6)
        C[0, 0] = bad
        L, dead = engine.regularise_factor(C)
        wL, wdead = factor_ref(C)
        assert dead == wdead and dead & 1 and not np.any(L[:, 0])
        assert np.array_equal(bits(L), bits(wL))


def test_factor_refusals():
    from smarc_navigation_amd import _lib
    lib = _lib.load()
    c, l, dead = np.zeros(21), np.full(21, -7.0), ctypes.c_int32(-7)
    for dims in (-1, 0, 1, 2, 4, 5, 7):
        assert lib.mcl_regularise_factor(c.ctypes.data, dims, l.ctypes.data, ctypes.byref(dead)) == ERR_INVALID
    assert lib.mcl_regularise_factor(None, 3, l.ctypes.data, ctypes.byref(dead)) == ERR_INVALID
    assert lib.mcl_regularise_factor(c.ctypes.data, 3, None, ctypes.byref(dead)) == ERR_INVALID
    assert lib.mcl_regularise_factor(c.ctypes.data, 3, l.ctypes.data, None) == ERR_INVALID
    assert dead.value == -7 and np.all(l == -7.0)         # nothing is written on a refusal


# ------------------------------------------------------------------ configurations
def _check(scale, shrink, dims):
    from smarc_navigation_amd import _lib, engine
    cfg, why = engine.make_regularise_config(scale, shrink, dims), ctypes.c_char_p()
    st = _lib.load().mcl_regularise_config_check(ctypes.byref(cfg), ctypes.byref(why))
    return st, (why.value or b'').decode()


def test_config_check_accepts_what_the_header_allows():
    for scale in (5e-324, 0.5, 1.0, 1e300):
        for shrink in (False, True):
            for dims in (3, 6):
                assert _check(scale, shrink, dims) == (0, '')


@pytest.mark.parametrize('scale', [0.0, -0.0, -1.0, float('nan'), float('inf'), -float('inf')])
def test_config_check_names_the_scale_it_refuses(scale):
    from smarc_navigation_amd import _lib, engine
    assert _check(scale, True, 3) == (ERR_INVALID, 'scale must be finite and > 0')
    assert _check(scale, False, 7)[1] == 'scale must be finite and > 0'            # the first of two
    assert engine.regularise_config_check(scale) == 'scale must be finite and > 0'
    cfg = engine.make_regularise_config(scale, True, 3)
    assert _lib.load().mcl_regularise_config_check(ctypes.byref(cfg), None) == ERR_INVALID   # the reason is optional


@pytest.mark.parametrize('dims', [-3, 0, 1, 2, 4, 5, 7, 9])
def test_config_check_names_the_dims_it_refuses(dims):
    from smarc_navigation_amd import engine
    assert _check(1.0, True, dims) == (ERR_INVALID, 'dims must be 3 (x, y, yaw) or 6 (x, y, yaw, cx, cy, bw)')
    assert engine.regularise_config_check(1.0, True, dims).startswith('dims must be 3')


def test_null_arguments_are_refused():
    from smarc_navigation_amd import _lib, engine
    lib = _lib.load()
    why = ctypes.c_char_p()
    assert lib.mcl_regularise_config_check(None, ctypes.byref(why)) == ERR_INVALID and why.value == b'null config'
    assert lib.mcl_regularise_config_check(None, None) == ERR_INVALID
    cfg, res = engine.make_regularise_config(1.0, True, 3), _lib.RegulariseResult()
    assert lib.mcl_regularise(None, ctypes.byref(cfg), None) == ERR_INVALID
    assert lib.mcl_regularise_last(None, ctypes.byref(res)) == ERR_INVALID
    assert engine.regularise_config_check(1.0) is None and engine.regularise_config_check(0.3, False, 6) is None


# ------------------------------------------------------------------ the same arithmetic under ASan + UBSan
def test_the_device_free_arithmetic_is_clean_under_asan_and_ubsan():
    """a stand-alone program (tests/host_san/regularise_driver.cpp, its own main) over the functions the two entry points
    forward to, built with g++ -fsanitize=address,undefined and run on the CPU"""
    if shutil.which('g++') is None or shutil.which('make') is None:
        pytest.skip('no g++ / make')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'smarc_navigation_amd', 'csrc'), 'host-asan-regularise'],
                          stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(ROOT, 'build', 'host_san', 'regularise_asan')], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=300, cwd=ROOT)
    for marker in ('AddressSanitizer', 'runtime error', 'LeakSanitizer'):
        assert marker not in p.stdout, p.stdout[-4000:]
    assert p.returncode == 0 and 'regularise_driver: ok' in p.stdout, p.stdout[-4000:]
