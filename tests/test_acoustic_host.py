"""CPU tests of the delayed acoustic updates (include/mcl_acoustic.h): the symbols are declared, exported and bound at ABI
version 4 in a ctypes table of their own, and mcl_history_bracket (pure host arithmetic: no handle, no device) finds where
a stamp falls among the frames' stamps -- exact hits, midpoints, both clamps, one frame, refusals -- with frac in [0, 1)
and, for 200 random rings, interpolating the stamps themselves with the returned (lag, frac) gives the stamp back."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mcl_update_fix', 'mcl_update_beacon_ranges', 'mcl_history_bracket')
ERR_INVALID = -1


def _declared():
    src = open(os.path.join(ROOT, 'include', 'mcl_acoustic.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src)))


def test_acoustic_symbols_declared_exported_and_bound_at_abi_4():
    from smarc_navigation_amd import _lib
    assert _declared() == sorted(NAMES)
    assert sorted(_lib.ACOUSTIC_SYMBOLS) == sorted(NAMES)
    assert not set(NAMES) & (set(_lib.SYMBOLS) | set(_lib.RECOVERY_SYMBOLS) | set(_lib.MODES_SYMBOLS) |
                             set(_lib.HISTORY_SYMBOLS))
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), 'libmcl_hip.so does not export %s' % n
    lib = _lib.load()
    assert lib.mcl_abi_version() == 4
    for n in NAMES:
        assert getattr(lib, n).argtypes is not None, n
    counts = dict(mcl_update_fix=8, mcl_update_beacon_ranges=10, mcl_history_bracket=6)
    for n in NAMES:
        assert len(_lib.ACOUSTIC_SYMBOLS[n][1]) == counts[n], n


def test_nothing_in_the_base_header_moved():
    src = open(os.path.join(ROOT, 'include', 'mcl.h')).read()
    assert re.search(r'#define\s+MCL_ABI_VERSION\s+4\b', src)
    assert re.search(r'\bMCL_K_COUNT\s*=\s*15\b', src) or re.search(r'#define\s+MCL_K_COUNT\s+15\b', src)
    assert re.search(r'#define\s+MCL_ACOUSTIC_MAX_BEACONS\s+8\b', open(os.path.join(ROOT, 'include', 'mcl_acoustic.h')).read())


def bracket(stamps, stamp, held=None):
    """(status, lag, frac, where); the outputs keep their sentinels when the call refuses"""
    from smarc_navigation_amd import _lib
    s = np.ascontiguousarray(stamps, dtype=np.float64)
    lag, frac, where = ctypes.c_int32(-7), ctypes.c_double(-7.0), ctypes.c_int32(-7)
    st = _lib.load().mcl_history_bracket(s.ctypes.data, len(s) if held is None else held, float(stamp), ctypes.byref(lag),
                                         ctypes.byref(frac), ctypes.byref(where))
    return st, lag.value, frac.value, where.value


RING = [50.0, 48.5, 47.0, 41.0, 40.75]      # newest first


def test_exact_hits_give_frac_zero():
    assert bracket(RING, 50.0) == (0, 0, 0.0, 1)          # the newest: "not older than the newest frame"
    for k in (1, 2, 3):
        assert bracket(RING, RING[k]) == (0, k, 0.0, 0), k
    assert bracket(RING, 40.75) == (0, 4, 0.0, -1)        # the oldest: "not newer than the oldest"


def test_midpoints_and_other_fractions():
    for k in range(4):
        assert bracket(RING, 0.5 * (RING[k] + RING[k + 1])) == (0, k, 0.5, 0), k
    assert bracket(RING, 44.0) == (0, 2, 0.5, 0)
    assert bracket(RING, 48.875) == (0, 0, 0.75, 0)
    assert bracket(RING, 42.5) == (0, 2, 0.75, 0)


def test_both_clamps():
    assert bracket(RING, 50.001) == (0, 0, 0.0, 1)
    assert bracket(RING, 1e9) == (0, 0, 0.0, 1)
    assert bracket(RING, 40.7) == (0, 4, 0.0, -1)
    assert bracket(RING, -1e9) == (0, 4, 0.0, -1)


def test_one_frame():
    assert bracket([12.0], 12.0) == (0, 0, 0.0, 1)
    assert bracket([12.0], 13.0) == (0, 0, 0.0, 1)
    assert bracket([12.0], 11.0) == (0, 0, 0.0, -1)


@pytest.mark.parametrize('stamps,stamp', [([3.0, 4.0, 2.0], 3.5), ([5.0, 4.0, 4.0, 3.0], 3.5), ([5.0, 5.0], 5.0),
                                          ([5.0, float('nan'), 3.0], 4.0), ([float('nan')], 1.0), ([5.0, 4.0], float('nan')),
                                          ([5.0, 4.0], float('inf')), ([float('inf'), 4.0], 4.5), ([1.0, 2.0], 1.5)])
def test_unsorted_equal_or_non_finite_stamps_are_refused(stamps, stamp):
    assert bracket(stamps, stamp) == (ERR_INVALID, -7, -7.0, -7)      # nothing is written on a refusal


def test_no_frames_and_null_pointers_are_refused():
    from smarc_navigation_amd import _lib
    lib = _lib.load()
    assert bracket(RING, 45.0, held=0)[0] == ERR_INVALID
    assert bracket(RING, 45.0, held=-1)[0] == ERR_INVALID
    s = np.array(RING)
    lag, frac, where = ctypes.c_int32(0), ctypes.c_double(0.0), ctypes.c_int32(0)
    assert lib.mcl_history_bracket(None, 5, 45.0, ctypes.byref(lag), ctypes.byref(frac), ctypes.byref(where)) == ERR_INVALID
    assert lib.mcl_history_bracket(s.ctypes.data, 5, 45.0, None, ctypes.byref(frac), ctypes.byref(where)) == ERR_INVALID
    assert lib.mcl_history_bracket(s.ctypes.data, 5, 45.0, ctypes.byref(lag), None, ctypes.byref(where)) == ERR_INVALID
    assert lib.mcl_history_bracket(s.ctypes.data, 5, 45.0, ctypes.byref(lag), ctypes.byref(frac), None) == ERR_INVALID


def test_frac_stays_below_one_next_to_the_older_stamp():
    # one ulp above the older stamp: both differences may round to the same number
    for newer, older in ((50.0, 48.5), (1.7e9 + 0.02, 1.7e9), (3.0, 1.0), (1e-3, 0.0)):
        st, lag, frac, where = bracket([newer, older], np.nextafter(older, newer))
        assert (st, lag, where) == (0, 0, 0) and 0.0 <= frac < 1.0, (newer, older, frac)


def test_interpolating_the_stamps_gives_the_stamp_back():
    """200 random rings (1 ... 64 frames, steps from milliseconds to seconds, epochs up to 1.7e9 s): s_k + frac (s_{k+1} -
    s_k) == stamp within 1e-12 relative; frac always in [0, 1); the engine's helper returns the same triple"""
    from smarc_navigation_amd import engine
    rs = np.random.RandomState(5)
    inside = 0
    for ring in range(200):
        held = int(rs.randint(1, 65))
        t0 = float(rs.choice([0.0, 100.0, 1.7e9])) + 10.0 * rs.rand()
        steps = np.exp(rs.uniform(np.log(1e-3), np.log(5.0), held))
        s = (t0 + np.cumsum(steps))[::-1].copy()
        assert np.all(np.diff(s) < 0)
        for stamp in np.concatenate([rs.uniform(s[-1] - 1.0, s[0] + 1.0, 6), s[rs.randint(0, held, 2)]]):
            st, lag, frac, where = bracket(s, stamp)
            assert st == 0 and 0 <= lag < held and 0.0 <= frac < 1.0
            assert engine.history_bracket(s, stamp) == (lag, frac, where)
            if where > 0:
                assert stamp >= s[0] and (lag, frac) == (0, 0.0)
            elif where < 0:
                assert stamp <= s[-1] and (lag, frac) == (held - 1, 0.0)
            else:
                assert s[lag] >= stamp > s[lag + 1]
                back = s[lag] + frac * (s[lag + 1] - s[lag])
                assert abs(back - stamp) <= 1e-12 * abs(stamp), (ring, stamp, back)
                inside += 1
    assert inside > 500
