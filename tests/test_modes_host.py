"""CPU tests of the dominant-mode pose estimate (include/mcl_modes.h): the two symbols are exported and bound at ABI
version 4, the ctypes table and structures match the header, and mcl_mode_grid_check (pure host arithmetic) accepts and
refuses what the header says it does."""
import ctypes
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mcl_mode_grid_check', 'mcl_pose_modes')
ERR_INVALID = -1


def _declared():
    src = open(os.path.join(ROOT, 'include', 'mcl_modes.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src)))


def test_mode_symbols_exported_and_bound_at_abi_4():
    from smarc_navigation_amd import _lib
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), 'libmcl_hip.so does not export %s' % n
    lib = _lib.load()
    assert lib.mcl_abi_version() == 4
    assert lib.mcl_pose_modes.argtypes is not None and lib.mcl_mode_grid_check.argtypes is not None


def test_modes_symbols_table_matches_the_header():
    from smarc_navigation_amd import _lib
    assert _declared() == sorted(NAMES)
    assert sorted(_lib.MODES_SYMBOLS) == sorted(NAMES)
    # the tables of the other headers hold none of them
    assert not set(NAMES) & (set(_lib.SYMBOLS) | set(_lib.RECOVERY_SYMBOLS))
    # argument counts as declared: (g, n_cells) and (h, g, k_max, modes, n_modes, n_outside)
    assert len(_lib.MODES_SYMBOLS['mcl_mode_grid_check'][1]) == 2
    assert len(_lib.MODES_SYMBOLS['mcl_pose_modes'][1]) == 6


def test_structure_layouts():
    from smarc_navigation_amd import _lib
    assert ctypes.sizeof(_lib.ModeGrid) == 40
    assert ctypes.sizeof(_lib.Mode) == 112
    assert _lib.Mode.mean6.offset == 32 and _lib.Mode.cov_xy.offset == 80 and _lib.Mode.yaw_R.offset == 104
    assert _lib.ModeGrid.nx.offset == 24


def _check(x0=0.0, y0=0.0, cell=1.0, nx=4, ny=5, n_yaw=6):
    from smarc_navigation_amd import _lib
    g = _lib.ModeGrid(x0, y0, cell, nx, ny, n_yaw, 0)
    n = ctypes.c_int64(-7)
    return _lib.load().mcl_mode_grid_check(ctypes.byref(g), ctypes.byref(n)), n.value


def test_grid_check_accepts_a_valid_grid_and_returns_the_cell_count():
    from smarc_navigation_amd import _lib
    assert _check() == (0, 120)
    assert _check(x0=-96.0, y0=-96.0, cell=1.0, nx=192, ny=192, n_yaw=36) == (0, 192 * 192 * 36)
    assert _check(nx=1, ny=1, n_yaw=1) == (0, 1)
    assert _check(n_yaw=64) == (0, 4 * 5 * 64)
    assert _check(cell=1e-300, x0=-1e300, y0=1e300) == (0, 120)
    # n_cells is optional
    g = _lib.ModeGrid(0.0, 0.0, 1.0, 4, 5, 6, 0)
    assert _lib.load().mcl_mode_grid_check(ctypes.byref(g), None) == 0


def test_grid_check_cell_count_limit_is_two_to_the_24():
    assert _check(nx=4096, ny=4096, n_yaw=1) == (0, 1 << 24)
    assert _check(nx=1 << 24, ny=1, n_yaw=1) == (0, 1 << 24)
    assert _check(nx=512, ny=512, n_yaw=64) == (0, 1 << 24)
    assert _check(nx=(1 << 24) + 1, ny=1, n_yaw=1)[0] == ERR_INVALID
    assert _check(nx=4096, ny=4097, n_yaw=1)[0] == ERR_INVALID
    assert _check(nx=512, ny=513, n_yaw=64)[0] == ERR_INVALID
    # products that would overflow 32 and 64 bits
    assert _check(nx=0x7fffffff, ny=0x7fffffff, n_yaw=64)[0] == ERR_INVALID
    assert _check(nx=65536, ny=65536, n_yaw=1)[0] == ERR_INVALID


@pytest.mark.parametrize('kw', [
    dict(cell=0.0), dict(cell=-1.0), dict(cell=math.nan), dict(cell=math.inf),
    dict(x0=math.nan), dict(x0=math.inf), dict(y0=-math.inf), dict(y0=math.nan),
    dict(nx=0), dict(nx=-3), dict(ny=0), dict(n_yaw=0), dict(n_yaw=-1), dict(n_yaw=65),
])
def test_grid_check_refuses_each_invalid_case(kw):
    st, n = _check(**kw)
    assert st == ERR_INVALID
    assert n == -7                      # nothing is written on a refusal


def test_grid_check_refuses_a_null_grid():
    from smarc_navigation_amd import _lib
    n = ctypes.c_int64(0)
    assert _lib.load().mcl_mode_grid_check(None, ctypes.byref(n)) == ERR_INVALID
