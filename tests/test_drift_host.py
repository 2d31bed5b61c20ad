"""CPU tests of the per-particle drift states (include/mcl_drift.h): every symbol of the header is exported and bound at
ABI version 4, mcl_drift_bytes (pure host arithmetic) gives the header's byte count, mcl_drift_config_check names the std it
refuses, and synth.odom_stream with a current / a yaw-rate bias changes the truth and nothing the odometry reports."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mcl_drift_bytes', 'mcl_drift_config_check', 'mcl_drift_enable', 'mcl_drift_reset', 'mcl_drift_disable',
         'mcl_drift_advance', 'mcl_drift_get', 'mcl_drift_set', 'mcl_drift_mean_cov')
ERR_INVALID = -1


def _declared():
    src = open(os.path.join(ROOT, 'include', 'mcl_drift.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src)))


def test_drift_symbols_declared_exported_and_bound_at_abi_4():
    from smarc_navigation_amd import _lib
    assert _declared() == sorted(NAMES)
    assert sorted(_lib.DRIFT_SYMBOLS) == sorted(NAMES)
    others = (set(_lib.SYMBOLS) | set(_lib.RECOVERY_SYMBOLS) | set(_lib.MODES_SYMBOLS) | set(_lib.HISTORY_SYMBOLS) |
              set(_lib.ACOUSTIC_SYMBOLS) | set(_lib.TEMPER_SYMBOLS))
    assert not set(NAMES) & others
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), 'libmcl_hip.so does not export %s' % n
    lib = _lib.load()
    assert lib.mcl_abi_version() == 4
    counts = dict(mcl_drift_bytes=2, mcl_drift_config_check=2, mcl_drift_enable=3, mcl_drift_reset=2, mcl_drift_disable=1,
                  mcl_drift_advance=3, mcl_drift_get=2, mcl_drift_set=2, mcl_drift_mean_cov=3)
    for n in NAMES:
        assert getattr(lib, n).argtypes is not None, n
        assert len(_lib.DRIFT_SYMBOLS[n][1]) == counts[n], n


def test_abi_version_timing_table_and_config_layout_are_unchanged():
    from smarc_navigation_amd import _lib
    assert re.search(r'#define\s+MCL_ABI_VERSION\s+4\b', open(os.path.join(ROOT, 'include', 'mcl.h')).read())
    assert ctypes.sizeof(_lib.Timing) == 15 * 16          # MCL_K_COUNT entries of (double ms, int64 launches)
    assert ctypes.sizeof(_lib.DriftConfig) == 48
    assert _lib.DriftConfig.init_std.offset == 0 and _lib.DriftConfig.walk_std.offset == 24


def _bytes(n):
    from smarc_navigation_amd import _lib
    b = ctypes.c_int64(-7)
    return _lib.load().mcl_drift_bytes(n, ctypes.byref(b)), b.value


def test_drift_bytes_is_the_headers_count():
    # 24 B per particle (three doubles), 9 x 2048 reduction records and 12 result words of 8 B
    for n in (1, 63, 1000, 4096, 1 << 20, (1 << 31) - 1):
        assert _bytes(n) == (0, 24 * n + 8 * 9 * 2048 + 8 * 12), n
    assert _bytes(1 << 20)[1] == 24 * (1 << 20) + 147552
    from smarc_navigation_amd import engine
    assert engine.drift_bytes(4096) == 24 * 4096 + 147552


@pytest.mark.parametrize('n', [0, -1, 1 << 31])
def test_drift_bytes_refusals(n):
    from smarc_navigation_amd import _lib
    assert _bytes(n) == (ERR_INVALID, -7)                 # nothing is written on a refusal
    assert _lib.load().mcl_drift_bytes(1000, None) == ERR_INVALID


def _check(init_std, walk_std):
    from smarc_navigation_amd import _lib, engine
    cfg, why = engine.make_drift_config(init_std, walk_std), ctypes.c_char_p()
    st = _lib.load().mcl_drift_config_check(ctypes.byref(cfg), ctypes.byref(why))
    return st, (why.value or b'').decode()


def test_config_check_accepts_zeros_and_positive_stds():
    assert _check([0.0, 0.0, 0.0], [0.0, 0.0, 0.0]) == (0, '')
    assert _check([0.2, 0.2, 1e-3], [0.005, 0.005, 1e-5]) == (0, '')
    assert _check([-0.0, 1e300, 5e-324], [0.0, 0.0, 0.0]) == (0, '')


@pytest.mark.parametrize('bad', [-1.0, -1e-300, float('nan'), float('inf'), -float('inf')])
@pytest.mark.parametrize('which', range(6))
def test_config_check_names_the_std_it_refuses(which, bad):
    from smarc_navigation_amd import _lib, engine
    stds = [0.1, 0.2, 0.3, 0.01, 0.02, 0.03]
    stds[which] = bad
    st, why = _check(stds[:3], stds[3:])
    assert st == ERR_INVALID
    assert why.startswith('%s[%d]' % ('init_std' if which < 3 else 'walk_std', which % 3)), why
    assert engine.drift_config_check(stds[:3], stds[3:]) == why
    # the reason is optional, a null configuration is refused too
    cfg = engine.make_drift_config(stds[:3], stds[3:])
    assert _lib.load().mcl_drift_config_check(ctypes.byref(cfg), None) == ERR_INVALID
    assert _lib.load().mcl_drift_config_check(None, None) == ERR_INVALID


def test_config_check_names_the_first_of_two():
    assert _check([0.1, -1.0, 0.0], [float('nan'), 0.0, 0.0])[1].startswith('init_std[1]')


def test_calls_refuse_a_null_handle():
    from smarc_navigation_amd import _lib, engine
    lib = _lib.load()
    cfg = engine.make_drift_config([0, 0, 0], [0, 0, 0])
    buf = np.zeros(9)
    assert lib.mcl_drift_enable(None, ctypes.byref(cfg), None) == ERR_INVALID
    assert lib.mcl_drift_reset(None, None) == ERR_INVALID
    assert lib.mcl_drift_disable(None) == ERR_INVALID
    assert lib.mcl_drift_advance(None, 0.02, None) == ERR_INVALID
    assert lib.mcl_drift_get(None, buf.ctypes.data) == ERR_INVALID
    assert lib.mcl_drift_set(None, buf.ctypes.data) == ERR_INVALID
    assert lib.mcl_drift_mean_cov(None, buf.ctypes.data, buf.ctypes.data) == ERR_INVALID


# ------------------------------------------------------------------ the synthetic stream
ODOM_FIELDS = ('stamp', 'dt', 't0', 'v', 'wz', 'q', 'z', 'rpy')


def test_default_stream_is_bit_for_bit_the_stream_without_the_keywords():
    from smarc_navigation_amd import synth
    a = synth.odom_stream(700)
    b = synth.odom_stream(700, current=(0.0, 0.0), yaw_rate_bias=0.0)
    assert sorted(a) == sorted(b) == sorted(ODOM_FIELDS + ('truth',))
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_a_current_moves_the_truth_and_nothing_the_odometry_reports():
    from smarc_navigation_amd import synth
    n, cur = 700, (0.15, -0.10)
    a, b = synth.odom_stream(n), synth.odom_stream(n, current=cur)
    assert sorted(a) == sorted(b)
    for k in ODOM_FIELDS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    t = (np.arange(n) + 1) * a['dt']                      # the time integrated up to sample k
    want = a['truth'].copy()
    want[:, 0] += cur[0] * t
    want[:, 1] += cur[1] * t
    assert np.array_equal(b['truth'], want)
    assert abs(b['truth'][-1, 0] - a['truth'][-1, 0] - 0.15 * n * 0.02) < 1e-12


def test_a_yaw_rate_bias_turns_the_truth_and_nothing_the_odometry_reports():
    from smarc_navigation_amd import synth
    n, bias = 400, 2e-3
    a, b = synth.odom_stream(n), synth.odom_stream(n, yaw_rate_bias=bias)
    for k in ODOM_FIELDS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    t = (np.arange(n) + 1) * a['dt']
    d = synth.wrap_pi(b['truth'][:, 5] - a['truth'][:, 5] - bias * t)
    assert np.max(np.abs(d)) < 1e-12
    assert np.array_equal(a['truth'][:, 2:5], b['truth'][:, 2:5])
    assert not np.array_equal(a['truth'][:, :2], b['truth'][:, :2])     # the path bends with the heading


# ------------------------------------------------------------------ replay: the synthetic stream and its flags
def test_synthetic_stream_carries_the_truth_the_fixes_and_the_drift_it_was_made_with():
    from smarc_navigation_amd import replay, synth
    st = replay.synthetic_stream(300, current=(0.15, -0.10), yaw_rate_bias=1e-3)
    ref = synth.odom_stream(300, current=(0.15, -0.10), yaw_rate_bias=1e-3)
    for k in ODOM_FIELDS + ('truth',):
        assert np.array_equal(np.asarray(st[k]), np.asarray(ref[k])), k
    assert np.array_equal(st['truth_xyz'], ref['truth'][:, :3])
    assert st['drift_truth'].tolist() == [0.15, -0.10, 1e-3]
    assert st['gps_idx'].tolist() == list(range(49, 300, 50)) and st['gps_xy_utm'].shape == (6, 2)
    assert np.max(np.abs(st['gps_xy_utm'] - ref['truth'][st['gps_idx'], :2])) < 3.0      # fixes of 0.5 m around the truth
    assert len(replay.SYNTH_PARAMS['motion_covariance'].split(', ')) == 6


@pytest.mark.parametrize('argv', [['some.npz', '--current', '0.1', '0.0'], ['some.npz', '--yaw-rate-bias', '0.001'],
                                  ['synth', '--drift-init-std', '0.1', '0.1', '0.0'], ['synth:100', '--bag'],
                                  ['synth', '--estimate-drift', '--recover']])
def test_replay_refuses_flag_combinations_that_mean_nothing(argv, capsys):
    from smarc_navigation_amd import replay
    with pytest.raises(SystemExit) as ei:
        replay.main(argv)
    assert ei.value.code == 2
