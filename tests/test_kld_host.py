"""Host tests of KLD-sampling across handles (include/mcl_kld.h; no GPU): the ABI, mcl_kld_bound against a Python
restatement (the anchors of the header's definition, a sweep of k, both clamps, every refused argument), mcl_kld_grid_check
at its limits, the ladder policy adaptive.KldLadder, adaptive.AdaptiveCloud over recording engines, the summary of
replay_recover with and without --kld, and the sanitizer driver tests/host_san/kld_driver.cpp."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1
NAMES = ('mcl_kld_grid_check', 'mcl_kld_bins', 'mcl_kld_bound', 'mcl_resample_into', 'mcl_transfer_last_indices')
Z99 = 2.3263478740408408
ANCHOR_K = (2, 3, 10, 30, 100, 1000, 10000, 100000)
ANCHORS = {0.05: (66, 93, 217, 497, 1347, 11060, 103310, 1010424),
           0.01: (330, 462, 1085, 2481, 6733, 55297, 516546, 5052116)}


@pytest.fixture(scope='module')
def lib():
    from smarc_navigation_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def bound_ref(k, epsilon, z, n_min, n_max):
    """the header's steps in Python doubles, written here from the header (not imported from the package)"""
    if k <= 1:
        return n_min
    a = 2.0 / (9.0 * (k - 1))
    t = (1.0 - a) + math.sqrt(a) * z
    v = (((k - 1) / (2.0 * epsilon)) * t) * t * t
    if not math.isfinite(v):
        return n_max
    return min(max(int(math.ceil(v)), n_min), n_max)


# ------------------------------------------------------------------ the ABI
def test_every_symbol_of_the_header_is_exported_and_bound_in_a_table_of_its_own(lib):
    from smarc_navigation_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'mcl_kld.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(NAMES) == sorted(_lib.KLD_SYMBOLS)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    for table in (_lib.SYMBOLS, _lib.RECOVERY_SYMBOLS, _lib.MODES_SYMBOLS, _lib.RESEED_SYMBOLS, _lib.DRIFT_SYMBOLS):
        assert not set(table) & set(NAMES)
    assert lib.mcl_abi_version() == 4
    assert ctypes.sizeof(_lib.Timing) == 15 * 16                 # no timing slot was added
    for other in ('mcl.h', 'mcl_modes.h', 'mcl_recovery.h', 'mcl_drift.h', 'mcl_history.h', 'mcl_reseed.h'):
        assert 'kld' not in open(os.path.join(ROOT, 'include', other)).read().lower()   # the existing headers are what they were
    assert '#define MCL_KLD_MAX_CELLS (1 << 27)' in src and '#define MCL_KLD_MAX_YAW 1024' in src


# ------------------------------------------------------------------ the bound
@pytest.mark.parametrize('eps', [0.05, 0.01])
def test_the_anchors(eng, eps):
    from smarc_navigation_amd import adaptive
    for k, want in zip(ANCHOR_K, ANCHORS[eps]):
        assert eng.kld_bound(k, eps) == want == bound_ref(k, eps, Z99, 1, 2 ** 31) == adaptive.kld_bound(k, eps)


@pytest.mark.parametrize('eps', [0.05, 0.01, 1e-4])
def test_the_bound_equals_the_restatement_on_a_sweep_of_k(eng, eps):
    from smarc_navigation_amd import adaptive
    rs = np.random.RandomState(7)
    ks = [0, 1, 2, 3] + [2 ** j for j in range(28)] + [2 ** j - 1 for j in range(2, 28)] + [int(v) for v in rs.randint(0, 2 ** 27, 300)]
    ks += [int(v) for v in rs.randint(0, 5000, 300)]
    for k in ks:
        for z in (Z99, 0.0, 1.6448536269514722):
            want = bound_ref(k, eps, z, 1, 2 ** 31)
            assert eng.kld_bound(k, eps, z) == want == adaptive.kld_bound(k, eps, z), (k, eps, z)
    assert eng.kld_bound(2 ** 27, 1e-4) == 2 ** 31                  # (the upper clamp is reached inside the sweep)


def test_both_clamps_and_k_below_two(eng):
    assert eng.kld_bound(0, n_min=7) == 7 and eng.kld_bound(1, n_min=7) == 7
    assert eng.kld_bound(2, n_min=100, n_max=200) == 100            # 66 below n_min
    assert eng.kld_bound(1000, n_min=100, n_max=200) == 200         # 11 060 above n_max
    assert eng.kld_bound(30, n_min=497, n_max=497) == 497
    assert eng.kld_bound(10 ** 6, 1e-300, 1e300) == 2 ** 31         # v overflows: n_max
    assert eng.kld_bound(2, 5e-324, n_max=77) == 77


def test_every_refused_argument(lib, eng):
    n = ctypes.c_int64(-7)
    ok = [2, 0.05, Z99, 1, 2 ** 31]

    def call(i, v, out=True):
        a = list(ok)
        a[i] = v
        return lib.mcl_kld_bound(a[0], a[1], a[2], a[3], a[4], ctypes.byref(n) if out else None)
    assert call(0, 2) == 0 and n.value == 66
    n.value = -7
    assert call(0, -1) == ERR_INVALID
    for e in (0.0, -0.05, float('inf'), float('-inf'), float('nan')):
        assert call(1, e) == ERR_INVALID, e
    for z in (-1e-300, -1.0, float('inf'), float('-inf'), float('nan')):
        assert call(2, z) == ERR_INVALID, z
    assert call(3, 0) == ERR_INVALID and call(3, -5) == ERR_INVALID
    assert call(4, 2 ** 31 + 1) == ERR_INVALID and call(4, 0) == ERR_INVALID
    assert lib.mcl_kld_bound(2, 0.05, Z99, 9, 8, ctypes.byref(n)) == ERR_INVALID
    assert call(0, 2, out=False) == ERR_INVALID
    assert n.value == -7                                            # a refused call writes nothing
    with pytest.raises(Exception):
        eng.kld_bound(-1)


# ------------------------------------------------------------------ the lattice check
def test_the_lattice_check_at_its_limits(lib, eng):
    assert eng.kld_grid_check(eng.make_mode_grid(0.0, 0.0, 0.5, 1 << 12, 1 << 12, 8)) == 2 ** 27
    assert eng.kld_grid_check(eng.make_mode_grid(0.0, 0.0, 0.5, (1 << 12) + 1, 1 << 12, 8)) is None      # one row more
    assert eng.kld_grid_check(eng.make_mode_grid(0.0, 0.0, 0.5, 2 ** 27, 1, 1)) == 2 ** 27
    assert eng.kld_grid_check(eng.make_mode_grid(0.0, 0.0, 0.5, 2 ** 27 + 1, 1, 1)) is None               # one cell more
    assert eng.kld_grid_check(eng.make_mode_grid(0.0, 0.0, 0.5, 4, 4, 1024)) == 16384
    assert eng.kld_grid_check(eng.make_mode_grid(0.0, 0.0, 0.5, 4, 4, 1025)) is None
    assert eng.kld_grid_check(eng.make_mode_grid(0.0, 0.0, 0.5, 2 ** 31 - 1, 2 ** 31 - 1, 1024)) is None  # no overflow
    # AMCL's default bins on a 768 m map fit (pose_modes' lattice check refuses them)
    g = eng.make_mode_grid(-384.0, -384.0, 0.5, 1536, 1536, 36)
    assert eng.kld_grid_check(g) == 1536 * 1536 * 36 < 2 ** 27 and lib.mcl_mode_grid_check(ctypes.byref(g), None) == ERR_INVALID
    for bad in (dict(cell=0.0), dict(cell=float('nan')), dict(cell=float('inf')), dict(x0=float('nan')), dict(y0=float('inf')),
                dict(nx=0), dict(ny=-1), dict(n_yaw=0)):
        kw = dict(x0=0.0, y0=0.0, cell=0.5, nx=4, ny=4, n_yaw=4)
        kw.update(bad)
        assert eng.kld_grid_check(eng.make_mode_grid(**kw)) is None, bad
    assert lib.mcl_kld_grid_check(None, None) == ERR_INVALID
    assert lib.mcl_kld_grid_check(ctypes.byref(eng.make_mode_grid(0.0, 0.0, 0.5, 4, 4, 4)), None) == 0   # n_cells may be NULL


# ------------------------------------------------------------------ the ladder
SIZES = [2 ** 11, 2 ** 14, 2 ** 17, 2 ** 20]


def k_for(ladder, rung):
    """a k whose want() is exactly `rung`"""
    for k in (2, 40, 100, 300, 1000, 3000, 10000, 10 ** 5, 10 ** 6):
        if ladder.want(k) == rung:
            return k
    raise AssertionError(rung)


def test_want_is_the_smallest_size_that_holds_headroom_times_the_bound():
    from smarc_navigation_amd.adaptive import KldLadder, kld_bound
    lad = KldLadder(SIZES, 0.05, headroom=2.0)
    for k in (0, 1, 2, 50, 69, 70, 71, 100, 580, 600, 1000, 5000, 6000, 10 ** 5, 10 ** 7):
        need = 2.0 * kld_bound(k, 0.05)
        fits = [i for i, s in enumerate(SIZES) if s >= need]
        assert lad.want(k) == (fits[0] if fits else 3), k
    assert lad.want(10 ** 7) == 3 and lad.want(0) == 0
    assert KldLadder(SIZES, 0.05, headroom=1.0).want(100) == 0 and lad.want(100) == 1      # 1 347 vs 2 694 particles
    assert lad.rung == 3                                                                  # it starts on top


def test_up_at_once_and_down_only_after_patience():
    from smarc_navigation_amd.adaptive import KldLadder
    lad = KldLadder(SIZES, 0.05, patience=5)
    low, mid, top = k_for(lad, 0), k_for(lad, 1), k_for(lad, 3)
    assert [lad.decide(low) for _ in range(4)] == [3, 3, 3, 3]      # four calls that want less: nothing yet
    assert lad.decide(low) == 0                                     # the fifth
    assert lad.decide(mid) == 1                                     # up at once
    assert lad.decide(top) == 3                                     # ... by any number of rungs
    assert [lad.decide(low) for _ in range(5)] == [3, 3, 3, 3, 0]


def test_a_streak_is_broken_by_one_higher_want():
    from smarc_navigation_amd.adaptive import KldLadder
    lad = KldLadder(SIZES, 0.05, patience=3)
    low, top = k_for(lad, 0), k_for(lad, 3)
    assert [lad.decide(k) for k in (low, low, top, low, low)] == [3, 3, 3, 3, 3]      # the want of the own rung breaks it
    assert lad.decide(low) == 0
    lad.reset()
    two = k_for(lad, 2)
    assert [lad.decide(k) for k in (low, low, two)] == [3, 3, 2]                      # three lower wants: down to the HIGHEST of them
    lad.reset()
    assert [lad.decide(k) for k in (low, two, low)] == [3, 3, 2]


def test_down_goes_to_the_highest_rung_wanted_during_the_streak():
    from smarc_navigation_amd.adaptive import KldLadder
    lad = KldLadder(SIZES, 0.05, patience=4)
    low, mid, two = k_for(lad, 0), k_for(lad, 1), k_for(lad, 2)
    assert [lad.decide(k) for k in (low, mid, low, low)] == [3, 3, 3, 1]
    assert [lad.decide(k) for k in (low, low, low, low)] == [1, 1, 1, 0]              # a new streak from the new rung
    lad.reset()
    assert [lad.decide(k) for k in (two, low, low, low)] == [3, 3, 3, 2]
    # the streak's maximum does not survive the streak
    lad.reset()
    assert [lad.decide(k) for k in (two, k_for(lad, 3), low, low, low, low)] == [3, 3, 3, 3, 3, 0]


def test_a_single_rung_ladder_never_moves_and_bad_ladders_are_refused():
    from smarc_navigation_amd.adaptive import KldLadder
    lad = KldLadder([4096], 0.05, patience=1)
    assert [lad.decide(k) for k in (0, 1, 10, 10 ** 7, 2)] == [0] * 5 and lad.want(10 ** 9) == 0
    for bad in ([], [0, 4], [8, 8], [16, 8]):
        with pytest.raises(ValueError):
            KldLadder(bad, 0.05)
    for kw in (dict(epsilon=0.0), dict(epsilon=float('nan')), dict(z=-1.0), dict(headroom=0.5), dict(patience=0)):
        with pytest.raises(ValueError):
            KldLadder(**dict(dict(sizes=SIZES, epsilon=0.05), **kw))


def test_the_ladder_is_a_function_of_the_sequence_of_k_alone():
    from smarc_navigation_amd.adaptive import KldLadder
    rs = np.random.RandomState(3)
    ks = [int(10 ** rs.uniform(0, 6)) for _ in range(400)]
    a, b = KldLadder(SIZES, 0.05), KldLadder(SIZES, 0.05)
    ra = [a.decide(k) for k in ks]
    assert ra == [b.decide(k) for k in ks] and len(set(ra)) > 1
    for i in range(1, len(ks)):                                    # never below what the call itself wanted; up means wanted
        assert ra[i] >= a.want(ks[i]) and (ra[i] <= ra[i - 1] or ra[i] == a.want(ks[i]))


# ------------------------------------------------------------------ the cloud over recording engines
class RecordingEngine(object):
    """what AdaptiveCloud drives, without a device: every call is logged in one shared list; kld_bins answers from a
    script of k"""

    def __init__(self, n, log, script):
        self.n, self.log, self.script = n, log, script

    def set_map_grid(self, z, origin, res):
        self.log.append((self.n, 'set_map_grid'))

    def set_map_mesh(self, verts, tris, **kw):
        self.log.append((self.n, 'set_map_mesh', kw))

    def resample(self, uniforms=None, normals=None):
        self.log.append((self.n, 'resample', uniforms, normals))

    def kld_grid(self, cell, n_yaw, box):
        self.log.append((self.n, 'kld_grid', cell, n_yaw, box))
        return ('grid', cell, n_yaw, box)

    def kld_bins(self, cell=None, n_yaw=36, box=None, grid=None):
        self.log.append((self.n, 'kld_bins', grid))
        return self.script.pop(0), 0

    def resample_into(self, dst, uniform=None):
        self.log.append((self.n, 'resample_into', dst.n))

    def predict(self, *a):
        self.log.append((self.n, 'predict'))

    def close(self):
        self.log.append((self.n, 'close'))


def make_cloud(script, patience=2, **kw):
    from smarc_navigation_amd.adaptive import AdaptiveCloud, KldLadder
    log = []
    engines = [RecordingEngine(s, log, script) for s in SIZES]
    return AdaptiveCloud(engines, KldLadder(SIZES, 0.05, patience=patience), 0.5, 36, **kw), log


def test_the_cloud_resamples_counts_decides_and_moves_in_that_order():
    from smarc_navigation_amd.adaptive import KldLadder
    lad = KldLadder(SIZES, 0.05)
    low, top = k_for(lad, 0), k_for(lad, 3)
    cloud, log = make_cloud([low, low, low, top], box=(0.0, 8.0, 0.0, 8.0))
    cloud.set_map_grid(None, (0, 0), 1.0)
    assert [c[0] for c in log] == SIZES and all(c[1] == 'set_map_grid' for c in log)       # every engine gets the map
    del log[:]
    assert cloud.active.n == 2 ** 20
    cloud.predict()                                                                       # what the class lacks is the active engine's
    assert log == [(2 ** 20, 'predict')]
    del log[:]
    assert cloud.resample() == 2 ** 20                                                    # the rung stays: no transfer
    g = ('grid', 0.5, 36, (0.0, 8.0, 0.0, 8.0))
    assert log == [(2 ** 20, 'resample', None, None), (2 ** 20, 'kld_grid', 0.5, 36, (0.0, 8.0, 0.0, 8.0)), (2 ** 20, 'kld_bins', g)]
    del log[:]
    assert cloud.resample(ping=17) == 2 ** 11                                             # the second lower want: down
    assert log == [(2 ** 20, 'resample', None, None), (2 ** 20, 'kld_bins', g), (2 ** 20, 'resample_into', 2 ** 11)]
    assert cloud.active.n == 2 ** 11 and cloud.moves == 1
    del log[:]
    assert cloud.resample(uniforms=0.25) == 2 ** 11
    assert log == [(2 ** 11, 'resample', 0.25, None), (2 ** 11, 'kld_bins', g)]             # no transfer while the rung stays
    del log[:]
    assert cloud.resample() == 2 ** 20                                                    # up at once, from the small engine
    assert log[-1] == (2 ** 11, 'resample_into', 2 ** 20) and cloud.moves == 2
    from smarc_navigation_amd.adaptive import kld_bound
    assert cloud.trace == [(0, low, kld_bound(low), 2 ** 20), (17, low, kld_bound(low), 2 ** 11), (2, low, kld_bound(low), 2 ** 11),
                           (3, top, kld_bound(top), 2 ** 20)]


def test_to_top_moves_the_cloud_once_and_forgets_the_streak():
    from smarc_navigation_amd.adaptive import KldLadder
    low = k_for(KldLadder(SIZES, 0.05), 0)
    cloud, log = make_cloud([low] * 6)
    assert cloud.to_top() is False and log == []                                          # on top already
    cloud.resample()
    cloud.resample()
    assert cloud.active.n == 2 ** 11
    del log[:]
    assert cloud.to_top() is True and log == [(2 ** 11, 'resample_into', 2 ** 20)] and cloud.active.n == 2 ** 20
    cloud.resample()
    assert cloud.active.n == 2 ** 20                                                      # one lower want after it: not yet
    cloud.close()
    assert [c for c in log if c[1] == 'close'] == [(s, 'close') for s in SIZES]


def test_the_cloud_refuses_engines_that_are_not_the_ladder():
    from smarc_navigation_amd.adaptive import AdaptiveCloud, KldLadder
    log = []
    with pytest.raises(ValueError):
        AdaptiveCloud([RecordingEngine(s, log, []) for s in reversed(SIZES)], KldLadder(SIZES, 0.05))


# ------------------------------------------------------------------ replay_recover's summary
class _Stats(object):
    def __init__(self, lml):
        self.log_mean_lik, self.n_eff = lml, 100.0


class FakeEngine(object):
    """what replay_recover drives, without a device: every engine logs into one shared list; the cells collapse at ping 4"""
    calls, resamples = [], [0]

    def __init__(self, n, **kw):
        self.n, self.m2o = int(n), np.identity(4)
        FakeEngine.calls.append((self.n, 'create'))

    def _log(self, name, *a):
        FakeEngine.calls.append((self.n, name) + a)

    def set_map_grid(self, z, origin, res):
        self._log('set_map_grid')

    def init_particles_uniform(self, box=None, frame='map', yaw=(-math.pi, math.pi), uniforms=None):
        self._log('init_particles_uniform')

    def predict(self, *a, **kw):
        self._log('predict')

    def update_mbes(self, ranges, angles, sigma, r_max):
        self._log('update_mbes')

    def weight_stats(self):
        return _Stats(-16.0)

    def resample(self, uniforms=None, normals=None):
        FakeEngine.resamples[0] += 1
        self._log('resample')

    def kld_grid(self, cell, n_yaw, box):
        self._log('kld_grid', cell, n_yaw)
        return 'grid'

    def kld_bins(self, cell=None, n_yaw=36, box=None, grid=None):
        self._log('kld_bins')
        return (10 ** 6 if FakeEngine.resamples[0] < 4 else 2), 0

    def resample_into(self, dst, uniform=None):
        self._log('resample_into', dst.n)

    def mean_cov(self):
        return np.array([1.0, 2.0, -2.0, 0.0, 0.0, 0.0]), 0.5, np.zeros(9)

    def close(self):
        self._log('close')


def _stream():
    from smarc_navigation_amd import synth
    st = synth.odom_stream(n_steps=40, dt=0.5)
    st['mbes_idx'] = np.arange(1, 40, 2)
    st['mbes_angles'] = synth.beam_angles(16)
    st['mbes_ranges'] = np.full((20, 16), 20.0, np.float32)
    st['truth_xyz'] = st['truth'][:, :3]
    return st


def test_replay_recover_is_unchanged_without_kld_and_gains_its_keys_with_it(eng, monkeypatch):
    from smarc_navigation_amd import replay
    monkeypatch.setattr(eng, 'Engine', FakeEngine)
    grid = dict(z=np.zeros((8, 8), np.float32), origin=(0.0, 0.0), res=1.0)
    FakeEngine.calls, FakeEngine.resamples = [], [0]
    plain = replay.replay_recover(_stream(), grid=grid, particles=4096)
    assert sorted(plain['summary']) == ['final_error_vs_truth', 'injected_total', 'pf_distance', 'pf_final', 'pings']
    assert 'kld_trace' not in plain
    names = [c[1] for c in FakeEngine.calls]
    assert set(c[0] for c in FakeEngine.calls) == {4096}                                   # one engine
    assert names[:3] == ['create', 'set_map_grid', 'init_particles_uniform'] and names[-1] == 'close'
    assert set(names[3:-1]) == {'predict', 'update_mbes', 'resample'} and names.count('resample') == 20      # the calls of before
    FakeEngine.calls, FakeEngine.resamples = [], [0]
    res = replay.replay_recover(_stream(), grid=grid, particles=4096, kld=0.05, kld_cell=0.25, kld_n_yaw=18)
    s = res['summary']
    assert sorted(s) == sorted(list(plain['summary']) + ['kld_sizes_used', 'kld_final_size', 'kld_moves'])
    assert s['kld_sizes_used'] == [256, 4096] and s['kld_final_size'] == 256 and s['kld_moves'] == 1
    created = [c[0] for c in FakeEngine.calls if c[1] == 'create']
    assert created == [256, 512, 4096]                                                    # particles, / 8, / 64 and / 512 held at 256
    assert [c for c in FakeEngine.calls if c[1] == 'kld_grid'] == [(4096, 'kld_grid', 0.25, 18)]
    assert [c for c in FakeEngine.calls if c[1] == 'resample_into'] == [(4096, 'resample_into', 256)]
    assert [c[0] for c in FakeEngine.calls if c[1] == 'init_particles_uniform'] == [4096]   # the search starts on the largest
    first_move = [i for i, c in enumerate(FakeEngine.calls) if c[1] == 'resample_into'][0]
    assert any(c[1] == 'resample' for c in FakeEngine.calls[:first_move])                 # no move before the first resample
    assert len(res['kld_trace']) == 20 and tuple(int(v) for v in res['kld_trace'][0]) == (0, 10 ** 6, eng.kld_bound(10 ** 6), 4096)
    explicit = replay.replay_recover(_stream(), grid=grid, particles=4096, kld=0.05, kld_sizes=[4096, 64])
    assert explicit['summary']['kld_sizes_used'] == [4096] and explicit['summary']['kld_moves'] == 0      # 2 x 66 particles do not fit 64
    with pytest.raises(ValueError):
        replay.replay_recover(_stream(), grid=grid, particles=4096, kld=0.05, smooth_lag=4)
    with pytest.raises(ValueError):
        replay.replay_recover(_stream(), grid=grid, particles=4096, kld=-1.0)


def test_the_command_line_takes_kld_only_with_recover():
    from smarc_navigation_amd import replay
    for bad in (['synth:100', '--kld', '0.05'], ['x.npz', '--recover', '--kld', '-1'],
                ['x.npz', '--recover', '--kld-sizes', '64'], ['x.npz', '--recover', '--kld', '0.05', '--kld-cell', '0'],
                ['x.npz', '--recover', '--kld', '0.05', '--kld-n-yaw', '1025'],
                ['x.npz', '--recover', '--kld', '0.05', '--smooth', '4']):
        with pytest.raises(SystemExit):
            replay.main(bad)


# ------------------------------------------------------------------ the sanitizer driver
def test_the_host_arithmetic_runs_clean_under_the_sanitizers_as_a_program(tmp_path):
    """tests/host_san/kld_driver.cpp: its own main over the device-free functions, g++ -fsanitize=address,undefined, run as a
    program (nothing loaded into Python runs under a sanitizer)"""
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no g++ / make')
    san = str(tmp_path / 'host_san')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'smarc_navigation_amd', 'csrc'), 'host-asan-kld', 'SAN_DIR=' + san],
                          stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(san, 'kld_asan')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                       timeout=300, cwd=ROOT)
    for marker in ('AddressSanitizer', 'runtime error', 'LeakSanitizer'):
        assert marker not in p.stdout, p.stdout[-2000:]
    assert p.returncode == 0 and 'kld_driver: ok' in p.stdout, p.stdout[-2000:]
