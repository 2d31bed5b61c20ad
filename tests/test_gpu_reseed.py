"""GPU tests of the sensor resetting (include/mcl_reseed.h; csrc/mcl_reseed.h): the state mcl_inject_gaussian leaves against
the numpy restatement of tests/reseed_ref.py bit for bit (Philox, the word rules, the library's Box-Muller, the component
rule, the apply rule), REPLAY mode at its edges, the shared injection counter, shards, drift and genealogy, the errors, the
visiting-order rule, the moments of a million draws, and two runs on the closed loops' scene of tests/test_gpu_recovery.py:
a global search that finds the truth, and a kidnap that the guided injection recovers from with a cloud so small that the
uniform injection does not."""
import math

import numpy as np
import pytest

from smarc_navigation_amd import synth
from tests import reseed_ref as ref
from tests.test_gpu_recovery import (BOX, ERR_INVALID, ERR_STATE, LOOP_COV, LOOP_ORIGIN, LOOP_RMAX, LOOP_SIGMA, YAW, _grid_scene,
                                     expect_status, loop_scene)

pytestmark = pytest.mark.gpu

SEED = 0x1234567890abcdef
INIT_COV = [1, 1, 0.5, 0.1, 0.1, 0.2]


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ component tables
def full_factor(rs, sx=2.0, sw=0.1):
    """a packed lower-triangular factor with every entry set: (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)"""
    return np.array([sx * (0.5 + rs.rand()), sx * rs.randn(), sx * (0.5 + rs.rand()), sw * rs.randn(), sw * rs.randn(), sw * (0.5 + rs.rand())])


def table(eng, kind, seed=3):
    rs = np.random.RandomState(seed)
    if kind == '1':        # one component, a full factor, the yaw mean just below +pi: about half the draws wrap
        c = np.zeros(1, eng.ReseedComponent)
        c['mean'], c['chol'], c['mass'] = (12.5, -7.25, math.pi - 1e-3), full_factor(rs), 7
    elif kind == '2':      # an all-zero factor at yaw -pi (the mean's bits) and a dead middle column
        c = np.zeros(2, eng.ReseedComponent)
        c['mean'] = [(-3.0, 4.0, -math.pi), (30.0, -20.0, 0.5)]
        c['chol'][1] = full_factor(rs)
        c['chol'][1][[2, 4]] = 0.0
        c['mass'] = (3, 2)
    elif kind == '2z':     # the first component has no mass: never drawn
        c = np.zeros(2, eng.ReseedComponent)
        c['mean'] = [(1e6, 1e6, 0.0), (5.0, 6.0, -0.7)]
        c['chol'][0], c['chol'][1] = full_factor(rs), full_factor(rs)
        c['mass'] = (0, 1)
    else:                  # 256 components, masses of every size, zeros first, last and in the middle
        c = np.zeros(256, eng.ReseedComponent)
        c['mean'][:, 0], c['mean'][:, 1] = 80.0 * rs.randn(256), 80.0 * rs.randn(256)
        c['mean'][:, 2] = rs.uniform(-math.pi, math.pi, 256)
        c['chol'] = np.stack([full_factor(rs) for _ in range(256)])
        c['mass'] = rs.randint(1, 1 << 22, 256)
        c['mass'][[0, 100, 101, 255]] = 0
        c['mass'][7] = 1 << 28                         # a heavy one: most draws
        c['chol'][7] = 0.0                             # ... an all-zero factor,
        c['mean'][7, 2] = -math.pi                     # at yaw -pi
        c['mass'][8] = 1 << 27
        c['chol'][8][[2, 4]] = 0.0                     # a dead middle column
        c['mass'][9] = 1 << 27
        c['mean'][9, 2] = math.pi - 1e-3               # wraps
        c['mass'][254] = 1                             # the last one that can be drawn, almost never
    return c


# ------------------------------------------------------------------ NATIVE mode against the restatement
@pytest.mark.parametrize('n,kind,fraction', [(65, '1', 1.0), (65, '2', 1.0), (65, '256', 0.05), (100003, '1', 0.05),
                                             (100003, '2', 1.0), (100003, '2z', 1.0), (100003, '256', 1.0),
                                             (1048576, '1', 0.05), (1048576, '2', 0.05), (1048576, '256', 0.05)])
def test_native_injection_equals_the_restatement_bit_for_bit(eng, n, kind, fraction):
    comps = table(eng, kind)
    e = eng.Engine(n, seed=SEED, init_cov=INIT_COV)
    e.init_particles()
    s0 = e.get_particles()
    k = e.inject_gaussian(fraction, comps)
    s1 = e.get_particles()
    want, count, sel, c = ref.restate_native(s0, comps, fraction, SEED, 0)
    assert k == count == int(sel.sum())                                    # n_injected is the restated count
    assert abs(count - fraction * n) <= 5.0 * math.sqrt(n * fraction * (1.0 - fraction)) + (0 if fraction < 1.0 else 0)
    assert np.array_equal(bits(s1[:, ~sel]), bits(s0[:, ~sel]))            # an unselected particle keeps every bit
    assert np.array_equal(bits(s1[2:5]), bits(s0[2:5]))                    # a selected one its z, roll and pitch
    assert np.array_equal(bits(s1), bits(want))                            # x, y, yaw of the selected: the restatement's bits
    assert np.all(comps['mass'][c] > 0)                                    # a component without mass is never drawn
    assert np.all((s1[5, sel] >= -math.pi) & (s1[5, sel] < math.pi))
    if kind == '2':      # the all-zero factor: the mean's own bits, yaw -pi among them
        zero = np.flatnonzero(sel)[c == 0]
        assert zero.size > 0 and np.all(bits(s1[0, zero]) == bits(-3.0)) and np.all(bits(s1[5, zero]) == bits(-math.pi))
    if kind == '1' and n > 65:
        assert np.any(s1[5, sel] < 0.0) and np.any(s1[5, sel] > 3.0)       # both sides of the seam
    if kind == '256' and count > 10000:
        assert {7, 8, 9} <= set(np.unique(c)) and np.unique(c).size > 100
    e.close()


def test_two_successive_calls_draw_differently_and_the_init_calls_reset_the_counter(eng):
    n, comps = 100003, table(eng, '256')
    e = eng.Engine(n, seed=SEED, init_cov=INIT_COV)
    e.init_particles()
    s0 = e.get_particles()
    e.inject_gaussian(0.3, comps, count=False)
    s1 = e.get_particles()
    assert e.inject_gaussian(0.3, comps, count=False) is None
    s2 = e.get_particles()
    w1, _, sel1, _ = ref.restate_native(s0, comps, 0.3, SEED, 0)
    w2, _, sel2, _ = ref.restate_native(s1, comps, 0.3, SEED, 1)            # the counter moved on
    assert np.array_equal(bits(s1), bits(w1)) and np.array_equal(bits(s2), bits(w2)) and not np.array_equal(sel1, sel2)
    e.init_particles()
    e.inject_gaussian(0.3, comps, count=False)
    assert np.array_equal(bits(e.get_particles()), bits(s1))
    e.close()


def test_fraction_zero_and_one_and_the_counter_shared_with_the_uniform_injection(eng):
    n, comps = 65536, table(eng, '2')
    a, b, c = [eng.Engine(n, seed=SEED, init_cov=INIT_COV) for _ in range(3)]
    for e in (a, b, c):
        e.init_particles()
    s0 = a.get_particles()
    a.timing_enable(True)
    assert a.inject_gaussian(0.0, comps) == 0
    assert a.timing_get()['noise'][1] == 0                                  # nothing was launched
    assert np.array_equal(bits(a.get_particles()), bits(s0))
    # ... and the counter stayed: the next uniform injection is a fresh handle's first
    assert a.inject_uniform(0.4, BOX, frame='odom', yaw=YAW) == b.inject_uniform(0.4, BOX, frame='odom', yaw=YAW)
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    # fraction 1 replaces all; it launched, so the uniform injection behind it draws at counter 2 -- as the third uniform
    # injection of a handle does (the purposes differ: the uniform draws keep their bits)
    assert a.inject_gaussian(1.0, comps) == n
    assert a.timing_get()['noise'][1] == 2
    s1 = a.get_particles()
    assert np.all(np.isin(s1[0], [-3.0]) | (s1[0] != s0[0])) and np.array_equal(bits(s1[2:5]), bits(s0[2:5]))
    want, count, _, _ = ref.restate_native(s0, comps, 1.0, SEED, 1)
    assert count == n and np.array_equal(bits(s1[[0, 1, 5]]), bits(want[[0, 1, 5]]))
    b.inject_uniform(1.0, BOX, frame='odom', yaw=YAW)
    assert a.inject_uniform(1.0, BOX, frame='odom', yaw=YAW) == n and b.inject_uniform(1.0, BOX, frame='odom', yaw=YAW) == n
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    # the other way round: a uniform injection moves the gaussian one's counter
    c.inject_uniform(0.1, BOX, frame='odom', yaw=YAW)
    sc = c.get_particles()
    c.inject_gaussian(0.5, comps)
    assert np.array_equal(bits(c.get_particles()), bits(ref.restate_native(sc, comps, 0.5, SEED, 1)[0]))
    for e in (a, b, c):
        e.close()


# ------------------------------------------------------------------ REPLAY mode
def test_replay_mode_at_its_edges(eng):
    n, frac = 65, 0.25
    comps = table(eng, '256')
    rs = np.random.RandomState(8)
    u = np.column_stack([rs.rand(n), rs.rand(n), rs.randn(n, 3)])
    u[0, 0] = frac                               # u_select == fraction: not replaced
    u[1, 0] = np.nextafter(frac, 0.0)            # the last value that is
    u[2, :2] = 0.0, 0.0                          # u_comp = 0: the first component with a positive mass
    u[3, :2] = 0.0, 1.0 - 2.0 ** -53             # ... the last
    u[4, :2] = 0.0, 2.0 ** -53                   # t = 1
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
    s0 = rs.randn(6, n)
    e.set_particles(s0)
    k = e.inject_gaussian(frac, comps, normals=u)
    s1 = e.get_particles()
    t = (u[:, 1] * ref.TWO53).astype(np.uint64)
    want, count, sel, c = ref.restate_inject(s0, comps, frac, u[:, 0], t, u[:, 2:].T.copy())
    assert k == count and not sel[0] and sel[1] and np.array_equal(bits(s1), bits(want))
    picked = dict(zip(np.flatnonzero(sel), c))
    positive = np.flatnonzero(comps['mass'] > 0)
    assert picked[2] == positive[0] == 1 and picked[3] == positive[-1] == 254 and picked[4] == 1
    assert np.array_equal(bits(s1[:, ~sel]), bits(s0[:, ~sel])) and np.array_equal(bits(s1[2:5]), bits(s0[2:5]))
    # what REPLAY mode refuses; the state stays
    expect_status(eng, ERR_INVALID, e.inject_gaussian, frac, comps)                       # no draws
    for bad in (1.0, -2.0 ** -60, math.nan):
        v = u.copy()
        v[n - 1, 1] = bad
        expect_status(eng, ERR_INVALID, e.inject_gaussian, frac, comps, normals=v)
    assert np.array_equal(bits(e.get_particles()), bits(s1))
    e.close()


# ------------------------------------------------------------------ shards, drift, genealogy
def test_eight_shards_equal_the_unsharded_cloud(eng):
    n, W = 1 << 20, 8
    comps = table(eng, '256')
    one = eng.Engine(n, seed=SEED)
    many = [eng.Engine(n // W, rank=r, world=W, n_global=n, global_offset=r * (n // W), seed=SEED) for r in range(W)]
    for s in many + [one]:
        s.init_particles_uniform(BOX, frame='odom', yaw=YAW)
    for rnd in range(2):
        k1 = one.inject_gaussian(0.3, comps)
        km = [s.inject_gaussian(0.3, comps) for s in many]
        assert sum(km) == k1 and min(km) > 0
        assert np.array_equal(bits(np.concatenate([s.get_particles() for s in many], axis=1)), bits(one.get_particles()))
    for s in many + [one]:
        s.close()


def test_drift_states_and_ancestor_links_of_replaced_slots_are_untouched(eng):
    n = 100003
    rs = np.random.RandomState(12)
    e = eng.Engine(n, seed=SEED, init_cov=INIT_COV, resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4])
    e.init_particles()
    e.drift_enable([0.2, 0.1, 1e-3], [0.0, 0.0, 0.0])
    e.history_enable(4)
    for stamp in (1.0, 2.0):
        e.set_log_weights(rs.randn(n))
        e.resample()
        e.history_record(stamp)
    e.set_log_weights(rs.randn(n))
    e.resample()                                   # a link that no frame holds yet
    d0, s0 = e.drift_get(), e.get_particles()
    anc0 = [e.history_ancestors(lag) for lag in (0, 1)]
    frames0 = e.history_frames()
    assert e.inject_gaussian(0.5, table(eng, '2')) > 0
    assert np.any(e.get_particles() != s0)
    assert np.array_equal(bits(e.drift_get()), bits(d0))
    for lag in (0, 1):
        assert np.array_equal(e.history_ancestors(lag), anc0[lag])
    assert e.history_frames()[:2] == frames0[:2]
    assert np.any(anc0[0] != np.arange(n))         # (the links were not the identity)
    e.close()


# ------------------------------------------------------------------ errors
def test_every_error_of_the_header_leaves_the_state_as_it_was(eng):
    n = 4099
    comps = table(eng, '2')
    e = eng.Engine(n, seed=SEED, init_cov=INIT_COV)
    e.init_particles()
    s0 = e.get_particles()
    for f in (1.5, -0.1, math.nan, math.inf):
        expect_status(eng, ERR_INVALID, e.inject_gaussian, f, comps)
    expect_status(eng, ERR_INVALID, e.inject_gaussian, 0.5, np.zeros(0, eng.ReseedComponent))          # n_comp = 0 (and a null table)
    big = np.zeros(257, eng.ReseedComponent)
    big['mass'] = 1
    expect_status(eng, ERR_INVALID, e.inject_gaussian, 0.5, big)
    assert e.lib.mcl_inject_gaussian(e.h, 0.5, None, 1, None, None) == ERR_INVALID
    assert e.lib.mcl_inject_gaussian(None, 0.5, comps.ctypes.data, 2, None, None) == ERR_INVALID
    for field, k, v in (('mean', 0, math.nan), ('mean', 2, math.inf), ('chol', 1, math.nan), ('chol', 5, -math.inf), ('chol', 0, -1.0),
                        ('chol', 2, -1e-300), ('chol', 5, -0.5)):
        bad = comps.copy()
        bad[field][1, k] = v
        expect_status(eng, ERR_INVALID, e.inject_gaussian, 0.5, bad)
        expect_status(eng, ERR_INVALID, e.inject_gaussian, 0.0, bad)                                    # ... whatever the fraction
    bad = comps.copy()
    bad['mass'] = 0
    expect_status(eng, ERR_INVALID, e.inject_gaussian, 0.5, bad)                                        # W = 0
    bad['mass'] = (1 << 31, 1)
    expect_status(eng, ERR_INVALID, e.inject_gaussian, 0.5, bad)                                        # W > 2^31
    assert np.array_equal(bits(e.get_particles()), bits(s0))
    bad['mass'] = (1 << 31, 0)                                                                           # W = 2^31 is legal
    assert e.inject_gaussian(0.0, bad) == 0
    e.set_log_weights(np.zeros(n))
    expect_status(eng, ERR_STATE, e.inject_gaussian, 0.5, comps)                                        # pending log-weights
    expect_status(eng, ERR_STATE, e.inject_gaussian, 0.0, comps)
    assert np.array_equal(bits(e.get_particles()), bits(s0))
    e.resample()
    s1 = e.get_particles()
    # none of the refused calls moved the shared counter: this one draws at counter 0
    assert e.inject_gaussian(0.5, bad) > 0
    assert np.array_equal(bits(e.get_particles()), bits(ref.restate_native(s1, bad, 0.5, SEED, 0)[0]))
    e.close()


# ------------------------------------------------------------------ the visiting-order rule
@pytest.mark.parametrize('kind', ['grid', 'tin'])
def test_update_after_an_injection_equals_a_fresh_handle_with_the_same_state(eng, kind):
    """the injection voids the visiting order the resample prepared: no log-likelihood depends on it"""
    n = 1 << 19   # (above the size from which a resample prepares the spatial visiting order)
    z, origin, ba, soa, ranges = _grid_scene(eng, n)
    cov = dict(process_cov=[1e-4, 1e-4, 0, 0, 0, 1e-6], resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4], seed=9)

    def with_map(e):
        if kind == 'grid':
            e.set_map_grid(z, origin, 1.0)
        else:
            v, t = synth.mesh_tin(z, 1.0, origin, seed=7)
            e.set_map_mesh(v, t, heightfield=True)
        return e

    a = with_map(eng.Engine(n, **cov))
    a.set_particles(soa)
    q = synth.quat_from_rpy(0.0, 0.0, 0.2)
    for _ in range(2):   # the node's sequence: the second resample follows a predict + update and prepares the order
        a.predict([1.0, 0.0, 0.0], 0.0, q, -2.0, 0.02)
        a.update_mbes(ranges, ba, 0.2, 60.0)
        a.resample()
    comps = np.zeros(2, eng.ReseedComponent)
    comps['mean'] = [(-4.0, 3.0, 0.2), (5.0, -2.0, 0.25)]
    comps['chol'][:, 0], comps['chol'][:, 2], comps['chol'][:, 5] = 1.5, 1.5, 0.05
    comps['mass'] = (1, 2)
    assert a.inject_gaussian(0.2, comps) > 0
    state = a.get_particles()
    a.update_mbes(ranges, ba, 0.2, 60.0)
    b = with_map(eng.Engine(n, **cov))
    b.set_particles(state)
    b.update_mbes(ranges, ba, 0.2, 60.0)
    assert np.array_equal(a.get_log_weights(), b.get_log_weights())
    a.close()
    b.close()


# ------------------------------------------------------------------ moments
def test_moments_of_a_million_draws(eng):
    """n = 2^20, fraction 1, one component with a full factor: the sample mean within 6 standard errors sqrt(C_rr / n) of the
    mean, every entry of the sample covariance within 6 of its own, sqrt((C_ii C_jj + C_ij^2) / n) for a Gaussian.  The seed
    is fixed: the test is deterministic."""
    n = 1 << 20
    L = np.array([[1.5, 0.0, 0.0], [-0.8, 0.9, 0.0], [0.02, -0.03, 0.05]])
    comps = np.zeros(1, eng.ReseedComponent)
    comps['mean'], comps['chol'], comps['mass'] = (20.0, -35.0, 0.3), L[np.tril_indices(3)], 1
    e = eng.Engine(n, seed=SEED)
    e.init_particles()
    assert e.inject_gaussian(1.0, comps) == n
    s = e.get_particles()[[0, 1, 5]]
    e.close()
    C = L.dot(L.T)
    mean = s.mean(axis=1)
    se_mean = np.sqrt(np.diag(C) / n)
    dev = np.abs(mean - comps['mean'][0]) / se_mean
    print('moments: mean off by', dev, 'standard errors')
    assert np.all(dev <= 6.0)
    d = s - np.asarray(comps['mean'][0])[:, None]          # about the true mean: the entries' variance is the formula's
    S = d.dot(d.T) / n
    se_cov = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C * C) / n)
    devc = np.abs(S - C) / se_cov
    print('moments: covariance off by', devc[np.tril_indices(3)], 'standard errors')
    assert np.all(devc <= 6.0)


# ------------------------------------------------------------------ the closed loops' scene: global search, kidnap
# The defaults of recovery.SensorResetting: pitch 8 m, 4 yaws; with the window of +-0.4 rad about the dead-reckoned heading the
# yaw cells are 0.2 rad wide, so a start is at most 0.1 rad off: the row "pitch 8 m, yaw offset 0.1 rad" of the basin table of
# tools/reseed_timing.py -- 89 % of the starts within one pitch of the truth end within 0.5 m of it, and about
# three lattice nodes lie that close.
PITCH, N_YAW, YAW_WINDOW, SWATH_PINGS = 8.0, 4, 0.4, 4
SELECT = dict(max_components=16, min_beams=128, max_rms=0.5, sep_xy=1.0, sep_yaw=0.1, add_std_xy=0.25, add_std_yaw=0.02,
              dead_std_xy=PITCH, dead_std_yaw=2.0 * YAW_WINDOW / N_YAW)
WIDE = 768                   # nodes per side of the kidnap runs' map: the closed loops' terrain, 16 times the area (see the test)
LOOP_SMALL_N = 4096          # the particle count of the kidnap runs (see the test)
LOOP_SEEDS = (17, 18, 19)
GUIDED_BOUND = 0.5           # m: the worst measured final error, 0.087 m, times the factor of six KIDNAP_BOUND has over its own


def wide_scene(eng, pings, size):
    """loop_scene of tests/test_gpu_recovery.py (its terrain's seed, swell and relief, its beams, its track) on a map of
    size x size nodes about the origin"""
    origin = (-0.5 * size, -0.5 * size)
    z = synth.bathymetry_grid(size, size, 1.0, origin, seed=2, swell=2.0, fbm_amp=3.0)
    ba = synth.beam_angles(64)
    st = synth.odom_stream(n_steps=pings, dt=1.0, x0=-40.0, y0=-30.0, yaw0=0.5)
    t = eng.Engine(64)
    t.set_map_grid(z, origin, 1.0)
    ranges = []
    for k in range(pings):
        t.set_particles(np.repeat(st['truth'][k][:, None], 64, axis=1))
        ranges.append(t.mbes_expected(0, 1, ba, LOOP_RMAX)[0].copy())
    t.close()
    return z, ba, st, ranges, origin


def test_global_search_from_the_lattice_finds_the_truth(eng):
    """match_swath of four noise-free pings from reseed_starts over the whole footprint (pitch, n_yaw and yaw window the
    defaults): reseed_select's first component is the truth, and no taken component has an rms above max_rms"""
    pings = 34
    z, ba, st, ranges = loop_scene(eng, pings)
    e = eng.Engine(64)
    e.set_map_grid(z, LOOP_ORIGIN, 1.0)
    ring = list(range(pings - SWATH_PINGS, pings))
    truth = st['truth'][ring[-1]]
    starts = e.reseed_starts(None, PITCH, (truth[5] - YAW_WINDOW, truth[5] + YAW_WINDOW), N_YAW, z=truth[2])
    offsets = eng.swath_offsets(np.array([st['truth'][k] for k in ring]).T, -1)
    match = e.match_swath(starts, np.stack([ranges[k] for k in ring]), ba, offsets, LOOP_SIGMA, LOOP_RMAX)
    comps, idx = eng.reseed_select(match, **SELECT)
    e.close()
    assert starts.shape[1] == 24 * 24 * N_YAW and len(comps) >= 1
    err_xy = math.hypot(comps[0]['mean'][0] - truth[0], comps[0]['mean'][1] - truth[1])
    err_yaw = abs(float(ref.wrap_yaw(comps[0]['mean'][2] - truth[5])))
    print('global search: %d starts, %d converged, %d components; the first is %.4f m, %.5f rad from the truth (rms %.4f m); rms of '
          'the taken: %s' % (starts.shape[1], int(np.sum(match.status == 0)), len(comps), err_xy, err_yaw, match.rms[idx[0]],
                             ' '.join('%.3f' % match.rms[i] for i in idx)))
    assert err_xy <= 0.5 and err_yaw <= 0.05
    assert np.all(match.rms[idx] <= SELECT['max_rms']) and np.all(match.status[idx] == 0)


def run_kidnap(eng, scene, n, seed, guided, kidnap_at=30, kidnap_shift=(40.0, -30.0)):
    """tests/test_gpu_recovery.py's run_loop with n particles and the injection either the parent's (AugmentedMCL +
    inject_uniform over the footprint) or SensorResetting's, both over the same yaw window about the dead-reckoned heading
    (the scene's odometry is exact: the truth's pose is the dead-reckoned one; the kidnap moves the cloud)"""
    from smarc_navigation_amd.recovery import AugmentedMCL, SensorResetting
    z, ba, st, ranges, origin = scene
    e = eng.Engine(n, seed=seed, **LOOP_COV)
    e.set_map_grid(z, origin, 1.0)
    rs = np.random.RandomState(1)
    s = np.zeros((6, n))
    s[0], s[1], s[5] = -40.0 + 2.0 * rs.randn(n), -30.0 + 2.0 * rs.randn(n), 0.5 + 0.1 * rs.randn(n)
    e.set_particles(s)
    aug = AugmentedMCL(0.001, 0.1, 0.1)
    sr = SensorResetting(aug, eng.make_reseed_select_config(**SELECT), PITCH, N_YAW, yaw_window=YAW_WINDOW, pings=SWATH_PINGS)
    rec = dict(err=[], frac=[], injected=[], sr=sr)
    for k in range(len(ranges)):
        if k == kidnap_at:
            s = e.get_particles()
            s[0] += kidnap_shift[0]
            s[1] += kidnap_shift[1]
            e.set_particles(s)
        e.predict(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], 1.0)
        e.update_mbes(ranges[k], ba, LOOP_SIGMA, LOOP_RMAX)
        ws = e.weight_stats()
        e.resample()
        aug.observe(ws, int(np.count_nonzero(ranges[k] > 0)))
        sr.push(ranges[k], st['truth'][k])
        frac = aug.fraction()
        rec['frac'].append(frac)
        if frac > 0.0 and guided:
            rec['injected'].append(sr.step(e, ba, LOOP_SIGMA, LOOP_RMAX))
        elif frac > 0.0:
            h = st['truth'][k][5]
            rec['injected'].append(e.inject_uniform(frac, yaw=(h - YAW_WINDOW, h + YAW_WINDOW)))
            aug.injected()
        else:
            rec['injected'].append(0)
        mean = e.mean_cov()[0]
        rec['err'].append(float(np.hypot(mean[0] - st['truth'][k][0], mean[1] - st['truth'][k][1])))
    e.close()
    return rec


def test_closed_loop_kidnap_recovery_with_a_small_cloud(eng):
    """The kidnap of tests/test_gpu_recovery.py -- the cloud moved by (40, -30) m at ping 30 of 90, 64 beams, its terrain,
    track and covariances -- with LOOP_SMALL_N = 4096 particles instead of 2^20, on three seeds, on a map of 768 x 768 nodes.
    The parent's policy -- AugmentedMCL + inject_uniform over the footprint, the yaw within +-0.4 rad of the dead-reckoned
    heading -- ends farther than half the kidnap distance from the truth on every seed: at most a tenth of the cloud per
    ping over 589 000 m^2 is one particle per 1 400 m^2.  SensorResetting (K = 4, the same yaw window, its defaults) ends
    within GUIDED_BOUND.  fraction() was 0 on every ping before the kidnap in both runs, and the guided run injected through
    at least one call that was no fallback.
    Measured on one MI355X, final errors on the seeds 17 / 18 / 19:
      768 x 768, n = 4096:   uniform 325.1 / 129.1 / 88.1 m;   guided 0.038 / 0.087 / 0.028 m (the mean pose back within 1 m six to
                             nine pings after the kidnap; 4 calls, no fallback, 16 components each, 219 - 244 particles injected)
      768 x 768, n = 16384:  uniform 137.9 / 0.046 / 0.014 m (recovers on two seeds);  n = 65536: 0.081 / 0.044 / 0.036 m
      -- so 4096 is the largest power of two at which the uniform policy fails on each of the three seeds.
      192 x 192 (the map of tests/test_gpu_recovery.py): the uniform policy recovers even with 1024 particles (0.10 / 0.09 /
      0.03 m): the yaw window and 60 pings of patience are enough on 36 864 m^2; hence the wider map.
    GUIDED_BOUND: the worst of the three guided runs, 0.087 m, times the margin KIDNAP_BOUND (0.5 m) has over its measured
    0.083 m, a factor of six: 0.52, set to 0.5 m."""
    pings, at, shift = 90, 30, (40.0, -30.0)
    scene = wide_scene(eng, pings, WIDE)
    dist = math.hypot(*shift)
    for seed in LOOP_SEEDS:
        uni = run_kidnap(eng, scene, LOOP_SMALL_N, seed, False, at, shift)
        gui = run_kidnap(eng, scene, LOOP_SMALL_N, seed, True, at, shift)
        sr = gui['sr']
        print('kidnap, n = %d, seed %d: uniform, error per ping' % (LOOP_SMALL_N, seed), ' '.join('%.2f' % v for v in uni['err']))
        print('kidnap, n = %d, seed %d: guided, error per ping' % (LOOP_SMALL_N, seed), ' '.join('%.2f' % v for v in gui['err']))
        print('kidnap, seed %d: final error uniform %.2f m, guided %.3f m (kidnap distance %.1f m); guided: %d calls, %d fallbacks, '
              '%d components, %d particles injected; uniform: %d particles in %d pings' % (
                  seed, uni['err'][-1], gui['err'][-1], dist, sr.calls, sr.fallbacks, sr.components, sr.injected,
                  sum(uni['injected']), int(np.count_nonzero(uni['injected']))))
        assert all(f == 0.0 for f in uni['frac'][:at]) and all(f == 0.0 for f in gui['frac'][:at])
        assert uni['err'][-1] > 0.5 * dist
        assert gui['err'][-1] < GUIDED_BOUND
        assert sr.calls > sr.fallbacks and sr.components > 0
