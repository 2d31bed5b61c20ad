"""GPU tests of global localisation and kidnap recovery (include/mcl_recovery.h; csrc/mcl_recovery.h): the uniform
initialisation and the injection against a numpy restatement of Philox4x32-10 and the documented word-to-double rule, the
weight statistics against math.fsum over fp64 exp, sharding / repetition bit for bit, and two closed loops on a synthetic
bathymetry -- localisation from a uniform cloud, recovery after the cloud is moved away -- each with the run that shows
that the feature, not the terrain, did it."""
import math

import numpy as np
import pytest

from smarc_navigation_amd import synth
from tests.helpers import philox4x32_10

pytestmark = pytest.mark.gpu

SEED = 0x1234567890abcdef
BOX = (-37.25, 91.5, 12.125, 140.0)      # x_min, x_max, y_min, y_max
YAW = (-2.5, 3.0)
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


# ------------------------------------------------------------------ numpy restatement of the draws
def u53(hi, lo):
    """include/mcl_recovery.h: U(hi, lo) = (((hi >> 5) << 26) | (lo >> 6)) 2^-53"""
    return (((hi >> np.uint64(5)) << np.uint64(26)) | (lo >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def native_uniforms(seed, step, purpose, gids):
    """u_x, u_y, u_yaw, u_select of the particles `gids` (purpose 5: uniform init, 6: injection)"""
    k0, k1 = seed & 0xffffffff, seed >> 32
    a = philox4x32_10(gids, 0, step, purpose, k0, k1)
    b = philox4x32_10(gids, 1, step, purpose, k0, k1)
    return np.stack([u53(a[0], a[1]), u53(a[2], a[3]), u53(b[0], b[1]), u53(b[2], b[3])])


def from_box(u, lo, hi):
    return np.minimum(lo + u * (hi - lo), hi)


def within_one_ulp(a, b):
    return np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b))))


def expect_status(eng, status, fn, *a, **kw):
    with pytest.raises(eng.MclError) as ei:
        fn(*a, **kw)
    assert ei.value.status == status, ei.value


# ------------------------------------------------------------------ uniform initialisation
@pytest.mark.parametrize('n', [65536, 1048576])
def test_uniform_init_native_equals_the_philox_restatement(eng, n):
    e = eng.Engine(n, seed=SEED)
    e.init_particles_uniform(BOX, frame='odom', yaw=YAW)
    s = e.get_particles()
    assert np.all(s[2:5] == 0.0)
    for c, (lo, hi) in ((0, BOX[0:2]), (1, BOX[2:4]), (5, YAW)):
        assert np.all((s[c] >= lo) & (s[c] <= hi))
    u = native_uniforms(SEED, 0, 5, np.arange(n))
    for c, k, (lo, hi) in ((0, 0, BOX[0:2]), (1, 1, BOX[2:4]), (5, 2, YAW)):
        assert within_one_ulp(s[c], from_box(u[k], lo, hi)), c
    # a second handle: the same bits; with the identity m2o the map frame gives them too
    e2 = eng.Engine(n, seed=SEED)
    e2.init_particles_uniform(BOX, frame='map', yaw=YAW)
    assert np.array_equal(e2.get_particles(), s)
    e.init_particles_uniform(BOX, frame='odom', yaw=YAW)
    assert np.array_equal(e.get_particles(), s)
    if n >= 1 << 20:
        # moments of n draws of U(lo, hi), w = hi - lo: mean (lo + hi) / 2 with standard error w / sqrt(12 n); the mean
        # of (x - mu)^2 is w^2 / 12 with standard error w^2 / sqrt(180 n)  (E (x - mu)^4 = w^4 / 80)
        for c, (lo, hi) in ((0, BOX[0:2]), (1, BOX[2:4]), (5, YAW)):
            w, mu = hi - lo, 0.5 * (lo + hi)
            assert abs(s[c].mean() - mu) <= 5.0 * w / math.sqrt(12.0 * n), c
            assert abs(np.mean((s[c] - mu) ** 2) - w * w / 12.0) <= 5.0 * w * w / math.sqrt(180.0 * n), c
    e.close()
    e2.close()


def test_uniform_init_replay_mode_uses_the_callers_uniforms(eng):
    n = 65536
    u = np.random.RandomState(4).rand(n, 3)
    u[0], u[1] = 0.0, 1.0 - 2.0 ** -53
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
    e.init_particles_uniform(BOX, frame='odom', yaw=YAW, uniforms=u)
    s = e.get_particles()
    for c, k, (lo, hi) in ((0, 0, BOX[0:2]), (1, 1, BOX[2:4]), (5, 2, YAW)):
        assert within_one_ulp(s[c], from_box(u[:, k], lo, hi)), c
        assert np.all((s[c] >= lo) & (s[c] <= hi))
    assert np.all(s[2:5] == 0.0)
    expect_status(eng, ERR_INVALID, e.init_particles_uniform, BOX, frame='odom', yaw=YAW)   # REPLAY without uniforms
    e.close()


def test_uniform_init_map_frame_box_and_error_cases(eng):
    n = 65536
    m2o = synth.rigid_matrix(120.5, -45.25, 3.0, 0.0, 0.0, 0.7)
    e = eng.Engine(n, seed=7, m2o=m2o)
    e.init_particles_uniform(BOX, frame='map', yaw=YAW)
    s = e.get_particles()
    assert np.all(s[2:5] == 0.0)
    p = m2o.dot(np.vstack([s[0:3], np.ones(n)]))
    assert np.all((p[0] >= BOX[0] - 1e-9) & (p[0] <= BOX[1] + 1e-9))
    assert np.all((p[1] >= BOX[2] - 1e-9) & (p[1] <= BOX[3] + 1e-9))
    yaw_map = s[5] + 0.7
    k = np.round((yaw_map - 0.5 * (YAW[0] + YAW[1])) / (2.0 * math.pi))   # the turn that brings it next to the interval
    yaw_map = yaw_map - 2.0 * math.pi * k
    assert np.all((yaw_map >= YAW[0] - 1e-9) & (yaw_map <= YAW[1] + 1e-9))
    assert np.all((s[5] >= -math.pi) & (s[5] <= math.pi))
    # the map-frame draws are those of the odom-frame call, carried over
    e.init_particles_uniform(BOX, frame='odom', yaw=YAW)
    o = e.get_particles()
    assert np.allclose(p[0], o[0], rtol=0, atol=1e-9) and np.allclose(p[1], o[1], rtol=0, atol=1e-9)
    e.close()
    tilted = eng.Engine(1024, m2o=synth.rigid_matrix(1.0, 2.0, 3.0, 0.02, 0.0, 0.7))
    expect_status(eng, ERR_UNSUPPORTED, tilted.init_particles_uniform, BOX, frame='map', yaw=YAW)
    tilted.init_particles_uniform(BOX, frame='odom', yaw=YAW)   # the state's own frame needs no m2o
    expect_status(eng, ERR_INVALID, tilted.init_particles_uniform, (1.0, 0.0, 0.0, 1.0), frame='odom')
    expect_status(eng, ERR_INVALID, tilted.init_particles_uniform, (0.0, math.inf, 0.0, 1.0), frame='odom')
    expect_status(eng, ERR_INVALID, tilted.init_particles_uniform, (0.0, 1.0, math.nan, 1.0), frame='odom')
    expect_status(eng, ERR_INVALID, tilted.init_particles_uniform, BOX, frame='odom', yaw=(-3.2, 3.2))
    expect_status(eng, ERR_INVALID, tilted.init_particles_uniform, BOX, frame=7)
    expect_status(eng, ERR_STATE, tilted.map_bounds)
    tilted.close()


@pytest.mark.parametrize('n', [65536, 1048576])
def test_uniform_init_and_injection_of_eight_shards_equal_the_unsharded_cloud(eng, n):
    W = 8
    one = eng.Engine(n, seed=SEED)
    many = [eng.Engine(n // W, rank=r, world=W, n_global=n, global_offset=r * (n // W), seed=SEED) for r in range(W)]
    one.init_particles_uniform(BOX, frame='odom', yaw=YAW)
    for s in many:
        s.init_particles_uniform(BOX, frame='odom', yaw=YAW)
    assert np.array_equal(np.concatenate([s.get_particles() for s in many], axis=1), one.get_particles())
    box2 = (0.0, 10.0, -5.0, 5.0)
    for rnd in range(2):
        k1 = one.inject_uniform(0.3, box2, frame='odom', yaw=(0.0, 1.0))
        km = [s.inject_uniform(0.3, box2, frame='odom', yaw=(0.0, 1.0)) for s in many]
        assert sum(km) == k1
        assert np.array_equal(np.concatenate([s.get_particles() for s in many], axis=1), one.get_particles())
    for s in many + [one]:
        s.close()


# ------------------------------------------------------------------ weight statistics
def ref_stats(lw):
    """the definition: math.fsum over fp64 exp"""
    lw = np.asarray(lw, np.float64)
    fin = np.isfinite(lw)
    if not fin.any():
        return dict(n_live=0, argmax=-1, max_lw=-math.inf, sum_w=0.0, sum_w2=0.0, n_eff=0.0, log_mean_lik=-math.inf)
    m = float(lw[fin].max())
    ex = np.exp(lw[fin] - m)
    s, s2 = math.fsum(ex), math.fsum(np.exp(2.0 * (lw[fin] - m)))
    return dict(n_live=int(fin.sum()), argmax=int(np.flatnonzero(fin & (lw == m))[0]), max_lw=m, sum_w=s, sum_w2=s2,
                n_eff=s * s / s2, log_mean_lik=m + math.log(s / lw.size))


def check_stats(st, lw, soa, gid0=0, rel=1e-12):
    r = ref_stats(lw)
    print('weight stats: n_eff %.6g (ref %.6g) log_mean_lik %.17g (ref %.17g) sum_w rel err %.2e sum_w2 rel err %.2e' % (
        st.n_eff, r['n_eff'], st.log_mean_lik, r['log_mean_lik'],
        abs(st.sum_w - r['sum_w']) / r['sum_w'] if r['sum_w'] else 0.0,
        abs(st.sum_w2 - r['sum_w2']) / r['sum_w2'] if r['sum_w2'] else 0.0))
    assert st.n == len(lw) and st.n_live == r['n_live']
    assert st.max_lw == r['max_lw']
    assert st.argmax_gid == (gid0 + r['argmax'] if r['argmax'] >= 0 else -1)
    if r['argmax'] >= 0:
        assert np.array_equal(st.map_pose, soa[:, r['argmax']])
    else:
        assert np.all(st.map_pose == 0.0)
    for f in ('sum_w', 'sum_w2', 'n_eff', 'log_mean_lik'):
        got, want = getattr(st, f), r[f]
        assert got == want or abs(got - want) <= rel * abs(want), (f, got, want)


def lw_case(name, n, rs):
    if name.startswith('spread'):
        return -float(name[6:]) * rs.rand(n)
    if name == 'nonfinite':
        lw = -40.0 * rs.rand(n)
        lw[rs.rand(n) < 0.2] = -np.inf
        lw[rs.rand(n) < 0.1] = np.nan
        lw[rs.randint(n)] = np.inf     # not a log-likelihood: weight 0 like the others
        return lw
    if name == 'all_ninf':
        return np.full(n, -np.inf)
    if name == 'dup_max':
        lw = -25.0 * rs.rand(n) - 1.0
        lw[[n - 1, n // 2 + 17, n // 3]] = 0.5
        return lw
    raise KeyError(name)


@pytest.mark.parametrize('n', [100003, 1048576])
@pytest.mark.parametrize('case', ['spread0', 'spread30', 'spread20000', 'nonfinite', 'all_ninf', 'dup_max'])
def test_weight_stats_of_given_log_weights(eng, case, n):
    rs = np.random.RandomState(len(case) + n % 97)
    lw = lw_case(case, n, rs)
    soa = rs.randn(6, n)
    e = eng.Engine(n, seed=3)
    e.set_particles(soa)
    expect_status(eng, ERR_STATE, e.weight_stats)           # no log-weights yet
    e.set_log_weights(lw)
    st = e.weight_stats()
    check_stats(st, lw, soa)
    again = e.weight_stats()
    assert bytes(again.as_c()) == bytes(st.as_c())          # repeat calls: bit-identical
    e.close()


def _grid_scene(eng, n, seed=5):
    origin = (-64.0, -64.0)
    z = synth.bathymetry_grid(128, 128, 1.0, origin, seed=1)
    ba = synth.beam_angles(64)
    rs = np.random.RandomState(seed)
    soa = np.zeros((6, n))
    soa[0], soa[1], soa[2] = 2.0 * rs.randn(n), 2.0 * rs.randn(n), -2.0
    soa[5] = 0.2 + 0.05 * rs.randn(n)
    t = eng.Engine(64)
    t.set_map_grid(z, origin, 1.0)
    truth = np.zeros((6, 64))
    truth[2], truth[5] = -2.0, 0.2
    t.set_particles(truth)
    ranges = t.mbes_expected(0, 1, ba, 60.0)[0]
    t.close()
    return z, origin, ba, soa, ranges


def test_weight_stats_after_a_real_mbes_update_and_resample_unchanged_by_them(eng):
    n = 1 << 18
    z, origin, ba, soa, ranges = _grid_scene(eng, n)
    cov = dict(resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4], seed=9)
    a, b = eng.Engine(n, **cov), eng.Engine(n, **cov)
    for e in (a, b):
        e.set_map_grid(z, origin, 1.0)
        e.set_particles(soa)
        e.update_mbes(ranges, ba, 0.2, 60.0)
    lw = a.get_log_weights()
    st = a.weight_stats()
    check_stats(st, lw, soa)
    assert 1.0 - 1e-12 <= st.n_eff <= n
    assert bytes(a.weight_stats().as_c()) == bytes(st.as_c())
    a.resample()
    b.resample()                                            # ... without the statistics call
    assert np.array_equal(a.last_indices(), b.last_indices())
    assert np.array_equal(a.get_particles(), b.get_particles())
    expect_status(eng, ERR_STATE, a.weight_stats)           # the weights are spent
    a.close()
    b.close()


@pytest.mark.parametrize('case', ['spread30', 'spread20000', 'nonfinite', 'dup_max'])
def test_weight_stats_of_eight_shards_merge_to_the_unsharded_call(eng, case):
    n, W = 1 << 20, 8
    rs = np.random.RandomState(21)
    lw = lw_case(case, n, rs)
    if case == 'nonfinite':
        lw[:n // W] = -np.inf         # a shard with nothing finite
    soa = rs.randn(6, n)
    one = eng.Engine(n)
    one.set_particles(soa)
    one.set_log_weights(lw)
    whole = one.weight_stats()
    parts = []
    for r in range(W):
        s = eng.Engine(n // W, rank=r, world=W, n_global=n, global_offset=r * (n // W))
        sl = slice(r * (n // W), (r + 1) * (n // W))
        s.set_particles(np.ascontiguousarray(soa[:, sl]))
        s.set_log_weights(lw[sl])
        parts.append(s.weight_stats())
        check_stats(parts[-1], lw[sl], soa[:, sl], gid0=r * (n // W))
        s.close()
    m = eng.merge_weight_stats(parts)
    assert (m.n, m.n_live, m.argmax_gid) == (whole.n, whole.n_live, whole.argmax_gid)
    assert m.max_lw == whole.max_lw and np.array_equal(m.map_pose, whole.map_pose)
    for f in ('sum_w', 'sum_w2', 'n_eff', 'log_mean_lik'):
        assert abs(getattr(m, f) - getattr(whole, f)) <= 1e-12 * abs(getattr(whole, f)), f
    check_stats(m, lw, soa)
    one.close()


# ------------------------------------------------------------------ injection
def test_injection_fraction_zero_and_one(eng):
    n = 65536
    e = eng.Engine(n, seed=SEED, init_cov=[1, 1, 0.5, 0.1, 0.1, 0.2])
    e.init_particles()
    s0 = e.get_particles()
    e.timing_enable(True)
    assert e.inject_uniform(0.0, BOX, frame='odom', yaw=YAW) == 0
    assert e.timing_get()['noise'][1] == 0                  # nothing was launched
    assert np.array_equal(e.get_particles(), s0)
    assert e.inject_uniform(1.0, BOX, frame='odom', yaw=YAW) == n
    assert e.timing_get()['noise'][1] == 1
    s1 = e.get_particles()
    assert np.array_equal(s1[2:5], s0[2:5])                 # z, roll, pitch of the slot are kept
    u = native_uniforms(SEED, 0, 6, np.arange(n))
    for c, k, (lo, hi) in ((0, 0, BOX[0:2]), (1, 1, BOX[2:4]), (5, 2, YAW)):
        assert within_one_ulp(s1[c], from_box(u[k], lo, hi)), c
        assert not np.any(s1[c] == s0[c])
    expect_status(eng, ERR_INVALID, e.inject_uniform, 1.5, BOX, frame='odom')
    expect_status(eng, ERR_INVALID, e.inject_uniform, -0.1, BOX, frame='odom')
    expect_status(eng, ERR_INVALID, e.inject_uniform, math.nan, BOX, frame='odom')
    e.set_log_weights(np.zeros(n))
    expect_status(eng, ERR_STATE, e.inject_uniform, 0.5, BOX, frame='odom')   # pending log-weights
    expect_status(eng, ERR_STATE, e.inject_uniform, 0.0, BOX, frame='odom')
    e.close()


def test_injection_of_five_per_cent_at_a_million(eng):
    n, frac = 1 << 20, 0.05
    e = eng.Engine(n, seed=SEED, init_cov=[1, 1, 0.5, 0.1, 0.1, 0.2])
    e.init_particles()
    s0 = e.get_particles()
    k = e.inject_uniform(frac, BOX, frame='odom', yaw=YAW)
    s1 = e.get_particles()
    u = native_uniforms(SEED, 0, 6, np.arange(n))
    sel = u[3] < frac
    changed = np.any(s1 != s0, axis=0)
    assert np.array_equal(changed, sel)                     # WHICH particles: exactly the restatement's
    assert k == int(changed.sum())
    assert abs(k - frac * n) <= 5.0 * math.sqrt(n * frac * (1.0 - frac))
    assert np.array_equal(s1[:, ~sel], s0[:, ~sel])         # untouched particles keep every bit
    assert np.array_equal(s1[2:5], s0[2:5])
    for c, j, (lo, hi) in ((0, 0, BOX[0:2]), (1, 1, BOX[2:4]), (5, 2, YAW)):
        assert np.all((s1[c, sel] >= lo) & (s1[c, sel] <= hi))
        assert within_one_ulp(s1[c, sel], from_box(u[j, sel], lo, hi)), c
    # the counter advances: the second injection selects another set (step 1), the init calls reset it
    k2 = e.inject_uniform(frac, BOX, frame='odom', yaw=YAW, count=False)
    assert k2 is None
    s2 = e.get_particles()
    sel2 = native_uniforms(SEED, 1, 6, np.arange(n))[3] < frac
    assert np.array_equal(np.any(s2 != s1, axis=0), sel2) and not np.array_equal(sel2, sel)
    e.init_particles()
    assert np.array_equal(e.get_particles(), s0)
    assert e.inject_uniform(frac, BOX, frame='odom', yaw=YAW) == k
    assert np.array_equal(e.get_particles(), s1)
    e.close()


def test_injection_replay_mode(eng):
    n = 65536
    rs = np.random.RandomState(8)
    u = rs.rand(n, 4)
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
    s0 = rs.randn(6, n)
    e.set_particles(s0)
    k = e.inject_uniform(0.25, BOX, frame='odom', yaw=YAW, uniforms=u)
    sel = u[:, 3] < 0.25
    s1 = e.get_particles()
    assert k == int(sel.sum()) and np.array_equal(s1[:, ~sel], s0[:, ~sel]) and np.array_equal(s1[2:5], s0[2:5])
    for c, j, (lo, hi) in ((0, 0, BOX[0:2]), (1, 1, BOX[2:4]), (5, 2, YAW)):
        assert within_one_ulp(s1[c, sel], from_box(u[sel, j], lo, hi)), c
    e.close()


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
    box = (-6.0, 6.0, -6.0, 6.0)
    assert a.inject_uniform(0.2, box, frame='map', yaw=(0.0, 0.4)) > 0
    state = a.get_particles()
    a.update_mbes(ranges, ba, 0.2, 60.0)
    b = with_map(eng.Engine(n, **cov))
    b.set_particles(state)
    b.update_mbes(ranges, ba, 0.2, 60.0)
    assert np.array_equal(a.get_log_weights(), b.get_log_weights())
    a.close()
    b.close()


@pytest.mark.parametrize('last_dt', [0.1, 0.0])
@pytest.mark.parametrize('how', ['set_particles', 'uniform'])
def test_fused_step_after_the_state_was_replaced_equals_the_separate_calls(eng, how, last_dt):
    """A fused step leaves "z, roll, pitch are the odometry's on every particle" behind.  mcl_set_particles and
    mcl_init_particles_uniform void that: the next fused step -- with a predict, and with dt = 0, where no predict runs and
    the three components are read from the state -- equals predict + update_mbes + resample on a handle that went the
    same way, bit for bit.  (It fails if z, roll, pitch are still taken from the odometry after the state was replaced.)"""
    n, origin = 3001, (-32.0, -32.0)
    z = synth.bathymetry_grid(64, 64, 1.0, origin, seed=3)
    ba = synth.beam_angles(16)
    rs = np.random.RandomState(4)
    ranges = [(18.0 + rs.rand(16)).astype(np.float32) for _ in range(2)]
    X = rs.randn(6, n) * np.array([2.0, 2.0, 0.3, 0.05, 0.05, 0.2])[:, None]
    X[2] -= 3.0   # (depth, roll and pitch that are NOT the odometry's)
    cov = dict(process_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5], resample_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5], seed=11)
    od = ([1.0, 0.1, 0.0], 0.02, synth.quat_from_rpy(0.03, -0.02, 0.3), -2.0)
    a, b = eng.Engine(n, **cov), eng.Engine(n, **cov)
    for e in (a, b):
        e.set_map_grid(z, origin, 1.0)
        e.init_particles()
        e.step_mbes(*od, 0.1, ranges[0], ba, 0.3, 60.0)
        if how == 'set_particles':
            e.set_particles(X)
        else:
            e.init_particles_uniform((-8.0, 8.0, -8.0, 8.0), frame='odom', yaw=(-0.5, 0.5))   # (z = roll = pitch = 0)
    a.step_mbes(*od, last_dt, ranges[1], ba, 0.3, 60.0)
    b.predict(*od, last_dt)
    b.update_mbes(ranges[1], ba, 0.3, 60.0)
    lw_b = b.get_log_weights()
    b.resample()
    assert np.std(lw_b) > 0.0
    assert np.array_equal(a.get_log_weights(), lw_b)
    assert np.array_equal(a.last_indices(), b.last_indices())
    assert np.array_equal(a.get_particles(), b.get_particles())
    if last_dt == 0.0 and how == 'set_particles':   # no predict ran: the resampled particles carry X's own z (plus no noise: its variance is 0)
        assert np.all(np.isin(a.get_particles()[2], X[2]))
    a.close()
    b.close()


# ------------------------------------------------------------------ closed loops
# Scene of both loops: a 192 m x 192 m synthetic bathymetry with relief (swell 2 m, fBm 3 m), 1 m nodes; a 64-beam fan of
# +-60 degrees, sigma 1.5 m (a tempered likelihood: what a global search over 36 864 m^2 x the full circle needs at
# about 28 particles per square metre); 1 048 576 particles; one ping per metre of track; seeds fixed.
LOOP_N = 1 << 20
LOOP_SIGMA, LOOP_RMAX = 1.5, 80.0
LOOP_ORIGIN = (-96.0, -96.0)
LOOP_COV = dict(process_cov=[0.01, 0.01, 0, 0, 0, 1e-4], resample_cov=[0.09, 0.09, 0, 0, 0, 2.5e-3])


def loop_scene(eng, pings, x0=-40.0, y0=-30.0, yaw0=0.5):
    z = synth.bathymetry_grid(192, 192, 1.0, LOOP_ORIGIN, seed=2, swell=2.0, fbm_amp=3.0)
    ba = synth.beam_angles(64)
    st = synth.odom_stream(n_steps=pings, dt=1.0, x0=x0, y0=y0, yaw0=yaw0)
    t = eng.Engine(64)
    t.set_map_grid(z, LOOP_ORIGIN, 1.0)
    ranges = []
    for k in range(pings):
        t.set_particles(np.repeat(st['truth'][k][:, None], 64, axis=1))
        ranges.append(t.mbes_expected(0, 1, ba, LOOP_RMAX)[0].copy())
    t.close()
    return z, ba, st, ranges


def run_loop(eng, z, ba, st, ranges, init, kidnap_at=None, kidnap_shift=None, aug=None, seed=17, **engine_kw):
    """predict -> update_mbes -> weight_stats -> resample (-> inject_uniform) per ping; returns per-ping records"""
    e = eng.Engine(LOOP_N, seed=seed, **dict(LOOP_COV, **engine_kw))
    e.set_map_grid(z, LOOP_ORIGIN, 1.0)
    init(e)
    rec = dict(err=[], frac=[], lpb=[], n_eff=[], injected=[])
    for k in range(len(ranges)):
        if kidnap_at is not None and k == kidnap_at:
            s = e.get_particles()
            s[0] += kidnap_shift[0]
            s[1] += kidnap_shift[1]
            e.set_particles(s)
        e.predict(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], 1.0)
        e.update_mbes(ranges[k], ba, LOOP_SIGMA, LOOP_RMAX)
        ws = e.weight_stats()
        nv = int(np.count_nonzero(ranges[k] > 0))
        rec['lpb'].append(ws.log_mean_lik / nv)
        rec['n_eff'].append(ws.n_eff)
        e.resample()
        frac = 0.0
        if aug is not None:
            aug.observe(ws, nv)
            frac = aug.fraction()
        rec['frac'].append(frac)
        if frac > 0.0:
            rec['injected'].append(e.inject_uniform(frac))      # over the map's footprint, the full circle
            aug.injected()
        else:
            rec['injected'].append(0)
        mean = e.mean_cov()[0]
        rec['err'].append(float(np.hypot(mean[0] - st['truth'][k][0], mean[1] - st['truth'][k][1])))
    e.close()
    return rec


GLOBAL_BOUND = 0.5   # m; measured final error 0.148 m (0.01 - 0.16 m from the fourth ping on): DESIGN.md 5d
KIDNAP_BOUND = 0.5   # m; measured final error 0.083 m: DESIGN.md 5d


def test_closed_loop_global_localisation_from_a_uniform_cloud(eng):
    """Uniform over the map's footprint, yaw over the FULL circle: after 60 pings the mean pose is within GLOBAL_BOUND of
    the truth.  The same run started the reference's way -- mcl_init_particles, sigma 1 m around the odom origin, 50 m from
    the truth's start -- ends worse than half its initial error: the uniform start did it, not the terrain.
    Measured: final error 0.148 m with the uniform start, 53.3 m with the start at the origin (49 m off)."""
    pings = 60
    z, ba, st, ranges = loop_scene(eng, pings)
    assert math.hypot(st['truth'][0][0], st['truth'][0][1]) >= 30.0
    uni = run_loop(eng, z, ba, st, ranges, lambda e: e.init_particles_uniform())
    gauss = run_loop(eng, z, ba, st, ranges, lambda e: e.init_particles(), init_cov=[1.0, 1.0, 0, 0, 0, 0.01])
    gerr = gauss['err']
    initial = math.hypot(st['truth'][0][0], st['truth'][0][1])
    print('global localisation: uniform start, error per ping', ' '.join('%.2f' % v for v in uni['err']))
    print('global localisation: final error %.3f m (n_eff at ping 0: %.1f); gaussian start at the origin: initial %.1f m, '
          'final %.2f m' % (uni['err'][-1], uni['n_eff'][0], initial, gerr[-1]))
    assert gerr[-1] > 0.5 * initial
    assert uni['err'][-1] < GLOBAL_BOUND


def test_closed_loop_kidnap_recovery_by_injection(eng):
    """A filter tracks for 30 pings; then the whole cloud is moved by (40, -30) m with set_particles.  With AugmentedMCL's
    injection over the map's footprint (full circle) the mean pose is back within KIDNAP_BOUND of the truth at the end of the
    track; the identical run without injection stays farther than half the kidnap distance.  fraction() was 0 on every
    ping before the kidnap, and the log-likelihood per beam dropped at it.  Measured: 0.083 m at the end with
    injection (80 006 particles in two pings), 64.8 m without; log-likelihood per beam -1.334 -> -3.058 at the kidnap."""
    from smarc_navigation_amd.recovery import AugmentedMCL
    pings, at, shift = 90, 30, (40.0, -30.0)
    z, ba, st, ranges = loop_scene(eng, pings)

    def tracking(e):   # a cloud of sigma 2 m, 0.1 rad around the start of the track
        rs = np.random.RandomState(1)
        s = np.zeros((6, LOOP_N))
        s[0] = -40.0 + 2.0 * rs.randn(LOOP_N)
        s[1] = -30.0 + 2.0 * rs.randn(LOOP_N)
        s[5] = 0.5 + 0.1 * rs.randn(LOOP_N)
        e.set_particles(s)
    with_inj = run_loop(eng, z, ba, st, ranges, tracking, at, shift, AugmentedMCL(0.001, 0.1, 0.1))
    without = run_loop(eng, z, ba, st, ranges, tracking, at, shift, None)
    dist = math.hypot(*shift)
    print('kidnap: with injection, error per ping', ' '.join('%.2f' % v for v in with_inj['err']))
    print('kidnap: fraction per ping', ' '.join('%.3f' % v for v in with_inj['frac']))
    print('kidnap: log-likelihood per beam', ' '.join('%.3f' % v for v in with_inj['lpb']))
    print('kidnap: error before %.3f m; final with injection %.3f m, without %.2f m (kidnap distance %.1f m); injected %d '
          'particles in %d pings' % (with_inj['err'][at - 1], with_inj['err'][-1], without['err'][-1], dist,
                                     sum(with_inj['injected']), int(np.count_nonzero(with_inj['injected']))))
    assert dist >= 30.0
    assert all(f == 0.0 for f in with_inj['frac'][:at])          # recovery does not disturb a healthy filter
    assert with_inj['lpb'][at] < min(with_inj['lpb'][:at])       # the likelihood per beam dropped at the kidnap
    assert without['err'][-1] > 0.5 * dist
    assert with_inj['err'][-1] < KIDNAP_BOUND
