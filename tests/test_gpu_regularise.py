"""GPU tests of the regularised resampling (include/mcl_regularise.h; csrc/mcl_regularise.h).

The reference is numpy alone: the header's moments, and its apply restated below from the record mcl_regularise_last
returns (shift, dmean, chol, h, a) and the caller's normals; engine.regularise_factor (the host entry of the function the
device runs, itself pinned to a numpy restatement by tests/test_regularise_host.py); oracle.native_normals for the Philox
draws (purpose 8).  Tolerances: the moments within 1e-12 x the largest magnitudes involved; the factor bit for bit (the
device's fp64 sqrt and / are correctly rounded: measured equal on an MI355X); x, y and the drift words within
2 ulp (np.spacing) of the expected value and a yaw within 4 ulp of pi as a circular difference (the kernel rounds every
product and sum separately, as numpy does); everything that must not move (z, roll, pitch, the log-weights, the slot map,
the genealogy, a dead dimension) bit for bit."""
import ctypes
import math

import numpy as np
import pytest

from smarc_navigation_amd import synth

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
ZERO3 = [0.0, 0.0, 0.0]
SIZES = [1, 2, 63, 65, 257, 2049]
BIG = 524288 + 257          # 256 x 2048 lanes, then a second trip of the grid-stride loop
DIM_NAMES = ('x', 'y', 'yaw', 'cx', 'cy', 'bw')


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def within_ulp(got, want, k):
    return np.all(np.abs(got - want) <= k * np.spacing(np.abs(want)))


def status_of(eng, call):
    with pytest.raises(eng.MclError) as ei:
        call()
    return ei.value.status


# ------------------------------------------------------------------ the definition, restated
def centre(v, s, r):
    """e of dimension r: the difference to the shift, the yaw's (r = 2) taken into [-pi, pi)"""
    t = v - s
    if r != 2:
        return t
    return np.where((t >= -np.pi) & (t < np.pi), t, synth.wrap_pi(t))


def moments_ref(v):
    """v (D, n) -> shift, e, mean about the shift, covariance (two-pass, fp64)"""
    s = v[:, 0].copy()
    e = np.array([centre(v[r], s[r], r) for r in range(v.shape[0])])
    m = e.mean(axis=1)
    d = e - m[:, None]
    return s, e, m, d @ d.T / v.shape[1]


def apply_ref(v, res, xi, shrink):
    """the header's apply: v (D, n) current values, res = regularise_last(), xi (n, D) -> the new (D, n)"""
    L, m, s, h, a = res['chol'], res['dmean'], res['shift'], res['h'], res['a']
    out = v.copy()
    for r in range(v.shape[0]):
        if not np.any(L[r, :r + 1]):
            continue
        z = L[r, 0] * xi[:, 0]
        for c in range(1, r + 1):
            z = z + L[r, c] * xi[:, c]
        t5 = h * z
        if shrink:
            t1 = centre(v[r], s[r], r) - m[r]
            t2 = a * t1
            t3 = m[r] + t2
            t4 = s[r] + t3
            new = t4 + t5
        else:
            new = v[r] + t5
        if r == 2:
            new = np.where((new >= -np.pi) & (new < np.pi), new, synth.wrap_pi(new))
        out[r] = new
    return out


def make_cloud(n, rs):
    """a pose cloud with correlated x / y, yaws within 1e-3 of +-pi on both sides, and a drift"""
    soa = rs.randn(6, n) * np.array([[50.0], [50.0], [5.0], [0.1], [0.1], [1.0]])
    soa[1] += 0.6 * soa[0]
    soa[5] = (np.pi - 1e-3 * rs.rand(n)) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    d = np.array([[0.15], [-0.10], [2e-3]]) + rs.randn(3, n) * np.array([[0.2], [0.05], [1e-3]])
    d[0] += 1e-3 * soa[0]                                  # the current correlates with the position
    return soa, d


def stacked(soa, d, dims):
    v = np.array([soa[0], soa[1], soa[5]])
    return v if dims == 3 else np.concatenate([v, d])


def check_record(eng, res, v):
    """moments against numpy, the factor against the host entry point"""
    D, n = v.shape
    s, e, m, cov = moments_ref(v)
    big = np.maximum(np.abs(v).max(axis=1), np.abs(e).max(axis=1))
    assert res['n'] == n and res['dims'] == D
    assert np.array_equal(bits(res['shift']), bits(s))
    assert np.all(np.abs((res['dmean'] + res['shift']) - (s + m)) <= 1e-12 * big), (res['dmean'], m)
    assert np.all(np.abs(res['cov'] - cov) <= 1e-12 * np.outer(big, big)), (res['cov'], cov)
    L, dead = eng.regularise_factor(res['cov'])
    assert res['dead'] == dead
    assert np.all(np.abs(res['chol'] - L) <= 1e-12 * np.abs(L).max())
    assert np.array_equal(bits(res['chol']), bits(L)), np.abs(res['chol'] - L).max()
    return e


def check_apply(got, want):
    """got, want: (D, n) stacked states"""
    for r in range(want.shape[0]):
        if r == 2:
            circ = np.abs(synth.wrap_pi(got[r] - want[r]))
            assert np.all(circ <= 4 * np.spacing(np.pi)), circ.max()
            assert np.all(got[r] >= -np.pi) and np.all(got[r] < np.pi)
        else:
            assert within_ulp(got[r], want[r], 2), (DIM_NAMES[r], np.abs(got[r] - want[r]).max())


# ------------------------------------------------------------------ moments, factor, apply: REPLAY
def run_replay_case(eng, n, dims, shrink):
    rs = np.random.RandomState(1000 * dims + 10 * n % 9973 + int(shrink))
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY, seed=5)
    soa0, d = make_cloud(n, rs)
    e.set_particles(soa0)
    # a resample first, so that there is a slot map to keep: mild weights, most particles survive
    e.set_log_weights(0.1 * rs.randn(n))
    need = e.resample_prepare()
    e.resample(rs.rand(need), rs.randn(n, 6))                      # (resample_cov is zero: the normals add nothing)
    soa = e.get_particles()
    idx = e.last_indices()
    e.drift_enable(ZERO3, ZERO3)
    e.drift_set(d)
    lw = rs.randn(n)
    e.set_log_weights(lw)                                          # pending weights: ignored, and kept
    xi = rs.randn(n, dims)
    e.regularise(scale=1.0, shrink=shrink, with_drift=dims == 6, normals=xi)
    res = e.regularise_last()
    got_soa, got_d = e.get_particles(), e.drift_get()
    v = stacked(soa, d, dims)
    check_record(eng, res, v)
    h, a = eng.regularise_bandwidth(n, dims, 1.0, shrink)
    assert (res['h'], res['a']) == (h, a)
    want = apply_ref(v, res, xi, shrink)
    check_apply(stacked(got_soa, got_d, dims), want)
    # what is never written
    assert np.array_equal(bits(got_soa[2:5]), bits(soa[2:5]))      # z, roll, pitch
    assert np.array_equal(bits(e.get_log_weights()), bits(lw))
    assert np.array_equal(e.last_indices(), idx)
    if dims == 3:
        assert np.array_equal(bits(got_d), bits(d))
    # a second look at the record: the same bits (nothing was recomputed)
    res2 = e.regularise_last()
    assert all(np.array_equal(bits(res[k]), bits(res2[k])) for k in ('shift', 'dmean', 'cov', 'chol'))
    e.close()
    return res, v, want


@pytest.mark.parametrize('shrink', [False, True])
@pytest.mark.parametrize('dims', [3, 6])
@pytest.mark.parametrize('n', SIZES)
def test_replay_is_the_numpy_statement(n, dims, shrink, eng):
    res, v, want = run_replay_case(eng, n, dims, shrink)
    if n == 1:
        assert res['dead'] == (1 << dims) - 1 and np.array_equal(bits(want), bits(v))     # one particle: nothing moves
    if n >= 63:
        assert res['dead'] == 0
        moved = want != v
        assert np.all(moved.mean(axis=1) > 0.9)
        # the yaws sit at both ends of [-pi, pi): the wrap in e and in the store were both taken
        assert np.any(v[2] > 3.0) and np.any(v[2] < -3.0) and abs(res['dmean'][2]) < 2e-3
        assert np.any(np.abs(want[2] - v[2]) > 6.0)


def test_replay_where_the_grid_stride_loop_takes_a_second_trip(eng):
    res, v, want = run_replay_case(eng, BIG, 6, True)
    assert res['dead'] == 0 and res['n'] == BIG
    assert np.all((want != v)[:, 524288:].mean(axis=1) > 0.9)      # the slots of the second trip moved too


def test_two_calls_on_the_same_state_agree_bit_for_bit(eng):
    n = 2049
    rs = np.random.RandomState(9)
    soa, d = make_cloud(n, rs)
    recs = []
    for _ in range(2):
        e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
        e.set_particles(soa)
        e.regularise(normals=np.zeros((n, 3)))                     # zero normals, no shrink needed: h z = 0
        recs.append(e.regularise_last())
        e.close()
    for k in ('shift', 'dmean', 'cov', 'chol'):
        assert np.array_equal(bits(recs[0][k]), bits(recs[1][k])), k


# ------------------------------------------------------------------ degenerate clouds
@pytest.mark.parametrize('shrink', [False, True])
def test_all_particles_at_one_pose_move_nothing(shrink, eng):
    n = 257
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
    soa = np.repeat(np.array([[12.5], [-7.25], [-3.0], [0.01], [0.02], [3.1]]), n, axis=1)
    e.set_particles(soa)
    e.drift_enable(ZERO3, ZERO3)
    d = np.repeat(np.array([[0.1], [-0.2], [1e-3]]), n, axis=1)
    e.drift_set(d)
    e.regularise(shrink=shrink, with_drift=True, normals=np.random.RandomState(1).randn(n, 6))
    res = e.regularise_last()
    assert res['dead'] == 63 and not np.any(res['chol']) and not np.any(res['cov']) and not np.any(res['dmean'])
    assert np.array_equal(bits(e.get_particles()), bits(soa)) and np.array_equal(bits(e.drift_get()), bits(d))
    e.close()


@pytest.mark.parametrize('shrink', [False, True])
def test_a_constant_yaw_keeps_every_yaw_bit_while_x_and_y_move(shrink, eng):
    n = 257
    rs = np.random.RandomState(2)
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
    soa, _ = make_cloud(n, rs)
    soa[5] = 3.1415926                                             # (its store would go through the wrap)
    e.set_particles(soa)
    xi = rs.randn(n, 3)
    e.regularise(shrink=shrink, normals=xi)
    res = e.regularise_last()
    got = e.get_particles()
    assert res['dead'] == 4 and not np.any(res['chol'][2]) and not np.any(res['cov'][2])
    assert np.array_equal(bits(got[5]), bits(soa[5]))
    assert np.all(got[0] != soa[0]) and np.all(got[1] != soa[1])
    check_apply(stacked(got, None, 3), apply_ref(stacked(soa, None, 3), res, xi, shrink))
    e.close()


# ------------------------------------------------------------------ native draws
COV = dict(init_cov=[4.0, 4.0, 0.0, 0.0, 0.0, 0.01], process_cov=[1e-4, 1e-4, 0.0, 0.0, 0.0, 1e-6], resample_cov=[0.0] * 6)


@pytest.mark.parametrize('dims', [3, 6])
@pytest.mark.parametrize('n', [63, 2049])
def test_native_draws_are_purpose_8_of_the_oracle_and_two_handles_agree(n, dims, eng, orc):
    """The expected state is the numpy apply over the oracle's normals.  The device's normals are within 2 ulp of the
    oracle's (the bound tests/test_gpu_drift.py holds the same generator to), so a value may differ from the expected one
    by 2 ulp of its own plus h sum_c |L_rc| 2 ulp(|xi_c|)."""
    seed = 0xBEE5 + n

    def make():
        e = eng.Engine(n, seed=seed, **COV)
        e.init_particles()
        e.drift_enable([0.2, 0.1, 1e-3], ZERO3)
        return e

    a, b = make(), make()
    for step in (0, 1):
        soa, d = a.get_particles(), a.drift_get()
        for e in (a, b):
            e.regularise(scale=1.0, shrink=bool(step), with_drift=dims == 6)
        res = a.regularise_last()
        v = stacked(soa, d, dims)
        check_record(eng, res, v)
        xi = orc.native_normals(n, 0, seed, 8, step)[:, :dims]
        want = apply_ref(v, res, xi, bool(step))
        got = stacked(a.get_particles(), a.drift_get(), dims)
        L = np.abs(res['chol'])
        for r in range(dims):
            slack = 2 * np.spacing(np.abs(want[r])) + res['h'] * (2 * np.spacing(np.abs(xi)) * L[r][None, :dims]).sum(axis=1)
            diff = np.abs(synth.wrap_pi(got[r] - want[r])) if r == 2 else np.abs(got[r] - want[r])
            assert np.all(diff <= slack + (4 * np.spacing(np.pi) if r == 2 else 0.0)), (step, DIM_NAMES[r], (diff - slack).max())
        assert np.all(got != v)                                     # ... and every word did move
        assert np.array_equal(bits(a.get_particles()), bits(b.get_particles())), step
        assert np.array_equal(bits(a.drift_get()), bits(b.drift_get())), step
        if dims == 3:
            assert np.array_equal(bits(a.drift_get()), bits(d))
    a.close()
    b.close()


# ------------------------------------------------------------------ statistics
def test_shrink_keeps_the_linear_gaussian_posterior_and_makes_every_particle_distinct(eng):
    """prior N(0, 4 m^2) in x and y, one fix with a std of 1 m: the posterior variance is 1 / (1 / 4 + 1) = 0.8 m^2"""
    n = 65536
    e = eng.Engine(n, seed=11, meas_std=1.0, **COV)
    e.init_particles()
    e.update_gps(0.5, -0.3)
    n_eff = e.weight_stats().n_eff
    assert 0.3 * n < n_eff < n
    e.resample()
    before = e.get_particles()
    assert len(np.unique(before[0])) < n                           # the resample left copies
    e.regularise(shrink=True)
    after = e.get_particles()
    se = 0.8 * math.sqrt(2.0 / n_eff)
    for c in (0, 1):
        var = float(np.var(after[c]))
        print('posterior variance of %s: %.4f (0.8 +- %.4f at 6 standard errors; n_eff %.0f)' % ('xy'[c], var, 6 * se, n_eff))
        assert abs(var - 0.8) <= 6 * se, (c, var, se)
    assert len(np.unique(after[0])) == n
    e.close()


def test_without_shrink_the_covariance_grows_by_one_plus_h_squared(eng):
    n = 65536
    e = eng.Engine(n, seed=12, **COV)
    e.init_particles()                                             # an equal-weight cloud
    before = e.get_particles()
    e.regularise(shrink=False)
    h = e.regularise_last()['h']
    assert h == eng.regularise_bandwidth(n, 3, 1.0, False)[0]
    after = e.get_particles()
    for c in (0, 1, 5):
        ratio = float(np.var(after[c]) / np.var(before[c]))
        print('variance ratio of %s: %.5f (1 + h^2 = %.5f)' % (DIM_NAMES[min(c, 2)], ratio, 1 + h * h))
        assert abs(ratio - (1.0 + h * h)) <= 6 * math.sqrt(2.0 / n), (c, ratio, h)
    e.close()


# ------------------------------------------------------------------ the sweep does not care
def test_the_sweep_gives_the_bits_of_a_fresh_handle_with_the_same_poses(eng):
    n = 2049
    origin = (-32.0, -32.0)
    grid = synth.bathymetry_grid(64, 64, 1.0, origin, seed=1)
    cov = dict(init_cov=[1.0, 1.0, 0.0, 0.0, 0.0, 0.01], process_cov=[1e-4, 1e-4, 0.0, 0.0, 0.0, 1e-6],
               resample_cov=[1e-3, 1e-3, 0.0, 0.0, 0.0, 1e-5])
    ba = synth.beam_angles(16, half_swath=math.pi / 6)             # (a fan of +-10 m at 18 m: inside the map)
    ranges = (18.0 / np.cos(ba)).astype(np.float32)
    st = synth.odom_stream(2)
    e = eng.Engine(n, seed=21, **cov)
    e.set_map_grid(grid, origin, 1.0)
    e.init_particles()
    e.predict(st['v'][0], st['wz'][0], st['q'][0], st['z'][0], st['dt'])
    e.update_mbes(ranges, ba, 0.5, 60.0)
    e.resample()                                                   # (leaves a visiting order for the next sweep)
    e.predict(st['v'][1], st['wz'][1], st['q'][1], st['z'][1], st['dt'])
    e.set_log_weights(np.random.RandomState(3).randn(n))
    e.resample()
    e.regularise(shrink=True)
    poses = e.get_particles()
    e.update_mbes(ranges, ba, 0.5, 60.0)
    lw = e.get_log_weights()
    f = eng.Engine(n, seed=22, **cov)
    f.set_map_grid(grid, origin, 1.0)
    f.set_particles(poses)
    f.update_mbes(ranges, ba, 0.5, 60.0)
    assert np.all(np.isfinite(lw)) and len(np.unique(lw)) > n // 2
    assert np.array_equal(bits(lw), bits(f.get_log_weights()))
    e.close()
    f.close()


# ------------------------------------------------------------------ status codes
def test_status_codes(eng):
    from smarc_navigation_amd import _lib
    n = 64
    e = eng.Engine(n, **COV)
    e.init_particles()
    assert status_of(eng, e.regularise_last) == ERR_STATE                           # before any call
    assert status_of(eng, lambda: e.regularise(with_drift=True)) == ERR_STATE       # six dimensions need the drift
    assert status_of(eng, e.regularise_last) == ERR_STATE                           # ... and a refused call is no call
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert status_of(eng, lambda: e.regularise(scale=bad)) == ERR_INVALID
    lib = _lib.load()
    for dims in (0, 2, 4, 7):
        cfg = eng.make_regularise_config(1.0, True, dims)
        assert lib.mcl_regularise(e.h, ctypes.byref(cfg), None) == ERR_INVALID
    assert lib.mcl_regularise(e.h, None, None) == ERR_INVALID
    before = e.get_particles()
    e.regularise()
    assert lib.mcl_regularise_last(e.h, None) == ERR_INVALID
    assert e.regularise_last()['dims'] == 3 and not np.array_equal(e.get_particles(), before)
    e.drift_enable([0.1, 0.1, 1e-3], ZERO3)
    e.regularise(with_drift=True)
    assert e.regularise_last()['dims'] == 6
    e.close()
    r = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
    r.set_particles(before)
    assert status_of(eng, lambda: r.regularise(normals=None)) == ERR_INVALID        # REPLAY needs its normals
    assert np.array_equal(bits(r.get_particles()), bits(before))
    r.close()


def test_shards_are_refused(eng):
    from smarc_navigation_amd import _lib
    shard = eng.Engine(256, rank=1, world=2, n_global=512, global_offset=256)
    assert status_of(eng, shard.regularise) == ERR_UNSUPPORTED
    assert status_of(eng, shard.regularise_last) == ERR_STATE
    shard.close()
    # a handle created for a LOCAL group (comm_mode = MCL_COMM_LOCAL, world 2), through the C ABI
    lib = _lib.load()
    cfg = _lib.Config()
    cfg.n_particles, cfg.n_global, cfg.global_offset = 256, 512, 0
    cfg.device, cfg.rank, cfg.world, cfg.comm_mode = 0, 0, 2, 2
    cfg.m2o[:] = [float(v) for v in np.identity(4).reshape(-1)]
    h = ctypes.c_void_p()
    assert lib.mcl_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    rc = eng.make_regularise_config(1.0, True, 3)
    assert lib.mcl_regularise(h, ctypes.byref(rc), None) == ERR_UNSUPPORTED
    lib.mcl_destroy(h)


# ------------------------------------------------------------------ beside the genealogy
def test_the_genealogy_is_what_it_was(eng):
    n = 1000
    rs = np.random.RandomState(4)
    e = eng.Engine(n, seed=8, **COV)
    e.init_particles()
    e.history_enable(2)
    for k in range(2):
        e.history_record(float(k))
        e.set_log_weights(2.0 * rs.randn(n))
        e.resample()
        anc, idx = e.history_ancestors(0), e.last_indices()
        assert np.count_nonzero(anc != np.arange(n)) > 0
        e.regularise(shrink=bool(k))
        assert np.array_equal(e.history_ancestors(0), anc) and np.array_equal(e.last_indices(), idx)
    e.close()


# ------------------------------------------------------------------ additivity
# launches per timing region of ten predict / update_gps / resample cycles on a handle that never calls regularise,
# counted on the commit before this feature (one MI355X, the cycle of tests/test_gpu_drift.py's "off is off")
CYCLES = 10
PARENT_LAUNCHES = dict(predict=10, update_gps=10, update_mbes=0, normalise=10, scan=10, resample=10, mean_cov=0, noise=0,
                       comm=0, mbes_main=0, comm_records=0, pack=0, comm_p2p=0, comm_moments=0, update_landmarks=0)


def test_a_handle_that_never_regularises_queues_what_it_always_queued(eng):
    n = 1000
    st = synth.odom_stream(CYCLES)
    idx, fixes = synth.gps_fixes(st['truth'], np.identity(4), every=1, sigma=0.5)
    cov = dict(init_cov=[1.0, 1.0, 0.0, 0.0, 0.0, 0.01], process_cov=[1e-4, 1e-4, 0.0, 0.0, 0.0, 1e-6],
               resample_cov=[1e-3, 1e-3, 0.0, 0.0, 0.0, 1e-5])
    plain, reg = (eng.Engine(n, seed=17, meas_std=0.5, **cov) for _ in range(2))
    for e in (plain, reg):
        e.init_particles()
        e.timing_enable(True)
        e.timing_get()
    for k in range(CYCLES):
        for e in (plain, reg):
            e.predict(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], st['dt'])
            e.update_gps(fixes[k][0], fixes[k][1])
            e.resample()
        reg.regularise()
    launches = {k: v[1] for k, v in plain.timing_get().items()}
    print('launches of a handle that never regularises:', launches)
    assert launches == PARENT_LAUNCHES
    # one that does: one more region per call under the moments' key and one under the noise's, nothing else
    assert {k: v[1] for k, v in reg.timing_get().items()} == dict(launches, mean_cov=launches['mean_cov'] + CYCLES,
                                                                 noise=launches['noise'] + CYCLES)
    plain.close()
    reg.close()
