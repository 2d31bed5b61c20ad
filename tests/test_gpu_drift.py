"""GPU tests of the per-particle drift states (include/mcl_drift.h; csrc/mcl_drift.h).

The reference is numpy alone: the header's three steps restated below, oracle.native_normals for the Philox draws
(purpose 7), resampling.slot_ancestors(engine.last_indices()) for the slot map of every resample, and numpy's fp64 mean
and covariance.  Tolerances: a position or a drift word within 2 ulp (np.spacing) of the expected value (the kernel rounds
the product and the sum separately, as numpy does, so that the bound also holds where the sum cancels: a fused
multiply-add misses it there); a yaw within 4 ulp of pi as a circular difference; the moments within
1e-12 x the largest magnitudes involved; everything that is a copy (the gather, z / roll / pitch, a particle with zero
drift, dt <= 0, "nothing else moves") bit for bit."""
import math

import numpy as np
import pytest

from smarc_navigation_amd import resampling, synth

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
COV = dict(init_cov=[1.0, 1.0, 0.0, 0.0, 0.0, 0.01], process_cov=[1e-4, 1e-4, 0.0, 0.0, 0.0, 1e-6],
           resample_cov=[1e-3, 1e-3, 0.0, 0.0, 0.0, 1e-5])
ZERO3 = [0.0, 0.0, 0.0]


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
def advance_ref(soa, d, dt, walk_std, xi):
    """steps 1 - 3 of include/mcl_drift.h: soa (6, n), d (3, n), xi (n, 3) -> the new (soa, d)"""
    soa, new_d = soa.copy(), d.copy()
    soa[0] = soa[0] + d[0] * dt
    soa[1] = soa[1] + d[1] * dt
    t = soa[5] + d[2] * dt
    inside = (t >= -np.pi) & (t < np.pi)
    soa[5] = np.where(inside, t, synth.wrap_pi(t))
    for c in range(3):
        new_d[c] = d[c] + (walk_std[c] * np.sqrt(dt)) * xi[:, c]
    return soa, new_d, inside


# ------------------------------------------------------------------ 1: the advance, REPLAY mode
@pytest.mark.parametrize('n', [1, 63, 65, 257, 1025])
def test_advance_is_the_numpy_statement(n, eng):
    rs = np.random.RandomState(100 + n)
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY, seed=3)
    soa = rs.randn(6, n) * np.array([[50.0], [50.0], [5.0], [0.1], [0.1], [1.0]])
    # yaws within 1e-3 of +-pi, so that bw dt (up to 5e-3) carries them across both ways -- and some stay inside
    near = (np.pi - 1e-3 * rs.rand(n)) * np.where(rs.rand(n) < 0.5, 1.0, -1.0)
    soa[5] = np.where(np.arange(n) % 4 == 3, soa[5].clip(-3.0, 3.0), near)
    e.set_particles(soa)
    walk = [0.005, 0.004, 1e-4]
    e.drift_enable(ZERO3, walk)                       # (a zero prior needs no normals)
    assert not np.any(e.drift_get())
    d = rs.randn(3, n) * np.array([[0.2], [0.2], [0.1]])
    d[:, ::5] = 0.0                                   # particles with zero drift
    e.drift_set(d)
    assert np.array_equal(bits(e.drift_get()), bits(d))
    dt = 0.05
    xi = rs.randn(n, 3)
    e.drift_advance(dt, xi)
    got, got_d = e.get_particles(), e.drift_get()
    want, want_d, inside = advance_ref(soa, d, dt, walk, xi)
    if n > 16:
        assert np.any(want[5][~inside] < 0) and np.any(want[5][~inside] > 0) and np.any(inside)   # wrapped both ways
    assert within_ulp(got[0], want[0], 2) and within_ulp(got[1], want[1], 2)
    assert within_ulp(got_d, want_d, 2)
    circ = np.abs(synth.wrap_pi(got[5] - want[5]))
    assert np.all(circ <= 4 * np.spacing(np.pi)), circ.max()
    assert np.all(got[5] >= -np.pi) and np.all(got[5] < np.pi)
    assert np.array_equal(bits(got[2:5]), bits(soa[2:5]))                  # z, roll, pitch: not touched
    zero = np.arange(n) % 5 == 0
    assert np.array_equal(bits(got[:, zero]), bits(soa[:, zero]))          # zero drift: every bit of the pose stays
    # dt = 0 and dt < 0: nothing moves (the normals are not even needed)
    for bad_dt in (0.0, -0.0, -0.02):
        e.drift_advance(bad_dt, None)
    assert np.array_equal(bits(e.get_particles()), bits(got)) and np.array_equal(bits(e.drift_get()), bits(got_d))
    assert status_of(eng, lambda: e.drift_advance(float('nan'), xi)) == ERR_INVALID
    assert status_of(eng, lambda: e.drift_advance(float('inf'), xi)) == ERR_INVALID
    assert status_of(eng, lambda: e.drift_advance(dt, None)) == ERR_INVALID      # a walk needs its normals
    assert np.array_equal(bits(e.get_particles()), bits(got)) and np.array_equal(bits(e.drift_get()), bits(got_d))
    e.close()


def test_replay_prior_is_std_times_the_normals_and_needs_them(eng):
    n = 257
    rs = np.random.RandomState(5)
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
    init = [0.2, 0.3, 0.0]
    assert status_of(eng, lambda: e.drift_enable(init, ZERO3, None)) == ERR_INVALID
    assert status_of(eng, e.drift_get) == ERR_STATE                                # ... and the drift stays off
    xi = rs.randn(n, 3)
    e.drift_enable(init, ZERO3, xi)
    d = e.drift_get()
    assert np.array_equal(d[0], 0.2 * xi[:, 0]) and np.array_equal(d[1], 0.3 * xi[:, 1]) and not np.any(d[2])
    e.drift_advance(0.02, None)                                                    # a zero walk needs no normals
    assert np.array_equal(bits(e.drift_get()), bits(d))
    xi2 = rs.randn(n, 3)
    e.drift_reset(xi2)
    assert np.array_equal(e.drift_get()[0], 0.2 * xi2[:, 0])
    e.close()


# ------------------------------------------------------------------ 2: native draws
@pytest.mark.parametrize('n', [63, 1000, 4097])
def test_native_draws_are_purpose_7_of_the_oracle(n, eng, orc):
    seed = 0xD21F7 + n
    init, walk, dt = np.array([0.2, 0.3, 0.01]), np.array([0.005, 0.004, 1e-4]), 0.02

    def make():
        e = eng.Engine(n, seed=seed, **COV)
        e.init_particles()
        e.drift_enable(init, walk)
        return e

    a, b = make(), make()
    d0 = a.drift_get()
    assert within_ulp(d0, (orc.native_normals(n, 0, seed, 7, 0)[:, :3] * init).T, 2)
    assert np.array_equal(bits(d0), bits(b.drift_get()))
    hist = [d0]
    for step in (1, 2):
        a.drift_advance(dt)
        b.drift_advance(dt)
        if step == 1:
            for nothing in (0.0, -1.0):                   # dt <= 0 is no advance: the next one is still step 2
                a.drift_advance(nothing)
        d = a.drift_get()
        xi = orc.native_normals(n, 0, seed, 7, step)[:, :3]
        assert within_ulp(d, hist[-1] + ((walk * np.sqrt(dt)) * xi).T, 2), step
        assert np.array_equal(bits(d), bits(b.drift_get())), step
        hist.append(d)
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    # reset: the prior's bits again, and the count starts again
    a.drift_reset()
    assert np.array_equal(bits(a.drift_get()), bits(d0))
    a.drift_advance(dt)
    assert np.array_equal(bits(a.drift_get()), bits(hist[1]))
    a.close()
    b.close()


@pytest.mark.parametrize('on', [(1, 0, 0), (0, 1, 0), (0, 0, 1)])
def test_a_component_with_zero_stds_stays_exactly_zero(on, eng, orc):
    n, seed, dt = 1000, 99, 0.02
    on = np.array(on, dtype=np.float64)
    init, walk = 0.2 * on, 0.005 * on
    e = eng.Engine(n, seed=seed, **COV)
    e.init_particles()
    e.drift_enable(init, walk)
    c = int(np.argmax(on))
    want = init[c] * orc.native_normals(n, 0, seed, 7, 0)[:, c]
    for step in range(4):
        d = e.drift_get()
        for o in range(3):
            if o != c:
                assert np.array_equal(bits(d[o]), bits(np.zeros(n))), (step, o)       # +0.0, every bit
        assert within_ulp(d[c], want, 2) and np.count_nonzero(d[c]) == n
        e.drift_advance(dt)
        want = d[c] + (walk[c] * np.sqrt(dt)) * orc.native_normals(n, 0, seed, 7, step + 1)[:, c]
    e.close()


# ------------------------------------------------------------------ 3, 6: nothing else moves; off is off
def test_zero_drift_changes_no_bit_of_the_filter_and_off_is_off(eng):
    n, steps = 1000, 20
    st = synth.odom_stream(steps)
    idx, fixes = synth.gps_fixes(st['truth'], np.identity(4), every=1, sigma=0.5)

    def make():
        e = eng.Engine(n, seed=17, meas_std=0.5, **COV)
        e.init_particles()
        return e

    plain, zero, onoff = make(), make(), make()
    zero.drift_enable(ZERO3, ZERO3)
    onoff.drift_enable([0.2, 0.2, 0.01], [0.005, 0.005, 1e-4])
    onoff.drift_mean_cov()
    onoff.drift_disable()                                 # (the prior draw and the query touched no pose)
    for e in (plain, onoff, zero):
        e.timing_enable(True)
        e.timing_get()
    for k in range(steps):
        zero.drift_advance(st['dt'])
        for e in (plain, zero, onoff):
            e.predict(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], st['dt'])
            e.update_gps(fixes[k][0], fixes[k][1])
            e.resample()
        want, want_idx = plain.get_particles(), plain.last_indices()
        for e in (zero, onoff):
            assert np.array_equal(bits(e.get_particles()), bits(want)), k
            assert np.array_equal(e.last_indices(), want_idx), k
    assert not np.any(zero.drift_get())
    t_plain, t_zero, t_onoff = (e.timing_get() for e in (plain, zero, onoff))
    launches = {k: v[1] for k, v in t_plain.items()}
    # enabled and disabled again: a never-enabled handle's launches
    assert {k: v[1] for k, v in t_onoff.items()} == launches
    # enabled: one more region per advance (under the predict's) and per resample (under the resample's), nothing else
    assert {k: v[1] for k, v in t_zero.items()} == dict(launches, predict=launches['predict'] + steps,
                                                        resample=launches['resample'] + steps)
    for e in (plain, zero, onoff):
        e.close()


def test_every_call_on_a_disabled_handle_is_a_state_error(eng):
    n = 64
    e = eng.Engine(n, **COV)
    e.init_particles()
    calls = (e.drift_reset, e.drift_disable, lambda: e.drift_advance(0.02), lambda: e.drift_advance(0.0), e.drift_get,
             lambda: e.drift_set(np.zeros((3, n))), e.drift_mean_cov)
    for call in calls:
        assert status_of(eng, call) == ERR_STATE
    assert e.drift_bytes() == 24 * n + 147552             # (needs no enabled drift)
    for bad in ([-0.1, 0.0, 0.0], [0.0, float('nan'), 0.0], [0.0, 0.0, float('inf')]):
        assert status_of(eng, lambda: e.drift_enable(bad, ZERO3)) == ERR_INVALID
        assert status_of(eng, lambda: e.drift_enable(ZERO3, bad)) == ERR_INVALID
    assert status_of(eng, e.drift_get) == ERR_STATE
    e.drift_enable([0.1, 0.1, 0.0], ZERO3)
    assert status_of(eng, lambda: e.drift_enable([0.1, 0.1, 0.0], ZERO3)) == ERR_STATE     # a second enable
    assert np.count_nonzero(e.drift_get()[:2]) == 2 * n                                    # ... which changed nothing
    e.drift_disable()
    for call in calls:
        assert status_of(eng, call) == ERR_STATE
    e.drift_enable(ZERO3, ZERO3)                          # disable, then enable: fine
    e.close()


def test_shards_are_refused(eng):
    import ctypes
    from smarc_navigation_amd import _lib
    shard = eng.Engine(256, rank=1, world=2, n_global=512, global_offset=256)
    assert status_of(eng, lambda: shard.drift_enable(ZERO3, ZERO3)) == ERR_UNSUPPORTED
    assert status_of(eng, shard.drift_get) == ERR_STATE
    shard.close()
    # a handle created for a LOCAL group (comm_mode = MCL_COMM_LOCAL, world 2), through the C ABI
    lib = _lib.load()
    cfg = _lib.Config()
    cfg.n_particles, cfg.n_global, cfg.global_offset = 256, 512, 0
    cfg.device, cfg.rank, cfg.world, cfg.comm_mode = 0, 0, 2, 2
    cfg.m2o[:] = [float(v) for v in np.identity(4).reshape(-1)]
    h = ctypes.c_void_p()
    assert lib.mcl_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    dc = eng.make_drift_config(ZERO3, ZERO3)
    assert lib.mcl_drift_enable(h, ctypes.byref(dc), None) == ERR_UNSUPPORTED
    assert lib.mcl_drift_advance(h, 0.02, None) == ERR_STATE
    lib.mcl_destroy(h)


# ------------------------------------------------------------------ 4: the gather is the slot map
def log_weight_cases(n, rs):
    heavy = np.full(n, -1e3)
    heavy[(2 * n) // 3] = 0.0
    return (('random', 2.0 * rs.randn(n)), ('one_heavy', heavy), ('all_equal', np.full(n, -3.0)),
            ('random_again', 3.0 * rs.randn(n)))


@pytest.mark.parametrize('n', [65, 1000, 1025])
@pytest.mark.parametrize('scheme', ['SYSTEMATIC', 'RESIDUAL', 'MULTINOMIAL'])
def test_resample_takes_the_drift_along_by_the_slot_map(scheme, n, eng):
    rs = np.random.RandomState(n)
    e = eng.Engine(n, seed=7, resample_scheme=getattr(eng, scheme), **COV)
    e.init_particles()
    e.drift_enable([0.2, 0.2, 0.01], [0.005, 0.005, 1e-4])
    moved = 0
    for name, lw in log_weight_cases(n, rs):
        before = e.drift_get()
        e.set_log_weights(lw)
        e.resample()
        A = resampling.slot_ancestors(e.last_indices()).astype(np.int64)
        after = e.drift_get()
        assert np.array_equal(bits(after), bits(before[:, A])), name
        lost = int(np.count_nonzero(A != np.arange(n)))
        moved += lost
        if name == 'one_heavy':
            assert lost == n - 1 and np.all(A == (2 * n) // 3)
            assert np.array_equal(bits(after), bits(np.repeat(before[:, (2 * n) // 3:(2 * n) // 3 + 1], n, axis=1)))
        if name == 'all_equal' and scheme == 'SYSTEMATIC':
            assert lost == 0 and np.array_equal(bits(after), bits(before))       # nobody is lost: the drift is untouched
        e.drift_advance(0.02)                                                    # (spread the copies again)
    assert moved > n
    e.close()


@pytest.mark.parametrize('scheme', ['SYSTEMATIC', 'STRATIFIED'])
def test_gather_beside_the_history(scheme, eng):
    n = 1000
    rs = np.random.RandomState(3)
    e = eng.Engine(n, seed=8, resample_scheme=getattr(eng, scheme), **COV)
    e.init_particles()
    e.history_enable(2)
    e.drift_enable([0.2, 0.2, 0.01], ZERO3)
    for name, lw in log_weight_cases(n, rs):
        e.history_record(0.0)                             # link = identity: after the resample it is A itself
        before = e.drift_get()
        e.set_log_weights(lw)
        e.resample()
        A = resampling.slot_ancestors(e.last_indices()).astype(np.int64)
        assert np.array_equal(e.history_ancestors(0), A), name
        assert np.array_equal(bits(e.drift_get()), bits(before[:, A])), name
    e.close()


def test_gather_through_a_fused_step(eng):
    n = 1000
    origin = (-16.0, -16.0)
    e = eng.Engine(n, seed=9, **COV)
    e.set_map_grid(synth.bathymetry_grid(32, 32, 1.0, origin, seed=1), origin, 1.0)
    e.init_particles()
    e.drift_enable([0.2, 0.2, 0.01], [0.005, 0.005, 1e-4])
    ba = synth.beam_angles(16, half_swath=math.pi / 6)    # (a fan of +-10 m at 18 m: inside the 32 m map)
    ranges = (18.0 / np.cos(ba)).astype(np.float32)
    st = synth.odom_stream(4)
    moved = 0
    for k in range(4):
        e.drift_advance(st['dt'])
        before = e.drift_get()
        e.step_mbes(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], st['dt'], ranges, ba, 0.5, 60.0)
        A = resampling.slot_ancestors(e.last_indices()).astype(np.int64)
        assert np.array_equal(bits(e.drift_get()), bits(before[:, A])), k
        moved += int(np.count_nonzero(A != np.arange(n)))
    assert moved > 0
    e.close()


# ------------------------------------------------------------------ 5: mean and covariance
@pytest.mark.parametrize('n', [1, 63, 257, 4097])
def test_mean_cov_against_numpy(n, eng):
    rs = np.random.RandomState(n)
    e = eng.Engine(n, **COV)
    e.init_particles()
    e.drift_enable(ZERO3, ZERO3)
    d = np.array([[0.15], [-0.10], [2e-3]]) + rs.randn(3, n) * np.array([[0.2], [0.05], [1e-3]])
    e.drift_set(d)
    mean, cov = e.drift_mean_cov()
    big = np.abs(d).max(axis=1)
    want_mean = d.mean(axis=1)
    r = d - want_mean[:, None]
    want_cov = np.array([[(r[a] * r[b]).mean() for b in range(3)] for a in range(3)])
    assert np.all(np.abs(mean - want_mean) <= 1e-12 * big), (mean, want_mean)
    assert np.all(np.abs(cov - want_cov) <= 1e-12 * np.outer(big, big)), (cov, want_cov)
    assert np.array_equal(cov, cov.T)
    mean2, cov2 = e.drift_mean_cov()
    assert np.array_equal(bits(mean), bits(mean2)) and np.array_equal(bits(cov), bits(cov2))
    if n == 1:
        assert np.array_equal(mean, d[:, 0]) and not np.any(cov)
    assert np.array_equal(bits(e.drift_get()), bits(d))                           # a query: nothing is written
    e.close()


# ------------------------------------------------------------------ 7: the closed loop
CURRENT = (0.15, -0.10)


def closed_loop(eng, drift, seed=1):
    """3000 odometry samples of a vehicle in a current the odometry does not see, a GPS fix of 0.5 m every second;
    returns (the mean-pose error just before every fix, drift_mean after every fix's resample, max |bw| seen)"""
    n = 4096
    st = synth.odom_stream(3000, current=CURRENT)
    idx, fixes = synth.gps_fixes(st['truth'], np.identity(4), every=50, sigma=0.5)
    e = eng.Engine(n, seed=seed, meas_std=0.5, init_cov=[0.01, 0.01, 0.0, 0.0, 0.0, 1e-4],
                   process_cov=[1e-4, 1e-4, 0.0, 0.0, 0.0, 1e-6], resample_cov=[0.0] * 6)
    e.init_particles()
    if drift:
        e.drift_enable([0.2, 0.2, 0.0], [0.005, 0.005, 0.0])
    at = {int(k): j for j, k in enumerate(idx)}
    err, means, bw = [], [], 0.0
    for k in range(len(st['stamp'])):
        if drift:
            e.drift_advance(st['dt'])
        e.predict(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], st['dt'])
        if k in at:
            mean = e.mean_cov()[0]
            err.append(math.hypot(mean[0] - st['truth'][k, 0], mean[1] - st['truth'][k, 1]))
            e.update_gps(fixes[at[k]][0], fixes[at[k]][1])
            e.resample()
            if drift:
                means.append(e.drift_mean_cov()[0])
                bw = max(bw, float(np.abs(e.drift_get()[2]).max()))
    e.close()
    return np.array(err), np.array(means), bw


def test_closed_loop_finds_the_current_and_follows_the_vehicle(eng):
    """Measured on an MI355X (seed 1): the current estimate (0.1532, -0.0986), 0.0035 m/s off; the mean-pose
    error before a fix 0.182 m with the drift, 0.821 m without.  The numpy restatement of the same filter stayed within
    0.024 m/s and 0.19 - 0.45 m against 0.50 - 1.04 m on five seeds."""
    err_on, means, bw = closed_loop(eng, True)
    err_off, _, _ = closed_loop(eng, False)
    assert len(err_on) == len(err_off) == 60 and means.shape == (60, 3)
    est = means[-10:].mean(axis=0)
    off = math.hypot(est[0] - CURRENT[0], est[1] - CURRENT[1])
    e_on, e_off = float(err_on[-20:].mean()), float(err_off[-20:].mean())
    print('closed loop: current estimate (%.4f, %.4f), off by %.4f m/s; mean-pose error before a fix %.3f m with the drift, '
          '%.3f m without' % (est[0], est[1], off, e_on, e_off))
    assert off <= 0.5 * math.hypot(*CURRENT)              # (a) within |c| / 2 = 0.09 m/s
    assert e_on < e_off                                   # (b)
    assert bw == 0.0 and not np.any(means[:, 2])          # (c) no std on the bias: exactly zero throughout


def test_replay_reports_the_drift_and_is_unchanged_without_it():
    from smarc_navigation_amd import replay
    st = replay.synthetic_stream(500, current=CURRENT)
    params = dict(replay.SYNTH_PARAMS, particle_count=1024, seed=4)
    off = replay.replay(st, params)
    off2 = replay.replay(st, dict(params, estimate_drift=False, drift_init_std='[9.0, 9.0, 9.0]'))
    on = replay.replay(st, dict(params, estimate_drift=True))
    assert not [k for k in off['summary'] if k.startswith('drift')]
    assert np.array_equal(bits(off['pf_xyz']), bits(off2['pf_xyz']))            # off: the poses are what they were
    s = on['summary']
    assert len(s['drift_mean']) == 3 and s['drift_mean'][2] == 0.0 and s['drift_bias_error'] == 0.0
    assert s['drift_error'] == math.hypot(s['drift_mean'][0] - CURRENT[0], s['drift_mean'][1] - CURRENT[1])
    assert s['drift_error'] < 0.2 * math.sqrt(2.0) * 3.0       # (no accuracy claim after ten fixes: inside 3 sigma of the prior)
    assert not np.array_equal(on['pf_xyz'], off['pf_xyz'])
