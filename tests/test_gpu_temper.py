"""GPU tests of ESS-targeted tempering (include/mcl_temper.h; kernels csrc/mcl_temper.h): the level, the sums and the scaled
log-weights against the restatement of tests/test_temper_host.py (Python integers over the oracle's det_exp, which
mcl_device.h promises to equal bit for bit), shards against the unsharded cloud bit for bit, the j = 0 no-op, the error
codes, a real MBES update and the node's `temper_ess_ratio`."""
import math

import numpy as np
import pytest

from smarc_navigation_amd import synth
from tests.test_temper_host import CASES, RATIOS, Cloud, beta_ref, case_lw, n_target_of, search_abi, search_ref

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
BLOCK = 256                      # MCL_BLOCK: a workgroup's particles per pass
SUMS_SPAN = 1024 * BLOCK         # TP_SUMS_GRID workgroups: beyond it the sums kernel strides over the cloud


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def expect_status(eng, status, fn, *a, **kw):
    with pytest.raises(eng.MclError) as ei:
        fn(*a, **kw)
    assert ei.value.status == status, ei.value


def planted(eng, lw, mode=None, **kw):
    e = eng.Engine(len(lw), **kw)
    e.set_log_weights(lw, eng.WEIGHT_LOG_SHIFT if mode is None else mode)
    return e


def scaled(lw, j):
    """the header's apply: one IEEE product on the finite entries, the others untouched"""
    out = np.array(lw, dtype=np.float64)
    fin = np.isfinite(out)
    out[fin] = beta_ref(j) * out[fin]
    return out


def check_against_restatement(eng, lw, tag):
    cloud = Cloud(lw)
    n = len(lw)
    e = planted(eng, lw)
    for ratio in RATIOS:
        n_t = n_target_of(ratio, n)
        j, floor_hit, levels = search_ref(cloud.sums, n_t)
        r = e.temper(ratio, apply=False)
        print('%s ratio %.1f: j %d (want %d) floor %d levels %d n_live %d' % (tag, ratio, r.j, j, r.floor_hit, r.levels_evaluated, r.n_live))
        assert (r.j, int(r.floor_hit), r.levels_evaluated) == (j, floor_hit, levels), (tag, ratio, r)
        assert r.n_live == cloud.n_live and r.n_target == n_t and r.beta == beta_ref(j), (tag, ratio, r)
        assert (r.max_lw == cloud.m) or (cloud.n_live == 0 and r.max_lw == -math.inf), (tag, r)
        assert np.array_equal(bits(e.get_log_weights()), bits(lw)), (tag, 'apply=False wrote the log-weights')
    # the last ratio once more, applied
    r2 = e.temper(RATIOS[-1], apply=True)
    assert r2 == r, (tag, r, r2)
    assert np.array_equal(bits(e.get_log_weights()), bits(scaled(lw, r.j))), (tag, r)
    e.close()
    return r


# ------------------------------------------------------------------ the level, and the apply
@pytest.mark.parametrize('n', [1, 2, 65, BLOCK - 1, BLOCK + 1, 1000, 4097])
@pytest.mark.parametrize('name', CASES)
def test_level_and_scaled_weights_equal_the_restatement(eng, name, n):
    check_against_restatement(eng, case_lw(name, n), '%s n=%d' % (name, n))


@pytest.mark.parametrize('name', ['peaked_nonfinite', 'gps'])
def test_level_where_the_sums_kernel_strides(eng, name):
    """one particle more than the sums launch covers in one pass; the log-weights drawn from 512 distinct values, so that
    the restatement's integer sums stay cheap (counts x per-value terms: exact)"""
    check_against_restatement(eng, case_lw(name, SUMS_SPAN + 1, pool=512), '%s n=%d' % (name, SUMS_SPAN + 1))


def test_results_cover_no_tempering_interior_levels_and_the_floor(eng):
    got = {}
    for name in CASES:
        lw = case_lw(name, 1000)
        e = planted(eng, lw)
        got[name] = e.temper(0.5, apply=False)
        e.close()
    assert got['flat'].j == 0 and got['flat'].levels_evaluated == 17 and got['gps'].j == 0
    assert 0 < got['peaked'].j < 2048 and got['peaked'].levels_evaluated == 39 and not got['peaked'].floor_hit
    assert got['floor'].j == 2048 and got['floor'].floor_hit and got['floor'].levels_evaluated == 17


# ------------------------------------------------------------------ j = 0 is no call at all
@pytest.mark.parametrize('name,mode', [('gps', 'log'), ('gps', 'floor'), ('flat', 'log')])
def test_level_zero_leaves_the_resample_as_it_was(eng, name, mode):
    n = 4097
    lw = case_lw(name, n)
    soa = np.random.RandomState(3).randn(6, n)
    wm = eng.WEIGHT_LOG_SHIFT if mode == 'log' else eng.WEIGHT_LINEAR_FLOOR
    cov = dict(resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4], seed=17)
    a, b = planted(eng, lw, wm, **cov), planted(eng, lw, wm, **cov)
    for e in (a, b):
        e.set_particles(soa)
        e.set_log_weights(lw, wm)
    r = a.temper(0.5)
    assert r.j == 0 and r.beta == 1.0
    assert np.array_equal(bits(a.get_log_weights()), bits(lw))
    a.resample()
    b.resample()
    assert np.array_equal(a.last_indices(), b.last_indices())
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    a.close()
    b.close()


# ------------------------------------------------------------------ the split form
@pytest.mark.parametrize('name,n', [('peaked_nonfinite', 4097), ('gps', 1000)])
def test_split_sums_equal_the_restatement(eng, name, n):
    lw = case_lw(name, n)
    cloud = Cloud(lw)
    e = planted(eng, lw)
    for levels in (list(range(0, 2049, 128)), [2048, 0, 1, 63, 64, 65, 700, 161, 5, 1999, 1024, 333, 12, 1500, 900, 47, 2047], [300]):
        s1, s2 = e.temper_sums(cloud.m, levels)
        want = [cloud.sums(j) for j in levels]
        assert s1 == [w[0] for w in want] and s2 == [w[1] for w in want], (name, levels)
    assert np.array_equal(bits(e.get_log_weights()), bits(lw))
    # a maximum from elsewhere (a larger one of another shard): the sums are those relative to it
    other = Cloud(lw, m=cloud.m + 3.5)
    s1, s2 = e.temper_sums(cloud.m + 3.5, [0, 64, 640])
    assert (s1, s2) == ([other.sums(j)[0] for j in (0, 64, 640)], [other.sums(j)[1] for j in (0, 64, 640)])
    assert e.temper_sums(-math.inf, [0, 5]) == ([0, 0], [0, 0])
    e.temper_apply(0)
    assert np.array_equal(bits(e.get_log_weights()), bits(lw))
    e.temper_apply(333)
    assert np.array_equal(bits(e.get_log_weights()), bits(scaled(lw, 333)))
    e.close()


# ------------------------------------------------------------------ shards
UNEQUAL = (1, 7, 100, 513, 1024, 1500, 2, 950)      # 4097 particles; the sums do not care how they are cut


@pytest.mark.parametrize('name', ['peaked', 'peaked_nonfinite', 'two_maxima'])
def test_eight_unequal_shards_equal_the_unsharded_cloud(eng, name):
    """mcl_create admits only equal shards of one world (n_global = world x n_particles), so the unequal split -- one shard
    of a single particle -- is eight handles that together hold the 4097 particles: mcl_group_temper takes any such set."""
    n = sum(UNEQUAL)
    assert n == 4097
    lw = case_lw(name, n)
    one = planted(eng, lw)
    cuts = np.cumsum((0,) + UNEQUAL)
    many = [planted(eng, lw[cuts[k]:cuts[k + 1]]) for k in range(8)]
    # the split calls, driven as ranks would drive them: maxima merged, integer sums added, the ABI's plan and predicate
    m = max(s.max_lw for s in (e.weight_stats() for e in many))
    cloud = Cloud(lw)
    assert m == cloud.m

    def sums(j):
        parts = [e.temper_sums(m, [j]) for e in many]
        return sum(p[0][0] for p in parts), sum(p[1][0] for p in parts)
    for ratio in RATIOS:
        r = one.temper(ratio, apply=False)
        g = eng.group_temper(many, ratio, apply=False)
        assert g == r, (ratio, r, g)
        assert search_abi(sums, n_target_of(ratio, n)) == (r.j, int(r.floor_hit)), ratio
    r = one.temper(0.5)
    g = eng.group_temper(many, 0.5)
    assert g == r and r.j > 0
    assert np.array_equal(bits(np.concatenate([e.get_log_weights() for e in many])), bits(one.get_log_weights()))
    for e in [one] + many:
        e.close()


def test_eight_shards_of_one_world_temper_and_resample_as_the_unsharded_cloud(eng):
    shards, nl = 8, 512
    n = shards * nl
    lw = case_lw('peaked', n)
    soa = np.random.RandomState(9).randn(6, n)
    cov = dict(resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4], seed=23)
    one = eng.Engine(n, **cov)
    many = [eng.Engine(nl, rank=r, world=shards, n_global=n, global_offset=r * nl, **cov) for r in range(shards)]
    one.set_particles(soa)
    one.set_log_weights(lw)
    for r, e in enumerate(many):
        e.set_particles(np.ascontiguousarray(soa[:, r * nl:(r + 1) * nl]))
        e.set_log_weights(lw[r * nl:(r + 1) * nl])
    expect_status(eng, ERR_STATE, many[0].temper, 0.5)          # a shard alone: the group call or the split calls
    want = one.temper(0.5)
    got = eng.group_temper(many, 0.5)
    assert got == want and want.j > 0
    assert np.array_equal(bits(np.concatenate([e.get_log_weights() for e in many])), bits(one.get_log_weights()))
    one.resample()
    eng.group_resample(many)
    assert np.array_equal(one.last_indices(), np.concatenate([e.last_indices() for e in many]))
    assert np.array_equal(bits(one.get_particles()), bits(np.concatenate([e.get_particles() for e in many], axis=1)))
    for e in [one] + many:
        e.close()


# ------------------------------------------------------------------ at size
def test_a_million_particles_reach_the_target_and_no_level_below_does(eng):
    n, ratio = 1 << 20, 0.1
    lw = case_lw('peaked', n, seed=2)
    n_t = n_target_of(ratio, n)
    eps = 4.0 * 2.0 ** -32 / ratio ** 2     # the floors move S1 by <= 2^-32 / ratio, S2 by <= 2^-32 / ratio^2, relatively

    def ess(j):
        w = np.exp(beta_ref(j) * (lw - lw.max()))
        return float(w.sum()) ** 2 / float((w * w).sum())
    e = planted(eng, lw)
    r = e.temper(ratio, apply=False)
    print('1 M particles: j %d beta %.6g levels %d; ESS(j) / n_t - 1 = %.3e, ESS(j - 1) / n_t - 1 = %.3e'
          % (r.j, r.beta, r.levels_evaluated, ess(r.j) / n_t - 1.0, (ess(r.j - 1) / n_t - 1.0) if r.j else float('nan')))
    assert 0 < r.j < 2048 and not r.floor_hit and r.n_live == n and r.n_target == n_t
    assert ess(r.j) >= n_t * (1.0 - eps)
    assert ess(r.j - 1) < n_t * (1.0 + eps)
    e2 = planted(eng, lw)
    assert e2.temper(ratio) == r and e.temper(ratio) == r
    assert np.array_equal(bits(e.get_log_weights()), bits(e2.get_log_weights()))
    assert np.array_equal(bits(e.get_log_weights()), bits(scaled(lw, r.j)))
    e.close()
    e2.close()


# ------------------------------------------------------------------ errors
def test_error_codes(eng):
    n = 1000
    lw = case_lw('peaked', n)
    e = eng.Engine(n, seed=1)
    expect_status(eng, ERR_STATE, e.temper, 0.5)                          # no pending weights
    expect_status(eng, ERR_STATE, e.temper_sums, 0.0, [0])
    expect_status(eng, ERR_STATE, e.temper_apply, 3)
    expect_status(eng, ERR_STATE, eng.group_temper, [e], 0.5)
    e.set_particles(np.zeros((6, n)))
    e.set_log_weights(lw)
    for bad in (0, -3, n + 1):
        expect_status(eng, ERR_INVALID, e.temper, n_target=bad)
        expect_status(eng, ERR_INVALID, eng.group_temper, [e], n_target=bad)
    expect_status(eng, ERR_INVALID, e.temper_sums, 0.0, list(range(18)))
    expect_status(eng, ERR_INVALID, e.temper_sums, 0.0, [2049])
    expect_status(eng, ERR_INVALID, e.temper_sums, math.nan, [0])
    expect_status(eng, ERR_INVALID, e.temper_sums, math.inf, [0])
    expect_status(eng, ERR_INVALID, e.temper_apply, 2049)
    expect_status(eng, ERR_INVALID, e.temper_apply, -1)
    assert np.array_equal(bits(e.get_log_weights()), bits(lw))
    assert e.temper(n_target=n).n_target == n and e.temper(n_target=1, apply=False).j == 0
    e.set_log_weights(lw)
    want = search_ref(Cloud(lw).sums, n_target_of(0.5, n))[0]
    assert e.temper(0.5, wait=False) is None                              # out = NULL: no wait, no failure
    assert np.array_equal(bits(e.get_log_weights()), bits(scaled(lw, want)))
    e.resample()
    expect_status(eng, ERR_STATE, e.temper, 0.5)                          # after a resample
    e.set_log_weights(np.exp(lw - lw.max()), eng.WEIGHT_LINEAR)
    expect_status(eng, ERR_STATE, e.temper, 0.5)                          # linear weights are no logarithms
    expect_status(eng, ERR_STATE, e.temper_sums, 0.0, [0])
    expect_status(eng, ERR_STATE, e.temper_apply, 3)
    e.close()


def test_more_than_two_to_the_24_particles_are_refused(eng):
    n = (1 << 24) + 1
    e = eng.Engine(n)
    e.set_log_weights(np.zeros(n))
    expect_status(eng, ERR_UNSUPPORTED, e.temper, 0.5)
    expect_status(eng, ERR_UNSUPPORTED, eng.group_temper, [e], 0.5)
    e.close()


# ------------------------------------------------------------------ after a real update
ORIGIN = (-64.0, -64.0)


@pytest.fixture(scope='module')
def seabed():
    z = synth.bathymetry_grid(128, 128, 1.0, ORIGIN, seed=1)
    return z, synth.beam_angles(64)


def ping_at(eng, z, ba, x, y, yaw):
    t = eng.Engine(1)
    t.set_map_grid(z, ORIGIN, 1.0)
    t.set_particles(np.array([[x], [y], [-2.0], [0.0], [0.0], [yaw]]))
    r = t.mbes_expected(0, 1, ba, 60.0)[0]
    t.close()
    return r


def test_a_real_ping_is_tempered_to_the_target_and_can_be_accumulated_onto(eng, seabed):
    z, ba = seabed
    n, ratio = 4096, 0.5
    ranges = ping_at(eng, z, ba, 0.5, -0.3, 0.1)
    pair = []
    for _ in range(2):
        e = eng.Engine(n, init_cov=[4, 4, 0, 0, 0, 0.01], seed=5)
        e.set_map_grid(z, ORIGIN, 1.0)
        e.init_particles()
        e.predict([0.0, 0.0, 0.0], 0.0, [0.0, 0.0, 0.0, 1.0], -2.0, 0.02)
        pair.append(e)
    a, b = pair
    a.update_mbes(ranges, ba, 0.05, 60.0)
    lw = a.get_log_weights()
    before = a.weight_stats().n_eff
    r = a.temper(ratio)
    n_t = n_target_of(ratio, n)
    eps = 4.0 * 2.0 ** -32 / ratio ** 2
    after = a.weight_stats().n_eff
    print('64-beam ping, sigma 0.05, n 4096: n_eff %.2f -> %.2f (target %d), j %d beta %.4g' % (before, after, n_t, r.j, r.beta))
    assert r.beta < 1.0 and r.j == search_ref(Cloud(lw).sums, n_t)[0] and before < n_t
    assert after >= n_t * (1.0 - eps)
    lw_t = a.get_log_weights()
    assert np.array_equal(bits(lw_t), bits(scaled(lw, r.j)))
    # a DVL range accumulated onto the tempered weights: what it adds onto the same weights planted by hand
    dirs, rng = np.array([[0.0, 0.0, -1.0]]), np.array([ranges[len(ranges) // 2]])
    b.set_log_weights(lw_t)
    for e in (a, b):
        e.update_ranges(rng, dirs, 0.2, 60.0, accumulate=True)
    acc = a.get_log_weights()
    assert np.array_equal(bits(acc), bits(b.get_log_weights())) and not np.array_equal(bits(acc), bits(lw_t))
    a.resample()
    b.resample()
    assert np.array_equal(a.last_indices(), b.last_indices())
    a.close()
    b.close()


# ------------------------------------------------------------------ the node
def run_node(seabed, ratio, forbid=False):
    from smarc_navigation_amd import auv_pf, engine, msgs
    z, ba = seabed
    params = {'particle_count': 4096, 'seed': 11, 'init_covariance': '[1.0, 1.0, 0.0, 0.0, 0.0, 0.01]',
              'motion_covariance': '[0.001, 0.001, 0.0, 0.0, 0.0, 0.00001]',
              'resampling_noise_covariance': '[0.01, 0.01, 0.0, 0.0, 0.0, 0.0001]', 'mbes_std': 0.1}
    if ratio is not None:
        params['temper_ess_ratio'] = ratio
    pf = auv_pf.auv_pf(params)
    pf.set_map_grid(z, ORIGIN, 1.0)
    if forbid:
        def boom(*a, **kw):
            raise AssertionError('temper called with temper_ess_ratio = 0')
        pf.particles.temper = boom
    pf.start_timing(100.0)
    ainc = float(ba[1] - ba[0])
    betas, t = [], 100.0
    for k in range(10):
        t += 0.1
        om = msgs.Odometry()
        om.header.stamp = msgs.Time(t)
        om.twist.twist.linear.x = 1.0
        om.pose.pose.position.z = -2.0
        pf.odom_callback(om)
        x_true = 1.0 * (t - 100.0)
        pf.mbes_cb(msgs.LaserScan(ping_at(engine, z, ba, x_true, 0.0, 0.0), float(ba[0]), ainc, 60.0))
        betas.append(pf.temper_last_beta)
    mean, yaw, cov9 = pf.update_loc_pose()
    poses = pf.particles.get_particles()
    out = dict(betas=betas, mean=np.array(mean), cov=np.array(cov9).reshape(3, 3), poses=poses, tempered=pf.tempered_updates,
               err=float(np.hypot(mean[0] - x_true, mean[1])))
    pf.particles.close()
    return out


def test_node_parameter_tempers_every_ping_and_keeps_the_cloud_wide(seabed):
    on = run_node(seabed, 0.5)
    off = run_node(seabed, 0.0, forbid=True)
    default = run_node(seabed, None, forbid=True)
    print('node, 10 pings of 64 beams, mbes_std 0.1, 4096 particles: betas %s' % ' '.join('%.4g' % b for b in on['betas']))
    print('position error after 10 pings: tempered %.3f m, untempered %.3f m; trace of cov(x, y): tempered %.4g, untempered %.4g'
          % (on['err'], off['err'], on['cov'][0, 0] + on['cov'][1, 1], off['cov'][0, 0] + off['cov'][1, 1]))
    assert all(b < 1.0 for b in on['betas']) and on['tempered'] == 10
    assert all(b == 1.0 for b in off['betas']) and off['tempered'] == 0
    assert on['cov'][0, 0] + on['cov'][1, 1] > off['cov'][0, 0] + off['cov'][1, 1]
    # parameter 0 is the parent's path: temper is never called (it would have raised), and the default is 0
    assert np.array_equal(bits(off['poses']), bits(default['poses']))


# ------------------------------------------------------------------ replay.py --temper-ess
def test_replay_switch_reports_the_exponents(eng, tmp_path, capsys):
    import json
    from smarc_navigation_amd import replay
    steps, dt, speed = 80, 0.125, 1.5
    k = np.arange(steps)
    truth = np.stack([speed * (k + 1) * dt, np.zeros(steps), np.full(steps, -2.0)], axis=1)
    st = dict(stamp=100.0 + (k + 1) * dt, t0=100.0, v=np.tile([speed, 0.0, 0.0], (steps, 1)), wz=np.zeros(steps),
              q=np.tile([0.0, 0.0, 0.0, 1.0], (steps, 1)), z=np.full(steps, -2.0), truth_xyz=truth)
    origin = (-32.0, -64.0)
    z = synth.bathymetry_grid(128, 128, 1.0, origin, seed=1)
    ba = synth.beam_angles(64)
    one = eng.Engine(1)
    one.set_map_grid(z, origin, 1.0)
    idx, ranges = np.arange(0, steps, 2), []
    for i in idx:
        soa = np.zeros((6, 1))
        soa[:3, 0] = truth[i]
        one.set_particles(soa)
        ranges.append(one.mbes_expected(0, 1, ba, 60.0)[0])
    one.close()
    st.update(mbes_idx=idx, mbes_ranges=np.array(ranges), mbes_angles=ba, mbes_range_max=60.0)
    spath, gpath = str(tmp_path / 'stream.npz'), str(tmp_path / 'grid.npz')
    np.savez(spath, **st)
    np.savez(gpath, z=z, origin=np.array(origin), res=1.0)
    out = {}
    for tag, extra in (('on', ['--temper-ess', '0.5']), ('off', [])):
        replay.main([spath, '--map-grid', gpath, '--particles', '2048', '--seed', '4'] + extra)
        out[tag] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(out)
    on, off = out['on'], out['off']
    assert 'temper_beta_mean' not in off and 'temper_beta_min' not in off
    assert on['temper_ess_ratio'] == 0.5 and on['temper_resamplings'] == len(idx) and on['tempered_updates'] >= 1
    assert 0.0 < on['temper_beta_min'] <= on['temper_beta_mean'] <= 1.0 and on['temper_beta_min'] < 1.0
