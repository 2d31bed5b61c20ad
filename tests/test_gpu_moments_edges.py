"""The published estimate -- mean pose, mean wrapped yaw, covariance -- at its numeric edges, on every path that takes the
13 sums: the two-pass kernels (k_mean_partial / k_cov_partial / k_sum_final), the sums inside the resample gather
(k_resample_gather<MOMENTS>, <MOMENTS, UNI> and the STASH variant with its second pass and its re-read of the state
beyond four particles per thread), the reduction over the shards of a LOCAL group with either exchange, the two formats
of the pinned ring and its wrap, and the PoseArray payload.

The reference is tests/helpers.py: moments_reference (long double; anchored on the CPU by
tests/test_moments_predict_reference.py).  The bound is derived, not measured: every output lies within

    K 2^-53 U

of the reference.  K counts the roundings on the longest path from a particle to the output (helpers.sum_roundings, from
the kernels' launch constants: the per-thread chain ceil(n / (grid block)), 6 in the wave, block / 64 across the waves,
ceil(grid / 64) + 6 across the blocks, 8 for the products, the subtraction, the division and the un-shift; a LOCAL group
adds its shards one after the other: + shards - 1).  U is the size of what is rounded: |shift| + mean |d| for a mean of
x, y, z, mean |v| for the other means, mean |d_a d_b| + |mean d_a| |mean d_b| for a covariance, d = v - shift.  The shift
is the one-pass form's documented one -- the position of global particle 0 after the predict, before the resample, z the
odometry's depth where z is substituted -- and the long-double mean itself for the two-pass form.  With the shift outside
the cloud (family outlier0: D = 1400 m, sigma = 1 cm) U says what the one-pass form can deliver, eps (D / sigma)^2 relative
to the covariance: a limit of the form, written down in DESIGN.md, not a failure of the bound.

Each path is driven by the conditions plan_gather documents (mcl_host_resample.h); no test reads the variant back.  The
worst err / (2^-53 U) of every path is printed (pytest -s) and recorded in DESIGN.md; the asserted constant stays K."""
import numpy as np
import pytest

from smarc_navigation_amd import synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

L = np.longdouble
ODOM = dict(v=[1.2, 0.1, -0.05], wz=0.07, z=-3.5, dt=0.02)
RPY = (0.05, -0.03, 1.0)
B = 8
WORST = {}


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def clouds():
    """family, n -> (6, n) fp64, made once and handed out read-only"""
    cache = {}

    def get(family, n):
        if (family, n) not in cache:
            soa = H.moments_family(family, n)
            soa.setflags(write=False)
            cache[(family, n)] = soa
        return cache[(family, n)]
    return get


def _centre(family):
    return H.SURVEY_XY if family in ('survey', 'outlier0', 'one', 'identical') else (3.0, -2.0)


def _map_for(family):
    """a 128 x 128 m bathymetry grid with the cloud in its middle (outlier0's particle 0 lies off it)"""
    cx, cy = _centre(family)
    origin = (cx - 64.0, cy - 64.0)
    return synth.bathymetry_grid(128, 128, 1.0, origin, seed=3), origin


def _invalid_ping():
    """no beam carries a range (NaN / 0, as in test_all_beams_invalid_gives_uniform_weights): uniform weights, every
    particle survives in its slot"""
    ranges = np.full(B, np.nan, np.float32)
    ranges[::2] = 0.0
    return ranges, synth.beam_angles(B)


def _resample_cov(family, zrp=(0.0, 0.0, 0.0)):
    if family in ('one', 'identical'):
        xy, yaw = 0.0, 0.0          # the particles stay equal
    elif family in ('survey', 'outlier0'):
        xy, yaw = 1e-6, 1e-6
    else:
        xy, yaw = 1e-2, 1e-2 if family == 'seam' else 1e-4
    return [xy, xy, zrp[0], zrp[1], zrp[2], yaw]


def _check(path, label, got, soa, shift, K):
    if H.MOMENTS_N_CAP and soa.shape[1] > H.MOMENTS_N_CAP:
        pytest.skip('no extended precision on this host: the rational reference stops at n = %d' % H.MOMENTS_N_CAP)
    ref = H.moments_reference(soa, shift)
    rm, ry, rc = H.moments_errors(got, ref)
    worst = float(max(rm.max(), ry.max(), rc.max()))
    WORST[path] = max(WORST.get(path, 0.0), worst)
    print('%s %s: err / (2^-53 U) mean %.2f, wrapped yaw %.2f, cov %.2f (K = %d); worst of the path so far %.2f' % (
        path, label, rm.max(), ry.max(), rc.max(), K, WORST[path]))
    assert rm.max() <= K, (label, 'mean', rm)
    assert ry.max() <= K, (label, 'yaw', ry)
    assert rc.max() <= K, (label, 'cov', rc)
    assert got[2][6] == 0.0 and got[2][7] == 0.0 and got[2][3] == got[2][1]
    return ref


def _ld_mean(soa):
    return soa[:3].astype(L).sum(axis=1) / L(soa.shape[1])


def _shift_after_predict(eng, orc, p0, process_cov=(0,) * 6, seed=0, dt=ODOM['dt']):
    """the one-pass form's shift: global particle 0 after the predict, from a twin handle that runs mcl_predict alone (the
    draws are keyed by the global index; that the fused predict equals it bit for bit is pinned elsewhere); z is the
    odometry's"""
    if not dt > 0.0:
        return [p0[0], p0[1], p0[2]]
    twin = eng.Engine(1, process_cov=process_cov, seed=seed)
    twin.set_particles(np.ascontiguousarray(p0.reshape(6, 1)))
    twin.predict(ODOM['v'], ODOM['wz'], orc.quat_from_euler(*RPY), ODOM['z'], dt)
    s = twin.get_particles()[:, 0]
    twin.close()
    return [s[0], s[1], ODOM['z']]


def _substituted(got, K, orc):
    """z, roll, pitch are the odometry's on every particle: no covariance in z at all, means to K roundings"""
    roll, pitch, _ = orc.euler_from_quat(orc.quat_from_euler(*RPY))
    assert got[2][8] == 0.0 and got[2][2] == 0.0 and got[2][5] == 0.0
    for k, v in ((2, ODOM['z']), (3, roll), (4, pitch)):
        assert abs(got[0][k] - v) <= K * H.EPS53 * abs(v), (k, got[0][k], v)


def _fused_step(eng, orc, soa, family, dt, zrp, seed=5):
    z, origin = _map_for(family)
    e = eng.Engine(soa.shape[1], resample_cov=_resample_cov(family, zrp), seed=seed)
    e.set_map_grid(z, origin, 1.0)
    e.set_particles(soa)
    ranges, ba = _invalid_ping()
    e.step_mbes(ODOM['v'], ODOM['wz'], orc.quat_from_euler(*RPY), ODOM['z'], dt, ranges, ba, 0.2, 80.0)
    got = e.last_mean_cov()
    st = e.get_particles()
    assert np.array_equal(e.last_indices(), np.arange(soa.shape[1]))      # nobody died, outlier0's particle 0 included
    e.close()
    return got, st


# ------------------------------------------------------------------------------------------ the two-pass kernels
@pytest.mark.parametrize('family', H.MOMENT_FAMILIES)
def test_two_pass_mean_cov(family, eng, clouds):
    """mean_cov() after set_particles; 524288 + 1 is the first n whose grid strides.  A cloud of equal particles has no
    covariance: U is zero there and so is every entry."""
    for n in ([1] if family == 'one' else [63, 64, 65, 255, 257, 524288 + 1]):
        soa = clouds(family, n)
        e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
        e.set_particles(soa)
        got = e.mean_cov()
        e.close()
        _check('two-pass', '%s n=%d' % (family, n), got, soa, _ld_mean(soa), H.two_pass_roundings(n))
        if family in ('one', 'identical'):
            assert np.all(got[2] == 0.0) and np.array_equal(got[0][:3], soa[:3, 0])


# ------------------------------------------------------------------------------------------ the stash kernel
STASH_CASES = [('one', 1)] + [(f, n) for f in ('origin', 'survey', 'outlier0', 'seam', 'identical')
                              for n in (65, 1025, 262144 + 1, 4 * 262144 + 1)]


@pytest.mark.parametrize('family,n', STASH_CASES)
def test_fused_step_stash_kernel(family, n, eng, orc, clouds, monkeypatch):
    """step_mbes with dt > 0 and no resampling noise on z, roll, pitch: the stash kernel.  262144 + 1 particles put two on
    one thread, 4 * 262144 + 1 a fifth, which the second pass reads back from the state.  With and without the visiting
    order (the two large clouds are swept, so the second pass then also bins them) the sums are the same bits."""
    soa = clouds(family, n)
    K = H.gather_roundings(n)
    shift = _shift_after_predict(eng, orc, soa[:, 0])
    res = {}
    for visit in ('1', '0'):
        monkeypatch.setenv('MCL_VISIT', visit)
        res[visit] = _fused_step(eng, orc, soa, family, ODOM['dt'], (0.0, 0.0, 0.0))
    (ga, sa), (gb, sb) = res['1'], res['0']
    assert np.array_equal(sa, sb)
    for x, y in zip(ga, gb):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    _check('stash', '%s n=%d' % (family, n), ga, sa, shift, K)
    _substituted(ga, K, orc)
    if family in ('one', 'identical'):
        assert np.all(ga[2] == 0.0)
    if family == 'seam':
        assert np.count_nonzero((sa[5] < -np.pi) | (sa[5] >= np.pi)) > n // 50     # wrap works inside the sums


# ------------------------------------------------------------------------------------------ <MOMENTS, UNI>
@pytest.mark.parametrize('zrp', [(0.0, 1e-6, 1e-6), (1e-4, 1e-6, 1e-6)], ids=['noise_on_roll_pitch', 'noise_on_z_roll_pitch'])
@pytest.mark.parametrize('family,n', [(f, n) for f in ('origin', 'survey', 'outlier0', 'seam') for n in (65, 262144 + 1)])
def test_fused_step_moments_uni_kernel(family, n, zrp, eng, orc, clouds):
    """dt > 0 and resampling noise on roll and pitch (and z): z, roll, pitch are substituted, then carry their noise.
    Without noise on z the z column is the odometry's depth exactly -- no covariance in z, its mean to K roundings; with
    it the z moments are the noise's and only the bound speaks (the shift's z is the odometry's depth either way)."""
    soa = clouds(family, n)
    K = H.gather_roundings(n)
    got, st = _fused_step(eng, orc, soa, family, ODOM['dt'], zrp)
    _check('moments-uni', '%s n=%d z-noise %g' % (family, n, zrp[0]), got, st, _shift_after_predict(eng, orc, soa[:, 0]), K)
    if zrp[0] == 0.0:
        assert got[2][8] == 0.0 and got[2][2] == 0.0 and got[2][5] == 0.0
        assert abs(got[0][2] - ODOM['z']) <= K * H.EPS53 * abs(ODOM['z'])
    else:
        assert got[2][8] > 0.0


# ------------------------------------------------------------------------------------------ <MOMENTS>
@pytest.mark.parametrize('family,n', [(f, n) for f in ('origin', 'survey', 'outlier0', 'seam') for n in (65, 262144 + 1)])
def test_fused_step_moments_kernel_without_predict(family, n, eng, orc, clouds):
    """dt = 0: no predict in front of the gather, nothing is substituted, the shift is particle 0 as it was set"""
    soa = clouds(family, n)
    got, st = _fused_step(eng, orc, soa, family, 0.0, (1e-4, 1e-6, 1e-6))
    _check('moments', '%s n=%d' % (family, n), got, st, list(soa[:3, 0]), H.gather_roundings(n))
    assert not np.all(st[2] == st[2, 0])


# ------------------------------------------------------------------------------------------ the shift dies
def test_shift_outside_the_cloud_whose_particle_dies(eng, orc):
    """A real ping on the grid of test_fused_step_equals_separate_calls_bitwise; particle 0 sits 300 m off the map, gets no
    offspring -- and is still the shift of the sums, which hold the bound about it."""
    n = 8192 + 77
    origin = (-64.0, -64.0)
    z = synth.bathymetry_grid(128, 128, 1.0, origin, seed=3)
    ba = synth.beam_angles(96)
    cov = dict(process_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5], resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4], seed=31)
    soa = H.moments_family('origin', n, seed=3).copy()
    soa[2] = -2.0
    soa[0, 0] += 364.0
    q = orc.quat_from_euler(*RPY)
    truth = np.array([[3.0], [-2.0], [ODOM['z']], [RPY[0]], [RPY[1]], [0.4]])
    one = eng.Engine(1, rng_mode=eng.RNG_REPLAY)
    one.set_map_grid(z, origin, 1.0)
    one.set_particles(truth)
    ranges = one.mbes_expected(0, 1, ba, 80.0)[0]
    one.close()
    e = eng.Engine(n, **cov)
    e.set_map_grid(z, origin, 1.0)
    e.set_particles(soa)
    e.step_mbes(ODOM['v'], ODOM['wz'], q, ODOM['z'], ODOM['dt'], ranges, ba, 0.3, 80.0)
    got = e.last_mean_cov()
    idx = e.last_indices()
    st = e.get_particles()
    e.close()
    assert 0 not in idx and np.unique(idx).size < n
    assert st[0].max() < 100.0                                           # nothing of particle 0 is left in the cloud
    shift = _shift_after_predict(eng, orc, soa[:, 0], cov['process_cov'], cov['seed'])
    assert shift[0] > 300.0
    K = H.gather_roundings(n)
    _check('stash, shift dead', 'n=%d' % n, got, st, shift, K)
    _substituted(got, K, orc)


# ------------------------------------------------------------------------------------------ shards
@pytest.mark.parametrize('exchange', ['p2p', 'allgather'])
@pytest.mark.parametrize('family', ['survey', 'outlier0'])
def test_sharded_fused_step_and_group_mean_cov(family, exchange, eng, orc, clouds, monkeypatch):
    """group_step_mbes over 3 shards of 4099: the shards' sums reduced in scal[32..], the shift taken from the
    all-gathered state (allgather) or from the hand-over records (p2p); then the two-pass kernels over the same shards.
    A LOCAL group adds the shards' sums one after the other: K + 2."""
    if exchange == 'allgather':
        monkeypatch.setenv('MCL_EXCHANGE', 'allgather')
    else:
        monkeypatch.delenv('MCL_EXCHANGE', raising=False)
    ns, nl = 3, 4099
    n = ns * nl
    soa = clouds(family, n)
    z, origin = _map_for(family)
    many = [eng.Engine(nl, rank=r, world=ns, n_global=n, global_offset=r * nl, resample_cov=_resample_cov(family), seed=5)
            for r in range(ns)]
    for r, e in enumerate(many):
        e.set_map_grid(z, origin, 1.0)
        e.set_particles(np.ascontiguousarray(soa[:, r * nl:(r + 1) * nl]))
    ranges, ba = _invalid_ping()
    eng.group_step_mbes(many, ODOM['v'], ODOM['wz'], orc.quat_from_euler(*RPY), ODOM['z'], ODOM['dt'], ranges, ba, 0.2, 80.0)
    got = many[0].last_mean_cov()
    st = np.concatenate([e.get_particles() for e in many], axis=1)
    assert np.array_equal(np.concatenate([e.last_indices() for e in many]), np.arange(n))
    K = H.gather_roundings(nl) + ns - 1
    _check('sharded fused (%s)' % exchange, family, got, st, _shift_after_predict(eng, orc, soa[:, 0]), K)
    _substituted(got, K, orc)
    two = eng.group_mean_cov(many)
    _check('sharded two-pass', '%s (%s)' % (family, exchange), two, st, _ld_mean(st), H.two_pass_roundings(nl) + ns - 1)
    for e in many:
        e.close()


# ------------------------------------------------------------------------------------------ the ring
def test_ring_wraps_with_both_formats(eng, orc, clouds):
    """4096 + 5 results, fused steps (format 1) and mean_cov_async (format 0) taking turns: mean_history reads the last
    4096 across the wrap, each undone by its own format.  No noise anywhere and a ping without ranges: the state after a
    step is the predicted one slot for slot, so its particle 0 IS that step's shift."""
    n, total = 64, 4096 + 5
    soa = clouds('survey', n)
    z, origin = _map_for('survey')
    e = eng.Engine(n, seed=5)
    e.set_map_grid(z, origin, 1.0)
    e.set_particles(soa)
    ranges, ba = _invalid_ping()
    ranges, ba = ranges[:1], ba[:1]
    q = orc.quat_from_euler(*RPY)
    refs, fmt = [], []
    st = soa
    for k in range(total):
        if k % 2 == 0:
            e.step_mbes(ODOM['v'], ODOM['wz'], q, ODOM['z'], ODOM['dt'], ranges, ba, 0.2, 80.0)
            st = e.get_particles()
            refs.append(H.moments_reference(st, [st[0, 0], st[1, 0], ODOM['z']]))
            fmt.append(1)
        else:
            e.mean_cov_async()
            refs.append(H.moments_reference(st, _ld_mean(st)))
            fmt.append(0)
    K = {1: H.gather_roundings(n), 0: H.two_pass_roundings(n)}
    hist = e.mean_history(4096)
    worst = {0: 0.0, 1: 0.0}
    for row, ref, f in zip(hist, refs[-4096:], fmt[-4096:]):
        r = np.abs(row.astype(L) - ref['mean']) / (L(H.EPS53) * ref['u_mean'])
        worst[f] = max(worst[f], float(r.max()))
    print('ring: worst mean err / (2^-53 U) over the last 4096 entries: format 0 %.2f (K = %d), format 1 %.2f (K = %d)' % (
        worst[0], K[0], worst[1], K[1]))
    assert worst[0] <= K[0] and worst[1] <= K[1]
    assert np.ptp(hist[:, 0]) > 10.0 and np.ptp(hist[:, 5]) > 1.0          # the entries differ: a mixed-up slot would show
    last = e.last_mean_cov()
    assert np.array_equal(last[0], hist[-1])
    _check('ring', 'last entry (format %d)' % fmt[-1], last, st, [st[0, 0], st[1, 0], ODOM['z']], K[fmt[-1]])
    with pytest.raises(eng.MclError) as err:
        e.mean_history(4097)
    assert err.value.status == -1                                            # MCL_ERR_INVALID
    e.close()


# ------------------------------------------------------------------------------------------ poses
def test_poses_of_a_cloud_across_the_seam(eng, clouds):
    """poses() against quaternion_from_euler in long double: 4 * 2^-53 per component, positions bit for bit"""
    n = 1025
    soa = clouds('seam', n)
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
    e.set_particles(soa)
    poses = e.poses()
    e.close()
    assert np.array_equal(poses[:, :3], soa[:3].T)
    ref = H.quat_from_euler_ld(soa[3], soa[4], soa[5])
    err = np.abs(poses[:, 3:].astype(L) - ref) / L(H.EPS53)
    print('poses: worst quaternion component error %.2f x 2^-53' % float(err.max()))
    assert err.max() <= 4.0
