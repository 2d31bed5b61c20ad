"""GPU tests of the ping matching (include/mcl_match.h; kernel csrc/mcl_match.h): every traced evaluation's integers against
the definition over its own dumped ranges, every step of the loop against the restated solve / compare on the traced sums
(and against the library's own mcl_match_solve / mcl_match_better), the dumped rays against the fp64 oracle under the
precision contract of mcl_update_mbes, recovery of the truth from the starts the host restatement converges from, seabeds
whose answer is known, invariance (runs, the handle's cloud, batch and order of the poses, beams without a return),
match_estimate on a filter, the errors, and the largest pose count.  The scene is the one of tests/test_innovation_host.py;
the restatement lives in tests/test_match_host.py, which also checks without a GPU that the oracle alone keeps the scene
within the outlier cap at the poses compared here."""
import math

import numpy as np
import pytest

from smarc_navigation_amd import synth
from tests.helpers import outliers_explained
from tests.test_innovation_host import M2O, N, OFF, OUTLIER_CAP, R_MAX, SIGMA, scene, scene_map
from tests.test_match_host import (BC_RMAX, CONVERGED, FLAT_START, GRID_ORIGIN, LOCAL_STARTS, MAX_ITER, NO_OVERLAP, RIDGE_START,
                                   RIDGE_TRUTH, STALLED, TRUTH, c_cfg, default_cfg, flat_grid, horizontal_error, loop_ref,
                                   next_pose_ref, ping_at, rec_tuple, ridge_grid, rms_quanta, rough_reference, starts_of,
                                   sums_ref, variants, _grid_eval)

pytestmark = pytest.mark.gpu

KINDS = ('grid', 'mesh', 'tin')


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def _bits(v):
    return np.float64(v).tobytes()


@pytest.fixture(scope='module')
def world(eng):
    """per map kind: an engine that holds the scene's map and no particles (matching needs none), and the oracle's map"""
    z, origin, soa = scene()
    out = dict(z=z, origin=origin, soa=soa)
    for kind in KINDS:
        e = eng.Engine(16, m2o=M2O, rng_mode=eng.RNG_REPLAY)
        (how, args), omap = scene_map(kind, z, origin)
        e.set_map_grid(*args) if how == 'grid' else e.set_map_mesh(*args)
        out[kind] = (e, omap)
    yield out
    for kind in KINDS:
        out[kind][0].close()


def _match(e, poses, meas, ba, cfg, **kw):
    return e.match_ping(poses, meas, ba, SIGMA, R_MAX, OFF, cfg=c_cfg(cfg), **kw)


def _poses(M, dims, seed=7):
    """M starts: the first ones of starts_of, then more of their kind; pose 1 (if there is one) stands off the map"""
    rs = np.random.RandomState(seed)
    p = np.repeat(TRUTH[:, None], M, axis=1)
    p[0] += rs.uniform(-2.0, 2.0, M)
    p[1] += rs.uniform(-2.0, 2.0, M)
    p[5] += rs.uniform(-0.05, 0.05, M)
    if dims == 4:
        p[2] += 0.4
    if M > 1:
        p[0, 1] += 280.0
    return np.ascontiguousarray(p)


def _ping(omap, B, holes=True):
    ba = synth.beam_angles(B, 1.0)
    meas = ping_at(omap, TRUTH, ba).copy()
    if holes and B >= 64:
        meas[[3, 17, 40]] = [0.0, -1.0, np.nan]          # beams without a return
    return ba, meas


# ------------------------------------------------------------------ 1. the reduction and the loop are exact
def _check_pose_against_its_trace(eng, match, poses, i, meas, cfg):
    res, tr, rng = match.results[i], match.trace[i], match.ranges[i]
    T = cfg['max_iter'] + 1
    n_eval = int(res['evaluations'])
    assert 1 <= n_eval <= T
    # every traced evaluation's sums equal the definition over its own dumped ranges
    traced = []
    for t in range(n_eval):
        want = sums_ref(meas, rng[t], cfg)
        assert rec_tuple(tr[t]['sums']) == want, (i, t)
        with np.errstate(invalid='ignore'):
            counts = np.asarray(meas, np.float32) > 0
        assert np.all(np.isnan(rng[t][:, ~counts])) and np.all(np.isfinite(rng[t][:, counts]))
        traced.append(want)
    assert not tr[n_eval:].tobytes().strip(b'\0') and np.all(np.isnan(rng[n_eval:]))      # nothing ran past the last one
    # the loop, restated, fed with the traced sums: every pose it asks for is the traced one, bit for bit
    asked = []

    def evaluate(pose6):
        t = len(asked)
        assert t < n_eval, (i, 'the restated loop wants more evaluations than the kernel ran')
        row = tr[t]
        assert [_bits(pose6[0]), _bits(pose6[1]), _bits(pose6[5]), _bits(pose6[2])] == \
            [_bits(row['x']), _bits(row['y']), _bits(row['yaw']), _bits(row['z'])], (i, t)
        asked.append(t)
        return traced[t]
    start = [float(tr[0]['x']), float(tr[0]['y']), float(tr[0]['z']), float(poses[3, i]), float(poses[4, i]),
             float(tr[0]['yaw'])]
    run = loop_ref(evaluate, start, cfg)
    assert len(asked) == n_eval == run['evaluations']
    for t, (_, _, j, acc) in enumerate(run['trace']):
        assert (int(tr[t]['j']), int(tr[t]['accepted'])) == (j, acc), (i, t)
    # the result record is the loop's, and equals the last accepted trace row
    assert (int(res['status']), int(res['accepted']), int(res['j']), int(res['dead'])) == (run['status'], run['accepted'], run['j'], run['dead'])
    assert [_bits(res[f]) for f in ('x', 'y', 'yaw', 'z')] == [_bits(v) for v in run['pose']]
    assert rec_tuple(res['start']) == traced[0] and rec_tuple(res['final']) == run['final']
    last = [t for t in range(n_eval) if tr[t]['accepted']][-1] if run['status'] != NO_OVERLAP else 0
    assert res['final'].tobytes() == tr[last]['sums'].tobytes()
    assert [_bits(res[f]) for f in ('x', 'y', 'yaw', 'z')] == [_bits(tr[last][f]) for f in ('x', 'y', 'yaw', 'z')]
    return run


def _check_library_solve_on_the_trace(eng, match, i, cfg):
    """the same steps once more through the library's own device-free functions"""
    tr, n_eval = match.trace[i], int(match.results[i]['evaluations'])
    c = c_cfg(cfg)
    cur = 0
    for t in range(1, n_eval):
        delta, _ = eng.match_solve(tr[cur]['sums'], c, int(tr[t]['j']))
        q = next_pose_ref([float(tr[cur][f]) for f in ('x', 'y', 'yaw', 'z')], [float(v) for v in delta])
        assert [_bits(v) for v in q] == [_bits(tr[t][f]) for f in ('x', 'y', 'yaw', 'z')], (i, t)
        assert eng.match_better(tr[t]['sums'], tr[cur]['sums'], cfg['min_beams']) == bool(tr[t]['accepted'])
        if tr[t]['accepted']:
            cur = t


@pytest.mark.parametrize('dims', [3, 4])
@pytest.mark.parametrize('B', [1, 64, 65, 300, 513])     # a lane, a wave, a wave's tail, a chunk's tail, three rounds
@pytest.mark.parametrize('kind', KINDS)
def test_every_evaluation_and_every_step_equal_the_definition(world, eng, kind, B, dims):
    e, omap = world[kind]
    ba, meas = _ping(omap, B)
    seen = set()
    for M in (1, 2, 65):
        for max_iter in (1, 12):
            cfg = default_cfg(dims=dims, max_iter=max_iter, min_beams=1 if B == 1 else 8, jump_max=2.0)
            poses = _poses(M, dims)
            match = _match(e, poses, meas, ba, cfg, trace=True, dump=True)
            assert match.trace.shape == (M, max_iter + 1) and match.ranges.shape == (M, max_iter + 1, 1 + 2 * dims, B)
            for i in range(M):
                run = _check_pose_against_its_trace(eng, match, poses, i, meas, cfg)
                seen.add(run['status'])
                if i < 3:
                    _check_library_solve_on_the_trace(eng, match, i, cfg)
            if M > 1:
                assert match.results['status'][1] == NO_OVERLAP and match.results['evaluations'][1] == 1
            # production passes neither trace nor dump: the same results
            plain = _match(e, poses, meas, ba, cfg)
            assert plain.results.tobytes() == match.results.tobytes() and plain.trace is None and plain.ranges is None
    print('%s B=%d dims=%d: statuses seen %s' % (kind, B, dims, sorted(seen)))
    if B >= 64:
        assert CONVERGED in seen and MAX_ITER in seen and NO_OVERLAP in seen


# ------------------------------------------------------------------ 2. the rays are right
@pytest.mark.parametrize('kind', KINDS)
def test_dumped_ranges_against_the_oracle_at_the_traced_poses_under_the_precision_contract(world, orc, kind):
    e, omap = world[kind]
    B, dims = 300, 4
    ba = synth.beam_angles(B)
    meas = ping_at(omap, TRUTH, ba)
    cfg = default_cfg(dims=dims)
    poses = starts_of(dims)
    match = _match(e, poses, meas, ba, cfg, trace=True, dump=True)
    states, got = [], []
    for i in range(poses.shape[1]):
        for t in range(int(match.results['evaluations'][i])):
            row = match.trace[i, t]
            states.append(variants([row['x'], row['y'], row['z'], poses[3, i], poses[4, i], row['yaw']], cfg))
            got.append(match.ranges[i, t])
    states = np.ascontiguousarray(np.concatenate(states, axis=1))
    got = np.concatenate(got, axis=0).astype(np.float64)
    _, ref = orc.mbes_update(states, M2O, OFF, omap, ba, None, SIGMA, R_MAX, want_expected=True)
    err = np.abs(got - ref)
    print('%s: max |e - oracle| %.3e m over %d rays at %d states, %d beyond 1e-3 m' % (kind, err.max(), err.size, states.shape[1],
                                                                                         int((err > 1e-3).sum())))
    assert (err > 1e-3).mean() <= OUTLIER_CAP
    outliers_explained(orc, omap, states, ba, got, ref, R_MAX, m2o=M2O, off=OFF, label='match %s' % kind)


# ------------------------------------------------------------------ 3. recovery
@pytest.mark.parametrize('dims', [3, 4])
@pytest.mark.parametrize('kind', KINDS)
def test_recovery_from_every_start_the_restatement_converges_from(world, eng, kind, dims):
    """noise-free pings made by the oracle at TRUTH.  A cast is within 1e-3 m of the oracle's and a residual within half a
    quantum of its range, so the residual vector of the m beams at the truth is no longer than sqrt(m) (1e-3 + 2^-12) m, and
    the least-squares fix moves by no more than that over the root of the smallest eigenvalue of A -- on top of what the
    restatement itself, fed with the oracle's casts, is off by."""
    e, _ = world[kind]
    ref = rough_reference(dims, kind)
    cfg = ref['cfg']
    match = _match(e, ref['starts'], ref['meas'], ref['ba'], cfg)
    for k, run in enumerate(ref['runs']):
        if run['status'] != CONVERGED:
            continue
        r = match.results[k]
        J, cov = match.information(k), match.cov(k)
        assert np.array_equal(J, J.T) and np.array_equal(cov, cov.T) and np.any(np.triu(cov, 1) != 0.0)
        assert np.allclose(cov.dot(J), np.identity(dims), rtol=0, atol=1e-8)            # sigma^2 A^-1 times A / sigma^2
        A = J * SIGMA * SIGMA
        lam = float(np.linalg.eigvalsh(A, UPLO='U')[0])
        m = int(match.m[k])
        bound = horizontal_error(run) + math.sqrt(m) * (1e-3 + 2.0 ** -12) / math.sqrt(lam)
        err = math.hypot(r['x'] - TRUTH[0], r['y'] - TRUTH[1])
        print('%s dims %d start %d: status %d after %d evaluations, %.3e m off (restatement %.3e, bound %.3e), rms %.2e m' % (
            kind, dims, k, r['status'], r['evaluations'], err, horizontal_error(run), bound, match.rms[k]))
        assert r['status'] == CONVERGED and lam > 0.0 and m >= 8
        assert err <= bound


# ------------------------------------------------------------------ 4. seabeds whose answer is known
def _built(eng, z):
    e = eng.Engine(16, rng_mode=eng.RNG_REPLAY)
    e.set_map_grid(z, GRID_ORIGIN, 1.0)
    return e


def _built_ping(orc, z, truth, B=64):
    omap = orc.Grid(z, GRID_ORIGIN, 1.0)
    ba = synth.beam_angles(B)
    return ba, ping_at(omap, truth, ba, np.identity(4), [0] * 6, BC_RMAX)


def test_flat_seabed_x_y_and_yaw_return_the_starts_bits_and_z_is_recovered(eng, orc):
    z = flat_grid()
    truth = FLAT_START.copy()
    truth[2] = -2.0
    ba, meas = _built_ping(orc, z, truth)
    e = _built(eng, z)
    cfg = c_cfg(default_cfg(dims=4, jump_max=BC_RMAX))
    match = e.match_ping(FLAT_START[:, None], meas, ba, SIGMA, BC_RMAX, cfg=cfg)
    e.close()
    r = match.results[0]
    print('flat: status %d, %d evaluations, z %.6f, dead %d, S diag %s' % (r['status'], r['evaluations'], r['z'], r['dead'],
                                                                         [int(r['final']['S'][k]) for k in (0, 2, 5, 9)]))
    assert r['status'] == CONVERGED and r['dead'] == 1 | 2 | 4
    assert [_bits(r['x']), _bits(r['y']), _bits(r['yaw'])] == [_bits(FLAT_START[0]), _bits(FLAT_START[1]), _bits(FLAT_START[5])]
    assert abs(r['z'] - truth[2]) <= 1e-3 + 2.0 ** -12             # one cast's contract and a quantum
    assert np.isinf(match.cov(0)[0, 0]) and np.isfinite(match.cov(0)[3, 3])


def test_ridge_along_x_returns_the_bits_of_x_and_recovers_y(eng, orc):
    z = ridge_grid()
    ba, meas = _built_ping(orc, z, RIDGE_TRUTH)
    e = _built(eng, z)
    cfg = c_cfg(default_cfg(dims=3, jump_max=BC_RMAX))
    match = e.match_ping(RIDGE_START[:, None], meas, ba, SIGMA, BC_RMAX, cfg=cfg)
    e.close()
    r = match.results[0]
    print('ridge: status %d, %d evaluations, y %.6f (truth %.6f), dead %d' % (r['status'], r['evaluations'], r['y'], RIDGE_TRUTH[1], r['dead']))
    assert r['status'] == CONVERGED and r['dead'] & 1 and _bits(r['x']) == _bits(RIDGE_START[0])
    assert int(r['final']['S'][0]) == 0 and int(r['start']['S'][0]) == 0
    A = match.information(0)[1:, 1:] * SIGMA * SIGMA
    # the restatement's own error on the oracle's casts, then the derived term of the recovery test
    host = loop_ref(_grid_eval(z, RIDGE_TRUTH, default_cfg(dims=3, jump_max=BC_RMAX)), RIDGE_START, default_cfg(dims=3, jump_max=BC_RMAX))
    assert host['status'] == CONVERGED
    assert abs(r['y'] - RIDGE_TRUTH[1]) <= abs(host['pose'][1] - RIDGE_TRUTH[1]) + math.sqrt(int(match.m[0])) * (1e-3 + 2.0 ** -12) / math.sqrt(float(np.linalg.eigvalsh(A)[0]))
    assert np.isinf(match.cov(0)[0, 0]) and np.isfinite(match.cov(0)[1, 1])


@pytest.mark.parametrize('dims', [3, 4])
@pytest.mark.parametrize('kind', KINDS)
def test_off_the_map_and_a_local_minimum(world, eng, kind, dims):
    e, _ = world[kind]
    ref = rough_reference(dims, kind)
    far = TRUTH.copy()
    far[0] += 280.0
    poses = np.stack([far, LOCAL_STARTS[dims]], axis=1)
    match = _match(e, poses, ref['meas'], ref['ba'], ref['cfg'])
    r = match.results
    assert r['status'][0] == NO_OVERLAP and r['evaluations'][0] == 1 and r['accepted'][0] == 0 and int(match.m[0]) == 0
    assert [_bits(r[f][0]) for f in ('x', 'y', 'yaw', 'z')] == [_bits(far[0]), _bits(far[1]), _bits(far[5]), _bits(far[2])]
    print('%s dims %d local minimum: status %d after %d evaluations, rms %.4f -> %.4f m, %.2f m off' % (
        kind, dims, r['status'][1], r['evaluations'][1], match.start_rms[1], match.rms[1],
        math.hypot(r['x'][1] - TRUTH[0], r['y'][1] - TRUTH[1])))
    assert r['status'][1] in (MAX_ITER, STALLED)
    assert match.rms[1] <= match.start_rms[1] and match.best() is None
    assert rms_quanta(rec_tuple(r['final'][1])) > 100.0             # its final cost tells it apart


# ------------------------------------------------------------------ 5. invariance
def test_two_runs_give_the_same_bytes_and_a_populated_handle_is_left_untouched(world, eng):
    z, origin, soa = world['z'], world['origin'], world['soa']
    _, omap = world['tin']
    e = eng.Engine(N, m2o=M2O, seed=9)
    e.set_particles(soa)
    (_, args), _ = scene_map('tin', z, origin)
    e.set_map_mesh(*args)
    ba, meas = _ping(omap, 300)
    e.update_mbes(meas, ba, SIGMA, R_MAX, OFF)
    e.resample()                                            # (fixed-point weights exist from here on)
    e.update_mbes(meas, ba, SIGMA, R_MAX, OFF)              # pending log-weights: nothing here reads or writes them

    def fixed():
        q, total = e.fixed_weights()
        return q.tobytes(), total
    soa0, lw0, fw0 = e.get_particles().tobytes(), e.get_log_weights().tobytes(), fixed()
    cfg = default_cfg(dims=4)
    poses = _poses(40, 4)
    a = _match(e, poses, meas, ba, cfg, trace=True, dump=True)
    b = _match(e, poses, meas, ba, cfg, trace=True, dump=True)
    assert a.results.tobytes() == b.results.tobytes() and a.trace.tobytes() == b.trace.tobytes()
    assert a.ranges.tobytes() == b.ranges.tobytes()
    assert e.get_particles().tobytes() == soa0 and e.get_log_weights().tobytes() == lw0 and fixed() == fw0
    # the handle without particles gives the same bytes
    assert _match(world['tin'][0], poses, meas, ba, cfg).results.tobytes() == a.results.tobytes()
    e.close()


@pytest.mark.parametrize('kind', ['grid', 'tin'])
def test_poses_at_once_equal_each_alone_and_any_permutation(world, kind):
    e, omap = world[kind]
    ba, meas = _ping(omap, 65)
    cfg = default_cfg(dims=3)
    M = 24
    poses = _poses(M, 3)
    whole = _match(e, poses, meas, ba, cfg).results
    for i in range(M):
        assert _match(e, poses[:, i:i + 1], meas, ba, cfg).results.tobytes() == whole[i:i + 1].tobytes(), i
    perm = np.random.RandomState(1).permutation(M)
    assert _match(e, np.ascontiguousarray(poses[:, perm]), meas, ba, cfg).results.tobytes() == whole[perm].tobytes()


@pytest.mark.parametrize('dims', [3, 4])
def test_removing_the_beams_without_a_return_changes_no_bit(world, dims):
    e, omap = world['mesh']
    ba, meas = _ping(omap, 300)
    with np.errstate(invalid='ignore'):
        keep = meas > 0
    assert keep.sum() == 297
    cfg = default_cfg(dims=dims)
    poses = _poses(9, dims)
    assert _match(e, poses, meas, ba, cfg).results.tobytes() == _match(e, poses, meas[keep], ba[keep], cfg).results.tobytes()


# ------------------------------------------------------------------ 6. from the filter
def test_match_estimate_from_a_filter(eng, orc):
    n, B, steps = 4096, 64, 20
    origin = (-64.0, -64.0)
    z = synth.bathymetry_grid(128, 128, 1.0, origin, seed=1)
    g = orc.Grid(z, origin, 1.0)
    ba = synth.beam_angles(B)
    st = synth.odom_stream(steps)
    e = eng.Engine(n, init_cov=[1.0, 1.0, 0.0, 0.0, 0.0, 0.01], process_cov=[1e-4, 1e-4, 0.0, 0.0, 0.0, 1e-6],
                   resample_cov=[0.01, 0.01, 0.0, 0.0, 0.0, 1e-5], seed=3)
    e.set_map_grid(z, origin, 1.0)
    e.init_particles()
    meas = None
    for k in range(steps):
        e.predict(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], st['dt'])
        meas = ping_at(g, st['truth'][k], ba, np.identity(4), [0] * 6, 60.0)
        if k % 5 == 4:
            e.update_mbes(meas, ba, 0.2, 60.0)
            e.resample()
    soa0 = e.get_particles().tobytes()
    plain, best0 = e.match_estimate(meas, ba, 0.2, 60.0, modes=0)
    multi, best2 = e.match_estimate(meas, ba, 0.2, 60.0, modes=2)
    assert e.get_particles().tobytes() == soa0
    e.close()
    assert len(plain) == 1 and 1 <= len(multi) <= 3
    assert multi.results[:1].tobytes() == plain.results.tobytes()          # the first start is the cloud's mean both times
    for m in (plain, multi):
        assert np.all(m.rms <= m.start_rms)                                # the accept rule guarantees it
    print('match_estimate: %s; with 2 modes: %s' % (plain.pose(0), [multi.pose(i) for i in range(len(multi))]))
    if best0 is not None:
        assert best2 is not None and multi.rms[best2] <= plain.rms[best0]  # more starts: no worse
        truth = st['truth'][steps - 1]
        print('best fix %.4f m from the truth' % math.hypot(plain.results['x'][best0] - truth[0], plain.results['y'][best0] - truth[1]))


# ------------------------------------------------------------------ 7. errors
def test_argument_and_state_errors(world, eng):
    e, omap = world['grid']
    ba, meas = _ping(omap, 64)
    poses = _poses(4, 3)

    def status(*a, **k):
        with pytest.raises(eng.MclError) as ei:
            e.match_ping(*a, **k)
        return ei.value.status

    assert status(np.zeros((6, 0)), meas, ba, SIGMA, R_MAX, OFF) == -1
    assert status(np.zeros((6, 65537)), meas, ba, SIGMA, R_MAX, OFF) == -1
    nanpose = poses.copy()
    nanpose[5, 2] = np.nan
    assert status(nanpose, meas, ba, SIGMA, R_MAX, OFF) == -1
    infpose = poses.copy()
    infpose[0, 0] = np.inf
    assert status(infpose, meas, ba, SIGMA, R_MAX, OFF) == -1
    for kw in (dict(max_iter=0), dict(max_iter=33), dict(min_beams=0), dict(grad_floor_q=-1), dict(step_max_xy=0.0),
               dict(step_max_yaw=math.nan), dict(tol_xy=-1.0), dict(delta_xy=0.0), dict(delta_yaw=-0.01), dict(jump_max=R_MAX + 1.0)):
        assert status(poses, meas, ba, SIGMA, R_MAX, OFF, **kw) == -1, kw
    bad = eng.make_match_config(R_MAX)
    bad.dims = 5
    assert eng.match_config_check(bad, R_MAX) and status(poses, meas, ba, SIGMA, R_MAX, OFF, cfg=bad) == -1
    assert status(poses, meas, ba, 0.0, R_MAX, OFF) == -1 and status(poses, meas, ba, SIGMA, 4096.5, OFF) == -1
    assert status(poses, meas, ba, SIGMA, 0.0, OFF) == -1
    bad_ba = ba.copy()
    bad_ba[3] = np.nan
    assert status(poses, meas, bad_ba, SIGMA, R_MAX, OFF) == -1
    assert status(poses, np.ones(2049, np.float32), np.zeros(2049, np.float32), SIGMA, R_MAX, OFF) == -1
    # a dump too large: 2048 poses x 33 evaluations x 9 variants x 513 beams > 2^26 floats
    big_ba = synth.beam_angles(513)
    many = np.ascontiguousarray(np.tile(poses, (1, 512)))
    assert 2048 * 33 * 9 * 513 > 1 << 26
    assert status(many, np.ones(513, np.float32), big_ba, SIGMA, R_MAX, OFF, fit_z=True, max_iter=32, dump=True) == -1
    with pytest.raises(ValueError):
        e.match_ping(poses, meas[:10], ba, SIGMA, R_MAX, OFF)
    # the bounds themselves
    assert len(e.match_ping(poses, meas, ba, SIGMA, 4096.0, OFF, max_iter=32, jump_max=2048.0)) == 4
    bare = eng.Engine(16)
    with pytest.raises(eng.MclError) as ei:
        bare.match_ping(poses, meas, ba, SIGMA, R_MAX)
    assert ei.value.status == -5                                   # no map
    bare.close()


# ------------------------------------------------------------------ 8. the largest pose count
def test_the_largest_pose_count_runs(world):
    e, omap = world['grid']
    ba, meas = _ping(omap, 64)
    M = 65536
    base = _poses(1024, 3)
    match = e.match_ping(np.ascontiguousarray(np.tile(base, (1, M // 1024))), meas, ba, SIGMA, R_MAX, OFF, max_iter=2)
    r = match.results
    assert r.size == M and np.all(r['evaluations'] <= 3) and np.all(r['start']['n'] == 61)
    assert r[:1024].tobytes() == r[-1024:].tobytes()
    assert np.all(np.isin(r['status'], (CONVERGED, MAX_ITER, NO_OVERLAP))) and (r['status'] == MAX_ITER).any()
    # with a trace the scratch block of this call passes 64 MiB (360 + 4 x 192 bytes per pose): the library gives it back
    # before it returns, and the next call finds what it needs again
    few = e.match_ping(base[:, :8], meas, ba, SIGMA, R_MAX, OFF, max_iter=3)
    traced = e.match_ping(np.ascontiguousarray(np.tile(base, (1, M // 1024))), meas, ba, SIGMA, R_MAX, OFF, max_iter=3, trace=True)
    assert traced.trace.shape == (M, 4) and traced.results[:1024].tobytes() == traced.results[-1024:].tobytes()
    assert traced.trace[:1024].tobytes() == traced.trace[-1024:].tobytes() and np.all(traced.trace['accepted'][:, 0] == (r['status'] != NO_OVERLAP))
    assert e.match_ping(base[:, :8], meas, ba, SIGMA, R_MAX, OFF, max_iter=3).results.tobytes() == few.results.tobytes()
    assert traced.results[:8].tobytes() == few.results.tobytes()
