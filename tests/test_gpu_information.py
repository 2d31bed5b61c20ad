"""GPU tests of the ping information (include/mcl_information.h; kernel csrc/mcl_information.h): the nine integers per beam
against a numpy / Python-integer restatement of the definition over the dumped six ranges, the rays against the fp64 oracle
at the perturbed poses under the precision contract of mcl_update_mbes (1e-3 m; grazing rays excused only through
helpers.outliers_explained), the per-pose accumulation against the per-beam one, determinism over runs, group sizes and
shards, a handle left untouched, seabeds built so that the answer is known, the errors, the raster and the replay.  The
scene is the one of tests/test_innovation_host.py; the restatement lives in tests/test_information_host.py, which also
checks, without a GPU, that the oracle alone keeps the scene within the outlier cap at the six perturbed pose sets."""
import math

import numpy as np
import pytest

from smarc_navigation_amd import synth
from tests.helpers import outliers_explained
from tests.test_information_host import (DELTA_XY, DELTA_YAW, FIELDS, ints, matrix_ref, perturbed, records_ref)
from tests.test_innovation_host import (M2O, MAX_SAMPLES, N, OFF, OUTLIER_CAP, R_MAX, SIGMA, sample_ref, sampled_slots, scene,
                                        scene_map)

pytestmark = pytest.mark.gpu

KINDS = ('grid', 'mesh', 'tin')
COUNT = 586          # sampled particles: ceil(4096 / 7)
# what one quantised central difference may be off by: two rays within the 1e-3 m contract, and half a quantum of 2^-12 m
DIFF_TOL = 2 * 1e-3 + 2.0 ** -13


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def _engine(eng, kind, z, origin, soa, m2o=M2O, **kw):
    e = eng.Engine(soa.shape[1], m2o=m2o, rng_mode=eng.RNG_REPLAY, **kw)
    e.set_particles(soa)
    (how, args), _ = scene_map(kind, z, origin)
    e.set_map_grid(*args) if how == 'grid' else e.set_map_mesh(*args)
    return e


@pytest.fixture(scope='module')
def world(eng):
    """per map kind: the engine over the shared scene, the oracle's map, the sampled slots -- built once"""
    z, origin, soa = scene()
    stride, count = sample_ref(N, MAX_SAMPLES)
    slots = sampled_slots(N, stride)
    assert stride == 7 and count == slots.size == COUNT and COUNT % 7 and COUNT % 10
    out = dict(z=z, origin=origin, soa=soa, slots=slots)
    for kind in KINDS:
        out[kind] = (_engine(eng, kind, z, origin, soa), scene_map(kind, z, origin)[1])
    yield out
    for kind in KINDS:
        out[kind][0].close()


def _info(e, B, **kw):
    kw.setdefault('max_samples', MAX_SAMPLES)
    return e.ping_information(synth.beam_angles(B), SIGMA, R_MAX, OFF, **kw)


# ------------------------------------------------------------------ 1. the reduction is exact
@pytest.mark.parametrize('B', [1, 64, 65, 300, 512])     # a wave, a wave's tail, a chunk's tail (300), two chunks
@pytest.mark.parametrize('kind', KINDS)
def test_the_nine_integers_equal_the_definition_over_the_dumped_ranges(world, kind, B):
    e, _ = world[kind]
    tight = _info(e, B, jump_max=1.0, dump=True)
    assert tight.n_sampled == COUNT and tight.ranges.shape == (COUNT, 6, B)
    assert np.all(np.isfinite(tight.ranges)) and np.all(tight.ranges >= 0) and np.all(tight.ranges <= np.float32(R_MAX))
    want = records_ref(tight.ranges, R_MAX, 1.0)
    assert ints(tight.beams) == want
    n, n_miss, n_jump = (np.array([w[i] for w in want]) for i in range(3))
    assert np.all(n == COUNT) and np.all(n_miss >= 21) and np.all(n_miss + n_jump < n)     # the 21 samples past the edge
    print('%s B=%d: %d jumps at 1 m, %d misses' % (kind, B, n_jump.sum(), n_miss.sum()))
    if B == 300:
        assert n_jump.sum() > 0        # (the CPU oracle finds them in this scene: tests/test_information_host.py)
    # jump_max = r_max: no pair can jump; the same rays
    loose = _info(e, B, jump_max=R_MAX, dump=True)
    assert loose.ranges.tobytes() == tight.ranges.tobytes()
    want = records_ref(loose.ranges, R_MAX, R_MAX)
    assert ints(loose.beams) == want and not loose.beams['n_jump'].any()
    # production passes no dump: the same records; and None means min(r_max, 2048)
    plain = _info(e, B, jump_max=1.0)
    assert plain.beams.tobytes() == tight.beams.tobytes() and plain.ranges is None
    assert _info(e, B).beams.tobytes() == loose.beams.tobytes()
    # the derived matrix is the restatement's, bit for bit
    J, share = matrix_ref(want, SIGMA)
    assert [float(v) for v in loose.J] == J and loose.hit_share == share and loose.matrix.shape == (3, 3)
    assert np.array_equal(loose.matrix, loose.matrix.T) and loose.matrix[0, 2] == J[2] and loose.matrix[2, 2] == J[5]


# ------------------------------------------------------------------ 2. the rays are right
@pytest.mark.parametrize('kind', KINDS)
def test_dumped_ranges_against_the_oracle_at_the_perturbed_poses_under_the_precision_contract(world, orc, kind):
    e, omap = world[kind]
    ba = synth.beam_angles(300)
    got = _info(e, 300, dump=True).ranges.astype(np.float64)
    sub = np.ascontiguousarray(world['soa'][:, world['slots']])
    for v in range(6):
        s = perturbed(sub, v)
        _, ref = orc.mbes_update(s, M2O, OFF, omap, ba, None, SIGMA, R_MAX, want_expected=True)
        err = np.abs(got[:, v] - ref)
        print('%s variant %d: max |e - oracle| %.3e m over %d rays, %d beyond 1e-3 m' % (kind, v, err.max(), err.size, int((err > 1e-3).sum())))
        assert (err > 1e-3).mean() < OUTLIER_CAP
        outliers_explained(orc, omap, s, ba, np.ascontiguousarray(got[:, v]), ref, R_MAX, m2o=M2O, off=OFF,
                           label='information %s variant %d' % (kind, v))


# ------------------------------------------------------------------ 3. per pose equals per beam
@pytest.mark.parametrize('kind', KINDS)
def test_one_pose_per_pose_is_the_sum_of_its_per_beam_records(world, eng, kind):
    pose = np.ascontiguousarray(world['soa'][:, 8:9])
    one = _engine(eng, kind, world['z'], world['origin'], pose)
    ba = synth.beam_angles(300)
    per_beam = one.ping_information(ba, SIGMA, R_MAX, OFF, jump_max=1.0)
    per_pose = one.pose_information(pose, ba, SIGMA, R_MAX, OFF, jump_max=1.0)
    one.close()
    assert per_beam.n_sampled == 1 and per_pose.poses.size == 1
    assert ints(per_pose.poses)[0] == tuple(sum(int(v) for v in per_beam.beams[f]) for f in FIELDS)
    assert int(per_pose.poses['n'][0]) == 300 and int(per_pose.poses['sxx'][0]) > 0


@pytest.mark.parametrize('M', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('kind', KINDS)
def test_every_pose_record_is_the_sum_of_that_poses_dumped_pairs(world, eng, kind, M):
    B = 65 if M > 1 else 300                                   # two waves, the second with one beam; M = 1: two chunks' worth
    poses = np.ascontiguousarray(world['soa'][:, 3:3 + M])     # (slot 203 stands past the map's edge)
    cloud = _engine(eng, kind, world['z'], world['origin'], poses)
    ba = synth.beam_angles(B)
    dump = cloud.ping_information(ba, SIGMA, R_MAX, OFF, max_samples=32768, jump_max=1.0, dump=True)
    cloud.close()
    assert dump.n_sampled == M and dump.ranges.shape == (M, 6, B)
    e, _ = world[kind]                                         # an engine that holds OTHER particles: they play no part
    got = e.pose_information(poses, ba, SIGMA, R_MAX, OFF, jump_max=1.0)
    want = records_ref(dump.ranges, R_MAX, 1.0, per_pose=True)
    assert ints(got.poses) == want
    if M == 1000:
        assert want[200] == (B, B, 0, 0, 0, 0, 0, 0, 0) and got.hit_share[200] == 0.0 and got.rank_pos[200] == 0
    Js = matrix_ref(want, SIGMA, per_pose=True)
    assert all([float(v) for v in got.J[k]] == Js[k][0] and got.hit_share[k] == Js[k][1] for k in range(M))
    assert got.matrix.shape == (M, 3, 3) and got.crlb_weak.shape == (M,)


# ------------------------------------------------------------------ 4. determinism
def test_two_runs_give_the_same_bytes_and_the_handle_is_left_untouched(world, eng):
    e, _ = world['tin']
    ba = synth.beam_angles(300)
    ranges = e.mbes_expected(1, 1, ba, R_MAX, OFF)[0].astype(np.float32)
    e.update_mbes(ranges, ba, SIGMA, R_MAX, OFF)            # pending log-weights: nothing here reads or writes them
    soa0, lw0 = e.get_particles().tobytes(), e.get_log_weights().tobytes()
    a, b = _info(e, 300, jump_max=1.0, dump=True), _info(e, 300, jump_max=1.0, dump=True)
    assert a.beams.tobytes() == b.beams.tobytes() and a.ranges.tobytes() == b.ranges.tobytes()
    poses = np.ascontiguousarray(world['soa'][:, :100])
    p, q = (e.pose_information(poses, ba, SIGMA, R_MAX, OFF) for _ in range(2))
    assert p.poses.tobytes() == q.poses.tobytes()
    eng.group_ping_information([e], ba, SIGMA, R_MAX, OFF)
    assert e.get_particles().tobytes() == soa0 and e.get_log_weights().tobytes() == lw0


@pytest.mark.parametrize('group', ['1', '7', '10'])
def test_the_group_size_does_not_change_a_bit(world, eng, monkeypatch, group):
    ref_e, _ = world['grid']
    ba = synth.beam_angles(300)
    poses = np.ascontiguousarray(world['soa'][:, :135])
    want = _info(ref_e, 300, jump_max=1.0, dump=True)
    want_p = ref_e.pose_information(poses, ba, SIGMA, R_MAX, OFF, jump_max=1.0)
    monkeypatch.setenv('MCL_INFORMATION_GROUP', group)       # (read when the handle is created)
    e = _engine(eng, 'grid', world['z'], world['origin'], world['soa'])
    got = _info(e, 300, jump_max=1.0, dump=True)
    got_p = e.pose_information(poses, ba, SIGMA, R_MAX, OFF, jump_max=1.0)
    e.close()
    assert got.beams.tobytes() == want.beams.tobytes() and got.ranges.tobytes() == want.ranges.tobytes()
    assert got_p.poses.tobytes() == want_p.poses.tobytes()


@pytest.mark.parametrize('kind', ['grid', 'tin'])
def test_two_shards_merged_equal_the_unsharded_record(world, eng, kind):
    whole, _ = world[kind]
    want = _info(whole, 65, jump_max=1.0)
    ba = synth.beam_angles(65)
    half = N // 2
    parts = [_engine(eng, kind, world['z'], world['origin'], np.ascontiguousarray(world['soa'][:, s * half:(s + 1) * half]),
                     rank=s, world=2, n_global=N, global_offset=s * half) for s in range(2)]
    recs = [p.ping_information(ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES, jump_max=1.0) for p in parts]
    assert [r.n_sampled for r in recs] == [293, 293] and want.n_sampled == COUNT
    assert eng.merge_information(recs).tobytes() == want.beams.tobytes()
    assert eng.merge_information(recs[::-1]).tobytes() == want.beams.tobytes()
    got = eng.group_ping_information(parts[::-1], ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES, jump_max=1.0)
    assert got.beams.tobytes() == want.beams.tobytes() and got.n_sampled == want.n_sampled
    assert got.J.tobytes() == want.J.tobytes() and got.crlb_strong == want.crlb_strong
    for p in parts:
        p.close()


# ------------------------------------------------------------------ 5. seabeds whose answer is known
# 1 m grids, identity m2o, no sensor offset, delta_xy = 0.5 and x, y on multiples of 1/8: p + delta and p - delta stand one
# whole cell apart at the same place inside their cells, and the arithmetic relative to the own cell is the same.
GRID_N, GRID_ORIGIN, Z_VEHICLE, BC_RMAX = 128, (-64.0, -64.0), -2.0, 60.0


def _built(eng, z, soa):
    e = eng.Engine(soa.shape[1], rng_mode=eng.RNG_REPLAY)
    e.set_particles(soa)
    e.set_map_grid(z.astype(np.float32), GRID_ORIGIN, 1.0)
    return e


def _eighths(rs, n, span=12.0):
    return np.round(rs.uniform(-span, span, n) * 8.0) / 8.0


def _cloud(seed, n=N, level=True):
    rs = np.random.RandomState(seed)
    soa = np.zeros((6, n))
    soa[0], soa[1], soa[2] = _eighths(rs, n), _eighths(rs, n), Z_VEHICLE
    if not level:
        soa[3], soa[4] = 0.02 * rs.randn(n), 0.02 * rs.randn(n)
    soa[5] = rs.uniform(-math.pi, math.pi, n)
    return soa


def test_flat_seabed_fixes_nothing_horizontal(eng):
    e = _built(eng, np.full((GRID_N, GRID_N), -20.0), _cloud(11))
    B = 64
    inf = e.ping_information(synth.beam_angles(B), SIGMA, BC_RMAX, delta_xy=DELTA_XY, delta_yaw=DELTA_YAW)
    e.close()
    b = inf.beams
    assert np.all(b['n'] == 4096) and not b['n_miss'].any() and not b['n_jump'].any()
    for f in ('sxx', 'syy', 'sxy', 'sxw', 'syw'):
        assert not b[f].any(), f
    assert inf.rank_pos == 0 and inf.crlb_weak == math.inf and inf.crlb_strong == math.inf and inf.hit_share == 1.0
    # yaw moves no ray of a level vehicle over a level seabed: each difference is within the contract and the quantum
    bound = B * DIFF_TOL ** 2 / (4.0 * DELTA_YAW ** 2 * SIGMA ** 2)
    print('flat: J_ww %.3e (bound %.3e)' % (inf.J[5], bound))
    assert 0.0 <= inf.J[5] <= bound


def test_ridge_fixes_the_across_ridge_coordinate_only(eng):
    ix = np.arange(GRID_N, dtype=np.float64) + GRID_ORIGIN[0]
    z = np.repeat((-20.0 + 3.0 * np.sin(ix / 6.0) + 0.05 * ix)[:, None], GRID_N, axis=1)      # z a function of x only
    e = _built(eng, z, _cloud(12, level=False))
    ba = synth.beam_angles(64)
    inf = e.ping_information(ba, SIGMA, BC_RMAX, delta_xy=DELTA_XY, delta_yaw=DELTA_YAW)
    b = inf.beams
    assert np.all(b['n'] == 4096) and not b['n_miss'].any()
    for f in ('syy', 'sxy', 'syw'):
        assert not b[f].any(), f
    assert np.all(b['sxx'] > 0) and b['sww'].any()
    assert inf.rank_pos == 1 and inf.weak_axis == math.pi / 2 and math.isfinite(inf.crlb_strong) and inf.crlb_weak == math.inf
    print('ridge: crlb_strong %.4f m, J %s' % (inf.crlb_strong, inf.J))
    # the raster of the same map, run 64 m past its edge: every interior cell says the same; cells past the edge see nothing
    r = eng.localisability_map(e, 8.0, Z_VEHICLE, [0.0, 0.7], ba, SIGMA, BC_RMAX, margin=64.0)
    e.close()
    assert r['crlb_weak'].shape == r['weak_axis'].shape == r['hit_share'].shape == r['crlb_strong'].shape == (31, 31)
    assert r['x'][0] == -124.0 and r['x'][13] == -20.0 and r['y'][17] == 12.0
    inner = (slice(13, 18), slice(13, 18))          # cells whose whole swath lies on the map
    assert np.all(r['hit_share'][inner] == 1.0) and np.all(r['weak_axis'][inner] == math.pi / 2)
    assert np.all(np.isinf(r['crlb_weak'][inner])) and np.all(np.isfinite(r['crlb_strong'][inner]))
    far = np.ones((31, 31), bool)                   # cells 52 m and more past the edge: r_max sin(60 deg), the swath's reach
    far[2:30, 2:30] = False
    assert np.all(r['hit_share'][far] == 0.0) and np.all(np.isinf(r['crlb_strong'][far])) and np.all(np.isinf(r['crlb_weak'][far]))


def _rot(roll, pitch, yaw):
    sr, cr, sp, cp, sy, cy = math.sin(roll), math.cos(roll), math.sin(pitch), math.cos(pitch), math.sin(yaw), math.cos(yaw)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


PLANE_N = np.array([-0.25, -0.125, 1.0])         # z = -20 + 0.25 x + 0.125 y:  n . X = -20
PLANE_POSES = np.array([[3.0, -2.125, Z_VEHICLE, 0.01, -0.01, 0.4], [-5.5, 4.25, Z_VEHICLE, -0.03, 0.02, 2.1],
                        [0.0, 0.0, Z_VEHICLE, 0.0, 0.0, -1.3]]).T


def _plane():
    ix = np.arange(GRID_N, dtype=np.float64) + GRID_ORIGIN[0]
    return -20.0 + 0.25 * ix[:, None] + 0.125 * ix[None, :]


def _plane_gradients(eng, pose, ba):
    """(g_x, g_y, g_w) per beam at one pose: g_x = -n_x / (n.d), g_y = -n_y / (n.d), g_w = -n.(z^ x (hit - p)) / (n.d)"""
    d = _rot(*pose[3:]).dot(eng.innovation_dirs(ba).astype(np.float64).T)             # 3 x B, map frame
    nd = PLANE_N.dot(d)
    r = (-20.0 - PLANE_N.dot(pose[:3])) / nd
    lever = r * d                                                                      # hit - p
    return np.stack([-PLANE_N[0] / nd, -PLANE_N[1] / nd, -(PLANE_N[0] * -lever[1] + PLANE_N[1] * lever[0]) / nd])


def _j_bounds(g, tol, sigma):
    """from the analytic gradients g (3 x B) and the allowed error of each quantised difference tol (3 x B, metres): the
    analytic J (packed) and what each entry of the measured J may be off by"""
    dl = np.array([DELTA_XY, DELTA_XY, DELTA_YAW])
    T = 2.0 * dl[:, None] * g                                                          # the true differences, metres
    J, slack = [], []
    for j, k in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        scale = 4.0 * dl[j] * dl[k] * sigma * sigma
        J.append(float(np.sum(T[j] * T[k]) / scale))
        slack.append(float(np.sum(np.abs(T[j]) * tol[k] + np.abs(T[k]) * tol[j] + tol[j] * tol[k]) / scale))
    return np.array(J), np.array(slack)


def test_tilted_plane_against_the_analytic_gradients(eng, orc):
    """z = -20 + 0.25 x + 0.125 y.  The range is linear in x and y, so their central differences are the derivative; for yaw
    the oracle's own secant-versus-derivative gap is added beam by beam.  Each quantised difference may be off by DIFF_TOL."""
    z = _plane()
    e = _built(eng, z, PLANE_POSES.copy())
    ba = synth.beam_angles(64, math.pi / 4)
    got = e.pose_information(PLANE_POSES, ba, SIGMA, BC_RMAX, delta_xy=DELTA_XY, delta_yaw=DELTA_YAW)
    e.close()
    omap = orc.Grid(z.astype(np.float32), GRID_ORIGIN, 1.0)
    assert np.all(got.poses['n'] == 64) and not got.poses['n_miss'].any() and not got.poses['n_jump'].any()
    for k in range(PLANE_POSES.shape[1]):
        pose = PLANE_POSES[:, k]
        g = _plane_gradients(eng, pose, ba)
        ex = [orc.mbes_update(perturbed(pose[:, None], v), np.identity(4), [0] * 6, omap, ba, None, SIGMA, BC_RMAX)[1][0] for v in range(6)]
        secant = np.stack([(ex[0] - ex[1]) / (2 * DELTA_XY), (ex[2] - ex[3]) / (2 * DELTA_XY), (ex[4] - ex[5]) / (2 * DELTA_YAW)])
        gap = np.abs(secant - g)
        print('plane pose %d: oracle secant vs analytic: x %.2e, y %.2e, yaw %.2e' % (k, gap[0].max(), gap[1].max(), gap[2].max()))
        assert gap[0].max() < 1e-6 and gap[1].max() < 1e-6 and gap[2].max() < 1e-3       # the formulas are the oracle's
        tol = np.stack([np.full(64, DIFF_TOL), np.full(64, DIFF_TOL), DIFF_TOL + 2 * DELTA_YAW * gap[2]])
        J, slack = _j_bounds(g, tol, SIGMA)
        err = np.abs(got.J[k] - J)
        print('plane pose %d: J %s\n  |J - analytic| %s\n  allowed %s' % (k, got.J[k], err, slack))
        assert np.all(err <= slack)
        assert got.rank_pos[k] == 2 and math.isfinite(got.crlb_weak[k])


def test_the_filter_agrees_on_the_plane(eng):
    """-(lw+ + lw- - 2 lw0) / delta^2 of the unchanged update_mbes, for particles at p and p +- delta e_x pinged with the
    ranges expected at p, is J_xx of pose_information(p): sigma means to both what it means to the filter"""
    z = _plane()
    p = PLANE_POSES[:, 0]
    soa = np.stack([p, p, p], axis=1)
    soa[0, 1] += DELTA_XY
    soa[0, 2] -= DELTA_XY
    e = _built(eng, z, soa)
    B = 64
    ba = synth.beam_angles(B, math.pi / 4)
    ranges = e.mbes_expected(0, 1, ba, BC_RMAX)[0].astype(np.float32)
    assert ranges.max() < BC_RMAX - 1.0
    e.update_mbes(ranges, ba, SIGMA, BC_RMAX)
    lw = e.get_log_weights()
    F = -(lw[1] + lw[2] - 2.0 * lw[0]) / DELTA_XY ** 2
    got = e.pose_information(p[:, None], ba, SIGMA, BC_RMAX, delta_xy=DELTA_XY, delta_yaw=DELTA_YAW)
    e.close()
    g = np.abs(_plane_gradients(eng, p, ba)[0])
    J_true = float(np.sum(g * g)) / SIGMA ** 2
    # pose_information: the bound of the plane test, entry xx
    slack_J = float(np.sum(2 * (2 * DELTA_XY * g) * DIFF_TOL + DIFF_TOL ** 2)) / (4 * DELTA_XY ** 2 * SIGMA ** 2)
    # the filter: every residual r - e is two ranges within 1e-3 m of the truth each; the terms are summed in fp32
    eta = 2e-3
    slack_F = float(np.sum(2 * (2 * DELTA_XY * g * eta + eta ** 2) + 2 * eta ** 2)) / (2 * SIGMA ** 2 * DELTA_XY ** 2)
    slack_F += B * 2.0 ** -23 * 4 * float(np.sum((DELTA_XY * g + eta) ** 2)) / (2 * SIGMA ** 2 * DELTA_XY ** 2)
    print('filter: F %.6f, J_xx %.6f, analytic %.6f, allowed %.4f + %.4f' % (F, got.J[0, 0], J_true, slack_F, slack_J))
    assert abs(F - J_true) <= slack_F and abs(got.J[0, 0] - J_true) <= slack_J
    assert abs(F - got.J[0, 0]) <= slack_F + slack_J


# ------------------------------------------------------------------ 6. errors
def test_argument_and_state_errors(world, eng):
    e, _ = world['grid']
    ba = synth.beam_angles(64)
    poses = np.ascontiguousarray(world['soa'][:, :4])

    def status(f, *a, **k):
        with pytest.raises(eng.MclError) as ei:
            f(*a, **k)
        return ei.value.status

    for f, head in ((e.ping_information, ()), (e.pose_information, (poses,))):
        assert status(f, *head, ba, SIGMA, 4096.5) == -1                              # r_max beyond the quantised range
        assert status(f, *head, ba, SIGMA, 0.0) == -1
        assert status(f, *head, ba, SIGMA, 4096.0, jump_max=2048.5) == -1
        assert status(f, *head, ba, SIGMA, R_MAX, jump_max=R_MAX + 1.0) == -1
        assert status(f, *head, ba, SIGMA, R_MAX, jump_max=0.0) == -1
        assert status(f, *head, ba, SIGMA, R_MAX, delta_xy=0.0) == -1
        assert status(f, *head, ba, SIGMA, R_MAX, delta_xy=-0.5) == -1
        assert status(f, *head, ba, SIGMA, R_MAX, delta_yaw=0.0) == -1
        assert status(f, *head, ba, SIGMA, R_MAX, delta_yaw=math.nan) == -1
        assert status(f, *head, ba, 0.0, R_MAX) == -1                                 # sigma: the derived part refuses it
        assert status(f, *head, ba, -1.0, R_MAX) == -1
        bad = ba.copy()
        bad[3] = np.nan
        assert status(f, *head, bad, SIGMA, R_MAX) == -1
        assert status(f, *head, np.zeros(2049, np.float32), SIGMA, R_MAX) == -1
    assert status(e.ping_information, ba, SIGMA, R_MAX, max_samples=0) == -1
    assert status(e.ping_information, ba, SIGMA, R_MAX, max_samples=32769) == -1
    assert status(e.pose_information, np.zeros((6, 0)), ba, SIGMA, R_MAX) == -1
    assert status(e.pose_information, np.zeros((6, (1 << 20) + 1)), ba, SIGMA, R_MAX) == -1
    nanpose = poses.copy()
    nanpose[5, 2] = np.nan
    assert status(e.pose_information, nanpose, ba, SIGMA, R_MAX) == -1
    # the bounds themselves
    assert e.ping_information(ba, SIGMA, 4096.0, max_samples=32768, jump_max=2048.0).n_sampled == N
    assert e.ping_information(np.zeros(1, np.float32), SIGMA, R_MAX).beams.size == 1
    bare = eng.Engine(16)
    assert status(bare.pose_information, poses, ba, SIGMA, R_MAX) == -5               # no map
    bare.init_particles()
    assert status(bare.ping_information, ba, SIGMA, R_MAX) == -5                      # no map
    bare.close()
    mapped = eng.Engine(16, m2o=M2O)
    mapped.set_map_grid(world['z'], world['origin'], 1.0)
    assert status(mapped.ping_information, ba, SIGMA, R_MAX, OFF) == -5               # a map, no particles
    free = mapped.pose_information(poses, ba, SIGMA, R_MAX, OFF, jump_max=1.0)        # ... which the poses do not need
    mapped.close()
    assert free.poses.tobytes() == e.pose_information(poses, ba, SIGMA, R_MAX, OFF, jump_max=1.0).poses.tobytes()


def test_the_largest_pose_count_runs(world):
    e, _ = world['grid']
    M = 1 << 20
    poses = np.ascontiguousarray(np.tile(world['soa'][:, :1024], (1, M // 1024)))
    got = e.pose_information(poses, np.zeros(1, np.float32), SIGMA, R_MAX, OFF)
    assert got.poses.size == M and np.all(got.poses['n'] == 1)
    assert got.poses[:1024].tobytes() == got.poses[-1024:].tobytes()


# ------------------------------------------------------------------ 7. the replay
def test_replay_with_the_node_parameter_reports_the_summary_keys():
    from smarc_navigation_amd import replay
    st = replay.synthetic_stream(150, mbes_every=10, beams=64)
    params = dict(replay.SYNTH_PARAMS, particle_count=4096, mbes_information_every=5)
    s = replay.replay(st, params)['summary']
    print({k: s[k] for k in s if k.startswith('information') and k != 'information_per_ping'})
    assert s['mbes_information_every'] == 5 and s['information_pings'] == 3 == len(s['information_per_ping'])      # pings 0, 5, 10 of 15
    for k in ('information_crlb_strong_median', 'information_crlb_weak_median', 'information_rank_deficient_share',
              'information_hit_share_mean'):
        assert k in s
    assert 0.0 <= s['information_rank_deficient_share'] <= 1.0 and s['information_hit_share_mean'] > 0.5
    assert s['information_crlb_strong_median'] > 0.0
