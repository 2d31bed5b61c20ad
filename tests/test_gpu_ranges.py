"""GPU tests of the DVL / altimeter range update (mcl_update_ranges, mcl_ranges_expected; mcl_ranges.h): a few rays in
any direction per particle against the bathymetric map, checked against the fp64 oracle's ray casts (oracle.Grid.ray,
oracle.Mesh.ray) on every map storage the handle keeps, for accumulation onto other updates, for determinism under
sharding and permutation, in a closed loop, and at full size.  Precision contract of mcl_update_mbes (include/mcl.h)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from smarc_navigation_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA, R_MAX = 0.2, 60.0
OFF = [0.3, -0.1, -0.2, 0.03, -0.05, 0.08]   # a DVL mounted with a small rotation


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def _janus(tilt_deg=25.0):
    t = math.radians(tilt_deg)
    return np.array([[math.sin(t) * math.cos(a), math.sin(t) * math.sin(a), -math.cos(t)]
                     for a in (0.25 * math.pi, 0.75 * math.pi, 1.25 * math.pi, 1.75 * math.pi)], np.float32)


def _rot(r, p, y):
    return synth.rigid_matrix(0.0, 0.0, 0.0, r, p, y)[:3, :3]


def _unit(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _rays(soa, dirs, m2o, off):
    """origins (n, 3) and directions (n, B, 3) in the map frame, fp64, by the convention of orc_mbes_update"""
    m2o = np.asarray(m2o, np.float64)
    Rm, Ro = m2o[:3, :3], _rot(*off[3:])
    n = soa.shape[1]
    o = np.zeros((n, 3))
    d = np.zeros((n, len(dirs), 3))
    dd = np.asarray(dirs, np.float64)
    for i in range(n):
        Rmp = Rm.dot(_rot(soa[3, i], soa[4, i], soa[5, i]))
        o[i] = m2o[:3, :3].dot(soa[:3, i]) + m2o[:3, 3] + Rmp.dot(off[:3])
        d[i] = dd.dot(Rmp.dot(Ro).T)
    return o, d


def _oracle_ranges(omap, o, d, r_max):
    n, B = d.shape[:2]
    out = np.zeros((n, B))
    for i in range(n):
        for b in range(B):
            out[i, b] = omap.ray(o[i], d[i, b], r_max)
    return out


def _explained(omap, o, d, got, ref, r_max, tol=1e-3, delta=1e-3):
    """rays beyond tol whose GPU range the fp64 definition itself gives for a sensor moved by 1 mm (grazing rays)"""
    bad = np.argwhere(np.abs(got - ref) > tol)
    ok = np.ones(len(bad), bool)
    for k, (i, b) in enumerate(bad):
        hits = [abs(omap.ray(o[i] + delta * s, d[i, b], r_max) - got[i, b]) <= tol for s in np.vstack([np.eye(3), -np.eye(3)])]
        ok[k] = any(hits)
    return bad, ok


def _lw_ref(ranges, e, sigma):
    valid = (ranges > 0) & ~np.isnan(ranges)
    dr = np.where(valid[None, :], (ranges.astype(np.float64)[None, :] - e) / sigma, 0.0)
    return -0.5 * np.sum(dr * dr, axis=1) - valid.sum() * math.log(sigma * math.sqrt(2 * math.pi))


def _lw_ok(lw, ref):
    d = np.abs(lw - ref)
    return (d <= 1e-2) | (d <= 2e-4 * np.abs(ref))


# ------------------------------------------------------------------ 1. known answers
@pytest.mark.parametrize('kind', ['grid', 'mesh', 'tin'])
def test_flat_seabed_known_answers(eng, kind):
    origin, nx = (-48.0, -48.0), 97
    z = np.full((nx, nx), -30.0, np.float32)
    n = 16
    soa = np.zeros((6, n))
    soa[0] = np.linspace(-20, 20, n)
    soa[1] = np.linspace(10, -10, n)
    soa[2] = -4.0
    soa[5] = np.linspace(-3, 3, n)   # yaw does not matter on a flat bottom
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
    e.set_particles(soa)
    if kind == 'grid':
        e.set_map_grid(z, origin, 1.0)
    else:
        v, t = synth.mesh_from_grid(z, 1.0, origin)
        if kind == 'tin':
            v, t = synth.mesh_tin(z, 1.0, origin, seed=3)
        e.set_map_mesh(v, t)
    alt = e.ranges_expected(0, n, [[0, 0, -1]], R_MAX)
    np.testing.assert_allclose(alt, 26.0, rtol=0, atol=2e-4)
    jan = e.ranges_expected(0, n, _janus(25.0), R_MAX)
    np.testing.assert_allclose(jan, 26.0 / math.cos(math.radians(25.0)), rtol=0, atol=3e-4)
    # a direction of any length is normalised; up, or out of the map before the bottom: r_max
    np.testing.assert_allclose(e.ranges_expected(0, n, [[0, 0, -7.5]], R_MAX), 26.0, rtol=0, atol=2e-4)
    assert np.all(e.ranges_expected(0, n, [[0.1, 0.2, 1.0]], R_MAX) == R_MAX)
    assert np.all(e.ranges_expected(0, n, [[1.0, 0.0, -0.05]], 500.0) == 500.0)   # leaves the 96 m map 5 m down
    # the same through the update: the altitude itself gives the largest log-likelihood, the offset of one beam counts
    e.update_ranges([26.0], [[0, 0, -1]], SIGMA, R_MAX)
    lw = e.get_log_weights()
    np.testing.assert_allclose(lw, -math.log(SIGMA * math.sqrt(2 * math.pi)), rtol=0, atol=1e-6)
    e.update_ranges([26.2, 0.0, float('nan'), 26.0], [[0, 0, -1]] * 4, SIGMA, R_MAX)   # two invalid beams skipped
    np.testing.assert_allclose(e.get_log_weights(), -0.5 - 2 * math.log(SIGMA * math.sqrt(2 * math.pi)), rtol=0, atol=5e-3)


def test_argument_and_state_errors(eng):
    e = eng.Engine(8)
    e.init_particles()
    with pytest.raises(eng.MclError) as ei:
        e.update_ranges([10.0], [[0, 0, -1]], SIGMA, R_MAX)
    assert ei.value.status == -5   # no map
    e.set_map_grid(np.full((16, 16), -20.0, np.float32), (-8.0, -8.0), 1.0)
    with pytest.raises(eng.MclError) as ei:
        e.update_ranges([10.0], [[0, 0, -1]], SIGMA, R_MAX, accumulate=True)
    assert ei.value.status == -5   # nothing to accumulate onto
    for ranges, dirs, sigma, r_max in (([10.0] * 17, [[0, 0, -1]] * 17, SIGMA, R_MAX), ([10.0], [[0, 0, 0]], SIGMA, R_MAX),
                                       ([10.0], [[0, float('nan'), -1]], SIGMA, R_MAX), ([10.0], [[0, float('inf'), -1]], SIGMA, R_MAX),
                                       ([10.0], [[0, 0, -1]], 0.0, R_MAX), ([10.0], [[0, 0, -1]], SIGMA, 0.0)):
        with pytest.raises(eng.MclError) as ei:
            e.update_ranges(ranges, dirs, sigma, r_max)
        assert ei.value.status == -1
    lib = e.lib
    d = np.zeros(3, np.float32)
    r = np.ones(1, np.float32)
    assert lib.mcl_update_ranges(e.h, r.ctypes.data, d.ctypes.data, 0, SIGMA, R_MAX, None, 0) == -1
    assert lib.mcl_update_ranges(e.h, None, d.ctypes.data, 1, SIGMA, R_MAX, None, 0) == -1
    with pytest.raises(eng.MclError):
        e.ranges_expected(4, 8, [[0, 0, -1]], R_MAX)   # past the end of the cloud


# ------------------------------------------------------------------ 2. parity with the fp64 oracle
def _terrain(n=160, seed=5):
    origin = (-80.0, -80.0)
    return synth.bathymetry_grid(n, n, 1.0, origin, seed=seed), origin


def _parity_map(kind, orc):
    z, origin = _terrain()
    if kind == 'grid':
        return dict(z=z, origin=origin), orc.Grid(z, origin, 1.0)
    if kind in ('mesh', 'mesh2'):
        v, t = synth.mesh_from_grid(z, 1.0, origin, diagonal='00-11' if kind == 'mesh' else '10-01')
    elif kind == 'soup':   # a terrain with a vertical wall standing on it and a deck floating above it
        v, t = synth.mesh_from_grid(z, 1.0, origin)
        nv = v.shape[0]
        wall = np.array([[10.0, -20.0, -30.0], [10.0, 20.0, -30.0], [10.0, 20.0, -8.0], [10.0, -20.0, -8.0]], np.float32)
        deck = np.array([[-25.0, -15.0, -12.0], [-5.0, -15.0, -12.5], [-5.0, 15.0, -12.0], [-25.0, 15.0, -11.5]], np.float32)
        v = np.vstack([v, wall, deck]).astype(np.float32)
        t = np.vstack([t, np.array([[nv, nv + 1, nv + 2], [nv, nv + 2, nv + 3], [nv + 4, nv + 5, nv + 6], [nv + 4, nv + 6, nv + 7]],
                                   np.uint32)])
    else:
        v, t = synth.mesh_tin(z, 1.0, origin, seed=7)
        if kind in ('holes', 'ragged'):
            c = v[t.astype(np.int64)].mean(axis=1)
            gone = np.zeros(len(t), bool)
            rs = np.random.RandomState(4)
            for _ in range(12):
                p = rs.uniform(-40, 40, 2)
                gone |= np.hypot(c[:, 0] - p[0], c[:, 1] - p[1]) < rs.uniform(0.8, 3.0)
            t = np.ascontiguousarray(t[~gone])
            if kind == 'ragged':
                t = synth.mesh_ragged(v, t, seed=13, band=3.0, bays=6, bay_width=(2.0, 5.0), bay_depth=(8.0, 30.0))
    return dict(verts=v, tris=t), orc.Mesh(v, t)


def _parity_cloud(n, seed):
    """diving attitudes, random yaw; most particles over the map, some over its border and some off it"""
    rs = np.random.RandomState(seed)
    soa = np.zeros((6, n))
    soa[0] = rs.uniform(-70, 70, n)
    soa[1] = rs.uniform(-70, 70, n)
    edge = rs.rand(n) < 0.15
    soa[0][edge] = rs.choice([-1, 1], edge.sum()) * rs.uniform(76, 84, edge.sum())
    off = rs.rand(n) < 0.05
    soa[1][off] = rs.choice([-1, 1], off.sum()) * rs.uniform(85, 120, off.sum())
    soa[2] = rs.uniform(-6.0, -0.5, n)
    soa[3] = rs.uniform(-0.3, 0.3, n)
    soa[4] = rs.uniform(-0.6, 0.6, n)
    soa[5] = rs.uniform(-np.pi, np.pi, n)
    return soa


def _random_dirs(B, seed):
    rs = np.random.RandomState(seed)
    d = rs.randn(B, 3)
    d[:, 2] = -np.abs(d[:, 2]) * 1.5   # mostly down, some nearly horizontal
    if B >= 4:
        d[1] = [0.2, -0.1, 1.0]         # one looks up
    return _unit(d)


@pytest.mark.parametrize('kind', ['grid', 'mesh', 'mesh2', 'tin', 'holes', 'ragged', 'soup'])
def test_parity_with_the_fp64_oracle(eng, orc, kind):
    amap, omap = _parity_map(kind, orc)
    m2o = synth.rigid_matrix(1.5, -2.0, 0.0, 0.0, 0.0, 0.3)
    n = 4096
    soa = _parity_cloud(n, seed=len(kind))
    e = eng.Engine(n, m2o=m2o, rng_mode=eng.RNG_REPLAY)
    e.set_particles(soa)
    if 'z' in amap:
        e.set_map_grid(amap['z'], amap['origin'], 1.0)
    else:
        e.set_map_mesh(amap['verts'], amap['tris'])
    total = bad_total = 0
    for B in (1, 4, 16):
        dirs = _random_dirs(B, seed=B) if B != 1 else np.array([[0.0, 0.0, -1.0]], np.float32)
        got = e.ranges_expected(0, n, dirs, R_MAX, OFF).astype(np.float64)
        o, d = _rays(soa, dirs, m2o, OFF)
        ref = _oracle_ranges(omap, o, d, R_MAX)
        bad, ok = _explained(omap, o, d, got, ref, R_MAX)
        total += got.size
        bad_total += len(bad)
        print('%s B=%d: max |range error| %.3e m over %d rays, %d beyond 1e-3 (%d explained by a 1 mm shift); hits %.2f' % (
            kind, B, np.abs(got - ref).max(), got.size, len(bad), ok.sum(), (ref < R_MAX).mean()))
        assert ok.all(), [(i, b, got[i, b], ref[i, b]) for (i, b), k in zip(bad, ok) if not k][:5]
        assert (ref < R_MAX).mean() > 0.3 and (ref == R_MAX).any()
        # the update: measured = particle 7's expected ranges + noise, some beams invalid
        rs = np.random.RandomState(B)
        ranges = (ref[7] + SIGMA * rs.randn(B)).astype(np.float32)
        if B == 16:
            ranges[[2, 9]] = 0.0
            ranges[5] = np.nan
            ranges[11] = -3.0
        e.update_ranges(ranges, dirs, SIGMA, R_MAX, OFF)
        lw = e.get_log_weights()
        exp_ok = ref.copy()
        exp_ok[tuple(bad.T)] = got[tuple(bad.T)]   # (the explained grazing rays: the answer of the shifted sensor)
        lw_ref = _lw_ref(ranges, exp_ok, SIGMA)
        good = _lw_ok(lw, lw_ref)
        print('   lw: max |d| %.3e, max rel %.3e' % (np.abs(lw - lw_ref).max(), (np.abs(lw - lw_ref) / np.abs(lw_ref)).max()))
        assert good.all(), np.argwhere(~good)[:5]
        # and exactly the fp64 sum over the GPU's own expected ranges
        np.testing.assert_allclose(lw, _lw_ref(ranges, got, SIGMA), rtol=1e-12, atol=1e-9)
    assert bad_total <= max(3, total * 5e-4), bad_total


# ------------------------------------------------------------------ 3. accumulation
def test_accumulates_onto_mbes_and_under_landmarks(eng, orc):
    z, origin = _terrain()
    n = 8192
    rs = np.random.RandomState(3)
    soa = _parity_cloud(n, 3)
    ba = synth.beam_angles(64)
    mk = lambda: eng.Engine(n, rng_mode=eng.RNG_REPLAY)   # noqa: E731
    e, f = mk(), mk()
    for x in (e, f):
        x.set_particles(soa)
        x.set_map_grid(z, origin, 1.0)
    ping = (e.mbes_expected(0, 1, ba, 80.0)[0] + 0.2 * rs.randn(64)).astype(np.float32)
    dirs = _janus()
    dvl = (e.ranges_expected(0, 1, dirs, R_MAX)[0] + 0.1 * rs.randn(4)).astype(np.float32)
    e.update_mbes(ping, ba, 0.2, 80.0)
    lw_mbes = e.get_log_weights()
    e.update_ranges(dvl, dirs, SIGMA, R_MAX, OFF, accumulate=True)
    lw_sum = e.get_log_weights()
    f.update_ranges(dvl, dirs, SIGMA, R_MAX, OFF)
    lw_dvl = f.get_log_weights()
    assert np.array_equal(lw_sum, lw_mbes + lw_dvl)
    assert np.std(lw_dvl) > 1.0   # the DVL term discriminates
    # landmarks on top of both
    lm = synth.landmark_map(512, (-80.0, -80.0, 80.0, 80.0))
    det = lm[:3] - soa[:3, 0] + 0.05 * rs.randn(3, 3)
    e.set_landmarks(lm)
    e.update_landmarks(det, 0.3, k=2, gate=11.345, accumulate=True)
    lw3 = e.get_log_weights()
    ref = orc.landmark_update(soa, np.identity(4), [0] * 6, lm, det, 0.3, 2, 11.345)
    np.testing.assert_allclose(lw3 - lw_sum, ref, rtol=1e-9, atol=1e-7)
    # and the other way round: ranges accumulated onto a landmark update
    f.set_landmarks(lm)
    f.update_landmarks(det, 0.3, k=2, gate=11.345)
    lw_lm = f.get_log_weights()
    f.update_ranges(dvl, dirs, SIGMA, R_MAX, OFF, accumulate=True)
    assert np.array_equal(f.get_log_weights(), lw_lm + lw_dvl)


# ------------------------------------------------------------------ 4. determinism
COV = dict(init_cov=[4.0, 4.0, 0.0, 0.0, 0.0, 0.05], process_cov=[1e-3, 1e-3, 0.0, 0.0, 0.0, 1e-5],
           resample_cov=[1e-2, 1e-2, 0.0, 0.0, 0.0, 1e-4])


def test_runs_permutations_and_shards_give_the_same_bits(eng, orc):
    z, origin = _terrain()
    v, t = synth.mesh_tin(z, 1.0, origin, seed=7)
    n = 6144
    soa = _parity_cloud(n, 11)
    dirs = _random_dirs(5, 2)
    ranges = np.array([12.0, 0.0, 9.5, 30.0, 15.0], np.float32)
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
    e.set_map_mesh(v, t)
    e.set_particles(soa)
    e.update_ranges(ranges, dirs, SIGMA, R_MAX, OFF)
    lw1 = e.get_log_weights()
    e.update_ranges(ranges, dirs, SIGMA, R_MAX, OFF)
    assert np.array_equal(e.get_log_weights(), lw1)
    perm = np.random.RandomState(1).permutation(n)
    e.set_particles(np.ascontiguousarray(soa[:, perm]))
    e.update_ranges(ranges, dirs, SIGMA, R_MAX, OFF)
    assert np.array_equal(e.get_log_weights(), lw1[perm])
    e.close()
    # three shards of a NATIVE-rng filter against the unsharded one: log-likelihoods, then indices and states
    shards, NS = 3, 4096
    N = shards * NS
    m2o = synth.rigid_matrix(10.0, 5.0, 0.0, 0.0, 0.0, 0.0)
    one = eng.Engine(N, seed=5, m2o=m2o, **COV)
    many = [eng.Engine(NS, rank=r, world=shards, n_global=N, global_offset=r * NS, seed=5, m2o=m2o, **COV) for r in range(shards)]
    q = orc.quat_from_euler(0.05, -0.3, 0.4)
    dv = _janus()
    for x in [one] + many:
        x.set_map_mesh(v, t)
        x.init_particles()
    for step in range(3):
        for x in [one] + many:
            x.predict([1.0, 0.05, 0.0], 0.02, q, -3.0, 0.5)
            x.update_ranges([14.0, 13.0, 0.0, 15.5], dv, SIGMA, R_MAX, OFF)
        assert np.array_equal(one.get_log_weights(), np.concatenate([x.get_log_weights() for x in many])), step
        one.resample()
        eng.group_resample(many)
        assert np.array_equal(one.last_indices(), np.concatenate([x.last_indices() for x in many])), step
        assert np.array_equal(one.get_particles(), np.concatenate([x.get_particles() for x in many], axis=1)), step


# ------------------------------------------------------------------ 5. resampling after a DVL-only update
def test_resample_after_a_dvl_only_update_is_the_fixed_point_systematic(eng, orc):
    z, origin = _terrain()
    n = 16384
    e = eng.Engine(n, seed=11, **COV)
    e.set_map_grid(z, origin, 1.0)
    e.init_particles()
    e.predict([1.0, 0.0, 0.0], 0.0, orc.quat_from_euler(0.0, 0.1, 0.2), -2.5, 0.1)
    e.update_ranges([17.0, 18.5, 0.0, 18.0], _janus(), SIGMA, R_MAX)
    lw = e.get_log_weights()
    assert np.isfinite(lw).all() and np.std(lw) > 1.0
    e.resample()
    ref, _, _ = orc.systematic_fixed(lw, 1, orc.native_u53(11, 0))
    assert np.array_equal(e.last_indices(), ref)


# ------------------------------------------------------------------ 6. closed loop: terrain-aided navigation
def test_dvl_aided_filter_beats_odometry_alone_on_a_tin(eng):
    """A seeded track over an irregular TIN; the filter's odometry over-reads the speed by 8 % and drifts sideways by
    4 cm/s.  With the DVL's four Janus ranges against the map (2 Hz, no GPS, no MBES) the mean pose stays on the track;
    on odometry alone it drifts.  Measured run recorded in DESIGN.md 5c."""
    origin = (-64.0, -128.0)
    z = synth.bathymetry_grid(256, 256, 1.0, origin, seed=21)
    v, t = synth.mesh_tin(z, 1.0, origin, seed=7)
    steps, every = 600, 5
    st = synth.odom_stream(steps, dt=0.1, z_mean=-4.0)
    truth = st['truth']
    dirs = _janus()
    one = eng.Engine(1, rng_mode=eng.RNG_REPLAY)
    one.set_map_mesh(v, t)
    rs = np.random.RandomState(12)
    meas = {}
    for k in range(every - 1, steps, every):
        one.set_particles(truth[k][:, None].copy())
        meas[k] = (one.ranges_expected(0, 1, dirs, R_MAX)[0] + 0.05 * rs.randn(4)).astype(np.float32)
    one.close()
    cov = dict(init_cov=[1.0, 1.0, 0.0, 0.0, 0.0, 0.001], process_cov=[2e-3, 2e-3, 0.0, 0.0, 0.0, 1e-6],
               resample_cov=[2e-3, 2e-3, 0.0, 0.0, 0.0, 1e-6])
    err = {}
    for aided in (False, True):
        e = eng.Engine(16384, seed=3, **cov)
        e.set_map_mesh(v, t)
        e.init_particles()
        for k in range(steps):
            vb = st['v'][k] * np.array([1.08, 1.0, 1.0]) + np.array([0.0, 0.04, 0.0])
            e.predict(vb, st['wz'][k], st['q'][k], st['z'][k], st['dt'])
            if aided and k in meas:
                e.update_ranges(meas[k], dirs, 0.2, R_MAX)
                e.resample()
        mean = e.mean_cov()[0]
        err[aided] = float(np.hypot(mean[0] - truth[-1][0], mean[1] - truth[-1][1]))
        e.close()
    print('final mean-pose error: odometry only %.2f m, DVL-aided %.2f m' % (err[False], err[True]))
    assert err[False] > 3.0
    assert err[True] < 0.35 * err[False]


# ------------------------------------------------------------------ 7. size and speed
def test_full_size_one_million_particles_four_beams(eng, orc):
    origin = (-64.0, -256.0)
    z = synth.bathymetry_grid(512, 512, 1.0, origin, seed=3)
    n = 1 << 20
    rs = np.random.RandomState(2)
    soa = np.zeros((6, n))
    soa[0], soa[1] = rs.uniform(-80, 460, n), rs.uniform(-270, 270, n)   # (some over the border and beyond)
    soa[2] = rs.uniform(-5, -1, n)
    soa[3], soa[4], soa[5] = rs.uniform(-0.3, 0.3, n), rs.uniform(-0.6, 0.6, n), rs.uniform(-np.pi, np.pi, n)
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
    e.set_map_grid(z, origin, 1.0)
    e.set_particles(soa)
    dirs = _janus()
    ranges = np.array([18.0, 19.0, 0.0, 18.5], np.float32)
    e.update_ranges(ranges, dirs, SIGMA, R_MAX)
    lw = e.get_log_weights()
    assert np.isfinite(lw).all()
    pick = rs.choice(n, 1024, replace=False)
    sub = np.ascontiguousarray(soa[:, pick])
    o, d = _rays(sub, dirs, np.identity(4), [0.0] * 6)
    g = orc.Grid(z, origin, 1.0)
    ref = _oracle_ranges(g, o, d, R_MAX)
    got = e.ranges_expected(0, n, dirs, R_MAX)[pick].astype(np.float64)
    bad, ok = _explained(g, o, d, got, ref, R_MAX)
    assert ok.all()
    ref[tuple(bad.T)] = got[tuple(bad.T)]
    assert _lw_ok(lw[pick], _lw_ref(ranges, ref, SIGMA)).all()


def test_timing_tool_runs(eng):
    out = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'tools', 'ranges_timing.py'),
                          '--particles', '65536', '--reps', '20', '--warmup', '3', '--maps', 'grid,tin'],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=330)
    assert out.returncode == 0, out.stderr[-2000:]
    import json
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(rows) == 4 and all(r['source'].startswith('measured') and r['median_ms'] > 0 and r['lw_finite'] for r in rows)
