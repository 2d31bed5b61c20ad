"""Parity at BASELINE.json's full sizes (1 048 576 particles x 512 beams, 999 698-triangle mesh and
512x512 grid): spot checks of the HIP path against the oracle on random particle subsets, plus
size-independent properties of the resample step."""
import numpy as np
import pytest

from smarc_navigation_amd import synth

pytestmark = pytest.mark.gpu

N, B = 1 << 20, 512


def _cloud(seed):
    rs = np.random.RandomState(seed)
    soa = rs.randn(6, N) * np.array([1.5, 1.5, 0.0, 0.0, 0.0, 0.2])[:, None]
    soa[0] += 30.0
    soa[1] += -12.0
    soa[2] = -2.2
    soa[3] = 0.015
    soa[4] = -0.02
    return soa


@pytest.mark.parametrize('kind', ['mesh', 'grid', 'mesh_general', 'mesh_tin', 'mesh_tin_shuffled', 'mesh_tin_gaps', 'mesh_soup_irregular'])
def test_full_size_mbes_update_spot_check_vs_oracle(kind):
    from smarc_navigation_amd import engine as eng
    from oracle import oracle as orc
    from tests.helpers import live_particle_contract, live_picks
    ba = synth.beam_angles(B)
    if kind == 'grid':
        origin = (-64.0, -256.0)
        z = synth.bathymetry_grid(512, 512, 1.0, origin, seed=3)
        omap = orc.Grid(z, origin, 1.0)
    else:
        origin = (-64.0, -354.0)
        z = synth.bathymetry_grid(708, 708, 1.0, origin, seed=3)
        if kind in ('mesh_tin', 'mesh_tin_shuffled', 'mesh_tin_gaps', 'mesh_soup_irregular'):   # an irregular height-field TIN: the adjacency sweep (or, forced, the fan slice)
            verts, tris = synth.mesh_tin(z, 1.0, origin, seed=7)
            if kind == 'mesh_tin_gaps':   # ... with a data gap per 6 x 6 m (bench.py: punch_gaps; 13 % of the triangles missing): the walk crosses them by their rims
                import bench
                tris = bench.punch_gaps(dict(verts=verts, tris=tris, origin=origin, desc=''))['tris']
            if kind == 'mesh_tin_shuffled':   # ... in random vertex / triangle order (mesh_build's Morton pass)
                verts, tris = synth.mesh_shuffle(verts, tris, seed=9)
        else:
            verts, tris = synth.mesh_from_grid(z, 1.0, origin)
        omap = orc.Mesh(verts, tris)
    soa = _cloud(1)
    e = eng.Engine(N, rng_mode=eng.RNG_REPLAY)
    e.set_particles(soa)
    if kind == 'grid':
        e.set_map_grid(z, origin, 1.0)
    else:
        e.set_map_mesh(verts, tris, general=(kind in ('mesh_general', 'mesh_soup_irregular')))
    truth = np.array([[30.0], [-12.0], [-2.2], [0.015], [-0.02], [0.0]])
    _, ex = orc.mbes_update(truth, np.identity(4), [0] * 6, omap, ba, None, 0.2, 100.0)
    ranges = (ex[0] + 0.2 * np.random.RandomState(2).randn(B)).astype(np.float32)
    ranges[ex[0] >= 100.0] = 0.0    # (a beam that found nothing reports no range: only the TIN with gaps has such beams)
    e.update_mbes(ranges, ba, 0.2, 100.0)
    lw = e.get_log_weights()
    pick = np.random.RandomState(3).choice(N, 1024, replace=False)
    sub = np.ascontiguousarray(soa[:, pick])
    lw_ref, ex_ref = orc.mbes_update(sub, np.identity(4), [0] * 6, omap, ba, ranges, 0.2, 100.0)
    d = np.abs(lw[pick] - lw_ref)
    print('%s: full-size spot check, max |dlw| = %.3e (|lw| up to %.0f)' % (kind, d.max(), np.abs(lw_ref).max()))
    okm = (d <= 1e-2) | (d <= 2e-4 * np.abs(lw_ref))
    if kind == 'mesh_tin_gaps':
        # a surface with gaps is not continuous: a ray within rounding of a rim hits the seabed in one arithmetic and looks into
        # the gap in the other (here: 20 m against r_max, half of (80 / 0.2)^2 in the log-likelihood) -- every ping has ~ 70 rim
        # passages per particle.  Such particles must be FEW and each must carry an answer the oracle itself gives under a
        # 1 mm shift of the sensor
        from tests.helpers import lw_outliers_explained
        assert (~okm).sum() <= pick.size // 25, int((~okm).sum())
        lw_outliers_explained(orc, omap, sub, ba, ranges, 0.2, 100.0, lw[pick], lw_ref, label='mesh_tin_gaps 1 M x 512')
    else:
        assert np.all(okm)
    path, handed, _ = e.mbes_last_path()
    assert path == {'mesh_general': 2, 'mesh_soup_irregular': 2}.get(kind, 1), path   # fan sweep (1) / fan slice (2)
    if kind == 'mesh_tin_gaps':
        print('mesh_tin_gaps: the sweep handed over %d of %d particles (%d beams of the ping look into a gap)' % (handed, N, int((ex[0] >= 100.0).sum())))
        assert handed < N // 20
    # the contract where it bites: the particles that can receive offspring (lw >= max - 30) within |d| <= 1e-2 ABSOLUTE
    live = live_picks(lw, 1024, seed=6)
    lsub = np.ascontiguousarray(soa[:, live])
    lw_live, _ = orc.mbes_update(lsub, np.identity(4), [0] * 6, omap, ba, ranges, 0.2, 100.0)
    n_live, _, _ = live_particle_contract(orc, omap, lsub, ba, ranges, 0.2, 100.0, lw[live], lw_live, float(lw.max()),
                                          label='%s 1 M x 512' % kind)
    assert n_live >= 16
    got = e.mbes_expected(int(pick[0]), 1, ba, 100.0)
    assert np.abs(got[0] - ex_ref[0]).max() <= 1e-3
    # the update discriminates: the best particles are the ones nearest to the truth
    best = np.argsort(lw)[-100:]
    # (with gaps the likelihood has cliffs -- a valid beam of a displaced particle falls into a gap -- and the hundred best spread wider)
    assert np.median(np.hypot(soa[0, best] - 30.0, soa[1, best] + 12.0)) < (0.8 if kind == 'mesh_tin_gaps' else 0.3)


@pytest.mark.parametrize('kind', ['mesh', 'grid', 'mesh_general', 'mesh_tin'])
def test_full_size_log_likelihood_is_additive_over_the_beams_of_a_ping(kind):
    """A size-independent property over ALL 1 048 576 particles (no oracle needed): the log-likelihood of a ping is the
    sum over its valid beams, so the ping's even beams alone plus its odd beams alone give the whole ping -- for every
    particle, whatever path cast it (the sweep resolves a side's beams in one merge: an invalid beam must neither move a
    neighbour's expected range nor be counted), up to the fp32 summation order; and a ping without a valid beam weighs
    nothing."""
    from smarc_navigation_amd import engine as eng
    ba = synth.beam_angles(B)
    soa = _cloud(4)
    e = eng.Engine(N, rng_mode=eng.RNG_REPLAY)
    e.set_particles(soa)
    if kind == 'grid':
        origin = (-64.0, -256.0)
        e.set_map_grid(synth.bathymetry_grid(512, 512, 1.0, origin, seed=3), origin, 1.0)
    else:
        origin = (-64.0, -354.0)
        z = synth.bathymetry_grid(708, 708, 1.0, origin, seed=3)
        if kind == 'mesh_tin':
            verts, tris = synth.mesh_tin(z, 1.0, origin, seed=7)
        else:
            verts, tris = synth.mesh_from_grid(z, 1.0, origin)
        e.set_map_mesh(verts, tris, general=(kind == 'mesh_general'))
    rs = np.random.RandomState(5)
    ranges = (18.0 + 6.0 * rs.rand(B)).astype(np.float32)
    ranges[rs.choice(B, 9, replace=False)] = np.nan   # a few beams without a return
    parts = []
    for keep in (slice(None), slice(0, None, 2), slice(1, None, 2), slice(0, 0)):
        r = np.zeros(B, np.float32)
        r[keep] = ranges[keep]
        e.update_mbes(r, ba, 0.2, 100.0)
        parts.append(e.get_log_weights())
    whole, even, odd, none = parts
    assert np.all(np.isfinite(whole)) and np.std(whole) > 1.0
    assert np.array_equal(none, np.zeros(N))
    d = np.abs(whole - (even + odd))
    tol = 1e-3 + 2e-6 * np.abs(whole)
    print('%s: additivity over beams, max |d| %.3e at |lw| up to %.3e' % (kind, d.max(), np.abs(whole).max()))
    assert np.all(d <= tol), (d.max(), np.abs(whole)[np.argmax(d - tol)])


def test_full_size_resample_properties_and_shard_invariance():
    from smarc_navigation_amd import engine as eng
    rs = np.random.RandomState(9)
    lw = -0.5 * (rs.randn(N) * 4.0) ** 2
    soa = _cloud(4)
    one = eng.Engine(N, seed=77, resample_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5])
    one.set_particles(soa)
    one.set_log_weights(lw, eng.WEIGHT_LOG_SHIFT)
    one.resample()
    idx = one.last_indices()
    cdf = one.last_offspring_cdf()
    assert int(cdf[-1]) == N and np.all(np.diff(cdf.astype(np.int64)) >= 0)
    assert np.all(np.diff(idx.astype(np.int64)) >= 0) and idx[0] >= 0 and idx[-1] < N
    counts = np.diff(np.concatenate([[0], cdf.astype(np.int64)]))
    assert np.array_equal(np.bincount(idx, minlength=N), counts)
    # expected offspring ~ N * w (systematic resampling: |count - N w| < 1)
    w = np.exp(lw - lw.max())
    w /= w.sum()
    assert np.max(np.abs(counts - N * w)) < 1.0 + 1e-6
    # 4 shards on one GPU == 1 shard, bit for bit
    shards = [eng.Engine(N // 4, rank=r, world=4, n_global=N, global_offset=r * (N // 4), seed=77,
                         resample_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5]) for r in range(4)]
    for r, s in enumerate(shards):
        sl = slice(r * (N // 4), (r + 1) * (N // 4))
        s.set_particles(np.ascontiguousarray(soa[:, sl]))
        s.set_log_weights(lw[sl], eng.WEIGHT_LOG_SHIFT)
    eng.group_resample(shards)
    assert np.array_equal(np.concatenate([s.get_particles() for s in shards], axis=1), one.get_particles())


def _mesh_map():
    from oracle import oracle as orc
    origin = (-64.0, -354.0)
    z = synth.bathymetry_grid(708, 708, 1.0, origin, seed=3)
    verts, tris = synth.mesh_from_grid(z, 1.0, origin)
    return origin, z, verts, tris, orc.Mesh(verts, tris)


def _spot_check(e, orc, omap, soa, ba, ranges, r_max, pick, label):
    """log-likelihoods of `pick` against the oracle + expected ranges of a few of them"""
    lw = e.get_log_weights()
    sub = np.ascontiguousarray(soa[:, pick])
    lw_ref, ex_ref = orc.mbes_update(sub, np.identity(4), [0] * 6, omap, ba, ranges, 0.2, r_max)
    d = np.abs(lw[pick] - lw_ref)
    okm = (d <= 1e-2) | (d <= 2e-4 * np.abs(lw_ref))
    # a grazing ray may flip under fp32 (bounded in test_rough_terrain_...): tolerate isolated particles, report them
    print('%s: %d particles checked, max |dlw| %.3e, outside tolerance %d' % (label, pick.size, d.max(), int((~okm).sum())))
    assert (~okm).sum() <= max(2, pick.size // 500)
    from tests.helpers import lw_outliers_explained
    lw_outliers_explained(orc, omap, sub, ba, ranges, 0.2, r_max, lw[pick], lw_ref, label=label)
    for j in range(0, pick.size, max(1, pick.size // 16)):
        got = e.mbes_expected(int(pick[j]), 1, ba, r_max)[0]
        err = np.abs(got - ex_ref[j])
        assert (err > 1e-3).sum() <= 2, (label, j, err.max())
    return lw


@pytest.mark.parametrize('kind', ['mesh', 'grid', 'mesh_general'])
def test_full_size_cloud_straddling_the_map_border(kind, monkeypatch):
    """1 M particles centred ON the western map border: about half of them are off the map, every group's
    tile is clipped -- this is the deferred general kernel (k_mbes_cast<.,.,1>) at full size."""
    from smarc_navigation_amd import engine as eng
    from oracle import oracle as orc
    monkeypatch.setenv('MCL_DEBUG_WORK', '1')
    ba = synth.beam_angles(B)
    if kind == 'grid':
        origin = (-64.0, -256.0)
        z = synth.bathymetry_grid(512, 512, 1.0, origin, seed=3)
        omap = orc.Grid(z, origin, 1.0)
    else:
        origin, z, verts, tris, omap = _mesh_map()
    rs = np.random.RandomState(11)
    soa = rs.randn(6, N) * np.array([3.0, 3.0, 0.0, 0.02, 0.02, 0.3])[:, None]
    soa[0] += origin[0] + 1.0   # the border is at x = origin[0]
    soa[1] += 5.0
    soa[2] = -2.5
    e = eng.Engine(N, rng_mode=eng.RNG_REPLAY)
    e.set_particles(soa)
    if kind == 'grid':
        e.set_map_grid(z, origin, 1.0)
    else:
        e.set_map_mesh(verts, tris, general=(kind == 'mesh_general'))
    truth = np.array([[origin[0] + 4.0], [5.0], [-2.5], [0.0], [0.0], [0.1]])
    _, ex = orc.mbes_update(truth, np.identity(4), [0] * 6, omap, ba, None, 0.2, 100.0)
    ranges = (ex[0] + 0.2 * np.random.RandomState(2).randn(B)).astype(np.float32)
    e.update_mbes(ranges, ba, 0.2, 100.0)
    pick = np.random.RandomState(3).choice(N, 4096, replace=False)
    _spot_check(e, orc, omap, soa, ba, ranges, 100.0, pick, kind + ' border')


@pytest.mark.parametrize('kind', ['mesh', 'grid'])
def test_full_size_dispersed_cloud(kind):
    """sigma = 60 m cloud (global localisation): the fans of a group no longer share one LDS tile."""
    from smarc_navigation_amd import engine as eng
    from oracle import oracle as orc
    ba = synth.beam_angles(B)
    if kind == 'grid':
        origin = (-64.0, -256.0)
        z = synth.bathymetry_grid(512, 512, 1.0, origin, seed=3)
        omap = orc.Grid(z, origin, 1.0)
        centre = (190.0, 0.0)
    else:
        origin, z, verts, tris, omap = _mesh_map()
        centre = (290.0, 0.0)
    rs = np.random.RandomState(12)
    soa = rs.randn(6, N) * np.array([60.0, 60.0, 0.0, 0.02, 0.02, 3.0])[:, None]
    soa[0] += centre[0]
    soa[1] += centre[1]
    soa[2] = -2.5
    e = eng.Engine(N, rng_mode=eng.RNG_REPLAY)
    e.set_particles(soa)
    if kind == 'grid':
        e.set_map_grid(z, origin, 1.0)
    else:
        e.set_map_mesh(verts, tris)
    truth = np.array([[centre[0]], [centre[1]], [-2.5], [0.0], [0.0], [0.1]])
    _, ex = orc.mbes_update(truth, np.identity(4), [0] * 6, omap, ba, None, 0.2, 100.0)
    ranges = (ex[0] + 0.2 * np.random.RandomState(2).randn(B)).astype(np.float32)
    e.update_mbes(ranges, ba, 0.2, 100.0)
    pick = np.random.RandomState(3).choice(N, 4096, replace=False)
    lw = _spot_check(e, orc, omap, soa, ba, ranges, 100.0, pick, kind + ' dispersed')
    # resampling the dispersed cloud still concentrates it around the truth
    e2 = eng.Engine(N, seed=3, resample_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5])
    e2.set_particles(soa)
    e2.set_log_weights(lw, eng.WEIGHT_LOG_SHIFT)
    e2.resample()
    mean = e2.mean_cov()[0]
    assert np.hypot(mean[0] - centre[0], mean[1] - centre[1]) < 5.0


def test_config2_exact_shape_step_parity():
    """BASELINE config 2 as specified: 65 536 particles, 256 beams over +-60 deg, 512 x 512 grid, 1 m cells,
    sigma 0.2 m.  Per step: predict (Philox draws == oracle), MBES log-likelihoods (fp32 tolerance),
    resample indices bit-exact given the GPU's own log-weights, mean/cov."""
    from smarc_navigation_amd import engine as eng
    from oracle import oracle as orc
    n, Bc = 65536, 256
    origin = (-64.0, -256.0)
    z = synth.bathymetry_grid(512, 512, 1.0, origin, seed=3)
    g = orc.Grid(z, origin, 1.0)
    ba = synth.beam_angles(Bc)
    cov = dict(init_cov=[2.0, 2.0, 0.0, 0.0, 0.0, 0.05], process_cov=[1e-4, 1e-4, 0.0, 0.0, 0.0, 1e-6],
               resample_cov=[1e-3, 1e-3, 0.0, 0.0, 0.0, 1e-5])
    stream = synth.odom_stream(4)
    e = eng.Engine(n, seed=5, **cov)
    e.set_map_grid(z, origin, 1.0)
    e.init_particles()
    soa = np.zeros((6, n))
    orc.add_noise(soa, cov['init_cov'], orc.native_normals(n, 0, 5, 0, 0))
    np.testing.assert_allclose(e.get_particles(), soa, rtol=0, atol=1e-12)
    rs = np.random.RandomState(4)
    for k in range(3):
        prev = e.get_particles()
        e.predict(stream['v'][k], stream['wz'][k], stream['q'][k], stream['z'][k], stream['dt'])
        soa = e.get_particles()  # carry the GPU state: the checks are per phase
        orc.predict(prev, stream['v'][k], stream['wz'][k], stream['q'][k], stream['z'][k], stream['dt'],
                    cov['process_cov'], orc.native_normals(n, 0, 5, 1, k))
        np.testing.assert_allclose(soa, prev, rtol=0, atol=1e-11)
        ref = soa.copy()
        truth = stream['truth'][k][:, None].copy()
        _, ex = orc.mbes_update(truth, np.identity(4), [0] * 6, g, ba, None, 0.2, 100.0)
        ranges = (ex[0] + 0.2 * rs.randn(Bc)).astype(np.float32)
        e.update_mbes(ranges, ba, 0.2, 100.0)
        lw = e.get_log_weights()
        lw_ref, _ = orc.mbes_update(ref, np.identity(4), [0] * 6, g, ba, ranges, 0.2, 100.0)
        d = np.abs(lw - lw_ref)
        bad = ~((d <= 1e-2) | (d <= 2e-4 * np.abs(lw_ref)))
        print('config 2 step %d: max |dlw| %.3e (|lw| up to %.0f), outside tolerance %d of %d' % (
            k, d.max(), np.abs(lw_ref).max(), bad.sum(), n))
        assert bad.sum() <= 8
        e.resample()
        idx = e.last_indices()
        ref_idx, _, _ = orc.systematic_fixed(lw, 1, orc.native_u53(5, k))
        assert np.array_equal(idx, ref_idx)
        lost, dupes = orc.lost_dupes(ref_idx)
        orc.reassign(ref, lost, dupes)
        orc.add_noise(ref, cov['resample_cov'], orc.native_normals(n, 0, 5, 2, k))
        np.testing.assert_allclose(e.get_particles(), ref, rtol=0, atol=1e-12)
        mean, yaw, c9 = e.mean_cov()
        m6, _, c_ref = orc.mean_cov(ref)
        np.testing.assert_allclose(mean, m6, rtol=0, atol=1e-9)


def _dive_surface(kind):
    """(omap, engine map attachment, m2o) of a surface of the bench's legs (bench.py: build_map and the leg's own map <- odom
    transform; the round-6 legs through its punch_hole / synth.mesh_ragged)"""
    from oracle import oracle as orc
    import bench
    m = bench.build_map('grid' if kind == 'grid' else ('mesh' if kind == 'mesh' else 'mesh-tin'))
    m2o = None
    if kind == 'mesh_tin_gaps':
        m = bench.punch_gaps(m)
    elif kind == 'mesh_tin_hole_under_swath':
        m = bench.punch_hole(m, 1.0, 10.0)
    elif kind in ('mesh_tin_ragged_outline', 'mesh_tin_vehicle_off_the_map'):
        m = dict(m, tris=synth.mesh_ragged(m['verts'], m['tris']))
        m2o = synth.rigid_matrix(100.0, -330.0 if kind == 'mesh_tin_ragged_outline' else -360.0, 0.0, 0.0, 0.0, 0.0)
    omap = orc.Grid(m['z'], m['origin'], m['res']) if kind == 'grid' else orc.Mesh(m['verts'], m['tris'])
    return m, omap, m2o


_GAPS = ('mesh_tin_gaps', 'mesh_tin_hole_under_swath', 'mesh_tin_ragged_outline', 'mesh_tin_vehicle_off_the_map')


@pytest.mark.parametrize('kind,attitude', [(k, 'dive') for k in ('mesh', 'grid', 'mesh_tin') + _GAPS] +
                         [(k, 'level') for k in _GAPS[1:]])
def test_full_size_diving_cloud_and_the_round6_surfaces(kind, attitude):
    """1 M particles x 512 beams through the fan sweep with the whole cloud at one attitude far from level (pitch 0.26 rad =
    15 degrees, roll 0.05: a diving AUV, every particle the odometry's pitch) on every sweep surface of the bench, and level
    on the round-6 surfaces (a data gap under the swath, the ragged outline of a real survey, the vehicle off that map looking
    back in) -- one lane per side, the at-size code the small-cloud tests never reach.  A random sample of 1 024 and up to
    1 024 live particles against the oracle under the live-particle contract, at the metric's sigma and at the tempered
    filter's (where a thousand particles are live); on the surfaces with gaps mesh_tin_gaps' rule: a particle beyond the
    tolerance must own a ray that flips at a rim (an answer of the oracle under a 1 mm shift), at most one in 25."""
    from smarc_navigation_amd import engine as eng
    from oracle import oracle as orc
    from tests.helpers import live_particle_contract, live_picks
    bench_map, omap, m2o = _dive_surface(kind)
    roll, pitch = (0.05, 0.26) if attitude == 'dive' else (0.015, -0.02)
    ba = synth.beam_angles(B)
    rs = np.random.RandomState(21)
    soa = rs.randn(6, N) * np.array([1.5, 1.5, 0.0, 0.0, 0.0, 0.2])[:, None]
    if m2o is None and kind != 'mesh_tin_hole_under_swath':
        soa[0] += 30.0
        soa[1] += -12.0
    soa[2] = -2.2
    soa[3] = roll
    soa[4] = pitch
    m2o = np.identity(4) if m2o is None else m2o
    e = eng.Engine(N, m2o=m2o, rng_mode=eng.RNG_REPLAY)
    e.set_particles(soa)
    import bench
    bench.attach_map(e, bench_map)
    truth = np.array([[soa[0].mean()], [soa[1].mean()], [-2.2], [roll], [pitch], [0.0]])
    _, ex = orc.mbes_update(truth, m2o, [0] * 6, omap, ba, None, 0.2, 100.0)
    ranges = (ex[0] + 0.2 * np.random.RandomState(2).randn(B)).astype(np.float32)
    ranges[ex[0] >= 100.0] = 0.0
    label = '%s %s 1 M x 512' % (kind, attitude)
    from tests.helpers import lw_outliers_explained
    # sigma 0.2 (the metric's ping) and 0.2 sqrt(512) (bench.py's tempered filter: the cloud keeps a spread, so a thousand
    # particles are live even where one gap under a beam puts the rest 30 below the best)
    for sigma in (0.2, 0.2 * np.sqrt(B)):
        e.update_mbes(ranges, ba, sigma, 100.0)
        path, handed, _ = e.mbes_last_path()
        lw = e.get_log_weights()
        print('%s, sigma %.2f: path %d, the sweep handed over %d of %d (%d beams of the ping miss)' % (
            label, sigma, path, handed, N, int((ex[0] >= 100.0).sum())))
        assert path == 1, path
        # a random sample under the rule of the level test (surfaces with gaps: rim flips, few and each an oracle answer)
        pick = np.random.RandomState(3).choice(N, 1024, replace=False)
        sub = np.ascontiguousarray(soa[:, pick])
        lw_ref, _ = orc.mbes_update(sub, m2o, [0] * 6, omap, ba, ranges, sigma, 100.0)
        d = np.abs(lw[pick] - lw_ref)
        okm = (d <= 1e-2) | (d <= 2e-4 * np.abs(lw_ref))
        print('%s, sigma %.2f: random sample max |dlw| %.3e, outside tolerance %d' % (label, sigma, d.max(), int((~okm).sum())))
        if kind in _GAPS:
            assert (~okm).sum() <= pick.size // 25, int((~okm).sum())
            lw_outliers_explained(orc, omap, sub, ba, ranges, sigma, 100.0, lw[pick], lw_ref, m2o=m2o, label=label)
        else:
            assert np.all(okm)
        live = live_picks(lw, 1024, seed=6)
        lsub = np.ascontiguousarray(soa[:, live])
        lw_live, _ = orc.mbes_update(lsub, m2o, [0] * 6, omap, ba, ranges, sigma, 100.0)
        n_live, _, _ = live_particle_contract(orc, omap, lsub, ba, ranges, sigma, 100.0, lw[live], lw_live, float(lw.max()), m2o=m2o,
                                              label='%s, sigma %.2f' % (label, sigma), allow=live.size // 25 if kind in _GAPS else None)
        # (with a gap every 6 m a displaced particle's beams fall into gaps: even tempered, about ten particles of that cloud
        #  are live -- the random sample above covers the rest of it)
        assert n_live >= (16 if sigma > 1.0 and kind != 'mesh_tin_gaps' else 1)
    e.close()
