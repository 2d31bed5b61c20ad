"""GPU tests of the ping innovation statistics and the per-beam gate (include/mcl_innovation.h; kernel
csrc/mcl_innovation.h): the five integers per beam against a numpy restatement of the definition over the dumped expected
ranges, the rays against the fp64 oracle under the precision contract of mcl_update_mbes (1e-3 m; grazing rays excused
only through helpers.outliers_explained), determinism over runs, group sizes and shards, a handle left untouched, the gate
on a cloud built for it, and the node end to end.  The scene and the restatement live in tests/test_innovation_host.py,
which also checks, without a GPU, that the oracle alone keeps the scene within the outlier cap."""
import numpy as np
import pytest

from smarc_navigation_amd import synth
from tests.helpers import outliers_explained
from tests.test_innovation_host import (M2O, MAX_SAMPLES, N, OFF, OUTLIER_CAP, R_MAX, SIGMA, records_ref, sample_ref,
                                        sampled_slots, scene, scene_map)

pytestmark = pytest.mark.gpu

KINDS = ('grid', 'mesh', 'tin')
FIELDS = ('n', 'n_miss', 'n_within', 's1', 's2')
COUNT = 586          # sampled particles: ceil(4096 / 7)


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def _engine(eng, kind, z, origin, soa, **kw):
    e = eng.Engine(soa.shape[1], m2o=M2O, rng_mode=eng.RNG_REPLAY, **kw)
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
    # the stride does not divide N; the count is no multiple of the group size the library picks here (4), nor of 7 or 64
    assert stride == 7 and N % stride != 0 and count == slots.size == COUNT and COUNT % 4 and COUNT % 7 and COUNT % 64
    out = dict(z=z, origin=origin, soa=soa, slots=slots)
    for kind in KINDS:
        out[kind] = (_engine(eng, kind, z, origin, soa), scene_map(kind, z, origin)[1])
    yield out
    for kind in KINDS:
        out[kind][0].close()


def _ping(e, B, seed=1, invalid=True):
    """a plausible ping of B beams: what one particle of the cloud expects, plus noise; some beams without a return"""
    ba = synth.beam_angles(B)
    rs = np.random.RandomState(seed)
    ranges = (e.mbes_expected(1, 1, ba, R_MAX, OFF)[0] + SIGMA * rs.randn(B)).astype(np.float32)
    if invalid and B > 8:
        ranges[::7] = 0.0
        ranges[3] = np.nan
        ranges[5] = -1.0
    return ba, ranges


def _ints(rec):
    return [tuple(int(rec[f][b]) for f in FIELDS) for b in range(rec.size)]


# ------------------------------------------------------------------ 1. the reduction is exact
@pytest.mark.parametrize('B', [1, 64, 65, 300, 512])     # a wave, a wave's tail, a chunk's tail (300), two chunks
@pytest.mark.parametrize('kind', KINDS)
def test_the_five_integers_equal_the_definition_over_the_dumped_ranges(world, kind, B):
    e, _ = world[kind]
    ba, ranges = _ping(e, B)
    inn = e.ping_innovation(ranges, ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES, support_k=3.0, dump=True)
    assert inn.n_sampled == COUNT and inn.expected.shape == (COUNT, B)
    valid = ranges > 0
    assert np.all(np.isnan(inn.expected[:, ~valid])) and np.all(np.isfinite(inn.expected[:, valid]))
    assert np.all(inn.expected[:, valid] > 0) and np.all(inn.expected[:, valid] <= np.float32(R_MAX))
    want = records_ref(ranges, inn.expected, SIGMA, 3.0, R_MAX)
    assert _ints(inn.beams) == want
    n_miss = np.array([w[1] for w in want])
    assert np.all(n_miss[valid] >= 21) and np.all(n_miss[~valid] == 0)     # the 21 sampled particles past the edge
    assert all(w == (0, 0, 0, 0, 0) for w, v in zip(want, valid) if not v)
    # production passes no dump: the same records
    plain = e.ping_innovation(ranges, ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES)
    assert plain.beams.tobytes() == inn.beams.tobytes() and plain.expected is None


# ------------------------------------------------------------------ 2. the rays are right
@pytest.mark.parametrize('kind', KINDS)
def test_dumped_ranges_against_the_oracle_under_the_precision_contract(world, orc, kind):
    e, omap = world[kind]
    ba, ranges = _ping(e, 300, invalid=False)
    got = e.ping_innovation(ranges, ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES, dump=True).expected.astype(np.float64)
    sub = np.ascontiguousarray(world['soa'][:, world['slots']])
    _, ref = orc.mbes_update(sub, M2O, OFF, omap, ba, None, SIGMA, R_MAX, want_expected=True)
    err = np.abs(got - ref)
    print('%s: max |e - oracle| %.3e m over %d rays, %d beyond 1e-3 m' % (kind, err.max(), err.size, int((err > 1e-3).sum())))
    assert (err > 1e-3).mean() < OUTLIER_CAP
    outliers_explained(orc, omap, sub, ba, got, ref, R_MAX, m2o=M2O, off=OFF, label='innovation ' + kind)


@pytest.mark.parametrize('kind', ['grid', 'tin'])
def test_the_dump_is_the_range_updates_expected_range_byte_for_byte(world, eng, kind):
    """k_innovation and k_ranges_update share the direction, the frame's arithmetic and the map-ray entry (mcl_mbes.h:
    beam_in_vehicle, cast_map_ray): the same rays from the same particles give the same floats"""
    e, _ = world[kind]
    ba = synth.beam_angles(16)
    inn = e.ping_innovation(np.full(16, 10.0, np.float32), ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES, dump=True)
    exp = e.ranges_expected(0, N, eng.innovation_dirs(ba), R_MAX, OFF)[world['slots']]
    assert inn.expected.shape == exp.shape == (COUNT, 16) and np.any(exp < np.float32(R_MAX))
    assert inn.expected.tobytes() == np.ascontiguousarray(exp).tobytes()


# ------------------------------------------------------------------ 3. determinism
def test_two_runs_give_the_same_bytes_and_the_handle_is_left_untouched(world, eng):
    e, _ = world['tin']
    ba, ranges = _ping(e, 300)
    e.update_mbes(ranges, ba, SIGMA, R_MAX, OFF)            # pending log-weights: the statistics ignore them
    soa0, lw0 = e.get_particles().tobytes(), e.get_log_weights().tobytes()
    a = e.ping_innovation(ranges, ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES, dump=True)
    b = e.ping_innovation(ranges, ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES, dump=True)
    assert a.beams.tobytes() == b.beams.tobytes() and a.expected.tobytes() == b.expected.tobytes()
    e.gate_ping(ranges, ba, SIGMA, R_MAX, OFF)
    eng.group_ping_innovation([e], ranges, ba, SIGMA, R_MAX, OFF)
    assert e.get_particles().tobytes() == soa0 and e.get_log_weights().tobytes() == lw0


@pytest.mark.parametrize('group', ['1', '7', '64'])
def test_the_group_size_does_not_change_a_bit(world, eng, monkeypatch, group):
    ref_e, _ = world['grid']
    ba, ranges = _ping(ref_e, 300)
    want = ref_e.ping_innovation(ranges, ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES, dump=True)
    monkeypatch.setenv('MCL_INNOVATION_GROUP', group)       # (read when the handle is created)
    e = _engine(eng, 'grid', world['z'], world['origin'], world['soa'])
    got = e.ping_innovation(ranges, ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES, dump=True)
    e.close()
    assert got.beams.tobytes() == want.beams.tobytes() and got.expected.tobytes() == want.expected.tobytes()


@pytest.mark.parametrize('kind', ['grid', 'tin'])
def test_two_shards_merged_equal_the_unsharded_record(world, eng, kind):
    whole, _ = world[kind]
    ba, ranges = _ping(whole, 65)
    want = whole.ping_innovation(ranges, ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES)
    half = N // 2
    parts = [_engine(eng, kind, world['z'], world['origin'], np.ascontiguousarray(world['soa'][:, s * half:(s + 1) * half]),
                     rank=s, world=2, n_global=N, global_offset=s * half) for s in range(2)]
    recs = [p.ping_innovation(ranges, ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES) for p in parts]
    # the second shard starts at id 2048: its first sampled slot is 3 (2051 = 7 x 293)
    assert [r.n_sampled for r in recs] == [293, 293] and sum(r.n_sampled for r in recs) == want.n_sampled == COUNT
    assert eng.merge_innovation(recs).tobytes() == want.beams.tobytes()
    assert eng.merge_innovation(recs[::-1]).tobytes() == want.beams.tobytes()
    got = eng.group_ping_innovation(parts[::-1], ranges, ba, SIGMA, R_MAX, OFF, max_samples=MAX_SAMPLES)
    assert got.beams.tobytes() == want.beams.tobytes() and got.n_sampled == want.n_sampled
    for p in parts:
        p.close()


def test_argument_and_state_errors(world, eng):
    e, _ = world['grid']
    ba, ranges = _ping(e, 64)

    def status(f, *a, **k):
        with pytest.raises(eng.MclError) as ei:
            f(*a, **k)
        return ei.value.status

    assert status(e.ping_innovation, ranges, ba, SIGMA, 4096.5) == -1               # r_max beyond the quantised range
    assert status(e.ping_innovation, ranges, ba, SIGMA, 0.0) == -1
    assert status(e.ping_innovation, ranges, ba, 0.0, R_MAX) == -1
    assert status(e.ping_innovation, ranges, ba, SIGMA, R_MAX, support_k=-1.0) == -1
    assert status(e.ping_innovation, ranges, ba, SIGMA, R_MAX, max_samples=0) == -1
    assert status(e.ping_innovation, ranges, ba, SIGMA, R_MAX, max_samples=32769) == -1
    bad = ba.copy()
    bad[3] = np.nan
    assert status(e.ping_innovation, ranges, bad, SIGMA, R_MAX) == -1
    assert status(e.ping_innovation, np.ones(2049, np.float32), np.zeros(2049, np.float32), SIGMA, R_MAX) == -1
    assert e.ping_innovation(ranges, ba, SIGMA, 4096.0, max_samples=32768).n_sampled == N     # the bounds themselves
    bare = eng.Engine(16)
    bare.init_particles()
    assert status(bare.ping_innovation, ranges, ba, SIGMA, R_MAX) == -5              # no map
    bare.close()


# ------------------------------------------------------------------ 4. the gate, by construction
def test_gate_by_construction(eng, orc):
    origin = (-64.0, -64.0)
    z = synth.bathymetry_grid(128, 128, 1.0, origin, seed=1)
    B, n = 64, N
    ba = synth.beam_angles(B)
    pose = np.array([3.0, -2.0, -2.0, 0.01, -0.01, 0.4])
    _, ex = orc.mbes_update(pose[:, None].copy(), np.identity(4), [0] * 6, orc.Grid(z, origin, 1.0), ba, None, SIGMA, 60.0)
    clean = ex[0].astype(np.float32)
    assert clean.max() < 59.0
    e = eng.Engine(n, init_cov=[1e-4, 1e-4, 0, 0, 0, 1e-4], seed=3)
    e.set_map_grid(z, origin, 1.0)
    e.init_particles()
    soa = e.get_particles()
    soa += pose[:, None]                                   # the cloud: a spread of 1e-4 about the known pose
    e.set_particles(soa)
    # six beams shortened by 20 sigma: exactly those are gated
    hit = np.array([2, 9, 17, 30, 31, 60])
    short = clean.copy()
    short[hit] -= np.float32(20 * SIGMA)
    masked, v = e.gate_ping(short, ba, SIGMA, 60.0)
    assert np.array_equal(np.nonzero(v.mask)[0], hit) and v.n_gated == 6 and not v.inconsistent and v.n_valid == B
    assert np.all(masked[hit] == 0.0) and np.array_equal(np.delete(masked, hit), np.delete(short, hit))
    assert np.all(v.nis[hit] > 10.83) and np.all(v.support[hit] < 0.01) and np.all(v.nu[hit] < -19 * SIGMA)
    # every beam lengthened by 20 sigma: the ping disagrees as a whole, nothing is gated
    masked, v = e.gate_ping(clean + np.float32(20 * SIGMA), ba, SIGMA, 60.0)
    assert v.n_gated == 0 and v.inconsistent and v.n_candidates == B and not v.mask.any()
    assert np.array_equal(masked, clean + np.float32(20 * SIGMA))
    # clean ranges: nothing gated, the update computes what it computes without the gate, NIS well below 1
    masked, v = e.gate_ping(clean, ba, SIGMA, 60.0)
    print('clean ping: mean NIS per beam %.3e, mean nu %.3e m' % (v.mean_nis(), v.mean_nu))
    assert v.n_gated == 0 and not v.inconsistent and masked.tobytes() == clean.tobytes()
    assert v.mean_nis() < 1.0 and v.innovation.mean_nis() < 1.0
    e.update_mbes(masked, ba, SIGMA, 60.0)
    lw_gated = e.get_log_weights().tobytes()
    e.update_mbes(clean, ba, SIGMA, 60.0)
    assert e.get_log_weights().tobytes() == lw_gated
    e.close()


# ------------------------------------------------------------------ 5. the node end to end
def test_node_with_the_gate_on_and_outliers_injected_reports_gated_beams():
    from smarc_navigation_amd import replay
    st = replay.synthetic_stream(150, mbes_every=10, beams=64, outliers=(0.1, 6.0))
    assert st['mbes_outliers'].sum() > 20
    params = dict(replay.SYNTH_PARAMS, particle_count=4096, mbes_gate_nis=10.83)
    res = replay.replay(st, params)
    s = res['summary']
    print({k: s[k] for k in s if k.startswith('gate') or k.startswith('innovation')})
    assert s['gate_pings'] > 0 and s['gate_n_gated'] > 0
