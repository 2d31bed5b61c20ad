"""The motion step at its numeric edges, in both kernels that take it: k_predict (mcl_predict, here in REPLAY mode with
given normals) and the fused k_predict_pose (mcl_step_mbes; a ping without ranges and no resampling noise leave the
predicted state behind, slot for slot).  They share wrap_pi (mcl_device.h): a hand-written fast path for a yaw that has
not crossed +-pi, fmod with a zero case beyond.

Reference: tests/helpers.py predict_reference, auv_particle.py:38-70 with x and y in long double (anchored on the CPU by
tests/test_moments_predict_reference.py).  With a zero yaw process variance the yaw statement is exact in fp64 -- the
noise term is an exact zero, so a fused multiply-add changes no bit -- and yaw is asserted BIT FOR BIT
wrap(fl(yaw + fl(wz dt))), the results pi (from a sum a hair under -pi) and -pi included.  x and y lie within
4 2^-53 (|x'| + |m0| + |m1| + |sigma n|) of the reference; z, roll, pitch are the odometry's, exactly."""
import numpy as np
import pytest

from smarc_navigation_amd import synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

L = np.longdouble
ODOM = dict(v=[1.2, 0.1, -0.05], z=-3.5, dt=0.02)
RPY = (0.05, -0.03, 1.0)
N_EDGE = 4096 + H.PREDICT_EDGE_YAWS.size
PROCESS_COV = [1e-3, 2e-3, 0.0, 0.0, 0.0, 1e-4]
SEED = 0xABCDEF0123


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


def _map_at(where):
    cx, cy = (3.0, -2.0) if where == 'origin' else H.SURVEY_XY
    origin = (cx - 64.0, cy - 64.0)
    return synth.bathymetry_grid(128, 128, 1.0, origin, seed=3), origin


def _run(eng, orc, kernel, soa, where, wz, process_cov=(0.0,) * 6, normals=None):
    """the state after one motion step of `kernel`, and the normals it drew"""
    n = soa.shape[1]
    q = orc.quat_from_euler(*RPY)
    if kernel == 'predict':
        e = eng.Engine(n, process_cov=process_cov, rng_mode=eng.RNG_REPLAY)
        e.set_particles(soa)
        nz = np.zeros((n, 6)) if normals is None else normals
        e.predict(ODOM['v'], wz, q, ODOM['z'], ODOM['dt'], nz)
    else:
        z, origin = _map_at(where)
        e = eng.Engine(n, process_cov=process_cov, seed=SEED)
        e.set_map_grid(z, origin, 1.0)
        e.set_particles(soa)
        ranges = np.full(8, np.nan, np.float32)
        ranges[::2] = 0.0
        e.step_mbes(ODOM['v'], wz, q, ODOM['z'], ODOM['dt'], ranges, synth.beam_angles(8), 0.2, 80.0)
        assert np.array_equal(e.last_indices(), np.arange(n))      # the state is the predicted one, slot for slot
        nz = orc.native_normals(n, 0, SEED, 1, 0) if any(process_cov) else np.zeros((n, 6))
    st = e.get_particles()
    e.close()
    return st, nz


def _assert_exact_step(st, soa, wz, orc, sel=None):
    sel = np.arange(soa.shape[1]) if sel is None else sel
    q = orc.quat_from_euler(*RPY)
    ref = H.predict_reference(soa[:, sel], ODOM['v'], wz, q, ODOM['z'], ODOM['dt'], [0.0] * 6)
    got = st[:, sel]
    bad = np.flatnonzero(got[5].view(np.uint64) != ref['yaw'].view(np.uint64))
    assert bad.size == 0, (soa[5, sel][bad][:5], got[5][bad][:5], ref['yaw'][bad][:5])
    ex = np.abs(got[0].astype(L) - ref['x']) / (L(H.EPS53) * ref['u_x'])
    ey = np.abs(got[1].astype(L) - ref['y']) / (L(H.EPS53) * ref['u_y'])
    assert ex.max() <= 4.0 and ey.max() <= 4.0, (float(ex.max()), float(ey.max()))
    assert np.all(st[2] == ref['z']) and np.all(st[3] == ref['roll']) and np.all(st[4] == ref['pitch'])
    return float(max(ex.max(), ey.max())), ref


@pytest.mark.parametrize('where', ['origin', 'survey'])
@pytest.mark.parametrize('wzdt', H.PREDICT_EDGE_WZDT)
@pytest.mark.parametrize('kernel', ['predict', 'fused'])
def test_edge_yaws_wrap_bit_for_bit(kernel, wzdt, where, eng, orc):
    """+-pi and their two neighbouring doubles on each side, 0, -0.0, pi - 1e-3, 2 pi k, +-1e6, +-1e9 and 4096 yaws
    uniform in [-4 pi, 4 pi], turned by wz dt in {0, +-1e-3, +-0.5}"""
    soa = H.predict_family(N_EDGE, where)
    wz = wzdt / ODOM['dt']
    st, _ = _run(eng, orc, kernel, soa, where, wz)
    worst, ref = _assert_exact_step(st, soa, wz, orc)
    s = soa[5] + np.float64(wz) * np.float64(ODOM['dt']) + np.pi
    print('%s, wz dt %g, %s: %d of %d yaws off the fast path, results pi: %d, -pi: %d; worst x, y error %.2f x 2^-53 U' % (
        kernel, wzdt, where, np.count_nonzero((s < 0) | (s >= H.TWO_PI)), N_EDGE, np.count_nonzero(ref['yaw'] == np.pi),
        np.count_nonzero(ref['yaw'] == -np.pi), worst))


@pytest.mark.parametrize('kernel', ['predict', 'fused'])
def test_sizes_around_the_wave_the_block_and_the_grid(kernel, eng, orc):
    """n = 1, 63, 65, 257 and 524288 + 1, the first n whose grid strides; at survey coordinates, every step across the
    seam for a sixth of the cloud.  Checked on a 4096-particle sample plus the first and the last 65 slots."""
    wz = 0.5 / ODOM['dt']
    for n in (1, 63, 65, 257, 524288 + 1):
        soa = H.predict_family(n, 'survey', seed=n)
        st, _ = _run(eng, orc, kernel, soa, 'survey', wz)
        sel = np.arange(n)
        if n > 4096 + 130:
            sel = np.unique(np.concatenate([np.arange(65), np.arange(n - 65, n),
                                            np.random.RandomState(3).choice(n, 4096, replace=False)]))
        _assert_exact_step(st, soa, wz, orc, sel)
        # the slots outside the sample: the cheap invariants of the step
        assert np.all((st[5] >= -np.pi) & (st[5] <= np.pi)) and np.all(np.abs(st[:2] - soa[:2]) < 0.05)


@pytest.mark.parametrize('kernel', ['predict', 'fused'])
def test_yaw_noise_stays_within_four_ulp_of_pi(kernel, eng, orc):
    """Process noise on x, y and yaw (variance 1e-4), stored yaws in [-pi, pi) (what a predict leaves): yaw + wz dt, the
    noise, + pi and - pi round at magnitudes below 8 -- at most 0.5 + 0.5 + 1 + 0.5 ulp(pi) -- so yaw lies within 4 ulp(pi)
    of the long-double reference modulo 2 pi.  Only a sample whose unwrapped reference lies within 4 ulp of +-pi may land
    on the other side of the seam; none of these does (nor on the CPU oracle), so none may."""
    soa = H.predict_family(N_EDGE, 'origin', seed=1)
    soa[5] = H.wrap(soa[5])
    soa[5, soa[5] >= np.pi] = -np.pi
    q = orc.quat_from_euler(*RPY)
    normals = np.random.RandomState(7).randn(N_EDGE, 6)
    crossers, worst = 0, 0.0
    for wzdt in H.PREDICT_EDGE_WZDT:
        wz = wzdt / ODOM['dt']
        st, nz = _run(eng, orc, kernel, soa, 'origin', wz, PROCESS_COV, normals)
        ref = H.predict_reference(soa, ODOM['v'], wz, q, ODOM['z'], ODOM['dt'], PROCESS_COV, nz, yaw_t=st[5])
        err, crossed, to_seam = H.yaw_noise_check(st[5], ref)
        worst = max(worst, float(err.max()))
        assert err.max() <= 4.0, err.max()
        assert np.all(to_seam[crossed] <= 4.0)
        crossers += int(crossed.sum())
        assert np.all(np.abs(st[0].astype(L) - ref['x']) <= 4 * H.EPS53 * ref['u_x'])
        assert np.all(np.abs(st[1].astype(L) - ref['y']) <= 4 * H.EPS53 * ref['u_y'])
        assert np.all(st[2] == ref['z']) and np.all(st[3] == ref['roll']) and np.all(st[4] == ref['pitch'])
        assert np.count_nonzero(st[5] != H.wrap(soa[5] + np.float64(wz) * np.float64(ODOM['dt']))) > N_EDGE // 2   # the noise is on
    print('%s with yaw noise: worst yaw error %.2f ulp(pi), samples on the other side of the seam: %d' % (kernel, worst, crossers))
    assert crossers == 0
