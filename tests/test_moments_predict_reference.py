"""The extended-precision references of the moments and predict edge tests (tests/helpers.py: moments_reference,
predict_reference), anchored without a GPU:

  * the long-double moments equal an exact evaluation in rationals;
  * the CPU oracle -- the reference node's own arithmetic -- meets the bounds the GPU tests assert, on every input family;
  * the families are what they claim to be.
"""
import fractions

import numpy as np
import pytest

from tests import helpers as H

F = fractions.Fraction


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


def _frac(x):
    """a long double (or double) as an exact rational: its 64-bit significand splits into two doubles"""
    x = np.longdouble(x)
    hi = float(x)
    return F(hi) + F(float(x - np.longdouble(hi)))


def _cases():
    return [(f, 1 if f == 'one' else 257) for f in H.MOMENT_FAMILIES]


@pytest.mark.parametrize('family,n', _cases())
def test_long_double_moments_equal_exact_rationals(family, n):
    """moments_reference against the same quantities in exact rationals, for the one-pass shift (particle 0) and the
    two-pass one (the mean): every value and every unit to 2^-60 of the unit taken about the exact mean -- the smallest
    scale the assertions ever use, so `relative` here is at least as strict as relative to any unit they do use."""
    if not H.LONGDOUBLE_OK:
        pytest.skip('no extended precision: moments_reference IS the rational evaluation here')
    soa = H.moments_family(family, n)
    exact_mean = [sum(F(float(x)) for x in soa[a]) / n for a in range(3)]
    scale = H._moments_exact(soa, exact_mean)
    tol = F(1, 2 ** 60)
    L = np.longdouble
    for shift in (soa[:3, 0].astype(L), soa[:3].astype(L).sum(axis=1) / L(n)):   # both given to both evaluations as they are
        ref = H.moments_reference(soa, shift)
        ex = H._moments_exact(soa, [_frac(s) for s in shift])
        for a in range(6):
            assert abs(_frac(ref['mean'][a]) - ex['mean'][a]) <= tol * scale['u_mean'][a], (a, 'mean')
            assert abs(_frac(ref['u_mean'][a]) - ex['u_mean'][a]) <= tol * ex['u_mean'][a], (a, 'u_mean')
        assert abs(_frac(ref['yaw']) - ex['yaw']) <= tol * scale['u_yaw']
        assert abs(_frac(ref['u_yaw']) - ex['u_yaw']) <= tol * ex['u_yaw']
        for k, a, b in H.COV_PAIRS:
            assert abs(_frac(ref['cov'][k]) - ex['cov'][k]) <= tol * scale['u_cov'][k], (k, 'cov')
            assert abs(_frac(ref['u_cov'][k]) - ex['u_cov'][k]) <= tol * ex['u_cov'][k], (k, 'u_cov')
        assert ref['cov'][3] == ref['cov'][1] and ref['cov'][6] == 0 and ref['cov'][7] == 0


@pytest.mark.parametrize('family', H.MOMENT_FAMILIES)
def test_families_are_well_posed(family):
    for n in ([1] if family == 'one' else [1, 65, 4099]):
        soa = H.moments_family(family, n)
        assert soa.shape == (6, n) and np.all(np.isfinite(soa))
        if n == 1:
            continue
        centre = soa[:2].mean(axis=1, keepdims=True)
        dist = np.hypot(*(soa[:2] - centre))
        if family == 'outlier0':
            rest = np.hypot(*(soa[:2, 1:] - soa[:2, 1:].mean(axis=1, keepdims=True)))
            assert np.argmax(dist) == 0 and dist[0] > 1000.0 and rest.max() < 0.1   # the shift lies 1e4 cloud widths outside
        if family in ('survey', 'outlier0', 'identical'):
            assert abs(np.median(soa[0]) - H.SURVEY_XY[0]) < 1.0 and abs(np.median(soa[1]) - H.SURVEY_XY[1]) < 1.0
        if family == 'identical':
            assert np.all(soa == soa[:, :1])
        if family == 'seam':
            w = H.wrap(soa[5])
            assert np.count_nonzero(w > 2.0) > n // 8 and np.count_nonzero(w < -2.0) > n // 8    # both sides of +-pi
            assert np.count_nonzero((soa[5] < -np.pi) | (soa[5] >= np.pi)) > n // 16             # stored yaw out of range
            assert np.all(np.abs(w) > 1.0)                                                       # nothing near 0


@pytest.mark.parametrize('family', H.MOMENT_FAMILIES)
def test_oracle_mean_cov_meets_the_gpu_bound(family, orc):
    """oracle.mean_cov (auv_pf.py:218-252 in fp64, two passes) within K 2^-53 U of the extended-precision moments, K and U
    as the GPU test of the two-pass kernels takes them."""
    worst = 0.0
    for n in ([1] if family == 'one' else [63, 65, 257]):
        soa = H.moments_family(family, n)
        L = np.longdouble
        ref = H.moments_reference(soa, soa[:3].astype(L).sum(axis=1) / L(n))
        r = np.concatenate(H.moments_errors(orc.mean_cov(soa), ref))
        K = H.two_pass_roundings(n)
        worst = max(worst, r.max())
        assert r.max() <= K, (family, n, K, r)
    print('oracle.mean_cov, %s: worst err / (2^-53 U) = %.2f' % (family, worst))


def _odom(orc):
    return dict(v=[1.2, 0.1, -0.05], q=orc.quat_from_euler(0.05, -0.03, 1.0), z=-3.5, dt=0.02)


@pytest.mark.parametrize('where', ['origin', 'survey'])
@pytest.mark.parametrize('wzdt', H.PREDICT_EDGE_WZDT)
def test_oracle_predict_meets_the_gpu_bound_on_the_edge_yaws(wzdt, where, orc):
    n = 4096 + H.PREDICT_EDGE_YAWS.size
    soa = H.predict_family(n, where)
    o = _odom(orc)
    wz = wzdt / o['dt']
    ref = H.predict_reference(soa, o['v'], wz, o['q'], o['z'], o['dt'], [0.0] * 6)
    got = soa.copy()
    orc.predict(got, o['v'], wz, o['q'], o['z'], o['dt'], [0.0] * 6, np.zeros((n, 6)))
    assert np.array_equal(got[5].view(np.uint64), ref['yaw'].view(np.uint64))       # bit for bit, -pi and pi included
    assert np.all((ref['yaw'] >= -np.pi) & (ref['yaw'] <= np.pi))
    L = np.longdouble
    assert np.all(np.abs(got[0].astype(L) - ref['x']) <= 4 * H.EPS53 * ref['u_x'])
    assert np.all(np.abs(got[1].astype(L) - ref['y']) <= 4 * H.EPS53 * ref['u_y'])
    assert np.all(got[2] == ref['z']) and np.all(got[3] == ref['roll']) and np.all(got[4] == ref['pitch'])


def test_the_edge_yaws_reach_both_ends_of_the_wrap():
    """what the bitwise yaw assertion covers: results on both closed ends -- pi itself (a sum a hair under -pi) and
    -pi --, the fmod path and its zero case"""
    out = np.concatenate([H.wrap(H.PREDICT_EDGE_YAWS + w) for w in H.PREDICT_EDGE_WZDT])
    assert np.count_nonzero(out == np.pi) >= 1 and np.count_nonzero(out == -np.pi) >= 2
    s = np.concatenate([H.PREDICT_EDGE_YAWS + w for w in H.PREDICT_EDGE_WZDT]) + np.pi
    assert np.count_nonzero((s < 0.0) | (s >= H.TWO_PI)) > 20             # left the fast path
    assert np.count_nonzero(np.fmod(s, H.TWO_PI) == 0.0) >= 2             # fmod's zero case


def test_oracle_predict_with_yaw_noise_stays_within_four_ulp_of_pi(orc):
    """stored yaws in [-pi, pi) (what a predict leaves): yaw + wz dt, + noise, + pi and - pi round at magnitudes below 8 --
    0.5 + 0.5 + 1 + 0.5 ulp(pi)"""
    n = 4096 + H.PREDICT_EDGE_YAWS.size
    soa = H.predict_family(n, 'origin', seed=1)
    soa[5] = H.wrap(soa[5])
    soa[5, soa[5] >= np.pi] = -np.pi
    pc = [1e-3, 2e-3, 0, 0, 0, 1e-4]
    o = _odom(orc)
    normals = np.random.RandomState(7).randn(n, 6)
    crossers = 0
    for wzdt in H.PREDICT_EDGE_WZDT:
        wz = wzdt / o['dt']
        got = soa.copy()
        orc.predict(got, o['v'], wz, o['q'], o['z'], o['dt'], pc, normals)
        ref = H.predict_reference(soa, o['v'], wz, o['q'], o['z'], o['dt'], pc, normals, yaw_t=got[5])
        err, crossed, to_seam = H.yaw_noise_check(got[5], ref)
        assert err.max() <= 4.0, err.max()
        assert np.all(to_seam[crossed] <= 4.0)
        crossers += int(crossed.sum())
        L = np.longdouble
        assert np.all(np.abs(got[0].astype(L) - ref['x']) <= 4 * H.EPS53 * ref['u_x'])
        assert np.all(np.abs(got[1].astype(L) - ref['y']) <= 4 * H.EPS53 * ref['u_y'])
    print('samples on the other side of the seam: %d' % crossers)
    assert crossers == 0
