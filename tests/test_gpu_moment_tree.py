"""The summation tree of the moment kernels (csrc/mcl_device.h, "the fixed tree"), pinned bit for bit.

k_modes_moments, k_history_frame, k_drift_moments and k_reg_moments share one tree; helpers.moment_tree_sums restates it
in numpy, addition by addition.  Two of the four are reached here, the two whose every operation from the state to the
returned record is one IEEE fp64 operation (contraction is off on the device): mcl_regularise with three and with six
dimensions, and mcl_drift_mean_cov.  A change in the order of any addition -- inside the wave scan, over a wave's
grid-stride iterations, across the waves of a workgroup, across the workgroups -- moves a last bit somewhere in these
sums and fails the comparison; so does a zero of the wrong sign.

Inputs: x and y a metre wide around survey-sized coordinates, yaws in (-1, 1) (v - shift stays inside [-pi, pi): the
wrap is not reached), the drift words around 0.1; one fixed seed.  The counts are the smallest at which the tree can go
wrong: one live lane; the wave edge; the workgroup edge and a second workgroup with one live lane; four workgroups with a
ragged last wave; and MCL_MAX_GRID x MCL_BLOCK + 65, where the grid is capped and workgroup 0 alone takes a second
grid-stride iteration with one full and one ragged wave."""
import ctypes
import functools

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 255, 256, 257, 1000, helpers.MCL_MAX_GRID * helpers.MCL_BLOCK + 65]
ZERO3 = [0.0, 0.0, 0.0]


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def packed(r, c):
    """reg_packed (csrc/mcl_host_pure.h): the lower triangle row by row, r >= c"""
    return r * (r + 1) // 2 + c


@functools.lru_cache(maxsize=None)
def case(n):
    """the cloud of one count and the 27 sums of its six dimensions (x, y, yaw, cx, cy, bw) about slot 0, through the
    restated tree: the three-dimensional sums and the drift's are rows of the same table (a row's tree sees its own terms
    only).  Computed once per count; nothing writes to it afterwards."""
    rs = np.random.RandomState(20260 + n % 1000)
    soa = np.zeros((6, n))
    soa[0] = 1.0e5 + rs.randn(n)
    soa[1] = 1.2e5 + rs.randn(n)
    soa[2] = -20.0 + rs.randn(n)
    soa[3], soa[4] = 0.05 * rs.randn(n), 0.05 * rs.randn(n)
    soa[5] = rs.uniform(-1.0, 1.0, n)
    d = 0.1 + 0.02 * rs.randn(3, n)
    v = np.concatenate([soa[[0, 1, 5]], d])
    shift = v[:, 0].copy()
    e = v - shift[:, None]
    assert np.all(e[2] >= -np.pi) and np.all(e[2] < np.pi)
    S = helpers.moment_tree_sums(e)
    P = np.zeros(21)
    for r in range(6):
        P[packed(r, 0):packed(r, r) + 1] = helpers.moment_tree_sums(e[r] * e[:r + 1])
    for a in (soa, d, shift, S, P):
        a.setflags(write=False)
    return soa, d, shift, S, P


def record(e):
    """mcl_regularise_last as the library fills it: the covariance packed, no arithmetic on the way"""
    from smarc_navigation_amd import _lib
    r = _lib.RegulariseResult()
    e._ck(e.lib.mcl_regularise_last(e.h, ctypes.byref(r)))
    D = int(r.dims)
    return np.array(r.shift[:D]), np.array(r.dmean[:D]), np.array(r.cov[:D * (D + 1) // 2])


@pytest.mark.parametrize('dims', [3, 6])
@pytest.mark.parametrize('n', COUNTS)
def test_regularise_moments_are_the_restated_tree(n, dims, eng):
    soa, d, shift, S, P = case(n)
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY, seed=1)
    e.set_particles(soa)
    if dims == 6:
        e.drift_enable(ZERO3, ZERO3)
        e.drift_set(d)
    e.regularise(scale=1.0, shrink=False, with_drift=dims == 6, normals=np.zeros((n, dims)))   # zero normals: nothing moves
    got_shift, got_mean, got_cov = record(e)
    e.close()
    N = np.float64(n)
    want_mean = S[:dims] / N
    want_cov = np.array([P[packed(r, c)] / N - want_mean[r] * want_mean[c] for r in range(dims) for c in range(r + 1)])
    print('n %d dims %d: dmean differs in %d words, cov in %d' % (
        n, dims, np.count_nonzero(bits(got_mean) != bits(want_mean)), np.count_nonzero(bits(got_cov) != bits(want_cov))))
    assert np.array_equal(bits(got_shift), bits(shift[:dims]))
    assert np.array_equal(bits(got_mean), bits(want_mean)), (got_mean, want_mean)
    assert np.array_equal(bits(got_cov), bits(want_cov)), (got_cov, want_cov)


@pytest.mark.parametrize('n', COUNTS)
def test_drift_mean_is_the_restated_tree(n, eng):
    soa, d, shift, S, P = case(n)
    e = eng.Engine(n, seed=1)
    e.set_particles(soa)
    e.drift_enable(ZERO3, ZERO3)
    e.drift_set(d)
    mean, cov = e.drift_mean_cov()
    e.close()
    N = np.float64(n)
    m = S[3:] / N
    want_mean = m + shift[3:]
    want_cov = np.array([[P[packed(3 + max(a, b), 3 + min(a, b))] / N - m[a] * m[b] for b in range(3)] for a in range(3)])
    print('n %d: mean differs in %d words; cov off by at most %.3e' % (
        n, np.count_nonzero(bits(mean) != bits(want_mean)), np.abs(cov - want_cov).max()))
    assert np.array_equal(bits(mean), bits(want_mean)), (mean, want_mean)
    # the host may contract q - m m into one operation: the tolerance of tests/test_gpu_drift.py
    big = np.abs(d).max(axis=1)
    assert np.all(np.abs(cov - want_cov) <= 1e-12 * np.outer(big, big)), (cov, want_cov)
