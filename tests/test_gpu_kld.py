"""GPU tests of KLD-sampling across handles (include/mcl_kld.h; csrc/mcl_kld.h): mcl_kld_bins against len(np.unique(cells))
of a numpy restatement of the cell rule, exactly, on random, collapsed and fully dispersed clouds, at cell edges, with
particles outside and yaws beyond the circle, at the word and bitmap bounds of a 2^27-cell lattice, and that it leaves its
bitmap clean and the handle untouched; mcl_resample_into against the index rule evaluated in Python integers on the fixed-point
weights a twin of src decides on (every pair of sizes, every kind of weights, the uniforms at their ends), the state bit for
bit, src and dst afterwards against untouched twins, the NATIVE draw, drift, genealogy and the errors; and the global
localisation of tests/test_gpu_recovery.py run over a ladder of four sizes."""
import bisect
import math

import numpy as np
import pytest

from smarc_navigation_amd import synth
from tests import helpers
from tests.test_gpu_recovery import GLOBAL_BOUND

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
SEED = 0x1234567890abcdef
U_LAST = 1.0 - 2.0 ** -53


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


# ------------------------------------------------------------------ kld_bins: the numpy restatement
def ref_bins(soa, g):
    """(k, n_outside) by the cell rule of include/mcl_modes.h: IEEE double subtraction, then division, then floor"""
    x0, y0, cell, nx, ny, n_yaw = g.x0, g.y0, g.cell, g.nx, g.ny, g.n_yaw
    with np.errstate(invalid='ignore', over='ignore'):
        fx = np.floor((soa[0] - x0) / cell)
        fy = np.floor((soa[1] - y0) / cell)
        t = np.floor((soa[5] + np.pi) / ((2 * np.pi) / n_yaw))
        inside = (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny) & np.isfinite(t)
        w = np.mod(np.where(np.isfinite(t), t, 0.0), float(n_yaw))     # floored modulo; exact on integer-valued doubles
    c = (w[inside].astype(np.int64) * ny + fy[inside].astype(np.int64)) * nx + fx[inside].astype(np.int64)
    return len(np.unique(c)), int(soa.shape[1] - np.count_nonzero(inside)), c


def engine_with(eng, soa, **kw):
    e = eng.Engine(soa.shape[1], **kw)
    e.set_particles(soa)
    return e


def check_bins(eng, soa, g, e=None):
    own = e is None
    if own:
        e = engine_with(eng, soa)
    k, n_out = e.kld_bins(grid=g)
    rk, rout, cells = ref_bins(soa, g)
    assert (k, n_out) == (rk, rout), ((k, n_out), (rk, rout))
    if own:
        e.close()
    return k, n_out, cells


def random_cloud(n, seed, g, spread=1.0):
    rs = np.random.RandomState(seed)
    s = np.zeros((6, n))
    cx, cy = g.x0 + 0.5 * g.nx * g.cell, g.y0 + 0.5 * g.ny * g.cell
    s[0] = cx + spread * 0.3 * g.nx * g.cell * rs.randn(n)
    s[1] = cy + spread * 0.3 * g.ny * g.cell * rs.randn(n)
    s[2:5] = rs.randn(3, n)
    s[5] = rs.uniform(-4.0, 4.0, n)
    return s


@pytest.mark.parametrize('n', [1, 65, 100003])
def test_bins_of_random_clouds(eng, n):
    g = eng.make_mode_grid(-20.0, -10.0, 0.5, 80, 60, 36)
    for seed, spread in ((1, 1.0), (2, 0.05), (3, 3.0)):
        k, n_out, _ = check_bins(eng, random_cloud(n, seed + n, g, spread), g)
        assert 0 <= k <= n - n_out
    if n > 1000:
        assert check_bins(eng, random_cloud(n, 9, g, 1.0), g)[1] > 0      # some of them lie outside


@pytest.mark.parametrize('n', [1, 65, 100003])
def test_bins_of_a_cloud_in_one_cell_the_aggregation_path(eng, n):
    g = eng.make_mode_grid(-20.0, -10.0, 0.5, 80, 60, 36)
    rs = np.random.RandomState(n)
    s = np.zeros((6, n))
    s[0], s[1], s[5] = 3.0 + 0.49 * rs.rand(n), 4.5 + 0.49 * rs.rand(n), 0.01 + 0.1 * rs.rand(n)
    assert check_bins(eng, s, g)[:2] == (1, 0)
    s[0, ::2] += 0.5                                                   # two cells that share a bitmap word
    assert check_bins(eng, s, g)[0] == (2 if n > 1 else 1)


def test_bins_of_a_cloud_with_every_particle_in_its_own_cell_no_aggregation(eng):
    n = 100003
    g = eng.make_mode_grid(-100.0, 50.0, 0.25, 400, 300, 1)
    i = np.arange(n)
    s = np.zeros((6, n))
    s[0] = g.x0 + ((i % 400) + 0.5) * g.cell
    s[1] = g.y0 + ((i // 400) + 0.5) * g.cell
    rs = np.random.RandomState(0)
    s = s[:, rs.permutation(n)]                                        # neighbours in a wave are not neighbours in space
    assert check_bins(eng, s, g)[:2] == (n, 0)


def test_bins_at_cell_edges_corners_and_the_far_edge_of_the_box(eng):
    g = eng.make_mode_grid(-3.0, 7.0, 0.3, 11, 7, 8)                   # 0.3 is no binary fraction: the edges round
    xs = [g.x0 + j * g.cell for j in range(12)] + [np.nextafter(g.x0 + j * g.cell, -np.inf) for j in range(12)]
    xs += [np.nextafter(g.x0 + j * g.cell, np.inf) for j in range(12)] + [g.x0 + 11 * 0.3, -3.0, np.nextafter(-3.0, -4.0)]
    ys = [g.y0 + j * g.cell for j in range(8)] + [np.nextafter(g.y0 + 7 * g.cell, 0.0), g.y0 + 7 * 0.3, 7.0]
    dy = (2 * np.pi) / 8
    ws = [-np.pi + j * dy for j in range(9)] + [np.nextafter(-np.pi + j * dy, -10.0) for j in range(9)]
    xs += [g.x0 + (j + 0.5) * g.cell for j in range(11)]               # and the cells' centres: every cell holds a particle
    ys += [g.y0 + (j + 0.5) * g.cell for j in range(7)]
    ws += [-np.pi + (j + 0.5) * dy for j in range(8)]
    pts = [(x, y, w) for x in xs for y in ys for w in ws]
    s = np.zeros((6, len(pts)))
    s[0], s[1], s[5] = np.array(pts).T
    k, n_out, _ = check_bins(eng, s, g)
    assert k == 11 * 7 * 8 and n_out > 0                               # every cell is hit, the far edge is outside


def test_bins_leave_out_particles_that_are_not_finite_or_outside(eng):
    g = eng.make_mode_grid(-20.0, -10.0, 0.5, 80, 60, 36)
    s = random_cloud(300, 5, g, 0.5)
    bad = [np.nan, np.inf, -np.inf]
    for j, v in enumerate(bad):
        s[0, j], s[1, 10 + j], s[5, 20 + j] = v, v, v
    s[0, 30], s[0, 31], s[1, 32], s[1, 33] = -20.5, 20.0, -10.001, 20.0     # outside on all four sides
    s[0, 34], s[1, 35] = 1e300, -1e300
    s[2:5, 40:50] = np.nan                                             # z, roll and pitch decide nothing
    k, n_out, _ = check_bins(eng, s, g)
    assert n_out >= 15
    allout = np.full((6, 65), np.nan)
    assert check_bins(eng, allout, g)[:2] == (0, 65)


@pytest.mark.parametrize('n_yaw', [1, 2, 36, 1024])
def test_bins_of_yaws_at_plus_minus_pi_and_beyond_the_circle(eng, n_yaw):
    g = eng.make_mode_grid(0.0, 0.0, 1.0, 2, 2, n_yaw)
    yaws = [-np.pi, np.pi, np.nextafter(np.pi, 0.0), np.nextafter(-np.pi, 0.0), np.nextafter(np.pi, 4.0), 0.0, -0.0, 7.0, -9.5,
            3 * np.pi, -3 * np.pi, 1e6, -1e6, 1e300, -1e300, 1.7e308, -1.7e308, 2 ** 53 + 0.0, 123456.789]
    s = np.zeros((6, len(yaws)))
    s[0], s[1], s[5] = 0.5, 1.5, yaws
    k, n_out, _ = check_bins(eng, s, g)
    assert 1 <= k <= n_yaw
    if n_yaw == 1024:
        assert n_out == 2                                              # (+-1.7e308 + pi) / dyaw overflows: no cell
    if n_yaw == 1:
        assert (k, n_out) == (1, 0)


def at_cell(g, c):
    """a pose in the middle of cell c"""
    ix, r = c % g.nx, c // g.nx
    iy, iw = r % g.ny, r // g.ny
    return g.x0 + (ix + 0.5) * g.cell, g.y0 + (iy + 0.5) * g.cell, -np.pi + (iw + 0.5) * ((2 * np.pi) / g.n_yaw)


def test_bins_at_the_word_and_bitmap_bounds_of_the_largest_lattice(eng):
    g = eng.make_mode_grid(-1024.0, -1024.0, 0.5, 4096, 4096, 8)
    assert eng.kld_grid_check(g) == 2 ** 27
    cells = [0, 31, 32, 63, 64, 2 ** 27 - 1, 2 ** 27 - 32, 2 ** 27 - 33, 4095, 4096, 12345678]
    s = np.zeros((6, 3 * len(cells)))
    for j, c in enumerate(cells * 3):
        s[0, j], s[1, j], s[5, j] = at_cell(g, c)
    e = engine_with(eng, s)
    k, n_out, got = check_bins(eng, s, g, e)
    assert (k, n_out) == (len(cells), 0) and sorted(set(got.tolist())) == sorted(cells)
    assert e.kld_bins(grid=g) == (len(cells), 0)                       # the bitmap was left clean
    for c in (0, 31, 32, 2 ** 27 - 1):                                 # one cell at a time: nothing is left of the others
        one = np.zeros((6, 3 * len(cells)))
        one[0], one[1], one[5] = [np.full(one.shape[1], v) for v in at_cell(g, c)]
        e.set_particles(one)
        assert e.kld_bins(grid=g) == (1, 0)
    expect_status(eng, ERR_INVALID, e.kld_bins, grid=eng.make_mode_grid(-1024.0, -1024.0, 0.5, 4097, 4096, 8))      # one row more
    e.close()


def test_bins_on_a_lattice_of_one_cell(eng):
    g = eng.make_mode_grid(-1.0, -1.0, 2.0, 1, 1, 1)
    s = np.zeros((6, 65))
    s[0] = np.linspace(-1.5, 1.5, 65)
    s[5] = np.linspace(-20.0, 20.0, 65)
    k, n_out, _ = check_bins(eng, s, g)
    assert k == 1 and 0 < n_out < 65


def test_bins_twice_small_after_large_large_after_small_and_after_a_refused_call(eng):
    big = eng.make_mode_grid(-64.0, -64.0, 0.125, 1024, 1024, 16)      # 2^24 cells
    small = eng.make_mode_grid(-64.0, -64.0, 8.0, 16, 16, 2)           # 512 cells: 16 words
    tiny = eng.make_mode_grid(-64.0, -64.0, 128.0, 1, 1, 1)
    s = random_cloud(100003, 11, big, 0.6)
    e = engine_with(eng, s)
    first = check_bins(eng, s, small, e)[:2]                           # allocates the small bitmap
    assert check_bins(eng, s, small, e)[:2] == first                   # two successive calls: the bitmap was left clean
    kb = check_bins(eng, s, big, e)[:2]                                # growth
    assert kb[0] > first[0]
    assert check_bins(eng, s, small, e)[:2] == first                   # a small lattice after a large one: no stale bits
    assert check_bins(eng, s, tiny, e)[0] == 1
    assert check_bins(eng, s, big, e)[:2] == kb                        # ... and the reverse
    expect_status(eng, ERR_INVALID, e.kld_bins, grid=eng.make_mode_grid(0.0, 0.0, 0.5, 4, 4, 1025))
    expect_status(eng, ERR_INVALID, e.kld_bins, grid=eng.make_mode_grid(0.0, 0.0, -0.5, 4, 4, 4))
    assert check_bins(eng, s, big, e)[:2] == kb                        # a call after a refused call
    assert check_bins(eng, s, small, e)[:2] == first
    e.close()


def test_bins_errors(eng):
    g = eng.make_mode_grid(0.0, 0.0, 1.0, 4, 4, 4)
    e = eng.Engine(64)
    expect_status(eng, ERR_STATE, e.kld_bins, grid=g)                  # no particles yet
    e.init_particles()
    check_bins(eng, e.get_particles(), g, e)
    assert e.lib.mcl_kld_bins(e.h, None, None, None, None) == ERR_INVALID
    assert e.lib.mcl_kld_bins(None, None, None, None, None) == ERR_INVALID
    import ctypes
    assert e.lib.mcl_kld_bins(e.h, ctypes.byref(g), None, None, None) == 0      # every output may be NULL
    e.close()
    sh = eng.Engine(64, rank=0, world=2, n_global=128)
    sh.init_particles()
    expect_status(eng, ERR_UNSUPPORTED, sh.kld_bins, grid=g)
    sh.close()


def _grid_scene(eng, n, seed=5):
    origin = (-64.0, -64.0)
    z = synth.bathymetry_grid(128, 128, 1.0, origin, seed=1)
    ba = synth.beam_angles(64)
    rs = np.random.RandomState(seed)
    soa = np.zeros((6, n))
    soa[0], soa[1], soa[2] = 2.0 * rs.randn(n), 2.0 * rs.randn(n), -2.0
    soa[5] = 0.2 + 0.05 * rs.randn(n)
    t = eng.Engine(64)
    t.set_map_grid(z, origin, 1.0)
    truth = np.zeros((6, 64))
    truth[2], truth[5] = -2.0, 0.2
    t.set_particles(truth)
    ranges = t.mbes_expected(0, 1, ba, 60.0)[0].copy()
    t.close()
    return z, origin, ba, soa, ranges


COV = dict(process_cov=[0.01, 0.01, 0, 0, 0, 1e-4], resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4])


def test_bins_leave_the_handle_untouched(eng):
    n = 100003
    z, origin, ba, soa, ranges = _grid_scene(eng, n)
    a, b = eng.Engine(n, seed=9, **COV), eng.Engine(n, seed=9, **COV)
    g = eng.make_mode_grid(-8.0, -8.0, 0.25, 64, 64, 36)
    for e in (a, b):
        e.set_map_grid(z, origin, 1.0)
        e.set_particles(soa)
        e.predict([1.0, 0.0, 0.0], 0.0, [0.0, 0.0, 0.0, 1.0], -2.0, 0.5)
    k0 = a.kld_bins(grid=g)
    for e in (a, b):
        e.update_mbes(ranges, ba, 0.3, 60.0)
    assert a.kld_bins(grid=g) == k0                                    # pending log-weights are ignored
    assert np.array_equal(bits(a.get_log_weights()), bits(b.get_log_weights()))
    for e in (a, b):
        e.resample()
    a.kld_bins(grid=g)
    assert np.array_equal(a.last_indices(), b.last_indices())
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    qa, qb = a.fixed_weights(), b.fixed_weights()
    assert qa[1] == qb[1] and np.array_equal(qa[0], qb[0])
    for e in (a, b):
        e.step_mbes([1.0, 0.0, 0.0], 0.0, [0.0, 0.0, 0.0, 1.0], -2.0, 0.5, ranges, ba, 0.3, 60.0)
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    a.close()
    b.close()


# ------------------------------------------------------------------ resample_into: the index rule in Python integers
def index_sides(q, M):
    """the right-hand sides C_j M 2^53 of the index rule and T, as Python ints"""
    rhs, acc = [], 0
    for v in q:
        acc += int(v)
        rhs.append((acc * M) << 53)
    return rhs, acc


def index_ref(rhs, T, U, M):
    """idx_i = min{ j : (U + i 2^53) T < C_j M 2^53 }, i = 0 .. M - 1 (N - 1 where no j qualifies)"""
    n = len(rhs)
    return np.array([min(bisect.bisect_right(rhs, (U + (i << 53)) * T), n - 1) for i in range(M)], dtype=np.int32)


def replay_resample(twin, u):
    """mcl_resample with the caller's uniform (REPLAY mode; the normals multiply a zero covariance)"""
    twin.resample(uniforms=[u], normals=np.zeros((twin.n, 6)))


def state_of(n, seed):
    rs = np.random.RandomState(seed)
    s = rs.randn(6, n) * np.array([[30.0], [30.0], [1.0], [0.1], [0.1], [2.0]])
    return s


WEIGHT_KINDS = ('random', 'one_hot', 'nans', 'all_minus_inf')


def weights_of(kind, n, seed):
    rs = np.random.RandomState(seed)
    if kind == 'random':
        return -0.5 * (3.0 * rs.randn(n)) ** 2 - 300.0
    if kind == 'one_hot':
        lw = np.full(n, -np.inf)
        lw[(7 * n) // 11] = -12.5
        return lw
    if kind == 'nans':
        lw = -0.5 * (2.0 * rs.randn(n)) ** 2
        lw[rs.rand(n) < 0.3] = np.nan
        if n > 2:
            lw[0], lw[n - 1] = np.nan, -3.0
        return lw
    return np.full(n, -np.inf)


PAIRS = [(4096, 64), (65, 100003), (100003, 65), (1, 7), (7, 1), (1 << 20, 1 << 14)]


@pytest.mark.parametrize('N,M', PAIRS)
def test_resample_into_equals_the_index_rule_and_copies_the_state_bit_for_bit(eng, N, M):
    S = state_of(N, N + M)
    src = engine_with(eng, S, seed=3)
    twin = engine_with(eng, S, seed=3, rng_mode=eng.RNG_REPLAY)
    dst = eng.Engine(M, seed=5)
    s = 63 - max(0, (N - 1).bit_length())

    def check(rhs, T, u, label):
        src.resample_into(dst, u)
        idx = dst.transfer_indices()
        ref = index_ref(rhs, T, helpers.u53_of(u)[0], M)
        assert np.array_equal(idx, ref), (label, u, np.flatnonzero(idx != ref)[:5])
        assert np.array_equal(bits(dst.get_particles()), bits(S[:, idx])), (label, u)      # all six components, no noise
        return idx

    # ---- no pending weights at all: equal weights, q_j = 2^s
    rhs, T = index_sides([1 << s] * N, M)
    for u in (0.0, 0.37, U_LAST):
        idx = check(rhs, T, u, 'none')
        if u == 0.0:                                                   # every position sits ON an edge
            assert np.array_equal(idx, (np.arange(M, dtype=np.int64) * N) // M)
    # ---- the weights a twin's mcl_resample decides on
    for kind in WEIGHT_KINDS:
        lw = weights_of(kind, N, N)
        src.set_log_weights(lw)
        twin.set_particles(S)
        twin.set_log_weights(lw)
        replay_resample(twin, 0.5)
        q, T = twin.fixed_weights()
        rhs, T2 = index_sides(q, M)
        assert T2 == T and T > 0
        if kind == 'all_minus_inf':
            assert np.all(q == np.uint64(1 << s))                      # no finite value: equal weights
        if kind == 'nans' and np.isfinite(lw).any():                   # (N = 1: its one log-weight is the NaN -- no finite value)
            assert np.all(q[np.isnan(lw)] == 0)                        # a NaN is a particle without weight
        rs = np.random.RandomState(M)
        for u in (0.0, float(rs.random_sample()), U_LAST):
            idx = check(rhs, T, u, kind)
            if kind == 'all_minus_inf' and u == 0.0:
                assert np.array_equal(idx, (np.arange(M, dtype=np.int64) * N) // M)
            if kind == 'one_hot':
                assert np.all(idx == (7 * N) // 11)
    for e in (src, twin, dst):
        e.close()


@pytest.mark.parametrize('n', [1, 65, 4096, 100003])
def test_resample_into_with_equal_sizes_gives_the_indices_of_resample(eng, n):
    S = state_of(n, n)
    src = engine_with(eng, S, seed=3)
    twin = engine_with(eng, S, seed=3, rng_mode=eng.RNG_REPLAY)
    dst = eng.Engine(n, seed=5)
    for kind in ('random', 'nans'):
        lw = weights_of(kind, n, 2 * n)
        for u in (0.0, 0.6180339887, U_LAST):
            src.set_log_weights(lw)
            twin.set_particles(S)
            twin.set_log_weights(lw)
            replay_resample(twin, u)
            src.resample_into(dst, u)
            assert np.array_equal(dst.transfer_indices(), twin.last_indices()), (kind, u)
            # (the states differ by design: mcl_resample keeps survivors in their slots, the transfer lays the copies out in index order)
            assert np.array_equal(bits(dst.get_particles()), bits(S[:, dst.transfer_indices()]))
    for e in (src, twin, dst):
        e.close()


@pytest.mark.parametrize('weight_mode', [0, 1, 2])
def test_resample_into_takes_the_weight_mode_of_src(eng, weight_mode):
    N, M = 4097, 300
    S = state_of(N, 1)
    src, twin, dst = engine_with(eng, S), engine_with(eng, S, rng_mode=eng.RNG_REPLAY), eng.Engine(M)
    rs = np.random.RandomState(weight_mode)
    lw = rs.rand(N) if weight_mode == 2 else -0.5 * (2.0 * rs.randn(N)) ** 2 - (0.0 if weight_mode == 0 else 900.0)
    for e in (src, twin):
        e.set_log_weights(lw, weight_mode)
    replay_resample(twin, 0.5)
    q, T = twin.fixed_weights()
    rhs, _ = index_sides(q, M)
    src.resample_into(dst, 0.123)
    assert np.array_equal(dst.transfer_indices(), index_ref(rhs, T, helpers.u53_of(0.123)[0], M))
    for e in (src, twin, dst):
        e.close()


def snapshot(e, with_cdf):
    out = [bits(e.get_particles()), bits(e.get_log_weights())]
    if with_cdf:
        q, T = e.fixed_weights()
        out += [q, np.array([T], np.uint64), e.last_indices(), e.last_offspring_cdf()]
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('M', [64, 100003])
def test_src_is_untouched_its_getters_and_its_next_resample_equal_a_twins(eng, M):
    N = 4096
    z, origin, ba, soa, ranges = _grid_scene(eng, N)
    a, b = eng.Engine(N, seed=9, **COV), eng.Engine(N, seed=9, **COV)      # a is src, b the untouched twin
    dst = eng.Engine(M, seed=4)
    for e in (a, b):
        e.set_map_grid(z, origin, 1.0)
        e.set_particles(soa)
        e.predict([1.0, 0.0, 0.0], 0.0, [0.0, 0.0, 0.0, 1.0], -2.0, 0.5)
        e.update_mbes(ranges, ba, 0.3, 60.0)
        e.resample()                                                   # a resample behind it: its CDF, weights and indices are getters too
        e.predict([1.0, 0.0, 0.0], 0.0, [0.0, 0.0, 0.0, 1.0], -2.0, 0.5)
        e.update_mbes(ranges, ba, 0.3, 60.0)                           # ... and pending weights whose maximum the update left in its slots
    before = snapshot(a, True)
    a.resample_into(dst)
    a.resample_into(dst, 0.25)
    assert same(snapshot(a, True), before) and same(before, snapshot(b, True))
    q, T = None, None
    for e in (a, b):
        e.resample()
    q, T = b.fixed_weights()
    rhs, _ = index_sides(q, M)                                         # and the transfer had drawn from exactly these weights
    assert np.array_equal(dst.transfer_indices(), index_ref(rhs, T, helpers.u53_of(0.25)[0], M))
    assert same(snapshot(a, True), snapshot(b, True))
    for e in (a, b):
        e.step_mbes([1.0, 0.0, 0.0], 0.0, [0.0, 0.0, 0.0, 1.0], -2.0, 0.5, ranges, ba, 0.3, 60.0)
    assert same(snapshot(a, True), snapshot(b, True))
    for e in (a, b, dst):
        e.close()


@pytest.mark.parametrize('M', [65, 100003])
def test_dst_afterwards_behaves_as_a_handle_given_that_state_by_set_particles(eng, M):
    N = 4096
    z, origin, ba, soa, ranges = _grid_scene(eng, N)
    src = engine_with(eng, soa, seed=1)
    src.set_log_weights(weights_of('random', N, 3))
    d, t = eng.Engine(M, seed=9, **COV), eng.Engine(M, seed=9, **COV)      # d receives the transfer, t the same state by set_particles
    for e in (d, t):
        e.set_map_grid(z, origin, 1.0)
        e.init_particles()
        e.predict([1.0, 0.0, 0.0], 0.0, [0.0, 0.0, 0.0, 1.0], -7.0, 0.5)     # (z, roll and pitch are the odometry's: a stale flag would put them back)
    src.resample_into(d, 0.77)
    t.set_particles(d.get_particles())
    assert np.all(d.get_particles()[2] == -2.0)                            # src's depth, not the -7 of d's own predict
    for e in (d, t):
        e.predict([1.0, 0.1, 0.0], 0.02, [0.0, 0.0, 0.0, 1.0], -2.0, 0.5)
        e.update_mbes(ranges, ba, 0.3, 60.0)
    assert np.array_equal(bits(d.get_log_weights()), bits(t.get_log_weights()))
    for e in (d, t):
        e.resample()
    assert np.array_equal(d.last_indices(), t.last_indices())
    assert np.array_equal(bits(d.get_particles()), bits(t.get_particles()))
    # pending weights of dst are spent by the transfer
    d.update_mbes(ranges, ba, 0.3, 60.0)
    src.resample_into(d, 0.5)
    expect_status(eng, ERR_STATE, d.resample)
    for e in (src, d, t):
        e.close()


def helpers_native_u53(seed, step, purpose=3):
    x, y, _, _ = helpers.philox4x32_10(0xffffffff, 0, int(step), int(purpose), seed & 0xffffffff, seed >> 32)
    return ((int(x) >> 5) << 26) | (int(y) >> 6)


def test_native_mode_draws_with_purpose_10_from_dsts_seed_and_counts_transfers(eng):
    N, M = 4096, 1000
    S = state_of(N, 2)
    src, twin = engine_with(eng, S, seed=77), engine_with(eng, S, seed=77, rng_mode=eng.RNG_REPLAY)
    dst = eng.Engine(M, seed=SEED)
    lw = weights_of('random', N, 8)
    for e in (src, twin):
        e.set_log_weights(lw)
    replay_resample(twin, 0.5)
    q, T = twin.fixed_weights()
    rhs, _ = index_sides(q, M)
    seen = []
    for step in (0, 1, 2):                                             # the counter: + 1 per successful call
        src.resample_into(dst)
        want = index_ref(rhs, T, helpers_native_u53(SEED, step, 10), M)
        assert np.array_equal(dst.transfer_indices(), want), step
        seen.append(want)
    assert not np.array_equal(seen[0], seen[1])
    expect_status(eng, ERR_INVALID, src.resample_into, dst, 1.0)       # a refused call does not count
    src.resample_into(dst, 0.5)                                        # ... one with the caller's uniform does
    src.resample_into(dst)
    assert np.array_equal(dst.transfer_indices(), index_ref(rhs, T, helpers_native_u53(SEED, 4, 10), M))
    dst.init_particles()                                               # the filter starts again: so does the counter
    src.resample_into(dst)
    assert np.array_equal(dst.transfer_indices(), seen[0])
    assert helpers_native_u53(SEED, 0, 10) != helpers_native_u53(SEED, 0, 3)
    for e in (src, twin, dst):
        e.close()


def test_drift_states_follow_the_indices_and_drift_on_one_side_is_refused(eng):
    N, M = 4096, 777
    S = state_of(N, 4)
    src, dst = engine_with(eng, S, seed=1), eng.Engine(M, seed=2)
    src.set_log_weights(weights_of('random', N, 5))
    src.drift_enable([0.2, 0.3, 0.01], [0.0, 0.0, 0.0])
    dst.init_particles()
    before = bits(dst.get_particles())
    expect_status(eng, ERR_STATE, src.resample_into, dst, 0.3)         # exactly one of the two
    assert np.array_equal(bits(dst.get_particles()), before) and np.array_equal(bits(src.get_particles()), bits(S))
    expect_status(eng, ERR_STATE, dst.transfer_indices)
    dst.drift_enable([1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    D = src.drift_get()
    src.resample_into(dst, 0.3)
    idx = dst.transfer_indices()
    assert np.array_equal(bits(dst.drift_get()), bits(D[:, idx])) and np.array_equal(bits(dst.get_particles()), bits(S[:, idx]))
    assert np.array_equal(bits(src.drift_get()), bits(D))
    src.drift_disable()
    expect_status(eng, ERR_STATE, src.resample_into, dst, 0.3)         # ... the other one
    for e in (src, dst):
        e.close()


def test_a_dst_with_history_enabled_starts_clean(eng):
    N, M = 1000, 4096
    src, dst = engine_with(eng, state_of(N, 6)), eng.Engine(M, seed=2)
    dst.init_particles()
    dst.history_enable(4)
    dst.history_record(1.0)
    dst.history_record(2.0)
    assert dst.history_frames()[0] == 2
    src.resample_into(dst, 0.5)
    held, recorded = dst.history_frames()[:2]
    assert (held, recorded) == (0, 0)
    dst.history_record(3.0)
    assert dst.history_frames()[0] == 1 and np.array_equal(dst.history_ancestors(0), np.arange(M, dtype=np.uint32))
    for e in (src, dst):
        e.close()


def test_every_other_error_leaves_both_handles_unchanged(eng):
    N, M = 4096, 64
    S = state_of(N, 7)
    src, dst = engine_with(eng, S), eng.Engine(M, seed=2)
    src.set_log_weights(weights_of('random', N, 1))
    dst.init_particles()
    d0, s0 = bits(dst.get_particles()), snapshot(src, False)
    expect_status(eng, ERR_INVALID, src.resample_into, src, 0.5)       # src == dst
    for u in (1.0, -1e-300, 2.0, float('nan'), float('inf')):
        expect_status(eng, ERR_INVALID, src.resample_into, dst, u)
    assert src.lib.mcl_resample_into(None, dst.h, None) == ERR_INVALID and src.lib.mcl_resample_into(src.h, None, None) == ERR_INVALID
    empty = eng.Engine(N)                                              # never initialised: no particles
    expect_status(eng, ERR_STATE, empty.resample_into, dst, 0.5)
    sh = eng.Engine(N, rank=0, world=2, n_global=2 * N)
    sh.set_particles(S)
    expect_status(eng, ERR_UNSUPPORTED, sh.resample_into, dst, 0.5)    # a sharded src
    expect_status(eng, ERR_UNSUPPORTED, src.resample_into, sh, 0.5)    # ... or dst
    expect_status(eng, ERR_STATE, dst.transfer_indices)                # no transfer happened
    assert dst.lib.mcl_transfer_last_indices(None, None) == ERR_INVALID
    assert np.array_equal(bits(dst.get_particles()), d0) and same(snapshot(src, False), s0)
    assert np.array_equal(bits(sh.get_particles()), bits(S))
    src.resample_into(dst, 0.5)                                        # and the pair still works
    assert np.array_equal(bits(dst.get_particles()), bits(S[:, dst.transfer_indices()]))
    for e in (src, dst, empty, sh):
        e.close()


# ------------------------------------------------------------------ closed loop
# The global-localisation scene of tests/test_gpu_recovery.py, restated: a 192 m x 192 m synthetic bathymetry with relief
# (swell 2 m, fBm 3 m), 1 m nodes; a 64-beam fan of +-60 degrees, sigma 1.5 m; one ping per metre of track; a uniform start
# over the footprint and the full circle; seeds fixed.
LOOP_SIZES = (1 << 11, 1 << 14, 1 << 17, 1 << 20)
LOOP_SIGMA, LOOP_RMAX = 1.5, 80.0
LOOP_ORIGIN = (-96.0, -96.0)
LOOP_COV = dict(process_cov=[0.01, 0.01, 0, 0, 0, 1e-4], resample_cov=[0.09, 0.09, 0, 0, 0, 2.5e-3])


def loop_scene(eng, pings, x0=-40.0, y0=-30.0, yaw0=0.5):
    z = synth.bathymetry_grid(192, 192, 1.0, LOOP_ORIGIN, seed=2, swell=2.0, fbm_amp=3.0)
    ba = synth.beam_angles(64)
    st = synth.odom_stream(n_steps=pings, dt=1.0, x0=x0, y0=y0, yaw0=yaw0)
    t = eng.Engine(64)
    t.set_map_grid(z, LOOP_ORIGIN, 1.0)
    ranges = []
    for k in range(pings):
        t.set_particles(np.repeat(st['truth'][k][:, None], 64, axis=1))
        ranges.append(t.mbes_expected(0, 1, ba, LOOP_RMAX)[0].copy())
    t.close()
    return z, ba, st, ranges


def test_closed_loop_global_localisation_over_a_ladder_of_sizes(eng):
    """The uniform start of tests/test_gpu_recovery.py's global localisation, run with AdaptiveCloud over 2^20, 2^17, 2^14 and
    2^11 particles (cell 0.5 m, 36 yaw bins, the ladder's defaults: epsilon 0.05, headroom 2, patience 5): after 60 pings the
    mean pose is within that test's GLOBAL_BOUND of the truth, the cloud stands on fewer than 2^20 particles, and it did not
    move before the first resample.  Measured figures: DESIGN.md 5q."""
    from smarc_navigation_amd.adaptive import AdaptiveCloud, KldLadder
    pings = 60
    z, ba, st, ranges = loop_scene(eng, pings)
    engines = [eng.Engine(n, seed=17, **LOOP_COV) for n in LOOP_SIZES]
    cloud = AdaptiveCloud(engines, KldLadder(LOOP_SIZES, 0.05), cell=0.5, n_yaw=36)
    cloud.set_map_grid(z, LOOP_ORIGIN, 1.0)
    cloud.active.init_particles_uniform()
    err = []
    for k in range(pings):
        cloud.predict(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], 1.0)
        cloud.update_mbes(ranges[k], ba, LOOP_SIGMA, LOOP_RMAX)
        if k == 0:
            assert cloud.moves == 0 and cloud.active.n == 1 << 20 and cloud.trace == []      # nothing moved before the first resample
        cloud.resample(ping=k)
        mean = cloud.mean_cov()[0]
        err.append(float(np.hypot(mean[0] - st['truth'][k][0], mean[1] - st['truth'][k][1])))
    for (ping, kk, bound, size), e_ in zip(cloud.trace, err):
        print('kld loop: ping %2d  k %8d  bound %9d  size %8d  error %8.3f m' % (ping, kk, bound, size, e_))
    print('kld loop: final error %.3f m, final size %d, %d moves' % (err[-1], cloud.active.n, cloud.moves))
    final = cloud.active.n
    cloud.close()
    assert len(cloud.trace) == pings
    assert err[-1] < GLOBAL_BOUND
    assert final < 1 << 20
