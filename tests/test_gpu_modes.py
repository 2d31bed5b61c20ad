"""GPU tests of the dominant-mode pose estimate (include/mcl_modes.h; csrc/mcl_modes.h) against a numpy restatement of
the header's definition: the cell rule with true division, the set-window score, the greedy selection, math.fsum for the
moments.  Everything that decides which cells are modes is compared exactly (count, score, ix, iy, iyaw, n_modes,
n_outside); the moments within SURVEY 8(d)'s parity tolerances for mean and covariance: means 1e-9 absolute (the yaw as an
angle: the difference wrapped into [-pi, pi), and only where the resultant is not zero -- without one there is no
direction to compare), cov_xy 1e-9 relative + 1e-12 absolute, yaw_R 1e-9."""
import math

import numpy as np
import pytest

from smarc_navigation_amd import synth

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
PI = math.pi


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


# ------------------------------------------------------------------ the definition, restated
def circ(a, b, n_yaw):
    d = np.abs(a - b)
    return np.minimum(d, n_yaw - d)


def ref_cells(soa, g):
    """(ix, iy, iyaw, inside) of every particle: IEEE double subtraction, then division, then floor"""
    x0, y0, cell, nx, ny, n_yaw = g
    with np.errstate(invalid='ignore', over='ignore'):
        fx = np.floor((soa[0] - x0) / cell)
        fy = np.floor((soa[1] - y0) / cell)
        t = np.floor((soa[5] + np.pi) / ((2 * np.pi) / n_yaw))
        inside = (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny) & np.isfinite(t)
        w = np.mod(np.where(np.isfinite(t), t, 0.0), float(n_yaw))     # floored modulo; exact on integer-valued doubles
    z = np.zeros(soa.shape[1], np.int64)
    return (np.where(inside, fx, z).astype(np.int64), np.where(inside, fy, z).astype(np.int64),
            np.where(inside, w, z).astype(np.int64), inside)


def ref_modes(soa, g, k):
    x0, y0, cell, nx, ny, n_yaw = g
    ix, iy, iw, inside = ref_cells(soa, g)
    c = (iw * ny + iy) * nx + ix
    H = np.bincount(c[inside], minlength=nx * ny * n_yaw).reshape(n_yaw, ny, nx).astype(np.int64)
    P = np.zeros((n_yaw, ny + 2, nx + 2), np.int64)
    P[:, 1:-1, 1:-1] = H
    B = sum(P[:, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    S = np.zeros_like(B)
    for w in range(n_yaw):
        for b in sorted({(w - 1) % n_yaw, w, (w + 1) % n_yaw}):      # the yaw bins as a SET
            S[w] += B[b]
    alive = np.ones(S.shape, bool)
    wi, yi, xi = np.meshgrid(np.arange(n_yaw), np.arange(ny), np.arange(nx), indexing='ij')
    modes = []
    for _ in range(k):
        flat = np.where(alive, S, -1).ravel()
        best = int(np.argmax(flat))                                   # the first maximum: the lowest linear index
        if flat[best] <= 0:
            break
        pw, py, px = best // (nx * ny), (best // nx) % ny, best % nx
        alive &= ~((np.abs(xi - px) <= 2) & (np.abs(yi - py) <= 2) & (circ(wi, pw, n_yaw) <= 2))
        mem = inside & (np.abs(ix - px) <= 1) & (np.abs(iy - py) <= 1) & (circ(iw, pw, n_yaw) <= 1)
        cnt = int(mem.sum())
        cx, cy = x0 + (px + 0.5) * cell, y0 + (py + 0.5) * cell
        dx, dy = soa[0][mem] - cx, soa[1][mem] - cy
        sdx, sdy = math.fsum(dx), math.fsum(dy)
        ss, sc = math.fsum(np.sin(soa[5][mem])), math.fsum(np.cos(soa[5][mem]))
        mdx, mdy = sdx / cnt, sdy / cnt
        modes.append(dict(
            count=cnt, score=int(flat[best]), ix=px, iy=py, iyaw=pw,
            mean=np.array([cx + mdx, cy + mdy, math.fsum(soa[2][mem]) / cnt, math.fsum(soa[3][mem]) / cnt,
                           math.fsum(soa[4][mem]) / cnt, math.atan2(ss, sc)]),
            cov_xy=np.array([math.fsum(dx * dx) / cnt - mdx * mdx, math.fsum(dx * dy) / cnt - mdx * mdy,
                             math.fsum(dy * dy) / cnt - mdy * mdy]),
            yaw_R=math.hypot(ss, sc) / cnt))
    return modes, int((~inside).sum())


def wrap(a):
    return (a + PI) % (2 * PI) - PI


def check(got, n_out, ref, ref_out, what=''):
    assert n_out == ref_out, (what, n_out, ref_out)
    assert len(got) == len(ref), (what, len(got), len(ref))
    worst = dict(mean=0.0, yaw=0.0, cov=0.0, R=0.0)
    for m, (a, b) in enumerate(zip(got, ref)):
        assert (a.count, a.score, a.ix, a.iy, a.iyaw) == (b['count'], b['score'], b['ix'], b['iy'], b['iyaw']), (what, m, a, b)
        dm = np.abs(a.mean[:5] - b['mean'][:5]).max()
        dyaw = abs(wrap(a.mean[5] - b['mean'][5])) if b['yaw_R'] > 1e-6 else 0.0   # (no resultant: no direction)
        dc = np.abs(a.cov_xy - b['cov_xy'])
        worst = dict(mean=max(worst['mean'], dm), yaw=max(worst['yaw'], dyaw), cov=max(worst['cov'], dc.max()),
                     R=max(worst['R'], abs(a.yaw_R - b['yaw_R'])))
        assert dm <= 1e-9, (what, m, a.mean, b['mean'])
        assert dyaw <= 1e-9, (what, m, a.mean[5], b['mean'][5])
        assert np.all(dc <= 1e-9 * np.abs(b['cov_xy']) + 1e-12), (what, m, a.cov_xy, b['cov_xy'])
        assert abs(a.yaw_R - b['yaw_R']) <= 1e-9, (what, m, a.yaw_R, b['yaw_R'])
    print('modes %s: %d modes, n_outside %d; worst |d mean| %.2e |d yaw| %.2e |d cov| %.2e |d R| %.2e' % (
        what, len(got), n_out, worst['mean'], worst['yaw'], worst['cov'], worst['R']))


def run(eng, soa, g, k, e=None):
    """pose_modes of the state `soa` on the lattice g = (x0, y0, cell, nx, ny, n_yaw), and the restatement's answer"""
    own = e is None
    if own:
        e = eng.Engine(soa.shape[1])
    e.set_particles(soa)
    got, n_out = e.pose_modes(None, k=k, grid=eng.make_mode_grid(*g))
    if own:
        e.close()
    ref, ref_out = ref_modes(soa, g, k)
    return got, n_out, ref, ref_out


def cloud(n, seed, g, blobs=None, background=0.3):
    """1 ... 5 Gaussian blobs inside the lattice plus a uniform background that reaches beyond it"""
    x0, y0, cell, nx, ny, n_yaw = g
    rs = np.random.RandomState(seed)
    nb = int(rs.randint(1, 6)) if blobs is None else blobs
    soa = np.zeros((6, n))
    lx, ly = nx * cell, ny * cell
    soa[0] = x0 - 0.1 * lx + 1.2 * lx * rs.rand(n)
    soa[1] = y0 - 0.1 * ly + 1.2 * ly * rs.rand(n)
    soa[5] = rs.uniform(-PI, PI, n)
    which = rs.randint(0, nb, n)
    in_blob = rs.rand(n) >= background
    for b in range(nb):
        sel = in_blob & (which == b)
        k = int(sel.sum())
        soa[0][sel] = x0 + lx * rs.uniform(0.05, 0.95) + 0.4 * cell * rs.randn(k)
        soa[1][sel] = y0 + ly * rs.uniform(0.05, 0.95) + 0.4 * cell * rs.randn(k)
        soa[5][sel] = rs.uniform(-PI, PI) + 0.1 * rs.randn(k)       # (leaves [-pi, pi) now and then, like resample noise)
    soa[2] = -2.0 + 0.1 * rs.randn(n)
    soa[3], soa[4] = 0.02 * rs.randn(n), 0.02 * rs.randn(n)
    return soa


GRID = (-20.0, -15.0, 1.0, 40, 30, 12)


# ------------------------------------------------------------------ random clouds at every size
@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1023, 1025, 100003])
def test_random_clouds_equal_the_restatement(eng, n, seed):
    soa = cloud(n, 100 * seed + n % 89, GRID)
    got, n_out, ref, ref_out = run(eng, soa, GRID, 4)
    check(got, n_out, ref, ref_out, 'n=%d seed=%d' % (n, seed))
    if n >= 1023:
        assert len(got) >= 1


# ------------------------------------------------------------------ edges of the cell rule
def test_particles_on_cell_boundaries_box_edges_yaw_edges_and_non_finite_values(eng):
    x0, y0, cell, nx, ny, n_yaw = g = (-2.0, 1.0, 0.5, 8, 6, 8)
    rows = []
    for i in range(nx + 1):                                  # exact multiples of the cell: every boundary, x0 + nx cell too
        for j in range(ny + 1):
            rows.append((x0 + i * cell, y0 + j * cell, 0.1))
    rows += [(np.nextafter(x0, -np.inf), y0 + 0.25, 0.0), (x0 + 0.25, np.nextafter(y0, -np.inf), 0.0),
             (x0 + nx * cell, y0 + 0.25, 0.0), (np.nextafter(x0 + nx * cell, -np.inf), y0 + 0.25, 0.0),
             (x0, y0, 0.0), (-0.0 + x0, y0, -0.0)]
    for yaw in (-PI, PI, np.nextafter(-PI, -np.inf), np.nextafter(PI, np.inf), -PI - 0.3, PI + 0.3, 3 * PI, -5 * PI + 0.01,
                1.0e6, -1.0e6, 1.0e300, -1.0e300, 0.25 * PI, -0.25 * PI):   # (1e300: the quotient still finite)
        rows.append((x0 + 1.25, y0 + 1.25, yaw))
    for bad in (np.nan, np.inf, -np.inf):
        rows += [(bad, y0 + 0.3, 0.0), (x0 + 0.3, bad, 0.0), (x0 + 0.3, y0 + 0.3, bad)]
    rows.append((x0 + 0.3, y0 + 0.3, 1.7e308))               # the yaw quotient overflows: no cell
    soa = np.zeros((6, len(rows)))
    soa[0], soa[1], soa[5] = np.array(rows).T
    soa[2] = np.arange(len(rows))
    ix, iy, iw, inside = ref_cells(soa, g)
    # what the rule says about the hand-made rows, spelled out
    assert not inside[-1] and not inside[-10:-1].any()
    k0 = (nx + 1) * (ny + 1)
    # (the fourth: the double just below x0 + nx cell -- its difference from x0 rounds up to nx cell: outside by the rule)
    assert list(inside[k0:k0 + 6]) == [False, False, False, False, True, True]
    assert int((~inside[:k0]).sum()) == nx + ny + 1          # the far edges x0 + nx cell, y0 + ny cell are outside
    assert iw[k0 + 6] == 0 and iw[k0 + 7] == 0               # yaw = -pi and yaw = +pi share bin 0
    assert iw[k0 + 8] == n_yaw - 1 and iw[k0 + 9] == 0       # a little beyond either
    assert inside[k0 + 6:k0 + 20].all()
    for k in (1, 8):
        got, n_out, ref, ref_out = run(eng, soa, g, k)
        check(got, n_out, ref, ref_out, 'edges k=%d' % k)
    assert n_out == int((~inside).sum()) and n_out == 10 + nx + ny + 1 + 4


def test_blob_whose_yaw_straddles_pi_is_one_mode(eng):
    n = 1025
    rs = np.random.RandomState(5)
    soa = np.zeros((6, n))
    soa[0], soa[1] = 3.3 + 0.2 * rs.randn(n), -4.2 + 0.2 * rs.randn(n)
    soa[5] = PI + 0.05 * rs.randn(n)                          # unwrapped: half above pi ...
    soa[5][::2] = wrap(soa[5][::2])                           # ... and every second one wrapped to just above -pi
    got, n_out, ref, ref_out = run(eng, soa, GRID, 4)
    check(got, n_out, ref, ref_out, 'straddle')
    assert len(got) >= 1 and got[0].count > 0.9 * n
    assert abs(wrap(got[0].mean[5] - PI)) < 0.02 and got[0].yaw_R > 0.99


def test_blob_in_a_box_corner_has_a_clipped_window(eng):
    n = 1023
    rs = np.random.RandomState(6)
    soa = np.zeros((6, n))
    soa[0], soa[1] = GRID[0] + 0.3 + 0.3 * rs.randn(n), GRID[1] + 0.3 + 0.3 * rs.randn(n)   # part of it falls outside
    soa[5] = 0.1 * rs.randn(n)
    got, n_out, ref, ref_out = run(eng, soa, GRID, 2)
    check(got, n_out, ref, ref_out, 'corner')
    assert n_out > 0 and got[0].ix <= 1 and got[0].iy <= 1 and got[0].count == got[0].score


@pytest.mark.parametrize('n_yaw', [1, 2, 3])
def test_few_yaw_bins_count_no_bin_twice(eng, n_yaw):
    g = GRID[:5] + (n_yaw,)
    soa = cloud(1025, 40 + n_yaw, g)
    got, n_out, ref, ref_out = run(eng, soa, g, 4)
    check(got, n_out, ref, ref_out, 'n_yaw=%d' % n_yaw)
    assert sum(m.count for m in got) <= 1025 - n_out         # no particle in two modes, none counted twice
    if n_yaw <= 2:                                            # every yaw bin is in every window
        inside = ref_cells(soa, g)[3]
        ix, iy = ref_cells(soa, g)[0], ref_cells(soa, g)[1]
        assert got[0].count == int((inside & (np.abs(ix - got[0].ix) <= 1) & (np.abs(iy - got[0].iy) <= 1)).sum())


def test_one_cell_grid_and_every_particle_outside(eng):
    soa = cloud(1023, 9, GRID)
    g = (-5.0, -5.0, 10.0, 1, 1, 1)
    got, n_out, ref, ref_out = run(eng, soa, g, 8)
    check(got, n_out, ref, ref_out, '1x1x1')
    assert len(got) == 1 and got[0].count == 1023 - n_out and (got[0].ix, got[0].iy, got[0].iyaw) == (0, 0, 0)
    far = (1000.0, 1000.0, 1.0, 5, 5, 4)
    got, n_out, ref, ref_out = run(eng, soa, far, 8)
    check(got, n_out, ref, ref_out, 'all outside')
    assert got == [] and n_out == 1023


def _tight_blob(rs, n, x, y, yaw):
    s = np.zeros((6, n))
    s[0], s[1], s[5] = x + 0.05 * rs.randn(n), y + 0.05 * rs.randn(n), yaw + 0.01 * rs.randn(n)
    return s


def test_k_max_larger_than_the_number_of_separable_peaks(eng):
    rs = np.random.RandomState(3)
    soa = np.concatenate([_tight_blob(rs, 600, -10.5, -5.5, 0.3), _tight_blob(rs, 400, 10.5, 5.5, -2.0)], axis=1)
    got, n_out, ref, ref_out = run(eng, soa, GRID, 8)
    check(got, n_out, ref, ref_out, 'k_max 8, two blobs')
    assert len(got) == 2 and (got[0].count, got[1].count) == (600, 400)


def test_two_blobs_two_cells_apart_give_one_mode(eng):
    rs = np.random.RandomState(4)
    soa = np.concatenate([_tight_blob(rs, 700, 2.5, 3.5, 0.3), _tight_blob(rs, 325, 4.5, 3.5, 0.3)], axis=1)
    got, n_out, ref, ref_out = run(eng, soa, GRID, 4)
    check(got, n_out, ref, ref_out, 'two cells apart')
    assert len(got) == 1                                      # the second blob lies inside the first peak's suppression


def test_exact_copies_tie_and_the_lower_linear_index_wins(eng):
    g = (-8.0, -8.0, 0.5, 32, 32, 6)
    rs = np.random.RandomState(8)
    n = 512
    a = np.zeros((6, n))
    a[0] = 2.0 + rs.randint(-40, 41, n) / 64.0                # dyadic coordinates: a shift by whole cells is exact
    a[1] = -3.0 + rs.randint(-40, 41, n) / 64.0
    a[5] = 0.5 + 0.05 * rs.randn(n)
    b = a.copy()
    b[0] -= 7 * 0.5                                           # the copy lies at lower ix but HIGHER iy: iy weighs more in
    b[1] += 3 * 0.5                                           # the linear index, so the original comes first
    soa = np.concatenate([a, b], axis=1)[:, rs.permutation(2 * n)]
    got, n_out, ref, ref_out = run(eng, soa, g, 4)
    check(got, n_out, ref, ref_out, 'tie')
    assert len(got) >= 2 and got[0].score == got[1].score and got[0].count == got[1].count
    lin = [(m.iyaw * g[4] + m.iy) * g[3] + m.ix for m in got[:2]]
    assert lin[0] < lin[1]
    assert (got[1].ix - got[0].ix, got[1].iy - got[0].iy, got[1].iyaw - got[0].iyaw) == (-7, 3, 0)


def test_a_cloud_collapsed_into_one_cell_returns_the_exact_count(eng):
    n = 100003
    rs = np.random.RandomState(10)
    soa = np.zeros((6, n))
    soa[0], soa[1] = 4.0 + 0.999 * rs.rand(n), -7.0 + 0.999 * rs.rand(n)      # cell (24, 8) of GRID
    soa[5] = 0.05 + 0.4 * rs.rand(n)                                          # yaw bin 6 of 12: [0, pi / 6)
    ix, iy, iw, inside = ref_cells(soa, GRID)
    assert inside.all() and len(set(zip(ix, iy, iw))) == 1
    got, n_out, ref, ref_out = run(eng, soa, GRID, 4)
    check(got, n_out, ref, ref_out, 'one cell')
    assert len(got) == 1 and got[0].count == n and got[0].score == n and n_out == 0


# ------------------------------------------------------------------ what the call is for
def test_bimodal_cloud_the_mean_lies_on_neither_blob_the_modes_on_both(eng):
    n = 100003
    rs = np.random.RandomState(12)
    ca, cb = np.array([-25.0, 0.0]), np.array([25.0, 0.0])
    na = int(round(0.6 * n))
    soa = np.zeros((6, n))
    soa[0][:na], soa[1][:na], soa[5][:na] = ca[0] + 0.5 * rs.randn(na), ca[1] + 0.5 * rs.randn(na), 0.5 * PI + 0.05 * rs.randn(na)
    soa[0][na:], soa[1][na:], soa[5][na:] = cb[0] + 0.5 * rs.randn(n - na), cb[1] + 0.5 * rs.randn(n - na), -0.5 * PI + 0.05 * rs.randn(n - na)
    soa = soa[:, rs.permutation(n)]
    g = (-40.0, -20.0, 1.0, 80, 40, 36)
    ref, ref_out = ref_modes(soa, g, 4)
    assert len(ref) >= 2                                      # the restatement itself meets the bounds first
    assert np.hypot(*(ref[0]['mean'][:2] - ca)) <= 1.0 and np.hypot(*(ref[1]['mean'][:2] - cb)) <= 1.0
    e = eng.Engine(n)
    e.set_particles(soa)
    mean = e.mean_cov()[0]
    assert np.hypot(*(mean[:2] - ca)) > 15.0 and np.hypot(*(mean[:2] - cb)) > 15.0
    got, n_out = e.pose_modes(None, k=4, grid=eng.make_mode_grid(*g))
    check(got, n_out, ref, ref_out, 'bimodal')
    print('bimodal: mean pose (%.2f, %.2f); mode 0 (%.3f, %.3f) yaw %.3f count %d; mode 1 (%.3f, %.3f) yaw %.3f count %d' % (
        mean[0], mean[1], got[0].mean[0], got[0].mean[1], got[0].mean[5], got[0].count, got[1].mean[0], got[1].mean[1],
        got[1].mean[5], got[1].count))
    assert np.hypot(*(got[0].mean[:2] - ca)) <= 1.0 and got[0].count > got[1].count
    assert np.hypot(*(got[1].mean[:2] - cb)) <= 1.0
    assert abs(wrap(got[0].mean[5] - 0.5 * PI)) < 0.01 and abs(wrap(got[1].mean[5] + 0.5 * PI)) < 0.01
    # repeatability: a second call gives the same bits
    again, n_out2 = e.pose_modes(None, k=4, grid=eng.make_mode_grid(*g))
    assert n_out2 == n_out and [m.as_dict() for m in again] == [m.as_dict() for m in got]
    e.close()


def test_the_call_reads_the_handle_and_never_writes_it(eng):
    n = 65536
    origin = (-64.0, -64.0)
    z = synth.bathymetry_grid(128, 128, 1.0, origin, seed=1)
    ba = synth.beam_angles(64)
    rs = np.random.RandomState(5)
    soa = np.zeros((6, n))
    soa[0], soa[1], soa[2] = 2.0 * rs.randn(n), 2.0 * rs.randn(n), -2.0
    soa[5] = 0.2 + 0.05 * rs.randn(n)
    t = eng.Engine(64)
    t.set_map_grid(z, origin, 1.0)
    truth = np.zeros((6, 64))
    truth[2], truth[5] = -2.0, 0.2
    t.set_particles(truth)
    ranges = t.mbes_expected(0, 1, ba, 60.0)[0]
    t.close()
    cov = dict(resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4], seed=9)
    a, b = eng.Engine(n, **cov), eng.Engine(n, **cov)
    for e in (a, b):
        e.set_map_grid(z, origin, 1.0)
        e.set_particles(soa)
    before = a.get_particles()
    m1, o1 = a.pose_modes(1.0)                                # the map's footprint, 36 yaw bins, k = 4
    assert np.array_equal(a.get_particles(), before) and np.array_equal(before, soa)
    ref, ref_out = ref_modes(soa, (-64.0, -64.0, 1.0, 127, 127, 36), 4)
    check(m1, o1, ref, ref_out, 'footprint lattice')
    for e in (a, b):
        e.update_mbes(ranges, ba, 0.2, 60.0)
    m2, o2 = a.pose_modes(1.0)                                # between the update and the resample: pending weights ignored
    assert o2 == o1 and [m.as_dict() for m in m2] == [m.as_dict() for m in m1]
    assert np.array_equal(a.get_log_weights(), b.get_log_weights())
    a.resample()
    b.resample()                                              # ... without the call
    assert np.array_equal(a.last_indices(), b.last_indices())
    assert np.array_equal(a.get_particles(), b.get_particles())
    assert np.array_equal(a.mean_cov()[0], b.mean_cov()[0])
    a.close()
    b.close()


def test_footprint_lattice_through_a_rotated_m2o_holds_the_uniform_cloud(eng):
    m2o = synth.rigid_matrix(120.5, -45.25, 3.0, 0.0, 0.0, 0.7)
    e = eng.Engine(4096, seed=7, m2o=m2o)
    e.set_map_grid(synth.bathymetry_grid(64, 48, 1.0, (-10.0, 5.0), seed=1), (-10.0, 5.0), 1.0)
    e.init_particles_uniform()                                # over the map's footprint, carried into the odom frame
    g = e.mode_grid(2.0, 8)
    s = e.get_particles()
    assert g.x0 <= s[0].min() and s[0].max() <= g.x0 + g.nx * g.cell
    assert g.y0 <= s[1].min() and s[1].max() <= g.y0 + g.ny * g.cell
    got, n_out = e.pose_modes(2.0, n_yaw=8)
    ref, ref_out = ref_modes(s, (g.x0, g.y0, g.cell, g.nx, g.ny, g.n_yaw), 4)
    check(got, n_out, ref, ref_out, 'rotated footprint')
    assert n_out == 0
    e.close()
    tilted = eng.Engine(64, m2o=synth.rigid_matrix(1.0, 2.0, 3.0, 0.02, 0.0, 0.7))
    tilted.set_map_grid(synth.bathymetry_grid(8, 8, 1.0, (0.0, 0.0), seed=1), (0.0, 0.0), 1.0)
    tilted.init_particles()
    with pytest.raises(eng.MclError) as ei:
        tilted.pose_modes(1.0)
    assert ei.value.status == ERR_UNSUPPORTED
    assert tilted.pose_modes(1.0, box=(-4.0, 4.0, -4.0, 4.0))[1] >= 0     # a stated box needs no m2o
    tilted.close()


def expect_status(eng, status, fn, *a, **kw):
    with pytest.raises(eng.MclError) as ei:
        fn(*a, **kw)
    assert ei.value.status == status, ei.value


def test_error_cases(eng):
    g = eng.make_mode_grid(*GRID)
    e = eng.Engine(1024)
    expect_status(eng, ERR_STATE, e.pose_modes, None, grid=g)               # no particles yet
    e.init_particles()
    assert e.pose_modes(None, grid=g, k=1)[1] >= 0
    assert e.pose_modes(None, grid=g, k=8)[1] >= 0
    expect_status(eng, ERR_INVALID, e.pose_modes, None, grid=g, k=0)
    expect_status(eng, ERR_INVALID, e.pose_modes, None, grid=g, k=9)
    expect_status(eng, ERR_INVALID, e.pose_modes, None, grid=eng.make_mode_grid(0.0, 0.0, 0.0, 4, 4, 4))
    expect_status(eng, ERR_INVALID, e.pose_modes, None, grid=eng.make_mode_grid(0.0, 0.0, 1.0, 4, 4, 65))
    expect_status(eng, ERR_INVALID, e.pose_modes, None, grid=eng.make_mode_grid(0.0, 0.0, 1.0, 4097, 4096, 1))
    e.close()
    shard = eng.Engine(1024, rank=1, world=2, n_global=2048, global_offset=1024)
    shard.init_particles()
    expect_status(eng, ERR_UNSUPPORTED, shard.pose_modes, None, grid=g)     # a shard of a LOCAL group
    shard.close()


# ------------------------------------------------------------------ closed loop
def test_closed_loop_global_localisation_mode_against_mean(eng):
    """The global-localisation scenario of DESIGN.md 5d, unchanged (tests/test_gpu_recovery.py: scene, covariances, seed,
    60 pings, 1 048 576 particles), with pose_modes(cell 1 m, 36 yaw bins, the map's footprint) after every resample.
    Printed per ping: the error of mode 0 and of the mean pose.  Asserted -- what holds by construction once the cloud
    has one cluster, as 5d measured it has from the fourth ping on: at the last ping mode 0 holds at least half of the
    cloud and lies within one cell of the mean pose."""
    from tests.test_gpu_recovery import LOOP_COV, LOOP_N, LOOP_ORIGIN, LOOP_RMAX, LOOP_SIGMA, loop_scene
    pings = 60
    z, ba, st, ranges = loop_scene(eng, pings)
    e = eng.Engine(LOOP_N, seed=17, **LOOP_COV)
    e.set_map_grid(z, LOOP_ORIGIN, 1.0)
    e.init_particles_uniform()
    lattice = e.mode_grid(1.0, 36)
    assert (lattice.nx, lattice.ny, lattice.n_yaw) == (191, 191, 36)
    err_mode, err_mean, share = [], [], []
    for k in range(pings):
        e.predict(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], 1.0)
        e.update_mbes(ranges[k], ba, LOOP_SIGMA, LOOP_RMAX)
        e.resample()
        mean = e.mean_cov()[0]
        modes, n_out = e.pose_modes(None, k=4, grid=lattice)
        truth = st['truth'][k]
        err_mean.append(float(np.hypot(mean[0] - truth[0], mean[1] - truth[1])))
        err_mode.append(float(np.hypot(modes[0].mean[0] - truth[0], modes[0].mean[1] - truth[1])) if modes else float('nan'))
        share.append(modes[0].count / float(LOOP_N) if modes else 0.0)
    e.close()
    print('closed loop: error of mode 0 per ping', ' '.join('%.2f' % v for v in err_mode))
    print('closed loop: error of the mean per ping', ' '.join('%.2f' % v for v in err_mean))
    print('closed loop: share of the cloud in mode 0', ' '.join('%.3f' % v for v in share))
    assert modes and modes[0].count >= LOOP_N // 2
    assert math.hypot(modes[0].mean[0] - mean[0], modes[0].mean[1] - mean[1]) <= 1.0
