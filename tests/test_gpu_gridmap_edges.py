"""Map builder (include/mcl_map.h; kernels k_gm_add_pings, k_gm_mean, k_gm_fill in csrc/mcl_gridmap.h) at its loop,
border and rounding edges, against a reference written from the header alone:

  ref_points      4 x 4 matrices in long double, Euler composition from elementary rotations
  ref_accumulate  the documented node rule and depth quantum in fp64 numpy, integer sums
  ref_fill        Jacobi sweeps in float32 over shifted arrays, the documented neighbour order

Every case runs twice: on the C oracle (no GPU; it validates the reference and lets a mutation of the oracle's twin
lines turn a test red without a GPU) and, marked `gpu`, on the kernels.  Accumulators, means and fills are compared as
integers or float bit patterns; the one tolerance is that of the point cloud (see _oracle_multiple)."""
import functools

import numpy as np
import pytest

from smarc_navigation_amd import synth

LD = np.longdouble
FIX = 2.0 ** 20
EPS64 = float(np.finfo(np.float64).eps)


# ------------------------------------------------------------------------------------------------ the reference
def _rot4(axis, ang):
    """elementary rotation about x (0), y (1) or z (2) as a 4 x 4 long double matrix"""
    c, s = np.cos(LD(ang)), np.sin(LD(ang))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.identity(4, dtype=LD)
    m[i, i] = c
    m[j, j] = c
    m[i, j] = -s
    m[j, i] = s
    return m


def _rigid4(p6):
    """T(x, y, z) Rz(yaw) Ry(pitch) Rx(roll): the static-xyz Euler convention of mcl.h"""
    t = np.identity(4, dtype=LD)
    t[:3, 3] = [LD(v) for v in p6[:3]]
    return t.dot(_rot4(2, p6[5])).dot(_rot4(1, p6[4])).dot(_rot4(0, p6[3]))


def _valid(ranges, r_max):
    """mcl_map.h: a range is used iff 0 < r < (float)r_max, compared in float32 (NaN fails, +inf fails)"""
    with np.errstate(invalid='ignore'):
        return (ranges > np.float32(0)) & (ranges < np.float32(r_max))


def ref_points(poses, ranges, beam_angles, r_max, m2o=None, sensor_offset=None):
    """Swath points [n, B, 3] in long double: sensor pose = m2o * T(xyz) R(rpy) * T_off R_off, beam b along
    (0, sin a_b, -cos a_b) with sin / cos rounded to float32 (the beam table is single precision), NaN where the
    range is invalid."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 6)
    ba = np.asarray(beam_angles, dtype=np.float32)
    ranges = np.asarray(ranges, dtype=np.float32).reshape(poses.shape[0], ba.size)
    M = np.identity(4, dtype=LD) if m2o is None else np.asarray(m2o, dtype=np.float64).reshape(4, 4).astype(LD)
    S = _rigid4([0.0] * 6 if sensor_offset is None else sensor_offset)
    s = np.sin(ba.astype(np.float64)).astype(np.float32).astype(LD)
    c = np.cos(ba.astype(np.float64)).astype(np.float32).astype(LD)
    ok = _valid(ranges, r_max)
    out = np.full(ranges.shape + (3,), np.nan, dtype=LD)
    for p in range(poses.shape[0]):
        T = M.dot(_rigid4(poses[p])).dot(S)
        r = np.where(ok[p], ranges[p], np.float32(1)).astype(LD)
        d = np.stack([np.zeros(ba.size, LD), r * s, -(r * c), np.ones(ba.size, LD)])
        q = T.dot(d)[:3].T
        out[p][ok[p]] = q[ok[p]]
    return out


def ref_accumulate(points, nx, ny, origin, res):
    """(cnt uint32 [nx, ny], sum int64 [nx, ny]) of the points as given: node = floor((x - ox) (1 / res) + 0.5), taken when
    0 <= i < nx and 0 <= j < ny, stored at i * ny + j; quantum rint(z 2^20)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    p = p[~np.isnan(p).any(axis=1)]
    inv = 1.0 / np.float64(res)
    fi = np.floor((p[:, 0] - np.float64(origin[0])) * inv + 0.5)
    fj = np.floor((p[:, 1] - np.float64(origin[1])) * inv + 0.5)
    ok = (fi >= 0) & (fi < nx) & (fj >= 0) & (fj < ny)
    node = fi[ok].astype(np.int64) * ny + fj[ok].astype(np.int64)
    q = np.rint(p[ok, 2] * FIX).astype(np.int64)
    cnt = np.bincount(node, minlength=nx * ny).astype(np.uint32)
    acc = np.zeros(nx * ny, dtype=np.int64)
    np.add.at(acc, node, q)
    return cnt.reshape(nx, ny), acc.reshape(nx, ny)


def ref_mean(cnt, acc):
    """float32((sum / 2^20) / cnt), NaN where cnt == 0"""
    with np.errstate(invalid='ignore', divide='ignore'):
        z = ((acc.astype(np.float64) / FIX) / cnt.astype(np.float64)).astype(np.float32)
    z[cnt == 0] = np.float32(np.nan)
    return z


def ref_fill(z, passes):
    """`passes` Jacobi sweeps: an empty node takes the float32 mean of its non-empty 8-neighbours of the previous sweep,
    added in the order dx = -1..1 (outer), dy = -1..1 (inner), centre skipped.  Returns (grid, nodes still empty after the
    last sweep); stops early once no node is empty."""
    z = np.array(z, dtype=np.float32)
    nx, ny = z.shape
    empty = int(np.isnan(z).sum())
    for _ in range(int(passes)):
        if empty == 0:
            break
        pad = np.full((nx + 2, ny + 2), np.nan, dtype=np.float32)
        pad[1:-1, 1:-1] = z
        s = np.zeros((nx, ny), dtype=np.float32)
        k = np.zeros((nx, ny), dtype=np.int32)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                w = pad[1 + dx:1 + dx + nx, 1 + dy:1 + dy + ny]
                valid = ~np.isnan(w)
                s = s + np.where(valid, w, np.float32(0))
                k = k + valid
        hole = np.isnan(z)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = s / k.astype(np.float32)
        z = np.where(hole & (k > 0), mean, z).astype(np.float32)
        empty = int((hole & (k == 0)).sum())
    return z, empty


# ------------------------------------------------------------------------------------------------ the two backends
class _Oracle(object):
    """oracle.GridMapBuilder behind the interface of smarc_navigation_amd.gridmap.GridMapBuilder.  Its accumulators lie
    in front of a guard zone that must stay zero: a node index past the grid (a point accepted at i = nx, a row stride of
    nx instead of ny) is then an assertion, not a write into the heap."""

    def __init__(self, nx, ny, origin, res):
        from oracle import oracle as orc
        self.o = orc.GridMapBuilder(nx, ny, origin, res)
        self.nx, self.ny, self.origin, self.res = self.o.nx, self.o.ny, self.o.origin, self.o.res
        self.n = self.nx * self.ny
        guard = max(self.nx, self.ny) * (max(self.nx, self.ny) + 1)
        self._sum = np.zeros(self.n + guard, dtype=np.int64)
        self._cnt = np.zeros(self.n + guard, dtype=np.uint32)
        self.o.sum, self.o.cnt = self._sum[:self.n], self._cnt[:self.n]

    def add_pings(self, poses6, ranges, beam_angles, r_max, m2o=None, sensor_offset=None, want_points=False):
        pts = self.o.add_pings(poses6, ranges, beam_angles, r_max, m2o=m2o, sensor_off=sensor_offset, want_points=want_points)
        assert not self._cnt[self.n:].any() and not self._sum[self.n:].any(), 'a point was accumulated past the last node'
        return pts

    def finalize(self, fill_passes=0, want_counts=False):
        z, e = self.o.finalize(fill_passes)
        return (z, e, self.o.cnt.reshape(self.nx, self.ny).copy()) if want_counts else (z, e)

    def clear(self):
        self.o.sum[:] = 0
        self.o.cnt[:] = 0

    def close(self):
        pass


@pytest.fixture(params=[pytest.param('oracle', id='oracle'), pytest.param('gpu', id='gpu', marks=pytest.mark.gpu)])
def make(request):
    """make(nx, ny, origin, res) -> a map builder of the backend under test; closed after the test"""
    made = []

    def _make(nx, ny, origin, res):
        if request.param == 'gpu':
            from smarc_navigation_amd import gridmap
            b = gridmap.GridMapBuilder(nx, ny, origin, res)
        else:
            b = _Oracle(nx, ny, origin, res)
        made.append(b)
        return b
    yield _make
    for b in made:
        b.close()


# ------------------------------------------------------------------------------------------------ assertions
def _same_bits(a, b):
    """equal NaN pattern and equal bit patterns everywhere else (a NaN's payload is not part of the contract)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _check_exact(b, pts):
    """finalize(0) against ref_accumulate of the backend's OWN points: counts, mean bits and n_empty equal.  Returns
    (z, cnt, acc)."""
    z, empty, cnt = b.finalize(0, want_counts=True)
    rc, ra = ref_accumulate(pts, b.nx, b.ny, b.origin, b.res)
    assert np.array_equal(cnt, rc), 'hit counts differ at %d nodes' % int((cnt != rc).sum())
    assert _same_bits(z, ref_mean(rc, ra))
    assert empty == int((rc == 0).sum())
    return z, rc, ra


def _check_fill(b, z0, k):
    """finalize(k) against ref_fill(finalize(0), k): bits and n_empty; measured nodes keep their bits"""
    zk, ek = b.finalize(k)
    rk, rek = ref_fill(z0, k)
    assert _same_bits(zk, rk), 'fill with %d passes differs at %d nodes' % (
        k, int(((zk.view(np.uint32) != rk.view(np.uint32)) & ~(np.isnan(zk) & np.isnan(rk))).sum()))
    assert ek == rek
    m = ~np.isnan(z0)
    assert np.array_equal(zk.view(np.uint32)[m], z0.view(np.uint32)[m])
    return zk, ek


def _identity_points(poses, ranges, ba, r_max):
    """What the documented operations give, bit for bit in fp64, when attitude, m2o and sensor offset are identity
    (every rotation entry is exactly 0 or 1): (x, y + r s, z - r c)."""
    ba = np.asarray(ba, dtype=np.float32)
    ranges = np.asarray(ranges, dtype=np.float32).reshape(len(poses), ba.size)
    s = np.sin(ba.astype(np.float64)).astype(np.float32).astype(np.float64)
    c = np.cos(ba.astype(np.float64)).astype(np.float32).astype(np.float64)
    r = ranges.astype(np.float64)
    pts = np.stack([np.broadcast_to(poses[:, None, 0], r.shape), poses[:, None, 1] + r * s, poses[:, None, 2] + -r * c], axis=-1)
    pts[~_valid(ranges, r_max)] = np.nan
    return pts


def _stamp(b, mask, seed):
    """One nadir ping over every node of `mask`, each with its own float32 depth; returns finalize(0)'s grid."""
    rs = np.random.RandomState(seed)
    ii, jj = np.nonzero(mask)
    z0 = None
    if ii.size:
        poses = np.zeros((ii.size, 6))
        poses[:, 0] = b.origin[0] + ii * b.res
        poses[:, 1] = b.origin[1] + jj * b.res
        ranges = (10.0 + 20.0 * rs.rand(ii.size, 1)).astype(np.float32)
        pts = b.add_pings(poses, ranges, np.zeros(1, np.float32), 100.0, want_points=True)
        z0, cnt, _ = _check_exact(b, pts)
        assert np.array_equal(cnt > 0, mask)
    else:
        z0, empty = b.finalize(0)
    return z0


def _scatter(nx, ny, origin, res, n_pings, B, seed, depth=20.0):
    """Pings scattered over the grid and a margin around it (so that some points are rejected), modest attitudes"""
    rs = np.random.RandomState(seed)
    poses = np.zeros((n_pings, 6))
    poses[:, 0] = origin[0] + (rs.rand(n_pings) * (nx + 3) - 2.0) * res
    poses[:, 1] = origin[1] + (rs.rand(n_pings) * (ny + 3) - 2.0) * res
    poses[:, 2] = -2.0 + 0.5 * rs.randn(n_pings)
    poses[:, 3:5] = 0.05 * rs.randn(n_pings, 2)
    poses[:, 5] = rs.uniform(-np.pi, np.pi, n_pings)
    ba = synth.beam_angles(B, half_swath=0.6)
    ranges = (depth / np.cos(ba)[None, :] + 0.5 * rs.randn(n_pings, B)).astype(np.float32)
    return poses, ranges, ba


# ------------------------------------------------------------------------------------------------ 1. the reference, on the CPU
def test_reference_agrees_with_oracle():
    """ref_points to rounding, ref_accumulate / ref_mean and ref_fill bit for bit, against the C oracle on a survey with a
    non-trivial m2o and sensor offset on an nx != ny grid."""
    nx, ny, origin, res = 48, 70, (-20.0, -30.0), 0.75
    poses, ranges, ba = _scatter(nx, ny, origin, res, 120, 40, seed=6)
    ranges[3, 5] = np.nan
    ranges[4, :3] = -1.0
    ranges[7, 2] = 500.0
    m2o = synth.rigid_matrix(0.5, -0.25, 0.3, 0.02, -0.03, 0.4)
    off = [0.2, -0.1, -0.3, 0.01, -0.02, 0.03]
    guarded = _Oracle(nx, ny, origin, res)
    pts = guarded.add_pings(poses, ranges, ba, 60.0, m2o=m2o, sensor_offset=off, want_points=True)
    o = guarded.o
    ref = ref_points(poses, ranges, ba, 60.0, m2o=m2o, sensor_offset=off)
    assert np.array_equal(np.isnan(pts), np.isnan(ref)) and np.isnan(pts).sum() == 3 * 5
    ok = ~np.isnan(pts)
    scale = (np.abs(ref) + ranges[:, :, None].astype(LD))[ok]
    assert float(np.max(np.abs(pts[ok] - ref[ok]) / scale)) <= _M_LIMIT * EPS64
    cnt, acc = ref_accumulate(pts, nx, ny, origin, res)
    assert np.array_equal(cnt.reshape(-1), o.cnt) and np.array_equal(acc.reshape(-1), o.sum)
    z0, e0 = o.finalize(0)
    assert _same_bits(z0, ref_mean(cnt, acc)) and e0 == int((cnt == 0).sum()) and 0 < e0 < nx * ny
    last = None
    for k in (1, 2, 5, 64):
        zk, ek = o.finalize(k)
        rk, rek = ref_fill(z0, k)
        assert _same_bits(zk, rk) and ek == rek
        last = ek
    assert last == 0


# ------------------------------------------------------------------------------------------------ 2. points
def _points_setups():
    """name -> (poses, ranges, beam angles, r_max, m2o, sensor offset, (nx, ny, origin, res))"""
    out = {}
    rs = np.random.RandomState(11)
    n, B = 150, 33
    ba = synth.beam_angles(B)

    def ranges_of(seed):
        r = (15.0 + 25.0 * np.random.RandomState(seed).rand(n, B)).astype(np.float32)
        r[2, 3] = np.nan
        r[5, :2] = 0.0
        r[6, 7] = -3.0
        r[8, 1] = 90.0
        r[9, 4] = np.inf
        return r

    def poses_of(seed, att=0.2):
        q = np.random.RandomState(seed)
        p = np.zeros((n, 6))
        p[:, 0] = q.uniform(-20, 20, n)
        p[:, 1] = q.uniform(-20, 20, n)
        p[:, 2] = q.uniform(-5, 0, n)
        p[:, 3:5] = att * q.randn(n, 2)
        p[:, 5] = q.uniform(-np.pi, np.pi, n)
        return p
    grid = (96, 128, (-60.0, -70.0), 1.0)
    out['m2o'] = (poses_of(1), ranges_of(2), ba, 60.0, synth.rigid_matrix(12.0, -7.0, 3.0, 0.3, -0.4, 2.1), None, grid)
    out['offset'] = (poses_of(3), ranges_of(4), ba, 60.0, None, [0.8, -0.3, -0.45, 0.2, -0.15, 0.6], grid)
    p = poses_of(5)
    p[:, 4] = np.where(np.arange(n) % 2 == 0, 1.2, -1.2) + 0.05 * rs.randn(n)
    p[:, 5] = np.linspace(-np.pi, np.pi, n)
    p[1, 5], p[2, 5], p[3, 5], p[4, 5] = np.pi, -np.pi, np.nextafter(np.pi, 4.0), -3.1
    out['steep'] = (p, ranges_of(6), ba, 60.0, synth.rigid_matrix(1.0, 2.0, 0.5, 0.05, 0.02, -0.7), [0.1, 0.0, -0.2, 0.0, 0.1, 0.0], grid)
    p = poses_of(7)
    p[:, 0] += 651000.0
    p[:, 1] += 6452000.0
    out['far'] = (p, ranges_of(8), ba, 60.0, None, [0.2, 0.0, -0.1, 0.01, -0.02, 0.03], (200, 220, (650950.0, 6451945.0), 0.5))
    return out


# every coordinate is a sum of products through three compositions (m2o, pose, offset) and the beam: about twenty
# roundings of half an ulp each on partial sums no larger than a few times (|coordinate| + range) -- the C oracle,
# fp64 in the kernel's operation order, cannot be further from the long double reference than this many
# eps64 (|coordinate| + range)
_M_LIMIT = 16.0


@functools.lru_cache(maxsize=None)
def _points_reference():
    """name -> (reference points, oracle points, scale |coordinate| + range), computed once"""
    out = {}
    for name, (poses, ranges, ba, r_max, m2o, off, grid) in _points_setups().items():
        o = _Oracle(*grid)
        opts = o.add_pings(poses, ranges, ba, r_max, m2o=m2o, sensor_offset=off, want_points=True)
        ref = ref_points(poses, ranges, ba, r_max, m2o=m2o, sensor_offset=off)
        out[name] = (ref, opts, np.abs(ref) + ranges[:, :, None].astype(LD))
    return out


def _oracle_multiple():
    """The largest |C oracle - ref_points| over the four set-ups, in units of eps64 (|coordinate| + range)."""
    m = 0.0
    for ref, opts, scale in _points_reference().values():
        assert np.array_equal(np.isnan(ref), np.isnan(opts))
        ok = ~np.isnan(opts)
        m = max(m, float(np.max(np.abs(opts[ok] - ref[ok]) / (EPS64 * scale[ok]))))
    return m


def test_oracle_points_within_rounding_of_reference():
    """The C oracle (fp64, the kernel's operation order) against the long double reference on the four point set-ups:
    identical NaN pattern, and the measured multiple of eps64 (|coordinate| + range) that the GPU bound is built on
    stays below what the operation count allows (_M_LIMIT).  Measured: 1.75."""
    m = _oracle_multiple()
    print('oracle vs long double reference: %.3f eps64 (|coordinate| + range)' % m)
    assert 0.0 < m <= _M_LIMIT


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['m2o', 'offset', 'steep', 'far'])
def test_gpu_points_match_high_precision_reference(name):
    """add_pings(want_points=True) against ref_points: m2o with roll, pitch and yaw; a sensor offset with all six
    components; pitch near +-1.2 rad with yaw across +-pi; poses and origin near (651 000, 6 452 000) at 0.5 m.  The NaN
    pattern is identical and every coordinate is within 4 M eps64 (|coordinate| + range), where M is the largest distance
    of the fp64 C oracle from the same reference on these inputs, measured at run time (_oracle_multiple): M = 1.75, so
    the bound is 7.0 eps64 (|coordinate| + range); the factor 4 covers the device sincos differing from libm in the last
    ulp.  The accumulators of the same run are exact on the returned points."""
    from smarc_navigation_amd import gridmap
    poses, ranges, ba, r_max, m2o, off, grid = _points_setups()[name]
    ref, _, scale = _points_reference()[name]
    m = _oracle_multiple()
    g = gridmap.GridMapBuilder(*grid)
    try:
        pts = g.add_pings(poses, ranges, ba, r_max, m2o=m2o, sensor_offset=off, want_points=True)
        assert np.array_equal(np.isnan(pts), np.isnan(ref))
        ok = ~np.isnan(pts)
        err = float(np.max(np.abs(pts[ok] - ref[ok]) / (EPS64 * scale[ok])))
        print('%s: GPU %.3f, oracle %.3f, bound %.3f eps64 (|coordinate| + range)' % (name, err, m, 4.0 * m))
        assert err <= 4.0 * m
        _, cnt, _ = _check_exact(g, pts)
        assert cnt.sum() > 0.5 * ok.sum() / 3
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ 3. accumulators and mean
@pytest.mark.parametrize('B', [1, 255, 256, 257, 600])
def test_beams_per_block(make, B):
    """50 pings of B beams (the block has 256 threads): ping p sits over node row p + 1 and beam b lands on node column
    b + 1, so every (ping, beam) must be counted exactly once, in its own node, and nowhere else."""
    n, res, depth = 50, 0.25, 40.0
    nx, ny, origin = n + 2, B + 2, (-res, -(B // 2 + 1) * res)
    y = (np.arange(B) - B // 2) * res
    ba = np.arctan2(y, depth).astype(np.float32)
    ranges = np.tile(np.hypot(y, depth).astype(np.float32), (n, 1))
    poses = np.zeros((n, 6))
    poses[:, 0] = np.arange(n) * res
    poses[:, 2] = -0.125 * (np.arange(n) % 5)
    b = make(nx, ny, origin, res)
    pts = b.add_pings(poses, ranges, ba, 200.0, want_points=True)
    assert np.array_equal(pts, _identity_points(poses, ranges, ba, 200.0))
    _, cnt, _ = _check_exact(b, pts)
    want = np.zeros((nx, ny), np.uint32)
    want[1:n + 1, 1:B + 1] = 1
    assert np.array_equal(cnt, want)
    assert np.array_equal(cnt.sum(axis=1)[1:n + 1], np.full(n, B))


@pytest.mark.parametrize('n', [1, 65535, 65536, 70001])
def test_ping_grid_stride(make, n):
    """n pings of 3 beams around the cap of 65 535 workgroups: every ping's points are the known ones and are counted once"""
    nx = ny = 64
    p = np.arange(n)
    poses = np.zeros((n, 6))
    poses[:, 0] = p % 64
    poses[:, 1] = (p // 64) % 64
    poses[:, 2] = -0.125 * (p % 7)
    ba = np.array([-0.3, 0.0, 0.3], np.float32)
    ranges = np.tile((10.0 / np.cos(ba)).astype(np.float32), (n, 1))
    b = make(nx, ny, (0.0, 0.0), 1.0)
    pts = b.add_pings(poses, ranges, ba, 60.0, want_points=True)
    assert np.array_equal(pts, _identity_points(poses, ranges, ba, 60.0))
    _, cnt, _ = _check_exact(b, pts)
    # the nadir beam of ping p lands on node (p % 64, (p // 64) % 64); the side beams 3 nodes to either side, if inside
    want = np.zeros((nx, ny), np.int64)
    for dj in (-3, 0, 3):
        j = (p // 64) % 64 + dj
        ok = (j >= 0) & (j < ny)
        np.add.at(want, (p[ok] % 64, j[ok]), 1)
    assert np.array_equal(cnt, want)


def _contention(b, pose_z, node_xy):
    """len(pose_z) pings x 257 nadir beams of ranges 10 + b / 64, all over the one node at node_xy"""
    n, B = len(pose_z), 257
    poses = np.zeros((n, 6))
    poses[:, 0], poses[:, 1], poses[:, 2] = node_xy[0], node_xy[1], pose_z
    ranges = np.tile((10.0 + np.arange(B) / 64.0).astype(np.float32), (n, 1))
    return poses, b.add_pings(poses, ranges, np.zeros(B, np.float32), 100.0, want_points=True)


def test_contention_on_one_node(make):
    """4096 pings x 257 beams from one pose, all on ONE node: cnt = 1 052 672 and the mean that of the exact integer sum
    (one lost or doubled add of about 1.2e7 quanta moves the mean by 1e-5, ten float32 ulps)."""
    b = make(8, 9, (-4.0, -4.0), 1.0)
    poses, pts = _contention(b, np.full(4096, -1.5), (1.0, 2.0))
    z, cnt, acc = _check_exact(b, pts)
    assert cnt[5, 6] == 1052672 and cnt.sum() == 1052672
    quanta = np.rint((-1.5 - (10.0 + np.arange(257) / 64.0)) * FIX).astype(np.int64)
    assert int(acc[5, 6]) == 4096 * int(quanta.sum())
    assert z[5, 6] == np.float32((4096 * int(quanta.sum()) / FIX) / 1052672)


def test_mixed_sign_depths_cancel(make):
    """Poses above and below z = 0 over one node: depths 15 - r in [1, 5] and 9 - r in [-5, -1] (r = 10 + b / 64, mean 12)
    cancel to a sum of exactly 0 with cnt = 1 052 672, whose mean is +0.0, not NaN.  A second node takes the same
    cancelling pairs plus three points of 1, 2 and 4 quanta: its mean is that of a sum of exactly 7."""
    b = make(8, 9, (-4.0, -4.0), 1.0)
    _, pts = _contention(b, np.where(np.arange(4096) % 2 == 0, 15.0, 9.0), (1.0, 2.0))
    _, pts2 = _contention(b, np.where(np.arange(64) % 2 == 0, 15.0, 9.0), (-3.0, 3.0))
    assert (pts[..., 2] > 0).sum() == (pts[..., 2] < 0).sum() == 2048 * 257
    tiny = np.zeros((3, 6))
    tiny[:, 0], tiny[:, 1] = -3.0, 3.0
    tiny[:, 2] = 10.0 + np.array([1.0, 2.0, 4.0]) / FIX
    pts3 = b.add_pings(tiny, np.full((3, 1), 10.0, np.float32), np.zeros(1, np.float32), 100.0, want_points=True)
    assert np.array_equal(pts3[:, 0, 2] * FIX, [1.0, 2.0, 4.0])
    z, cnt, acc = _check_exact(b, np.concatenate([pts.reshape(-1, 3), pts2.reshape(-1, 3), pts3.reshape(-1, 3)]))
    assert cnt[5, 6] == 1052672 and acc[5, 6] == 0
    assert z[5, 6].view(np.uint32) == 0          # +0.0
    assert cnt[1, 7] == 64 * 257 + 3 and acc[1, 7] == 7
    assert z[1, 7] == np.float32((7.0 / FIX) / (64 * 257 + 3)) and z[1, 7] > 0
    assert np.isnan(z).sum() == 8 * 9 - 2


def test_borders_known_answers(make):
    """Identity attitude, one nadir beam, res = 0.5: (x - ox) / res of exactly -0.5 (node 0), -0.5 - 2^-30 (rejected),
    nx - 0.5 (rejected) and the double just below it (node nx - 1), the same along y, and every combination of the two
    (corners included).  Rejected points are still returned, finite."""
    nx, ny, ox, oy, res = 6, 5, -1.0, 0.5, 0.5
    us = [(-0.5, 0), (-0.5 - 2.0 ** -30, None), (2.0, 2), (nx - 0.5, None), (np.nextafter(nx - 0.5, 0.0), nx - 1)]
    vs = [(-0.5, 0), (-0.5 - 2.0 ** -30, None), (1.0, 1), (ny - 0.5, None), (np.nextafter(ny - 0.5, 0.0), ny - 1)]
    poses, want, depths = [], np.zeros((nx, ny), np.uint32), np.full((nx, ny), np.nan)
    for a, (u, i) in enumerate(us):
        for c, (v, j) in enumerate(vs):
            x, y = ox + u * res, oy + v * res
            # the set-up is exact: the kernel's (x - ox) * (1 / res) is u itself
            assert (x - ox) * (1.0 / res) == u and (y - oy) * (1.0 / res) == v
            poses.append([x, y, -(1.0 + a + 0.125 * c), 0.0, 0.0, 0.0])
            if i is not None and j is not None:
                want[i, j] += 1
                depths[i, j] = poses[-1][2] - 8.0
    poses = np.array(poses)
    b = make(nx, ny, (ox, oy), res)
    pts = b.add_pings(poses, np.full((len(poses), 1), 8.0, np.float32), np.zeros(1, np.float32), 60.0, want_points=True)
    assert np.isfinite(pts).all()
    assert np.array_equal(pts[:, 0, :2], poses[:, :2]) and np.array_equal(pts[:, 0, 2], poses[:, 2] - 8.0)
    z, cnt, _ = _check_exact(b, pts)
    assert np.array_equal(cnt, want) and want.sum() == 9 and want.max() == 1
    assert _same_bits(z, depths.astype(np.float32))


def test_range_validity(make):
    """mcl_map.h: a range is used iff 0 < r < (float)r_max, compared in float32.  0, -1, NaN, +inf and float32(r_max) are
    skipped, the float32 below r_max is used; an r_max that is no float32 (60.0000001) is rounded to one first, so a range
    of 60.0f is skipped although it is below that r_max as a double."""
    ba = np.zeros(1, np.float32)
    rm = np.float32(60.0)
    below = np.nextafter(rm, np.float32(0))
    ranges = np.array([0.0, -1.0, np.nan, np.inf, rm, below, 1e-30, 59.0], np.float32)[:, None]
    used = np.array([False, False, False, False, False, True, True, True])
    poses = np.zeros((len(ranges), 6))
    poses[:, 0] = np.arange(len(ranges))
    for r_max in (60.0, 60.0000001):
        assert np.float32(r_max) == rm
        b = make(10, 2, (0.0, 0.0), 1.0)
        pts = b.add_pings(poses, ranges, ba, r_max, want_points=True)
        assert np.array_equal(~np.isnan(pts[:, 0, :]), np.repeat(used[:, None], 3, axis=1))
        assert np.array_equal(pts[used, 0, 2], -ranges[used, 0].astype(np.float64))
        _, cnt, _ = _check_exact(b, pts)
        assert np.array_equal(cnt[:len(used), 0] == 1, used) and cnt.sum() == used.sum()
    # an r_max between two float32 that rounds UP admits the float32 below it
    up = 60.000002
    assert np.float32(up) > rm and float(rm) < up
    b = make(10, 2, (0.0, 0.0), 1.0)
    pts = b.add_pings(poses[:2], np.array([[rm], [np.float32(up)]], np.float32), ba, up, want_points=True)
    assert np.isfinite(pts[0]).all() and np.isnan(pts[1]).all()


def test_state_accumulates_and_clears(make):
    """Two add_pings calls accumulate; finalize is not destructive; clear() then the same pings gives the same bits."""
    nx, ny, origin, res = 37, 29, (-9.0, -7.0), 0.5
    poses, ranges, ba = _scatter(nx, ny, origin, res, 90, 17, seed=21, depth=6.0)
    b = make(nx, ny, origin, res)
    p1 = b.add_pings(poses[:40], ranges[:40], ba, 60.0, want_points=True)
    z_half, cnt_half, _ = _check_exact(b, p1)
    p2 = b.add_pings(poses[40:], ranges[40:], ba, 60.0, want_points=True)
    z, cnt, _ = _check_exact(b, np.concatenate([p1, p2]))
    assert cnt.sum() > cnt_half.sum() > 0 and np.all(cnt >= cnt_half)
    f3 = b.finalize(3)
    z_again, e_again, cnt_again = b.finalize(0, want_counts=True)
    assert _same_bits(z_again, z) and np.array_equal(cnt_again, cnt)
    f3_again = b.finalize(3)
    assert _same_bits(f3[0], f3_again[0]) and f3[1] == f3_again[1]
    b.clear()
    ze, ee, ce = b.finalize(0, want_counts=True)
    assert np.isnan(ze).all() and ee == nx * ny and not ce.any()
    b.add_pings(poses, ranges, ba, 60.0)
    z2, e2, cnt2 = b.finalize(0, want_counts=True)
    assert _same_bits(z2, z) and np.array_equal(cnt2, cnt) and e2 == e_again


def _large(make):
    """1031 x 1021 nodes (more than the 4096 x 256 threads of one mean / fill launch) under a sparse survey that also
    covers the last rows, whose node index lies beyond the first stride"""
    nx, ny, origin, res = 1031, 1021, (-500.0, -510.0), 1.0
    poses, ranges, ba = _scatter(nx, ny, origin, res, 400, 48, seed=31)
    poses[:40, 0] = origin[0] + np.linspace(1026.0, 1030.4, 40)
    b = make(nx, ny, origin, res)
    pts = b.add_pings(poses, ranges, ba, 60.0, want_points=True)
    return b, pts


def test_large_grid_beyond_first_stride(make):
    b, pts = _large(make)
    z, cnt, _ = _check_exact(b, pts)
    tail = cnt.reshape(-1)[4096 * 256:]
    assert tail.size == 1031 * 1021 - 1048576 and tail.sum() > 100 and (tail == 0).sum() > 100
    _check_fill(b, z, 2)


@pytest.mark.parametrize('shape', [(2, 2), (2, 300), (300, 2)])
def test_minimal_and_thin_grids(make, shape):
    nx, ny = shape
    origin, res = (3.0, -2.0), 0.5
    poses, ranges, ba = _scatter(nx, ny, origin, res, 60, 9, seed=41 + nx, depth=1.5)
    b = make(nx, ny, origin, res)
    pts = b.add_pings(poses, ranges, ba, 60.0, want_points=True)
    z, cnt, _ = _check_exact(b, pts)
    assert 0 < cnt.sum() < np.isfinite(pts[..., 0]).sum()      # some points land, some are rejected
    for k in (1, 2, 400):
        _check_fill(b, z, k)


# ------------------------------------------------------------------------------------------------ 4. hole filling
def test_fill_holes_on_edges_and_corners(make):
    """A measured 12 x 9 grid with holes on each edge and in each corner (single nodes, a 2 x 2 block, a run along an
    edge, an L round a corner), and one hole two nodes wide that needs a second sweep."""
    nx, ny = 12, 9
    mask = np.ones((nx, ny), bool)
    for i, j in [(0, 0), (0, ny - 1), (nx - 1, 0), (nx - 1, 1), (nx - 2, 0), (0, 4), (5, 0), (5, ny - 1), (6, ny - 1),
                 (nx - 1, 4), (nx - 1, 5), (nx - 2, 4), (nx - 2, 5), (nx - 1, ny - 1), (nx - 2, ny - 1), (nx - 1, ny - 2),
                 (3, 3), (3, 4), (3, 5), (4, 3), (4, 4), (4, 5), (5, 3), (5, 4), (5, 5)]:
        mask[i, j] = False
    b = make(nx, ny, (-3.0, 2.0), 0.5)
    z0 = _stamp(b, mask, seed=51)
    z1, e1 = _check_fill(b, z0, 1)
    assert e1 == 1 and np.isnan(z1[4, 4])
    for k in (2, 3, 4):
        zk, ek = _check_fill(b, z0, k)
        assert ek == 0 and np.isfinite(zk).all()


def test_fill_spreads_from_one_corner(make):
    """One measured node in a corner of an empty 40 x 33 grid: the filled square grows by one ring per sweep, n_empty
    falls to 0 after 39 sweeps and further sweeps change nothing."""
    nx, ny = 40, 33
    mask = np.zeros((nx, ny), bool)
    mask[nx - 1, 0] = True
    b = make(nx, ny, (0.0, 0.0), 1.0)
    z0 = _stamp(b, mask, seed=52)
    for k in (1, 2, 3):
        zk, ek = _check_fill(b, z0, k)
        filled = np.isfinite(zk)
        assert filled.sum() == (k + 1) ** 2 and filled[nx - 1 - k:, :k + 1].all() and ek == nx * ny - (k + 1) ** 2
    z38, e38 = _check_fill(b, z0, 38)
    assert e38 == ny                              # the far row is still empty
    z39, e39 = _check_fill(b, z0, 39)
    assert e39 == 0 and np.isfinite(z39).all()
    for k in (40, 41, 64):
        zk, ek = _check_fill(b, z0, k)
        assert ek == 0 and _same_bits(zk, z39)


def test_fill_of_an_empty_grid(make):
    """Nothing measured: all NaN and n_empty = nx ny for any number of passes (the pass loop runs them all and ends)"""
    nx, ny = 21, 17
    b = make(nx, ny, (0.0, 0.0), 1.0)
    for k in (0, 1, 2, 7):
        z, e, cnt = b.finalize(k, want_counts=True)
        assert np.isnan(z).all() and e == nx * ny and not cnt.any()
        assert ref_fill(z, k)[1] == nx * ny


def test_fill_of_a_full_grid(make):
    """Everything measured: any number of passes returns finalize(0) bit for bit with n_empty = 0 -- also after a fill of
    another map has left other depths in the second buffer (early stop, ping-pong buffer choice for even and odd k)."""
    nx, ny = 23, 19
    b = make(nx, ny, (0.0, 0.0), 1.0)
    holes = np.ones((nx, ny), bool)
    holes[::3, ::2] = False
    z_holes = _stamp(b, holes, seed=53)
    for k in (1, 2):
        _check_fill(b, z_holes, k)               # leaves a filled map in the ping-pong buffers
    b.clear()
    z0 = _stamp(b, np.ones((nx, ny), bool), seed=54)
    assert np.isfinite(z0).all()
    for k in (1, 4, 5):
        zk, ek = _check_fill(b, z0, k)
        assert ek == 0 and _same_bits(zk, z0)
