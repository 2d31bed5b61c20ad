"""The landmark updates at their edges (include/mcl.h: mcl_update_landmarks, mcl_update_landmarks_assign) against the
brute-force oracle: the assignment update fuzzed like the k-NN one (poses outside the grid, NaN and infinite poses, full
correlated covariances), both grid-stride loops of k_landmark_assign on their second trip, landmarks exactly on the gate
(the cell grid must cover the CLOSED gate), exact cost ties, and the k-NN update with correlated covariances and a gated
landmark in a diagonal neighbour cell.  The oracle is the reference throughout; bitwise comparisons of the kernel with
itself come on top of it, never instead."""
import numpy as np
import pytest

from smarc_navigation_amd import synth

pytestmark = pytest.mark.gpu

ISO = dict(rtol=1e-11, atol=1e-9)    # tests/test_gpu_landmark_assign.py, isotropic
MAHA = dict(rtol=1e-9, atol=1e-9)    # the same file, Mahalanobis (cofactors there, Gaussian elimination in the oracle)
EYE, OFF0 = np.identity(4), [0.0] * 6


def _rot(roll, pitch, yaw):
    """(n, 3, 3): R(static-xyz rpy) of synth.rigid_matrix, vectorised"""
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    R = np.empty((np.size(roll), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = -sp, cp * sr, cp * cr
    return R


def _map_points(soa, m2o, off, det):
    """(n, D, 3): every detection in the map frame seen from every particle, p = m2o T(x, y, z) R(rpy) T_off R_off z_d
    (plain numpy doubles; for the premises of the tests, the oracle stays the reference of the results)"""
    m2o, Mo = np.asarray(m2o, float), synth.rigid_matrix(*off)
    Rmp = np.einsum('ij,njk->nik', m2o[:3, :3], _rot(soa[3], soa[4], soa[5]))
    o = soa[:3].T.dot(m2o[:3, :3].T) + m2o[:3, 3] + Rmp.dot(Mo[:3, 3])
    Rs = Rmp.dot(Mo[:3, :3])
    return o[:, None, :] + np.einsum('nij,dj->ndi', Rs, np.asarray(det, float))


def _corr_cov(rs, m, scale):
    """m full correlated covariances (xx xy xz yy yz zz): A A^T + eps I with eps = lambda_max(A A^T) / 999, so the
    condition number is at most 1e3 (the tolerance MAHA was set for well-conditioned S)"""
    out = np.empty((m, 6))
    for j in range(m):
        A = rs.randn(3, 3) * scale * np.array([1.0, 0.6, 0.3])
        P = A.dot(A.T)
        S = P + np.linalg.eigvalsh(P)[-1] / 999.0 * np.identity(3)
        out[j] = [S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]]
    return out


def _lam_bound(s):
    """Gershgorin bound of a symmetric 3 x 3 (xx xy xz yy yz zz), as the host computes the gate radius"""
    s = np.atleast_2d(s)
    return np.max([s[:, 0] + abs(s[:, 1]) + abs(s[:, 2]), s[:, 3] + abs(s[:, 1]) + abs(s[:, 4]),
                   s[:, 5] + abs(s[:, 2]) + abs(s[:, 4])])


def _engine(soa, lm, m2o=None, cov6=None, Q6=None):
    from smarc_navigation_amd import engine as eng
    e = eng.Engine(soa.shape[1], m2o=m2o, rng_mode=eng.RNG_REPLAY)
    e.set_particles(soa)
    e.set_landmarks(lm)
    if cov6 is not None or Q6 is not None:
        e.set_landmark_noise(cov6, Q6)
    return e


def _rows_use_a_landmark_once(asg):
    for row in asg:
        used = row[row >= 0]
        if used.size != np.unique(used).size:
            return False
    return True


def _scatter_outside(soa, span, rs):
    """every fifth particle leaves the landmark grid: by one span, by several, by 1e7 and 1e9, in x, y or both"""
    far = np.arange(soa.shape[1]) % 5 == 4
    k = np.arange(far.sum())
    sx, sy = rs.choice([-1.0, 1.0], far.sum()), rs.choice([-1.0, 1.0], far.sum())
    soa[0, far] += sx * np.array([span, 3 * span + 50.0, 1e7, 1e9])[k % 4]
    soa[1, far] += sy * np.array([0.0, span, 1e9])[k % 3]
    if soa.shape[1] > 2:
        soa[0, 1] = np.nan
        soa[1, 2] = np.inf


def _scene(rs, n, n_lm, span, clustered, n_det, sigma, n_near):
    """a feature map, a cloud around one of its landmarks (a quarter with any heading) and detections of the n_near
    landmarks nearest to the cloud's centre, seen from there: fewer landmarks than detections = clashes everywhere"""
    lm = np.stack([rs.uniform(-span, span, n_lm), rs.uniform(-span, span, n_lm), rs.uniform(-3, 3, n_lm)], axis=1)
    if clustered:   # many landmarks inside one gate
        lm[:, :2] = lm[:, :2] * 0.02 + rs.uniform(-span, span, 2)
    m2o = synth.rigid_matrix(*(rs.randn(3) * 2.0), 0.0, 0.0, rs.uniform(-3, 3))
    off = list(rs.randn(6) * np.array([0.3, 0.3, 0.2, 0.02, 0.03, 0.1]))
    centre = np.linalg.solve(m2o, np.append(lm[rs.randint(n_lm)], 1.0))[:3]   # the pose that sits on a landmark
    centre[2] += 1.5
    yaw0 = rs.uniform(-3, 3)
    soa = np.zeros((6, n))
    soa[0] = centre[0] + rs.randn(n) * sigma * 3
    soa[1] = centre[1] + rs.randn(n) * sigma * 3
    soa[2] = centre[2] + rs.randn(n) * 0.3
    soa[3:5] = rs.randn(2, n) * 0.05
    soa[5] = np.where(rs.rand(n) < 0.25, rs.uniform(-3.1, 3.1, n), yaw0 + rs.randn(n) * 0.05)
    _scatter_outside(soa, span, rs)
    M = m2o.dot(synth.rigid_matrix(centre[0], centre[1], centre[2], 0.0, 0.0, yaw0)).dot(synth.rigid_matrix(*off))
    near = np.argsort(np.sum((lm - M[:3, 3]) ** 2, axis=1))[:n_near]
    seen = (lm[near] - M[:3, 3]).dot(M[:3, :3])
    det = seen[np.arange(n_det) % len(near)] + 0.7 * sigma * rs.randn(n_det, 3)
    if n_det > 2:
        det[1] = np.nan
    return lm, m2o, off, soa, det


# ---------------------------------------------------------------------------------------------- B1: assignment fuzz
# n, n_lm, span, clustered, n_det, k_cand, gate, new_mh, sigma, n_keep ('n' / 'n+5' / a number), Q given (odd seeds).
# Every value the kernel branches on is in some row: a block of 8 particles short, full, one over; a wave (4 particles
# x 16 lanes) likewise; 1 .. 3 000 landmarks; 1, 15, 16 detections; k_cand 1 .. 8; new_mh below and above the gate.
_FUZZ = [
    (1, 1, 2.0, False, 1, 1, 3.0, 2.0, 0.5, 'n', None),
    (7, 2, 2.0, False, 5, 2, 11.345, 15.0, 0.1, 'n+5', True),
    (8, 17, 30.0, False, 15, 3, 40.0, 9.0, 2.0, 1, None),
    (9, 3000, 30.0, True, 16, 8, 11.345, 11.345, 0.5, 'n', False),
    (63, 3000, 400.0, False, 16, 4, 3.0, 7.0, 2.0, 0, None),
    (64, 17, 2.0, True, 5, 5, 40.0, 50.0, 0.1, 'n', True),
    (65, 400, 30.0, False, 15, 6, 11.345, 9.0, 0.5, 'n+5', None),
    (2049, 400, 30.0, False, 16, 7, 40.0, 20.0, 0.5, 'n', False),
    (2049, 400, 400.0, True, 16, 8, 11.345, 9.0, 2.0, 'n', None),
    (700, 3000, 30.0, True, 5, 1, 3.0, 11.0, 0.1, 1, True),
    (700, 2, 2.0, False, 16, 2, 40.0, 30.0, 2.0, 'n+5', None),
    (65, 1, 2.0, False, 15, 8, 3.0, 1.0, 0.5, 'n', False),
]


@pytest.mark.parametrize('seed', range(len(_FUZZ)))
def test_assignment_fuzz_against_dense_oracle(seed):
    """Random feature maps, gates, detections (one NaN), k_cand, new-landmark costs; a fifth of the cloud outside the
    landmark grid by a span up to 1e9, a NaN pose and an infinite one (their query cell is clamped in double: no
    candidate, every detection a new landmark, as the oracle says); odd seeds with full correlated covariances, Q
    given and absent: every particle against the dense oracle, every kept assignment conflict-free and the oracle's."""
    from oracle import oracle as orc
    n, n_lm, span, clustered, n_det, k_cand, gate, new_mh, sigma, keep, with_q = _FUZZ[seed]
    rs = np.random.RandomState(300 + seed)
    lm, m2o, off, soa, det = _scene(rs, n, n_lm, span, clustered, n_det, sigma, min(n_lm, 12))
    cov6 = Q6 = None
    if seed % 2:
        cov6 = _corr_cov(rs, n_lm, 0.7 * sigma)
        Q6 = _corr_cov(rs, 1, sigma)[0] if with_q else None
        ref, rasg = orc.landmark_assign_update_maha(soa, m2o, off, lm, det, sigma, k_cand, gate, new_mh, lmcov=cov6,
                                                    Q6=Q6, want_assign=True)
        tol = MAHA
    else:
        ref, rasg = orc.landmark_assign_update(soa, m2o, off, lm, det, sigma, k_cand, gate, new_mh, want_assign=True)
        tol = ISO
    n_keep = {'n': n, 'n+5': n + 5}.get(keep, keep)
    e = _engine(soa, lm, m2o, cov6, Q6)
    asg = e.update_landmarks_assign(det, sigma, k_cand=k_cand, gate=gate, new_mh_dist=new_mh, sensor_offset=off,
                                    n_keep=n_keep)
    lw = e.get_log_weights()
    e.close()
    fin = np.isfinite(ref)
    print('seed %d: %d / %d finite, max |lw - ref| = %.3e, matched to a landmark %.3f of the oracle\'s entries'
          % (seed, fin.sum(), n, np.max(np.abs(lw[fin] - ref[fin])), np.mean(rasg >= 0)))
    assert np.array_equal(np.isfinite(lw), fin)
    np.testing.assert_allclose(lw[fin], ref[fin], **tol)
    if n_keep == 0:
        assert asg is None
        return
    kept = min(n_keep, n)
    assert asg.shape == (n_keep, n_det) and not asg[kept:].any()   # (rows past the cloud are not written)
    asg = asg[:kept]
    bad = np.isnan(det).any(axis=1)
    assert (asg[:, bad] == -2).all() and (asg[:, ~bad] >= -1).all() and (asg < n_lm).all()
    assert _rows_use_a_landmark_once(asg)
    # the detections are distinct, so the optimum is unique up to rounding: the oracle's assignment
    print('         agreement with the oracle\'s assignment %.4f' % np.mean(asg == rasg[:kept]))
    assert np.mean(asg == rasg[:kept]) >= 0.98


def test_assignment_fuzz_scenes_are_not_trivial():
    """the fuzz above would pass on "every detection a new landmark": over its scenes the oracle matches detections to
    landmarks, and conflicts (the independent cheapest choice reuses a landmark) are common  (CPU only, three seeds)"""
    from oracle import oracle as orc
    for seed in (6, 8, 10):
        n, n_lm, span, clustered, n_det, k_cand, gate, new_mh, sigma, keep, with_q = _FUZZ[seed]
        rs = np.random.RandomState(300 + seed)
        lm, m2o, off, soa, det = _scene(rs, n, n_lm, span, clustered, n_det, sigma, min(n_lm, 12))
        ref, rasg = orc.landmark_assign_update(soa, m2o, off, lm, det, sigma, k_cand, gate, new_mh, want_assign=True)
        # the independent choice: every detection alone, summed (no conflicts possible)
        alone = sum(orc.landmark_assign_update(soa, m2o, off, lm, det[d:d + 1], sigma, k_cand, gate, new_mh)
                    for d in range(n_det) if not np.isnan(det[d]).any())
        assert np.mean((rasg >= 0).any(axis=1)) > 0.5, seed   # (a fifth of the cloud is outside the grid)
        assert np.mean(alone - ref > 1e-6) > 0.3, seed
        assert np.std(ref[np.isfinite(ref)]) > 0.5, seed


# ---------------------------------------------------------------------------------------------- B2, B3: the strides
def _stride_subset(n, extra=()):
    return np.unique(np.concatenate([np.arange(64), np.arange(0, n, 61), np.arange(n - 64, n), np.asarray(extra, int)]))


def _check_subset(soa, lm, m2o, off, det, sigma, k_cand, gate, new_mh, idx, lw, asg, tied=()):
    """the oracle on the particles idx, and a second engine that holds only them (one loop trip): a particle's
    log-likelihood and assignment are a function of the particle alone, so bit for bit the same"""
    from oracle import oracle as orc
    sub = np.ascontiguousarray(soa[:, idx])
    ref, rasg = orc.landmark_assign_update(sub, m2o, off, lm, det, sigma, k_cand, gate, new_mh, want_assign=True)
    print('subset of %d: max |lw - ref| = %.3e' % (idx.size, np.max(np.abs(lw[idx] - ref))))
    np.testing.assert_allclose(lw[idx], ref, **ISO)
    e = _engine(sub, lm, m2o)
    asg_sub = e.update_landmarks_assign(det, sigma, k_cand=k_cand, gate=gate, new_mh_dist=new_mh, sensor_offset=off,
                                        n_keep=idx.size)
    lw_sub = e.get_log_weights()
    e.close()
    assert np.array_equal(lw[idx], lw_sub)
    assert np.array_equal(asg[idx], asg_sub)
    assert _rows_use_a_landmark_once(asg[idx])
    a, r = asg[idx].copy(), rasg.copy()
    if tied:   # bit-identical detections: which of them gets which landmark is not defined, the pair is
        a[:, tied], r[:, tied] = np.sort(a[:, tied], axis=1), np.sort(r[:, tied], axis=1)
    print('          agreement with the oracle\'s assignment %.4f' % np.mean(a == r))
    assert np.mean(a == r) >= 0.98
    return ref


def test_solver_worklist_longer_than_one_grid_trip():
    """k_landmark_assign<true> runs at most 2 048 blocks x 8 worklist entries per trip.  2 x 16 384 + 13 particles that
    ALL clash (detections 0 and 1 are bit-identical and their nearest landmark is cheaper than min(gate, new_mh) for
    every particle): the solver's loop makes a third trip, re-initialising u / v / p / flag in LDS each time."""
    rs = np.random.RandomState(41)
    n = 2 * 16384 + 13
    sigma, k_cand, gate, new_mh = 0.6, 8, 11.345, 9.0
    lm = np.stack([rs.uniform(-3, 3, 40), rs.uniform(-3, 3, 40), rs.uniform(-1, 1, 40)], axis=1)
    m2o = synth.rigid_matrix(0.5, -0.5, 0.0, 0.0, 0.0, 0.3)
    off = [0.1, 0.0, -0.2, 0.0, 0.01, 0.0]
    soa = rs.randn(6, n) * np.array([0.05, 0.05, 0.02, 0.005, 0.005, 0.01])[:, None]
    M = m2o.dot(synth.rigid_matrix(*off))
    det = rs.uniform(-2.5, 2.5, size=(16, 3)) * np.array([1.0, 1.0, 0.3])
    det[0] = (lm[np.argmin(np.sum(lm[:, :2] ** 2, axis=1))] - M[:3, 3]).dot(M[:3, :3]) + 0.05
    det[1] = det[0]
    assert det[1].tobytes() == det[0].tobytes()
    # the premise: every particle clashes, the worklist holds all n
    p0 = _map_points(soa, m2o, off, det[:1])[:, 0]
    cost = np.min(np.sum((p0[:, None, :] - lm[None]) ** 2, axis=2), axis=1) / sigma ** 2
    print('cheapest edge of detection 0: %.4f .. %.4f' % (cost.min(), cost.max()))
    assert cost.max() < 0.5 * min(gate, new_mh)
    e = _engine(soa, lm, m2o)
    asg = e.update_landmarks_assign(det, sigma, k_cand=k_cand, gate=gate, new_mh_dist=new_mh, sensor_offset=off, n_keep=n)
    lw = e.get_log_weights()
    e.close()
    assert np.all(np.isfinite(lw))
    both = (asg[:, 0] >= 0) & (asg[:, 1] >= 0)
    assert np.all(asg[both, 0] != asg[both, 1])
    _check_subset(soa, lm, m2o, off, det, sigma, k_cand, gate, new_mh, _stride_subset(n), lw, asg, tied=[0, 1])


def test_fast_kernel_cloud_longer_than_one_grid_trip():
    """k_landmark_assign<false> runs at most 32 768 blocks x 8 particles per trip.  262 144 + 8 x 2 048 + 5 particles
    over a sparse map, clashes rare -- and 300 particles placed where detections 14 and 15 see the same lone landmark,
    every other one of two runs of blocks, one run on the second trip: a clashing particle `continue`s beside answered
    ones under the barrier at the loop's top.  Then accumulate on top of it."""
    rs = np.random.RandomState(43)
    n = 262144 + 8 * 2048 + 5
    sigma, k_cand, gate, new_mh = 0.3, 8, 11.345, 9.0
    lone, probe = np.array([70.0, 70.0, -10.0]), np.array([5.0, 0.0, -8.0])
    lm = np.stack([rs.uniform(-90, 90, 200), rs.uniform(-90, 90, 200), rs.uniform(-12, -8, 200)], axis=1)
    keep = (np.hypot(lm[:, 0] - lone[0], lm[:, 1] - lone[1]) > 8.0) & (np.hypot(lm[:, 0] - 5.0, lm[:, 1]) > 4.0)
    lm = np.vstack([lm[keep], lone])
    soa = rs.randn(6, n) * np.array([0.1, 0.1, 0.05, 0.005, 0.005, 0.005])[:, None]
    soa[2] -= 2.0
    near = np.argsort(np.sum(lm[:, :2] ** 2, axis=1))[:14]
    det = np.vstack([lm[near] - [0.0, 0.0, -2.0] + 0.05 * rs.randn(14, 3), probe, probe + [0.02, 0.0, 0.0]])
    placed = np.concatenate([1001 + 2 * np.arange(150), 262144 + 1 + 2 * np.arange(150)])   # odd slots of their blocks
    soa[0, placed] += lone[0] - probe[0]
    soa[1, placed] += lone[1] - probe[1]
    blocks = np.unique(placed // 8)
    mates = np.setdiff1d((blocks[:, None] * 8 + np.arange(8)).ravel(), placed)
    assert placed.max() < n and (placed[150:] // 8 >= 32768).all() and (placed[:150] // 8 < 32768).all()
    idx = _stride_subset(n, np.concatenate([placed, mates]))

    # the premise, in numpy on the subset: which particles clash = two detections whose cheapest edge (cheaper than
    # the new-landmark hypothesis, inside the gate) leads to the same landmark
    def clashes(which):
        P = _map_points(soa[:, which], EYE, OFF0, det)
        out = np.zeros(which.size, bool)
        seen = np.full((which.size, 16), -1)
        for d in range(16):
            m = np.sum((P[:, d, None, :] - lm[None]) ** 2, axis=2) / sigma ** 2
            j = np.argmin(m, axis=1)
            seen[:, d] = np.where(m[np.arange(which.size), j] < min(gate, new_mh), j, -1 - d)
        for d in range(16):
            out |= np.any(seen[:, d, None] == seen[:, d + 1:], axis=1)
        return out
    assert clashes(placed).all() and not clashes(mates).any()
    rate = clashes(np.arange(0, n, 61)).mean()
    print('clash rate of the cloud %.4f' % rate)
    assert rate < 0.05

    e = _engine(soa, lm)
    asg = e.update_landmarks_assign(det, sigma, k_cand=k_cand, gate=gate, new_mh_dist=new_mh, n_keep=n)
    base = e.get_log_weights()
    assert np.all(np.isfinite(base))
    assert ((asg[placed, 14] == len(lm) - 1) ^ (asg[placed, 15] == len(lm) - 1)).all()
    assert (np.minimum(asg[placed, 14], asg[placed, 15]) == -1).all()
    ref = _check_subset(soa, lm, EYE, OFF0, det, sigma, k_cand, gate, new_mh, idx, base, asg)
    assert np.std(ref) > 1.0
    e.update_landmarks_assign(det, sigma, k_cand=k_cand, gate=gate, new_mh_dist=new_mh, accumulate=True)
    lw2 = e.get_log_weights()
    e.close()
    np.testing.assert_allclose(lw2[idx], base[idx] + ref, **ISO)
    assert np.array_equal(lw2, base + base)   # (x + x is exact: every particle of both trips added the same value)


# ---------------------------------------------------------------------------------------------- B4: the gate itself
# (gate radius = cell, sigma, gate): three radii whose product with their rounded reciprocal is below 1; 98 and 103 with
# sigma = 1 and again with a gate below the new-landmark cost of 100, so that the assignment has a reason to use them
_GATE_SCENES = [(49.0, 7.0, 49.0), (98.0, 1.0, 9604.0), (103.0, 1.0, 10609.0), (98.0, 14.0, 49.0), (103.0, 51.5, 4.0)]


def _gate_scene(cs, sigma, gate, mirror, inward=0.0):
    """pose 0 = the origin, detection (0, 0, 0), identity frames; a landmark ON the gate along x (y when mirrored), one
    at maha = gate - 1 along the other axis, one far away that spans the grid.  The grid starts one cell below the
    smallest landmark coordinate (0), so the origin sits on the corner of four cells: 200 more poses jittered by
    +-1e-9 .. +-1e-3 in x and y cross both cell boundaries."""
    assert sigma * np.sqrt(gate) == cs   # the gate radius the host computes, exactly
    assert cs * (1.0 / cs) < 1.0         # ... and the reason a cell of exactly that size lost the landmark
    lm = np.array([[0.0, 1000.0, 0.0], [cs * (1.0 - inward), 0.0, 0.0], [0.0, sigma * np.sqrt(gate - 1.0), 0.0]])
    rs = np.random.RandomState(int(cs))
    soa = np.zeros((6, 201))
    soa[:2, 1:] = rs.choice([-1.0, 1.0], (2, 200)) * 10.0 ** rs.uniform(-9, -3, (2, 200))
    soa[0, 1:9] = [1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3, 1e-9, -1e-9]
    soa[1, 1:9] = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1e-9, -1e-9]
    # no other pose may put the landmark within rounding of the gate (long double, from the definition in mcl.h)
    ld = np.longdouble
    m = ((ld(lm[1, 0]) - soa[0].astype(ld)) ** 2 + soa[1].astype(ld) ** 2) / (ld(sigma) * ld(sigma))
    clear = np.abs(m - ld(gate)) > 1e-12 * gate
    assert clear[1:].all() and (inward > 0.0 or m[0] == gate)
    assert (m < gate).sum() > 40 and (m > gate).sum() > 40
    if mirror:
        lm, soa = lm[:, [1, 0, 2]].copy(), soa[[1, 0, 2, 3, 4, 5]].copy()
    return lm, soa


@pytest.mark.parametrize('mirror', [False, True])
@pytest.mark.parametrize('cs,sigma,gate', _GATE_SCENES)
def test_knn_sees_a_landmark_exactly_on_the_gate(cs, sigma, gate, mirror):
    """maha == gate is inside the k-NN gate (<=).  With cells of exactly the gate radius the query at p - x0 = cs fell
    into cell 0 (cs * (1 / cs) < 1) and the landmark at 2 cs into cell 2: outside the 3 x 3 neighbourhood, and the
    answer short of log(1 + exp(-1/2)) = 0.47.  landmarks_build makes the cells a relative 2^-30 larger."""
    from oracle import oracle as orc
    lm, soa = _gate_scene(cs, sigma, gate, mirror)
    det = np.zeros((1, 3))
    ref = orc.landmark_update(soa, EYE, OFF0, lm, det, sigma, 2, gate)
    without = orc.landmark_update(soa[:, :1].copy(), EYE, OFF0, lm[[0, 2]], det, sigma, 2, gate)
    assert abs(ref[0] - without[0] - np.log1p(np.exp(-0.5))) < 1e-9    # the landmark on the gate counts
    e = _engine(soa, lm)
    e.update_landmarks(det, sigma, k=2, gate=gate)
    lw = e.get_log_weights()
    e.close()
    print('pose 0: lw %.15g, oracle %.15g, oracle without the landmark on the gate %.15g' % (lw[0], ref[0], without[0]))
    np.testing.assert_allclose(lw, ref, **ISO)


@pytest.mark.parametrize('mirror', [False, True])
@pytest.mark.parametrize('cs,sigma,gate', _GATE_SCENES)
def test_assignment_sees_a_landmark_just_inside_the_gate(cs, sigma, gate, mirror):
    """The assignment's gate is strict (<), the kernel computes |p - l|^2 * (1 / sigma^2) and the oracle |p - l|^2 /
    sigma^2: ON the gate the two may fall on different sides, so the landmark is moved one part in 1e9 inward, where
    both say inside for pose 0 (and _gate_scene keeps every jittered pose 1e-12 clear of the gate).  One detection as
    in the k-NN scene, and two bit-identical ones, so that the landmark near the gate is part of the optimum; new_mh =
    100: in the scenes with sigma = 1 (gate 9 604, 10 609) a new landmark is then cheaper than either gated one and the
    scene only says that nothing else breaks; in the other three the gated landmarks win."""
    from oracle import oracle as orc
    lm, soa = _gate_scene(cs, sigma, gate, mirror, inward=1e-9)
    e = _engine(soa, lm)
    for n_det in (1, 2):
        det = np.zeros((n_det, 3))
        ref = orc.landmark_assign_update(soa, EYE, OFF0, lm, det, sigma, 8, gate, 100.0)
        asg = e.update_landmarks_assign(det, sigma, k_cand=8, gate=gate, new_mh_dist=100.0, n_keep=1)
        np.testing.assert_allclose(e.get_log_weights(), ref, err_msg='%d detections' % n_det, **ISO)
        if n_det == 2 and gate < 100.0:
            assert sorted(asg[0]) == [1, 2]   # pose 0: the landmark near the gate and the one at gate - 1
            assert np.std(ref) > 1.0          # (the jittered poses outside the gate pay for a new landmark)
    e.close()


# ---------------------------------------------------------------------------------------------- B5: exact ties
def _tie_cloud(seed, n=65):
    rs = np.random.RandomState(seed)
    return rs.randn(6, n) * np.array([0.03, 0.03, 0.02, 0.005, 0.005, 0.01])[:, None]


@pytest.mark.parametrize('copies', [2, 3])
def test_duplicate_landmarks_give_equal_edges_to_different_columns(copies):
    """two / three landmarks with the same coordinates, two detections near them, five landmarks at most inside a gate
    (<= k_cand: the truncation does not meet the tie): both detections' cheapest edge is the first copy, the solver
    gives them different copies -- which ones is not defined, the total is."""
    from oracle import oracle as orc
    lm = np.array([[1.0, 0.0, -5.0]] * copies + [[1.6, 0.2, -5.0], [-20.0, 30.0, -5.0], [40.0, -10.0, -5.0]])
    det = np.array([[1.05, 0.0, -5.0], [0.95, 0.05, -5.0]])
    soa = _tie_cloud(51)
    sigma, gate, new_mh = 0.5, 11.345, 9.0
    ref = orc.landmark_assign_update(soa, EYE, OFF0, lm, det, sigma, 8, gate, new_mh)
    e = _engine(soa, lm)
    asg = e.update_landmarks_assign(det, sigma, k_cand=8, gate=gate, new_mh_dist=new_mh, n_keep=soa.shape[1])
    np.testing.assert_allclose(e.get_log_weights(), ref, **ISO)
    e.close()
    assert ((asg >= 0) & (asg < copies)).all() and (asg[:, 0] != asg[:, 1]).all()


@pytest.mark.parametrize('above', [True, False])
def test_two_identical_detections_and_one_landmark(above):
    """bit-identical detections always clash: with the new-landmark cost above the landmark's one of them gets the
    landmark and the other a new one, below it both get a new one."""
    from oracle import oracle as orc
    lm = np.array([[2.0, 0.0, -3.0], [50.0, 50.0, -3.0]])
    det = np.array([[2.1, 0.0, -3.0]] * 2)
    soa = _tie_cloud(52)
    sigma, gate = 0.5, 11.345
    cost = np.sum((_map_points(soa, EYE, OFF0, det[:1])[:, 0] - lm[0]) ** 2, axis=1) / sigma ** 2
    new_mh = 9.0 if above else 0.5 * cost.min()
    assert cost.max() < 9.0 and cost.min() > 1e-3
    ref = orc.landmark_assign_update(soa, EYE, OFF0, lm, det, sigma, 8, gate, new_mh)
    e = _engine(soa, lm)
    asg = e.update_landmarks_assign(det, sigma, k_cand=8, gate=gate, new_mh_dist=new_mh, n_keep=soa.shape[1])
    np.testing.assert_allclose(e.get_log_weights(), ref, **ISO)
    e.close()
    assert (np.sort(asg, axis=1) == ([-1, 0] if above else [-1, -1])).all()


def test_sixteen_identical_detections_over_eight_landmarks():
    """the longest augmenting chains the solver can see: every detection has the same eight edges, detection d finds
    the first min(d, 8) columns taken.  Eight detections end on the eight landmarks, eight on a new one."""
    from oracle import oracle as orc
    rs = np.random.RandomState(53)
    lm = np.vstack([[3.0, 0.0, -4.0] + rs.uniform(-0.6, 0.6, (8, 3)), [[60.0, 0.0, -4.0]]])
    det = np.array([[3.0, 0.0, -4.0]] * 16)
    soa = _tie_cloud(54)
    sigma, gate, new_mh = 0.5, 40.0, 30.0
    P = _map_points(soa, EYE, OFF0, det[:1])[:, 0]
    cost = np.sum((P[:, None, :] - lm[None, :8]) ** 2, axis=2) / sigma ** 2
    assert cost.max() < 0.9 * new_mh
    ref = orc.landmark_assign_update(soa, EYE, OFF0, lm, det, sigma, 8, gate, new_mh)
    e = _engine(soa, lm)
    asg = e.update_landmarks_assign(det, sigma, k_cand=8, gate=gate, new_mh_dist=new_mh, n_keep=soa.shape[1])
    np.testing.assert_allclose(e.get_log_weights(), ref, **ISO)
    e.close()
    assert (np.sort(asg, axis=1) == [-1] * 8 + list(range(8))).all()


# ---------------------------------------------------------------------------------------------- B6: k-NN, correlated
@pytest.mark.parametrize('seed', [0, 1])
def test_knn_fuzz_with_correlated_covariances(seed):
    """The k-NN fuzz of tests/test_gpu_landmarks.py with full correlated covariances (its own are diagonal): the cell
    grid's radius rests on Gershgorin bounds, which only differ from the diagonal with off-diagonal terms.  Pose 0 and
    landmark 0 are placed either side of a cell corner, so a gated landmark lies in a DIAGONAL neighbour cell -- read
    from the oracle's table, the cells from the builder's own arithmetic."""
    from oracle import oracle as orc
    rs = np.random.RandomState(500 + seed)
    n, n_lm, span, sigma, gate, k = (65, 700)[seed], 1200, 20.0, 0.5, 11.345, 2 + seed
    lm, m2o, off, soa, det = _scene(rs, n, n_lm, span, False, 17, sigma, 12)
    cov6 = _corr_cov(rs, n_lm, 0.7 * sigma)
    Q6 = _corr_cov(rs, 1, sigma)[0] if seed == 0 else None
    # the builder's grid (landmarks_build): radius from the Gershgorin bounds, cells a relative 2^-30 larger
    lam_q = _lam_bound(Q6) if Q6 is not None else sigma ** 2
    r = np.sqrt(gate * (_lam_bound(cov6) + lam_q))
    cs = r * (1.0 + 2.0 ** -30)
    x0, y0 = lm[1:, 0].min() - cs, lm[1:, 1].min() - cs
    centre = _map_points(soa[:, :1], m2o, off, det[:1])[0, 0]
    corner = np.array([x0 + np.floor((centre[0] - x0) / cs) * cs, y0 + np.floor((centre[1] - y0) / cs) * cs])
    lm[0, :2] = corner + 1e-3 * r
    assert lm[1:, 0].min() < lm[0, 0] < lm[1:, 0].max() and lm[1:, 1].min() < lm[0, 1] < lm[1:, 1].max()
    want = np.array([corner[0] - 1e-3 * r, corner[1] - 1e-3 * r, lm[0, 2]])
    soa[:3, 0] += np.linalg.solve(m2o[:3, :3], want - centre)   # (p is affine in the pose's position)
    p = _map_points(soa[:, :1], m2o, off, det[:1])[0, 0]
    cell = lambda x, y, scale: (np.floor(scale(x - x0)), np.floor(scale(y - y0)))
    qc, lc = cell(p[0], p[1], lambda v: v * (1.0 / cs)), cell(lm[0, 0], lm[0, 1], lambda v: v / cs)
    assert lc[0] - qc[0] == 1 and lc[1] - qc[1] == 1
    _, _, tab = orc.landmark_assign_update_maha(soa[:, :1].copy(), m2o, off, lm, det, sigma, n_lm, gate, gate, lmcov=cov6,
                                                Q6=Q6, want_assign=True, want_table=True)
    print('landmark 0 from pose 0, detection 0: maha %.4f (gate %g); gated landmarks per detection %s'
          % (tab[0, 0], gate, (tab[:n_lm] < 10000.0).sum(axis=0)))
    assert tab[0, 0] < gate
    ref = orc.landmark_update_maha(soa, m2o, off, lm, det, sigma, k, gate, lmcov=cov6, Q6=Q6)
    e = _engine(soa, lm, m2o, cov6, Q6)
    e.update_landmarks(det, sigma, k=k, gate=gate, sensor_offset=off)
    lw = e.get_log_weights()
    e.close()
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(lw), fin) and fin.sum() > 0.7 * n
    print('max |lw - ref| = %.3e' % np.max(np.abs(lw[fin] - ref[fin])))
    np.testing.assert_allclose(lw[fin], ref[fin], rtol=1e-10, atol=1e-8)   # the k-NN fuzz's own bounds
    assert np.std(ref[fin]) > 0.5
