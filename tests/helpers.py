"""Shared test helpers: golden loading and the scenario replay driver.

The replay driver re-enacts what oracle/ref_harness/gen_golden.py did to the reference node
(odom_callback per sample, update+resample per GPS fix, loc_loop per publish tick) against a
`backend` object, regenerating the reference's RNG draws from the recorded seed
(numpy legacy RandomState stream, consumption order SURVEY.md A.1)."""
import bisect
import fractions
import os

import numpy as np

from smarc_navigation_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def host_threads():
    """Host threads worth giving the oracle's OpenMP loops: the affinity mask capped by the cgroup CPU quota (the GPU
    box shows 256 hardware threads but grants 16 CPUs of time; oversubscribing them is slower)."""
    cores = len(os.sched_getaffinity(0))
    try:
        with open('/sys/fs/cgroup/cpu.max') as f:
            quota, period = f.read().split()[:2]
        if quota != 'max':
            cores = max(1, min(cores, int(-(-int(quota) // int(period)))))
    except (IOError, ValueError):
        pass
    return cores


def load(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)


class OracleBackend(object):
    """Reference-exact CPU oracle (fp64, reference resamplers)."""

    def __init__(self, g, resampler):
        from oracle import oracle as orc
        self.orc = orc
        self.n = int(g['n'])
        self.m2o = g['m2o']
        self.meas_std = float(g['meas_std'])
        self.motion_cov = g['motion_cov']
        self.res_cov = g['res_cov']
        self.resampler = resampler
        self.soa = np.zeros((6, self.n))
        self.last_indices = None
        self.last_w_raw = None
        self.last_w_norm = None

    def init(self, init_cov, normals):
        self.orc.add_noise(self.soa, init_cov, normals)

    def predict(self, v, wz, q, z, dt, normals):
        self.orc.predict(self.soa, v, wz, q, z, dt, self.motion_cov, normals)

    def update_resample(self, gx, gy, rs):
        w_raw, _ = self.orc.gps_weights(self.soa, self.m2o, gx, gy, self.meas_std)
        self.last_w_raw = w_raw + 1e-200
        w = self.orc.normalise_ref(w_raw)
        self.last_w_norm = w
        if self.resampler == 'systematic':
            idx, rc = self.orc.systematic_ref(w, rs.random_sample())
            assert rc == 0
        else:
            k = self.orc.residual_k(w)
            idx, k2 = self.orc.residual_ref(w, rs.random_sample(self.n - k))
            assert k == k2
        self.last_indices = idx
        lost, dupes = self.orc.lost_dupes(idx)
        self.orc.reassign(self.soa, lost, dupes)
        self.orc.add_noise(self.soa, self.res_cov, rs.randn(self.n, 6))

    def state(self):
        return self.orc.from_soa(self.soa)

    def mean_cov(self):
        return self.orc.mean_cov(self.soa)


def replay(g, backend, check=None):
    """Runs the golden scenario on `backend`; returns dict of produced observables."""
    n, n_steps = int(g['n']), int(g['n_steps'])
    stream = synth.odom_stream(n_steps)
    rs = np.random.RandomState(int(g['seed']))
    backend.init(g['init_cov'], rs.randn(n, 6))
    out = dict(init_state=backend.state(), ckpt_states=[], mean=[], yaw=[], cov=[], post_update_states=[],
               indices=[], weights_raw=[], weights_norm=[])
    fix_idx = list(g['fix_idx'])
    fix_xy = g['fix_xy_map']
    pub_every = int(g['pub_every'])
    fp = 0
    old_t = stream['t0']
    for k in range(n_steps):
        t = stream['stamp'][k]
        backend.predict(stream['v'][k], stream['wz'][k], stream['q'][k], stream['z'][k], t - old_t,
                        rs.randn(n, 6))
        old_t = t
        if fp < len(fix_idx) and fix_idx[fp] == k:
            backend.update_resample(fix_xy[fp][0], fix_xy[fp][1], rs)
            out['post_update_states'].append(backend.state())
            out['indices'].append(backend.last_indices)
            out['weights_raw'].append(backend.last_w_raw)
            out['weights_norm'].append(backend.last_w_norm)
            fp += 1
        if (k + 1) % pub_every == 0 or k == n_steps - 1:
            m, y, c = backend.mean_cov()
            out['mean'].append(m)
            out['yaw'].append(y)
            out['cov'].append(c)
        if (k + 1) % 25 == 0 or k == n_steps - 1:
            out['ckpt_states'].append(backend.state())
    return out


def outliers_explained(orc, omap, soa, ba, got, ref, r_max, m2o=None, off=None, tol=1e-3, delta=1e-3, label=''):
    """The a15 tolerance contract where it is relaxed (fp32 expected range within 1e-3 m of the fp64 oracle).
    A beam that grazes a crest or a triangle edge is ill-conditioned: the last bit of fp32 decides between the crest and
    the shadow behind it, and the range jumps by metres.  Tests therefore tolerate a bounded NUMBER of rays beyond the
    tolerance -- and this function bounds HOW FAR off such a ray may be: every ray further than `tol` from the oracle
    must be, within `tol`, an answer the fp64 oracle itself gives when the sensor moves by `delta` (1 mm) along one of the
    six axis directions (or lie between those answers when they span a continuous branch, grazing incidence without a
    hit / miss flip).  Asserts it ray by ray; returns (number of outliers, their largest deviation from the unperturbed
    oracle, the largest jump between neighbouring beams of the oracle's own profile at an outlier).  Only the particles
    that own an outlier are cast again."""
    m2o = np.identity(4) if m2o is None else m2o
    off = [0.0] * 6 if off is None else off
    err = np.abs(got - ref)
    bad = err > tol
    if not bad.any():
        return 0, 0.0, 0.0
    rows = np.unique(np.nonzero(bad)[0])
    sub = np.ascontiguousarray(soa[:, rows])
    cands = [ref[rows]]
    for axis in range(3):
        for sgn in (1.0, -1.0):
            s = sub.copy()
            s[axis] += sgn * delta
            _, ex = orc.mbes_update(s, m2o, off, omap, ba, None, 0.2, r_max)
            cands.append(ex)
    cands = np.stack(cands)                                    # 7 x rows x B
    g = got[rows]
    lo, hi = cands.min(axis=0), cands.max(axis=0)
    # candidates closer than 10 cm to one another span a continuous branch (grazing incidence: d range / d shift of 30
    # and more, without a hit / miss flip): any value between them is an oracle answer for a shift below delta.  The
    # seven candidates are clustered by that rule and the GPU value measured against the nearest cluster's interval
    cs = np.sort(cands, axis=0)
    cid = np.concatenate([np.zeros((1,) + cs.shape[1:], int), np.cumsum(np.diff(cs, axis=0) >= 0.1, axis=0)])
    dev = np.full(g.shape, np.inf)
    for k in range(cs.shape[0]):
        mk = cid == k
        if not mk.any():
            break
        clo = np.where(mk, cs, np.inf).min(axis=0)
        chi = np.where(mk, cs, -np.inf).max(axis=0)
        dev = np.minimum(dev, np.where(np.isfinite(clo), np.abs(g - np.clip(g, clo, chi)), np.inf))
    b = bad[rows]
    # the local shadow jump of the oracle's own range profile: an outlier sits where neighbouring beams differ by more
    # than the outlier is off, or where the ray's own answer moves under the 1 mm shift
    prof = ref[rows]
    jump = np.zeros_like(prof)
    if prof.shape[1] > 1:
        d = np.abs(np.diff(prof, axis=1))
        jump[:, :-1] = d
        jump[:, 1:] = np.maximum(jump[:, 1:], d)
    jump = np.maximum(jump, hi - lo)
    worst = np.unravel_index(np.argmax(np.where(b, dev, -1.0)), dev.shape)
    assert dev[b].max() <= tol, '%s ray (particle %d, beam %d): GPU %.5f m, oracle %.5f m, oracle under 1 mm shifts %s' % (
        label, rows[worst[0]], worst[1], g[worst], prof[worst], np.array2string(cands[(slice(None),) + worst], precision=4))
    unexplained = b & (err[rows] > jump + tol)
    assert not unexplained.any(), '%s: %d outlier rays are further off than the local jump of the oracle profile' % (label, int(unexplained.sum()))
    print('%s: %d of %d rays beyond %.0e m, the worst off by %.3e m; all are oracle answers under a 1 mm shift of the sensor '
          '(local jump of the oracle profile there: up to %.2f m)' % (label, int(bad.sum()), err.size, tol, err[bad].max(), jump[b].max()))
    return int(bad.sum()), float(err[bad].max()), float(jump[b].max())


def lw_outliers_explained(orc, omap, soa, ba, ranges, sigma, r_max, lw_got, lw_ref, m2o=None, off=None, delta=1e-3, label='',
                          select=None):
    """The log-likelihood side of the same contract (include/mcl.h, mcl_update_mbes: |d| <= 1e-2 or 2e-4 |lw|): a particle
    outside it must own a ray that flips between a crest and its shadow, i.e. its log-likelihood must lie inside the
    interval the fp64 oracle spans when the sensor moves by `delta` (1 mm) along the six axis directions -- widened by
    the usual tolerance.  Asserts it for every such particle; returns their number."""
    m2o = np.identity(4) if m2o is None else m2o
    off = [0.0] * 6 if off is None else off
    d = np.abs(lw_got - lw_ref)
    out = ~((d <= 1e-2) | (d <= 2e-4 * np.abs(lw_ref))) if select is None else np.asarray(select, bool)
    if not out.any():
        return 0
    rows = np.nonzero(out)[0]
    sub = np.ascontiguousarray(soa[:, rows])
    cands = [lw_ref[rows]]
    for axis in range(3):
        for sgn in (1.0, -1.0):
            s = sub.copy()
            s[axis] += sgn * delta
            lw_c, _ = orc.mbes_update(s, m2o, off, omap, ba, ranges, sigma, r_max)
            cands.append(lw_c)
    cands = np.stack(cands)
    lo, hi = cands.min(axis=0), cands.max(axis=0)
    slack = 1e-2 + 2e-4 * np.maximum(np.abs(lo), np.abs(hi))
    g = lw_got[rows]
    inside = (g >= lo - slack) & (g <= hi + slack)
    assert inside.all(), '%s: particle %d: log-likelihood %.4f outside the oracle interval [%.4f, %.4f] under 1 mm shifts' % (
        label, rows[np.argmin(inside)], g[np.argmin(inside)], lo[np.argmin(inside)], hi[np.argmin(inside)])
    print('%s: %d particles beyond the log-likelihood tolerance (worst |d| %.3e), each inside the oracle interval under a 1 mm '
          'shift of the sensor (widest interval %.2f)' % (label, rows.size, d[out].max(), (hi - lo).max()))
    return int(rows.size)


LIVE_SPAN = 30.0   # a particle's fixed-point weight q = floor(exp(lw - max) 2^s) is non-zero only for lw > max - s ln 2 (s = 63 - ceil(log2 N) = 43 at N = 2^20 -> 29.8); 30 covers every N >= 2^20


def live_particle_contract(orc, omap, soa, ba, ranges, sigma, r_max, lw_got, lw_ref, lw_max, m2o=None, off=None, label='',
                           allow=None):
    """The a15 contract WHERE IT BITES (include/mcl.h beside mcl_update_mbes): the relative arm of the
    log-likelihood tolerance (2e-4 |lw|) may only ever matter for particles that cannot receive offspring.  For every
    checked particle that is LIVE -- log-likelihood within LIVE_SPAN of the cloud's maximum `lw_max`, in the GPU's or in
    the oracle's arithmetic: its fixed-point weight is non-zero -- the absolute bound |d lw| <= 1e-2 must
    hold on its own.  The only exception is a particle that owns a ray grazing a crest (the last bit of fp32 decides
    between the crest and its shadow): it must lie inside the oracle's own interval under 1 mm shifts of the sensor, and
    there may be at most `allow` of them (default: 1 per 2 000 live particles, at least 1).  Prints the measured maximum
    on the live set; returns (live particles, max |d| among them, exceptions)."""
    d = np.abs(lw_got - lw_ref)
    live = (lw_got >= lw_max - LIVE_SPAN) | (lw_ref >= lw_max - LIVE_SPAN)
    n_live = int(live.sum())
    if n_live == 0:
        print('%s: no live particle (lw >= max - %.0f) among the %d checked' % (label, LIVE_SPAN, d.size))
        return 0, 0.0, 0
    viol = live & ~(d <= 1e-2)
    within = d[live & ~viol]
    print('%s: %d live particles (lw >= max - %.0f) of %d checked: max |dlw| %.3e on the live set (bound 1e-2)%s' % (
        label, n_live, LIVE_SPAN, d.size, within.max() if within.size else 0.0,
        '' if not viol.any() else '; %d beyond it (worst %.3e) -- must own a grazing ray' % (int(viol.sum()), d[viol].max())))
    n_exc = 0
    if viol.any():
        allow = max(1, n_live // 2000) if allow is None else allow
        assert viol.sum() <= allow, '%s: %d live particles beyond |dlw| <= 1e-2 (allowed %d)' % (label, int(viol.sum()), allow)
        n_exc = lw_outliers_explained(orc, omap, soa, ba, ranges, sigma, r_max, lw_got, lw_ref, m2o=m2o, off=off,
                                      label=label + ' (live)', select=viol)
    return n_live, float(within.max()) if within.size else 0.0, n_exc


def live_picks(lw, count, seed=0):
    """Indices of up to `count` LIVE particles of a cloud (lw >= max - LIVE_SPAN): the best ones and a random draw of the rest."""
    live = np.flatnonzero(lw >= np.max(lw) - LIVE_SPAN)
    if live.size <= count:
        return live
    best = live[np.argsort(lw[live])[-(count // 4):]]
    rest = np.setdiff1d(live, best)
    return np.concatenate([best, np.random.RandomState(seed).choice(rest, count - best.size, replace=False)])


# ------------------------------------------------------------------ the resamplers as an exact integer specification
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on uint64 arrays holding 32-bit words"""
    M = np.uint64(0xffffffff)
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & M for c in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return c0, c1, c2, c3


def native_draws_u53(seed, step, count):
    """The NATIVE uniforms of the explicit-index schemes (mcl_resample_alt.h: k_make_u53), as Python ints:
    U_i = ((x >> 5) << 26) | (y >> 6) of philox4x32(i, 0, step, 4; seed_lo, seed_hi), i = 0 .. count - 1."""
    x, y, _, _ = philox4x32_10(np.arange(int(count), dtype=np.uint64), 0, int(step), 4, seed & 0xffffffff, seed >> 32)
    return [int(v) for v in ((x >> np.uint64(5)) << np.uint64(26)) | (y >> np.uint64(6))]


def u53_of(u):
    """U = floor(u 2^53) of doubles in [0, 1), as Python ints (exact: u 2^53 is a power-of-two scaling)"""
    return [int(v * 9007199254740992.0) for v in np.atleast_1d(np.asarray(u, dtype=np.float64))]


EXACT_SCHEMES = ('systematic', 'naive', 'stratified', 'multinomial')


def exact_resample(q, U, scheme):
    """Ancestor indices of the four CDF schemes in plain Python integers (mcl_device.h: shl53_gt_mul,
    mcl_resample_alt.h).  q: the fixed-point weights (oracle.fixed_weights); U: 53-bit uniforms as ints -- one for
    systematic / naive, n for stratified / multinomial.  With C_j the inclusive sum of q, T = C_{n-1}, N = n:

        systematic   idx_i = min{ j : (U   + i 2^53) T <  C_j N 2^53 }
        naive        idx_i = min{ j : (U   + i 2^53) T <= C_j N 2^53 }
        stratified   idx_i = min{ j : (U_i + i 2^53) T <  C_j N 2^53 }
        multinomial  idx_i = min{ j : C_j 2^53 >= U_i T }

    and n - 1 where no j qualifies.  With T > 0 that never happens (the right-hand side at j = n - 1 is N T 2^53,
    above every left-hand side).  T = 0 (no weight at all; only linear weights that are all zero can give it) makes
    every product 0: the strict comparisons hold for no j -- index n - 1 everywhere --, the non-strict ones for j = 0
    -- index 0 everywhere.  The right-hand sides are non-decreasing in j, so min{j} is a bisection."""
    rhs, lhs, strict = _exact_sides(q, U, scheme)
    n = len(rhs)
    find = bisect.bisect_right if strict else bisect.bisect_left   # first j with rhs_j > lhs / rhs_j >= lhs
    return np.array([min(find(rhs, v), n - 1) for v in lhs], dtype=np.int32)


def exact_ties(q, U, scheme):
    """how many of the n positions sit exactly ON a CDF edge (left-hand side == a right-hand side of exact_resample):
    the decisions a `<` / `<=` mix-up would change"""
    rhs, lhs, _ = _exact_sides(q, U, scheme)
    return sum(1 for v in lhs if bisect.bisect_left(rhs, v) != bisect.bisect_right(rhs, v))


def _exact_sides(q, U, scheme):
    q = [int(v) for v in q]
    n = len(q)
    C, acc = [], 0
    for v in q:
        acc += v
        C.append(acc)
    T = C[-1]
    if scheme == 'multinomial':
        assert len(U) >= n
        return [c << 53 for c in C], [int(U[i]) * T for i in range(n)], False
    rhs = [(c * n) << 53 for c in C]
    if scheme == 'stratified':
        assert len(U) >= n
        return rhs, [(int(U[i]) + (i << 53)) * T for i in range(n)], True
    if scheme in ('systematic', 'naive'):
        return rhs, [(int(U[0]) + (i << 53)) * T for i in range(n)], scheme == 'systematic'
    raise ValueError(scheme)


# ------------------------------------------------------------------ mean / covariance and motion step: extended precision
# The reference the moments and predict edge tests measure the kernels against.  x87 long double (64-bit significand) where
# numpy has it; elsewhere exact rationals, which is why callers cap n at MOMENTS_N_CAP there.
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 1e-18)
MOMENTS_N_CAP = None if LONGDOUBLE_OK else 5000
TWO_PI = 2.0 * np.pi
EPS53 = 2.0 ** -53

# the kernels' launch constants (mcl_kernels.h, mcl_resample.h), restated: the rounding count below follows from them
MCL_BLOCK, MCL_MAX_GRID = 256, 2048        # k_mean_partial / k_cov_partial / k_sum_final
RS_BLOCK, GATHER_MAX_GRID = 1024, 256      # k_resample_gather


def wrap(a):
    """(a + pi) % (2 pi) - pi in fp64 with Python's floored modulo (auv_particle.py:48, auv_pf.py:229); numpy's mod on
    doubles is fmod plus the sign fix-up: exact"""
    return np.mod(np.asarray(a, dtype=np.float64) + np.pi, TWO_PI) - np.pi


def sum_roundings(n, block, max_grid):
    """K: roundings on the longest path from a particle to a published moment -- the per-thread chain of the grid-stride
    loop, the wave tree, the waves of a block, the blocks (64 per lane, then a wave tree), and 8 for the products, the
    subtraction, the division and the un-shift."""
    grid = min(-(-n // block), max_grid)
    return -(-n // (grid * block)) + 6 + block // 64 + -(-grid // 64) + 6 + 8


# The summation tree of the moment kernels (mcl_device.h, "the fixed tree": k_modes_moments, k_history_frame,
# k_drift_moments, k_reg_moments), restated operation by operation: every `+` below is one fp64 addition the device makes,
# in the device's order, so the sums agree bit for bit -- the sign of a zero included.
def _wave_sum_dpp(v):
    """wave_sum_dpp of (..., 64) lanes: wave_scan_incl_dpp, then lane 63.  A lane without a source adds +0.0."""
    row_lane = np.arange(64) % 16
    for k in (1, 2, 4, 8):                         # row_shr:k inside rows of 16 lanes
        src = np.zeros_like(v)
        src[..., k:] = v[..., :-k]
        src[..., row_lane < k] = 0.0
        v = v + src
    src = np.zeros_like(v)                         # row_bcast:15, row mask 0xa: lanes 15 and 47 into rows 1 and 3
    src[..., 16:32] = v[..., 15:16]
    src[..., 48:64] = v[..., 47:48]
    v = v + src
    src = np.zeros_like(v)                         # row_bcast:31, row mask 0xc: lane 31 into rows 2 and 3
    src[..., 32:64] = v[..., 31:32]
    v = v + src
    return v[..., 63]


def _wave_sum_shfl(v):
    """wave_sum of (..., 64) doubles: v += __shfl_down(v, o) for o = 32 ... 1 (a lane whose source lies past the wave reads
    itself); lane 0 holds the sum"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., np.where(lane + o < 64, lane + o, lane)]
    return v[..., 0]


def sum_final_tree(rec):
    """k_sum_final over one row of per-workgroup records: thread t adds records t, t + 256, ... to +0.0 in index order;
    block_sum: a __shfl_down tree per wave, then one over the four wave sums (the other lanes of wave 0 hold +0.0)"""
    rec = np.asarray(rec, dtype=np.float64)
    acc = np.zeros(MCL_BLOCK)
    for i in range(0, rec.size, MCL_BLOCK):
        chunk = rec[i:i + MCL_BLOCK]
        acc[:chunk.size] = acc[:chunk.size] + chunk
    sh = np.zeros(64)
    sh[:MCL_BLOCK // 64] = _wave_sum_shfl(acc.reshape(MCL_BLOCK // 64, 64))
    return _wave_sum_shfl(sh)


def moment_tree_sums(terms):
    """terms (rows, n): the term every lane contributes, one row per sum -> (rows,) what the moment kernel and k_sum_final
    leave.  Per grid-stride iteration of a wave (64 consecutive particles from blockIdx 256 + wave 64, stride grid x 256;
    the lanes past n hold +0.0; a wave whose first lane lies past n does not run) the wave's sum goes through
    _wave_sum_dpp and is added by lane 0 to the wave's accumulator, which starts at +0.0; the four accumulators of a
    workgroup are added in wave order; sum_final_tree adds the grid_for(n) records."""
    terms = np.atleast_2d(np.asarray(terms, dtype=np.float64))
    n = terms.shape[1]
    waves = MCL_BLOCK // 64
    grid = min(-(-n // MCL_BLOCK), MCL_MAX_GRID)
    stride = grid * MCL_BLOCK
    iters = -(-n // stride)
    base = (np.arange(iters)[:, None, None] * grid + np.arange(grid)[None, :, None]) * MCL_BLOCK + 64 * np.arange(waves)
    runs = base < n                                           # (iters, grid, waves)
    out = np.zeros(terms.shape[0])
    for j, t in enumerate(terms):
        v = np.zeros(iters * stride)
        v[:n] = t
        w = _wave_sum_dpp(v.reshape(iters, grid, waves, 64))
        acc = np.zeros((grid, waves))
        for it in range(iters):
            acc = np.where(runs[it], acc + w[it], acc)
        rec = acc[:, 0]
        for k in range(1, waves):
            rec = rec + acc[:, k]
        out[j] = sum_final_tree(rec)
    return out


def two_pass_roundings(n):
    return sum_roundings(n, MCL_BLOCK, MCL_MAX_GRID)


def gather_roundings(n):
    return sum_roundings(n, RS_BLOCK, GATHER_MAX_GRID)


COV_PAIRS = ((0, 0, 0), (4, 1, 1), (8, 2, 2), (1, 0, 1), (2, 0, 2), (5, 1, 2))   # (slot of cov9, a, b); [3] mirrors [1]


def _lay_cov(c):
    """six moments keyed by slot -> the 9 numbers as auv_pf.py:238-252 lays them out: [1,0] mirrored, [2,0], [2,1] zero"""
    out = np.zeros(9, dtype=np.result_type(*[np.asarray(v).dtype for v in c.values()]))
    for k, v in c.items():
        out[k] = v
    out[3] = out[1]
    return out


def moments_reference(soa, shift):
    """Mean pose, mean wrapped yaw and centred second moments of a (6, n) fp64 cloud in extended precision, and the error
    units U the assertions scale by (d = v - shift, taken in extended precision):

        mean of x, y, z                    U = |shift_a| + mean |d_a|
        mean of roll, pitch, yaw, wrap     U = mean |v|
        cov_ab                             U = mean |d_a d_b| + |mean d_a| |mean d_b|

    shift: three numbers (the one-pass form's shift, or the mean itself for the two-pass form).  Returns a dict of
    mean (6), yaw, cov (9), u_mean (6), u_yaw, u_cov (9), all np.longdouble (or floats rounded from exact rationals)."""
    soa = np.asarray(soa, dtype=np.float64)
    assert soa.ndim == 2 and soa.shape[0] == 6
    if not LONGDOUBLE_OK:
        return _moments_exact(soa, shift, as_float=True)
    n = soa.shape[1]
    L = np.longdouble
    v = soa.astype(L)
    sh = np.array([L(s) for s in shift], dtype=L)
    d = v[:3] - sh[:, None]
    md = d.sum(axis=1) / L(n)
    mean = np.concatenate([sh + md, v[3:].sum(axis=1) / L(n)])
    wy = wrap(soa[5]).astype(L)
    c = v[:3] - mean[:3, None]                                   # centred on the extended-precision mean: no cancellation
    cov, u_cov = {}, {}
    for k, a, b in COV_PAIRS:
        cov[k] = (c[a] * c[b]).sum() / L(n)
        u_cov[k] = np.abs(d[a] * d[b]).sum() / L(n) + abs(md[a]) * abs(md[b])
    u_mean = np.concatenate([np.abs(sh) + np.abs(d).sum(axis=1) / L(n), np.abs(v[3:]).sum(axis=1) / L(n)])
    return dict(mean=mean, yaw=wy.sum() / L(n), cov=_lay_cov(cov), u_mean=u_mean, u_yaw=np.abs(wy).sum() / L(n),
                u_cov=_lay_cov(u_cov))


def _moments_exact(soa, shift, as_float=False):
    """moments_reference in exact rationals (every double is one)"""
    F = fractions.Fraction
    n = soa.shape[1]
    v = [[F(float(x)) for x in row] for row in soa]
    sh = [F(float(s)) if not isinstance(s, F) else s for s in shift]
    d = [[x - sh[a] for x in v[a]] for a in range(3)]
    md = [sum(r) / n for r in d]
    mean = [sh[a] + md[a] for a in range(3)] + [sum(v[a]) / n for a in range(3, 6)]
    wy = [F(float(x)) for x in wrap(soa[5])]
    c = [[x - mean[a] for x in v[a]] for a in range(3)]
    cov, u_cov = {}, {}
    for k, a, b in COV_PAIRS:
        cov[k] = sum(p * q for p, q in zip(c[a], c[b])) / n
        u_cov[k] = sum(abs(p * q) for p, q in zip(d[a], d[b])) / n + abs(md[a]) * abs(md[b])
    u_mean = [abs(sh[a]) + sum(abs(x) for x in d[a]) / n for a in range(3)] + [sum(abs(x) for x in v[a]) / n for a in range(3, 6)]
    out = dict(mean=mean, yaw=sum(wy) / n, cov=cov, u_mean=u_mean, u_yaw=sum(abs(x) for x in wy) / n, u_cov=u_cov)
    if not as_float:
        return out
    f = lambda seq: np.array([float(x) for x in seq])  # noqa: E731
    lay = lambda m: _lay_cov({k: np.float64(float(x)) for k, x in m.items()})  # noqa: E731
    return dict(mean=f(mean), yaw=float(out['yaw']), cov=lay(cov), u_mean=f(u_mean), u_yaw=float(out['u_yaw']), u_cov=lay(u_cov))


def moments_errors(got, ref):
    """|got - ref| of (mean6, yaw, cov9) as mcl_mean_cov returns them, in units of 2^-53 U: three arrays (6, 1, 9); an
    entry whose unit is zero is 0 where the values agree exactly and inf where they do not"""
    L = np.longdouble if LONGDOUBLE_OK else np.float64

    def ratio(g, r, u):
        g, r, u = np.atleast_1d(np.asarray(g, dtype=L)), np.atleast_1d(np.asarray(r, dtype=L)), np.atleast_1d(np.asarray(u, dtype=L))
        err = np.abs(g - r)
        with np.errstate(divide='ignore', invalid='ignore'):
            q = err / (L(EPS53) * u)
        return np.where(u > 0, q, np.where(err == 0, 0.0, np.inf)).astype(np.float64)
    return ratio(got[0], ref['mean'], ref['u_mean']), ratio(got[1], ref['yaw'], ref['u_yaw']), ratio(got[2], ref['cov'], ref['u_cov'])


MOMENT_FAMILIES = ('origin', 'survey', 'outlier0', 'seam', 'one', 'identical')
SURVEY_XY = (6.5e5, 6.4e6)


def moments_family(name, n, seed=0):
    """The input families of the moments tests, (6, n) fp64:
    origin     sigma = (1, 0.7) m with xy correlation 0.6, a few metres from the origin
    survey     sigma = 1 cm at (6.5e5, 6.4e6): projected survey coordinates
    outlier0   survey, but particle 0 lies 1000 m away in x and -1000 m in y: a one-pass shift outside the cloud
    seam       origin, with yaw = wrap(N(pi, 0.2)) + N(0, 0.1): a cloud across +-pi whose stored yaw leaves [-pi, pi)
    one        the first particle of survey (n must be 1)
    identical  n copies of one survey particle"""
    rs = np.random.RandomState(1000 + seed)
    g = rs.randn(8, n)
    soa = np.zeros((6, n))
    if name in ('origin', 'seam'):
        soa[0] = 3.0 + g[0]
        soa[1] = -2.0 + 0.7 * (0.6 * g[0] + 0.8 * g[1])
        soa[2] = -5.0 + 0.3 * g[2]
        soa[3], soa[4] = 0.02 + 0.05 * g[3], -0.01 + 0.05 * g[4]
        soa[5] = 0.4 + 0.3 * g[5] if name == 'origin' else wrap(np.pi + 0.2 * g[5]) + 0.1 * g[6]
    elif name in ('survey', 'outlier0', 'one', 'identical'):
        soa[0] = SURVEY_XY[0] + 0.01 * g[0]
        soa[1] = SURVEY_XY[1] + 0.01 * g[1]
        soa[2] = -20.0 + 0.01 * g[2]
        soa[3], soa[4] = 0.02 + 0.01 * g[3], -0.01 + 0.01 * g[4]
        soa[5] = 1.0 + 0.05 * g[5]
        if name == 'outlier0':
            soa[0, 0] += 1000.0
            soa[1, 0] -= 1000.0
        elif name == 'one':
            assert n == 1
        elif name == 'identical':
            soa[:] = soa[:, :1]
    else:
        raise ValueError(name)
    return np.ascontiguousarray(soa)


def quat_from_euler_ld(roll, pitch, yaw):
    """tf.transformations.quaternion_from_euler (sxyz) -> (x, y, z, w), np.longdouble, arrays of angles"""
    L = np.longdouble
    r, p, y = [np.asarray(a, dtype=np.float64).astype(L) * L(0.5) for a in (roll, pitch, yaw)]
    sr, cr, sp, cp, sy, cy = np.sin(r), np.cos(r), np.sin(p), np.cos(p), np.sin(y), np.cos(y)
    return np.stack([cp * sr * cy - sp * cr * sy, cp * sr * sy + sp * cr * cy, cp * cr * sy - sp * sr * cy,
                     cp * cr * cy + sp * sr * sy], axis=-1)


def predict_reference(soa, v, wz, q, z, dt, process_cov, normals=None, yaw_t=None):
    """Particle.motion_pred (auv_particle.py:38-70) of a (6, n) fp64 cloud, x and y in np.longdouble.  Roll and pitch are
    the fp64 Euler angles of q (oracle.euler_from_quat: the reference evaluates them in fp64 too), z the odometry's.
    Yaw: with a zero yaw process variance the statement is fp64 and exact, wrap(fl(yaw + fl(wz dt))) -- returned as `yaw`
    (fp64, bit-comparable); otherwise `yaw` is the wrap of the extended-precision sum rounded to fp64 and `yaw_unwrapped`
    that sum.  Returns x, y (longdouble), z, roll, pitch (floats), yaw, yaw_unwrapped, and u_x, u_y =
    |x'| + |m0| + |m1| + |sigma n|, the unit of the position bound (m = (Ry' Rx)(v dt), rows 0 and 1).  yaw_t: evaluate
    x and y at this fp64 yaw instead (the yaw under test, where it carries noise: the position bound then does not
    inherit the yaw's rounding)."""
    from oracle import oracle as orc
    L = np.longdouble
    soa = np.asarray(soa, dtype=np.float64)
    n = soa.shape[1]
    sq = np.sqrt(np.asarray(process_cov, dtype=np.float64))
    nz = np.zeros((n, 6)) if normals is None else np.asarray(normals, dtype=np.float64).reshape(n, 6)
    roll, pitch, _ = [float(a) for a in orc.euler_from_quat(q)]
    wzdt = np.float64(wz) * np.float64(dt)
    if sq[5] == 0.0:
        yaw = wrap(soa[5] + wzdt)
        unwrapped = (soa[5] + wzdt).astype(L)
        yaw_l = yaw.astype(L)
    else:
        unwrapped = soa[5].astype(L) + L(wzdt) + L(sq[5]) * nz[:, 5].astype(L)
        two_pi_l, pi_l = L(2.0 * np.pi), L(np.pi)      # the fp64 constants the statement uses
        yaw_l = np.mod(unwrapped + pi_l, two_pi_l) - pi_l
        yaw = yaw_l.astype(np.float64)
    # fullRotation (auv_particle.py:84-100): Rz(yaw_t) (Ry' Rx), with the reference's own Ry' = [[cp,0,sp],[0,1,0],[-sp,cp,0]]
    cp, sp, cr, sr = np.cos(L(pitch)), np.sin(L(pitch)), np.cos(L(roll)), np.sin(L(roll))
    vdt = [L(float(c)) * L(float(dt)) for c in v]
    m0 = cp * vdt[0] + sp * sr * vdt[1] + sp * cr * vdt[2]
    m1 = cr * vdt[1] - sr * vdt[2]
    if yaw_t is not None:
        yaw_l = np.asarray(yaw_t, dtype=np.float64).astype(L)
    cy, sy = np.cos(yaw_l), np.sin(yaw_l)
    n0, n1 = L(sq[0]) * nz[:, 0].astype(L), L(sq[1]) * nz[:, 1].astype(L)
    x = soa[0].astype(L) + (cy * m0 - sy * m1) + n0
    y = soa[1].astype(L) + (sy * m0 + cy * m1) + n1
    return dict(x=x, y=y, z=float(z), roll=roll, pitch=pitch, yaw=yaw, yaw_unwrapped=unwrapped,
                u_x=np.abs(x) + abs(m0) + abs(m1) + np.abs(n0), u_y=np.abs(y) + abs(m0) + abs(m1) + np.abs(n1))


PREDICT_EDGE_YAWS = np.array(
    [np.pi, -np.pi, np.nextafter(np.pi, 4.0), np.nextafter(np.nextafter(np.pi, 4.0), 4.0), np.nextafter(np.pi, 0.0),
     np.nextafter(np.nextafter(np.pi, 0.0), 0.0), np.nextafter(-np.pi, -4.0), np.nextafter(np.nextafter(-np.pi, -4.0), -4.0),
     np.nextafter(-np.pi, 0.0), np.nextafter(np.nextafter(-np.pi, 0.0), 0.0), 0.0, -0.0, np.pi - 1e-3] +
    [TWO_PI * k for k in (1, -1, 7, -7, 1000, -1000)] + [1e6, -1e6, 1e9, -1e9])
PREDICT_EDGE_WZDT = (0.0, 1e-3, -1e-3, 0.5, -0.5)


def predict_family(n, where, seed=0):
    """(6, n) fp64 for the predict edge tests: the edge yaws first (as many as fit), then yaw uniform in [-4 pi, 4 pi];
    x, y metre-wide near the origin or at the survey coordinates"""
    rs = np.random.RandomState(2000 + seed)
    soa = np.zeros((6, n))
    cx, cy = (3.0, -2.0) if where == 'origin' else SURVEY_XY
    soa[0] = cx + rs.randn(n)
    soa[1] = cy + rs.randn(n)
    soa[2] = -4.0 + rs.randn(n)          # z, roll, pitch: overwritten by the odometry's
    soa[3], soa[4] = 0.1 * rs.randn(n), 0.1 * rs.randn(n)
    soa[5] = rs.uniform(-4.0 * np.pi, 4.0 * np.pi, n)
    k = min(n, PREDICT_EDGE_YAWS.size)
    soa[5, :k] = PREDICT_EDGE_YAWS[:k]
    return np.ascontiguousarray(soa)


ULP_PI = 2.0 ** -51          # spacing of the doubles in [2, 4)


def yaw_noise_check(got_yaw, ref):
    """yaw with process noise: |got - ref| modulo 2 pi in units of ulp(pi), and the samples that landed on the other
    side of the seam (those may only be ones whose unwrapped reference lies within 4 ulp of +-pi)"""
    L = np.longdouble
    two_pi = L(TWO_PI)
    diff = np.asarray(got_yaw, dtype=np.float64).astype(L) - ref['yaw'].astype(L)
    turns = np.rint(diff / two_pi)
    err = np.abs(diff - turns * two_pi) / L(ULP_PI)
    crossed = turns != 0
    s = ref['yaw_unwrapped'] + L(np.pi)
    to_seam = np.abs(s - np.rint(s / two_pi) * two_pi) / L(ULP_PI)
    return err.astype(np.float64), crossed, to_seam.astype(np.float64)
