"""CPU tests of the ping matching (include/mcl_match.h): every symbol of the header exported and bound in a table of its own,
the records' sizes and offsets, the device-free entry points -- solve, better, derived, config_check -- bit for bit against a
restatement in Python floats and integers, the restated loop on the fp64 oracle's casts rounded to fp32 (rough terrain, a
flat seabed, a ridge, a start off the map), and the stand-alone sanitizer driver of the host arithmetic.  The restatement
is what tests/test_gpu_match.py compares the kernel with.

Which starts the restated loop is run from (B = 64, the scene grid of tests/test_innovation_host.py, seed 5): the eight
starts per dims that starts_of draws from RandomState(START_SEEDS[dims - 3]) within +-2 m and +-0.05 rad of TRUTH -- this
restatement converges from all sixteen -- and LOCAL_STARTS, one start per dims 8 to 11 m away from which it does not: it
runs out of evaluations in a local minimum whose rms residual of about 530 quanta (13 cm) tells it apart."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from smarc_navigation_amd import synth
from tests.test_innovation_host import M2O, OFF, R_MAX, SIGMA, scene, scene_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mcl_match_config_check', 'mcl_match_solve', 'mcl_match_better', 'mcl_match_derived', 'mcl_match_ping')
ERR_INVALID = -1
CONVERGED, MAX_ITER, STALLED, NO_OVERLAP = 0, 1, 2, 3
J0, J_MIN, J_MAX = -10, -20, 20
D_MAX, RHO_MAX, MAX_BEAMS = 1 << 23, 1 << 24, 2048
TWO24 = 16777216.0


# ------------------------------------------------------------------ the restatement of include/mcl_match.h
def packed(r, c):
    return r * (r + 1) // 2 + c


def default_cfg(**kw):
    c = dict(dims=3, max_iter=12, min_beams=8, grad_floor_q=2, step_max_xy=2.0, step_max_yaw=0.1, tol_xy=1e-3, tol_yaw=1e-4,
             delta_xy=0.5, delta_yaw=0.01, jump_max=R_MAX)
    c.update(kw)
    return c


def c_cfg(cfg):
    from smarc_navigation_amd import engine
    return engine.make_match_config(R_MAX, cfg['dims'] == 4, cfg['max_iter'], cfg['min_beams'], cfg['grad_floor_q'], cfg['step_max_xy'],
                                    cfg['step_max_yaw'], cfg['tol_xy'], cfg['tol_yaw'], cfg['delta_xy'], cfg['delta_yaw'], cfg['jump_max'])


def variants(pose, cfg):
    """the 1 + 2 D states an evaluation casts from (6 x NV): one fp64 addition or subtraction on the stored number"""
    dxy, dyaw = cfg['delta_xy'], cfg['delta_yaw']
    rows = [(None, 0.0), (0, dxy), (0, -dxy), (1, dxy), (1, -dxy), (5, dyaw), (5, -dyaw), (2, dxy), (2, -dxy)][:1 + 2 * cfg['dims']]
    out = np.repeat(np.asarray(pose, np.float64).reshape(6, 1), len(rows), axis=1)
    for v, (row, step) in enumerate(rows):
        if row is not None:
            out[row, v] = out[row, v] + step if step > 0 else out[row, v] - (-step)
    return out


def sums_ref(meas, rng, cfg, r_max=R_MAX):
    """the nineteen integers of a record from the NV x B ranges of one evaluation (float32) and the ping, as Python ints:
    (n, n_miss, n_jump, S[10], C[4], s_rho, s_rho2).  int64 holds every sum exactly (the header's bound: below 2^60)."""
    D = cfg['dims']
    meas = np.asarray(meas, np.float32).reshape(-1)
    e = np.asarray(rng, np.float32).reshape(1 + 2 * D, meas.size)
    jq = int(math.floor(cfg['jump_max'] * 4096.0))
    with np.errstate(invalid='ignore'):
        counts = meas > 0                            # zero, negative and NaN do not count
    miss = counts & np.any(e == np.float32(r_max), axis=0)
    e64 = np.where(counts[None, :], e, np.float32(0)).astype(np.float64)
    d = [np.rint((e64[1 + 2 * k] - e64[2 + 2 * k]) * 4096.0).astype(np.int64) for k in range(D)]
    jump = counts & ~miss & np.any(np.abs(np.stack(d)) > jq, axis=0)
    use = counts & ~miss & ~jump
    x = (np.where(counts, meas, np.float32(0)).astype(np.float64) - e64[0]) * 4096.0
    rho = np.rint(np.clip(x, -float(RHO_MAX), float(RHO_MAX))).astype(np.int64)[use]
    d = [v[use] for v in d]
    S, Cv = [0] * 10, [0] * 4
    for j in range(D):
        for k in range(j + 1):
            S[packed(j, k)] = int(np.sum(d[j] * d[k]))
        Cv[j] = int(np.sum(d[j] * rho))
    return (int(counts.sum()), int(miss.sum()), int(jump.sum()), tuple(S), tuple(Cv), int(np.sum(rho)), int(np.sum(rho * rho)))


def m_of(rec):
    return rec[0] - rec[1] - rec[2]


def better_ref(q, p, min_beams):
    return m_of(q) >= min_beams and q[6] * m_of(p) < p[6] * m_of(q)


def reg_factor_ref(Cm, D):
    """the thresholded Cholesky factor of mcl_regularise.h over packed lists: (L, dead mask)"""
    L = [0.0] * len(Cm)
    dead = 0
    for j in range(D):
        cjj = Cm[packed(j, j)]
        p = cjj
        for k in range(j):
            l = L[packed(j, k)]
            p = p - l * l
        if p > cjj * 2.0 ** -26:
            d = math.sqrt(p)
            L[packed(j, j)] = d
            for i in range(j + 1, D):
                t = Cm[packed(i, j)]
                for k in range(j):
                    t = t - L[packed(i, k)] * L[packed(j, k)]
                L[packed(i, j)] = t / d
        else:
            dead |= 1 << j
            for i in range(j, D):
                L[packed(i, j)] = 0.0
    return L, dead


def _live(rec, cfg):
    lim = m_of(rec) * cfg['grad_floor_q'] ** 2
    return [k for k in range(cfg['dims']) if rec[3][packed(k, k)] > lim]


def _normal(rec, cfg, live):
    dl = (cfg['delta_xy'], cfg['delta_xy'], cfg['delta_yaw'], cfg['delta_xy'])
    nl = len(live)
    A, y = [0.0] * (nl * (nl + 1) // 2), [0.0] * nl
    for i, ki in enumerate(live):
        for k, kk in enumerate(live[:i + 1]):
            A[packed(i, k)] = float(rec[3][packed(ki, kk)]) / (((4.0 * dl[ki]) * dl[kk]) * TWO24)
        y[i] = float(rec[4][ki]) / ((2.0 * dl[ki]) * TWO24)
    return A, y


def _substitute(L, nl, kill, y):
    y = list(y)
    t = [0.0] * nl
    for i in range(nl):
        if kill >> i & 1:
            y[i] = 0.0
            continue
        s = y[i]
        for k in range(i):
            s = s - L[packed(i, k)] * y[k]
        y[i] = s / L[packed(i, i)]
    for i in range(nl - 1, -1, -1):
        if kill >> i & 1:
            continue
        s = y[i]
        for k in range(i + 1, nl):
            s = s - L[packed(k, i)] * t[k]
        t[i] = s / L[packed(i, i)]
    return t


def solve_ref(rec, cfg, j):
    """SOLVE: (delta over x, y, yaw, z as Python floats, dead mask)"""
    live = _live(rec, cfg)
    dead = sum(1 << k for k in range(4) if k not in live)
    delta = [0.0] * 4
    if not live:
        return delta, dead
    A, y = _normal(rec, cfg, live)
    lam = 2.0 ** j
    nl = len(live)
    for i in range(nl):
        A[packed(i, i)] = A[packed(i, i)] + lam * A[packed(i, i)]
    L, kill = reg_factor_ref(A, nl)
    t = _substitute(L, nl, kill, y)
    for i, k in enumerate(live):
        if kill >> i & 1:
            dead |= 1 << k
        else:
            delta[k] = t[i]
    h = math.sqrt(delta[0] * delta[0] + delta[1] * delta[1])
    s = 1.0
    if h > cfg['step_max_xy']:
        s = cfg['step_max_xy'] / h
    az, aw = abs(delta[3]), abs(delta[2])
    if az * s > cfg['step_max_xy']:
        s = cfg['step_max_xy'] / az
    if aw * s > cfg['step_max_yaw']:
        s = cfg['step_max_yaw'] / aw
    if s < 1.0:
        delta = [v * s for v in delta]
    return delta, dead


def derived_ref(rec, cfg, sigma):
    m = m_of(rec)
    rms = math.sqrt(float(rec[6]) / float(m)) / 4096.0 if m > 0 else 0.0
    mean = (float(rec[5]) / float(m)) / 4096.0 if m > 0 else 0.0
    z, s2 = rms / sigma, sigma * sigma
    live = _live(rec, cfg)
    dead = sum(1 << k for k in range(4) if k not in live)
    J, cov = [0.0] * 10, [0.0] * 10
    nl = len(live)
    A, _ = _normal(rec, cfg, live)
    for i, ki in enumerate(live):
        for k, kk in enumerate(live[:i + 1]):
            J[packed(ki, kk)] = A[packed(i, k)] / s2
    L, kill = reg_factor_ref(A, nl) if nl else ([], 0)
    for i, k in enumerate(live):
        if kill >> i & 1:
            dead |= 1 << k
    for c in range(nl):
        if kill >> c & 1:
            continue
        t = _substitute(L, nl, kill, [1.0 if i == c else 0.0 for i in range(nl)])
        for i in range(c, nl):
            if not kill >> i & 1:
                cov[packed(live[i], live[c])] = t[i] * s2
    for k in range(cfg['dims']):
        if dead >> k & 1:
            cov[packed(k, k)] = math.inf
    return dict(rms=rms, mean=mean, chi2=z * z, J=J, cov=cov, dead=dead, m=m)


def wrap_ref(t):
    """the library's rule for a yaw that moved"""
    if -math.pi <= t < math.pi:
        return t
    b = 2.0 * math.pi
    s = t + math.pi
    if 0.0 <= s < b:
        return s - math.pi
    m = math.fmod(s, b)
    if m != 0.0:
        if m < 0.0:
            m += b
    else:
        m = 0.0
    return m - math.pi


def next_pose_ref(cur, delta):
    """cur, delta over (x, y, yaw, z): one addition per coordinate that moves, the others keep their bits"""
    q = [c + d if d != 0.0 else c for c, d in zip(cur, delta)]
    if delta[2] != 0.0:
        q[2] = wrap_ref(cur[2] + delta[2])
    return q


def loop_ref(evaluate, pose6, cfg, solve=None, better=None):
    """THE LOOP.  evaluate(pose6) -> the record of that pose.  Returns dict(pose=(x, y, yaw, z), status, evaluations,
    accepted, j, dead, start, final, trace=[(pose4, record, j, accepted)]).  solve / better: what decides -- the
    restatement (solve_ref, better_ref), or library_rules()"""
    solve, better = solve or solve_ref, better or better_ref
    pose6 = [float(v) for v in pose6]

    def full(p4):
        return [p4[0], p4[1], p4[3], pose6[3], pose6[4], p4[2]]
    cur = [pose6[0], pose6[1], pose6[5], pose6[2]]
    rec = evaluate(full(cur))
    out = dict(start=rec, trace=[(list(cur), rec, J0, 1 if m_of(rec) >= cfg['min_beams'] else 0)])
    j, trials, accepted, dead = J0, 0, 0, 0
    status = NO_OVERLAP if m_of(rec) < cfg['min_beams'] else None
    while status is None:
        if rec[6] == 0:
            status = CONVERGED
            break
        delta, dead = solve(rec, cfg, j)
        if all(d == 0.0 for d in delta):
            status = CONVERGED
            break
        if trials == cfg['max_iter']:
            status = MAX_ITER
            break
        q = next_pose_ref(cur, delta)
        rq = evaluate(full(q))
        trials += 1
        ok = better(rq, rec, cfg['min_beams'])
        out['trace'].append((list(q), rq, j, 1 if ok else 0))
        if ok:
            cur, rec, accepted, j = q, rq, accepted + 1, max(j - 2, J_MIN)
            if (math.sqrt(delta[0] * delta[0] + delta[1] * delta[1]) < cfg['tol_xy'] and abs(delta[3]) < cfg['tol_xy']
                    and abs(delta[2]) < cfg['tol_yaw']):
                status = CONVERGED
        else:
            j += 2
            if j > J_MAX:
                status = STALLED
    out.update(pose=tuple(cur), status=status, evaluations=1 + trials, accepted=accepted, j=j, dead=dead, final=rec)
    return out


def library_rules():
    """(solve, better) with the signatures of solve_ref / better_ref, decided by the library's mcl_match_solve / mcl_match_better"""
    from smarc_navigation_amd import engine

    def solve(rec, cfg, j):
        delta, dead = engine.match_solve(rec_array(rec), c_cfg(cfg), j)
        return [float(v) for v in delta], dead

    def better(q, p, min_beams):
        return engine.match_better(rec_array(q), rec_array(p), min_beams)
    return solve, better


def loop_both(evaluate, pose6, cfg):
    """the loop run by the restatement and once more with the library's exported functions deciding every step: the two
    runs are the same down to the last bit of every pose (repr of a float names one double).  Returns the run."""
    mine = loop_ref(evaluate, pose6, cfg)
    theirs = loop_ref(evaluate, pose6, cfg, *library_rules())
    assert repr(mine) == repr(theirs)
    return mine


def rec_array(rec):
    from smarc_navigation_amd import engine
    a = np.zeros(1, engine.MATCH_SUMS)
    a['n'], a['n_miss'], a['n_jump'], a['s_rho'], a['s_rho2'] = rec[0], rec[1], rec[2], rec[5], rec[6]
    a['S'][0], a['C'][0] = rec[3], rec[4]
    return a


def rec_tuple(a):
    """a numpy record of MATCH_SUMS as the restatement's tuple of Python ints"""
    return (int(a['n']), int(a['n_miss']), int(a['n_jump']), tuple(int(v) for v in np.asarray(a['S']).reshape(-1)),
            tuple(int(v) for v in np.asarray(a['C']).reshape(-1)), int(a['s_rho']), int(a['s_rho2']))


def record_of(pairs, D=3, n_miss=0, n_jump=0):
    """a record from [(d_0 ... d_{D-1}, rho)] of the contributing beams"""
    S, Cv = [0] * 10, [0] * 4
    s1 = s2 = 0
    for p in pairs:
        d, rho = [int(v) for v in p[:D]], int(p[D])
        for j in range(D):
            for k in range(j + 1):
                S[packed(j, k)] += d[j] * d[k]
            Cv[j] += d[j] * rho
        s1 += rho
        s2 += rho * rho
    return (len(pairs) + n_miss + n_jump, n_miss, n_jump, tuple(S), tuple(Cv), s1, s2)


def random_record(rs, D=3, n=None, scale=None, rho_scale=None):
    n = int(rs.choice([1, 2, 7, 64, 300, 2044])) if n is None else n           # (with up to four misses and jumps: <= 2048)
    scale = int(rs.choice([3, 50, 4096, 1 << 16, D_MAX])) if scale is None else scale
    rho_scale = int(rs.choice([1, 40, 4096, RHO_MAX])) if rho_scale is None else rho_scale
    d = np.clip((rs.randn(n, D) * scale * np.array([1.0, 0.3, 0.1, 0.6])[:D]).round().astype(np.int64), -D_MAX, D_MAX)
    rho = np.clip((rs.randn(n, 1) * rho_scale).round().astype(np.int64), -RHO_MAX, RHO_MAX)
    return record_of(np.concatenate([d, rho], axis=1).tolist(), D, int(rs.randint(0, 3)), int(rs.randint(0, 3)))


def _bits(v):
    return np.float64(v).tobytes()


# ------------------------------------------------------------------ the scene: oracle casts rounded to fp32
TRUTH = np.array([20.0, -10.0, -2.0, 0.01, -0.02, 0.3])
B_HOST = 64
START_SEEDS = (11, 12)            # one RandomState per dims: eight starts each
LOCAL_STARTS = {3: np.array([30.75, -13.25, -2.0, 0.01, -0.02, 0.425]), 4: np.array([17.25, -18.875, -1.5, 0.01, -0.02, 0.3625])}


def starts_of(dims, count=8):
    """starts within +-2 m and +-0.05 rad of TRUTH; those that fit z also 0.4 m off in z"""
    rs = np.random.RandomState(START_SEEDS[dims - 3])
    out = np.repeat(TRUTH[:, None], count, axis=1)
    out[0] += rs.uniform(-2.0, 2.0, count)
    out[1] += rs.uniform(-2.0, 2.0, count)
    out[5] += rs.uniform(-0.05, 0.05, count)
    if dims == 4:
        out[2] += 0.4
    return out


class OracleEval(object):
    """evaluate(pose6) over the fp64 oracle: its ranges at the 1 + 2 D variants rounded to float32, then sums_ref"""

    def __init__(self, omap, ba, meas, cfg, m2o=M2O, off=OFF, r_max=R_MAX):
        from oracle import oracle as orc
        self.orc, self.omap, self.ba, self.meas, self.cfg, self.m2o, self.off, self.r_max = orc, omap, ba, meas, cfg, m2o, off, r_max
        self.calls, self.seen = 0, {}

    def ranges(self, pose6):
        v = np.ascontiguousarray(variants(pose6, self.cfg))
        return self.orc.mbes_update(v, self.m2o, self.off, self.omap, self.ba, None, SIGMA, self.r_max)[1].astype(np.float32)

    def __call__(self, pose6):
        key = tuple(float(v) for v in pose6)
        if key not in self.seen:                 # (a pose asked for again, by loop_both's second run: not cast again)
            self.calls += 1
            self.seen[key] = sums_ref(self.meas, self.ranges(pose6), self.cfg, self.r_max)
        return self.seen[key]


def ping_at(omap, pose6, ba, m2o=M2O, off=OFF, r_max=R_MAX):
    from oracle import oracle as orc
    return orc.mbes_update(np.asarray(pose6, np.float64).reshape(6, 1), m2o, off, omap, ba, None, SIGMA, r_max)[1][0].astype(np.float32)


_HOST_CACHE = {}


def rough_reference(dims, kind='grid'):
    """the restated loop from every start of starts_of(dims) on the scene's map of that kind -- computed once, shared with
    the GPU tests"""
    if (dims, kind) not in _HOST_CACHE:
        z, origin, _ = scene()
        _, omap = scene_map(kind, z, origin)
        ba = synth.beam_angles(B_HOST, 1.0)
        meas = ping_at(omap, TRUTH, ba)
        cfg = default_cfg(dims=dims)
        ev = OracleEval(omap, ba, meas, cfg)
        starts = starts_of(dims)
        _HOST_CACHE[(dims, kind)] = dict(cfg=cfg, ba=ba, meas=meas, starts=starts, omap=omap,
                                         runs=[loop_both(ev, starts[:, k], cfg) for k in range(starts.shape[1])])
    return _HOST_CACHE[(dims, kind)]


def horizontal_error(run):
    return math.hypot(run['pose'][0] - TRUTH[0], run['pose'][1] - TRUTH[1])


# flat seabed / ridge / off the map: 1 m grids, identity m2o, no sensor offset (tests/test_gpu_information.py section 5)
GRID_N, GRID_ORIGIN, BC_RMAX = 128, (-64.0, -64.0), 60.0
FLAT_START = np.array([3.125, -2.25, -2.4, 0.0, 0.0, 0.7])
RIDGE_TRUTH = np.array([3.125, -2.25, -2.0, 0.01, -0.02, 0.2])
RIDGE_START = np.array([3.5, -1.0, -2.0, 0.01, -0.02, 0.2])


def flat_grid():
    return np.full((GRID_N, GRID_N), -20.0, np.float32)


def ridge_grid():
    """heights that depend on y only: a ridge along x"""
    iy = np.arange(GRID_N, dtype=np.float64) + GRID_ORIGIN[1]
    return np.repeat((-20.0 + 3.0 * np.sin(iy / 6.0) + 0.05 * iy)[None, :], GRID_N, axis=0).astype(np.float32)


# ------------------------------------------------------------------ the ABI
@pytest.fixture(scope='module')
def lib():
    from smarc_navigation_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def test_every_symbol_of_the_header_is_exported_and_bound_in_a_table_of_its_own(lib):
    from smarc_navigation_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'mcl_match.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(NAMES) == sorted(_lib.MATCH_SYMBOLS)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    others = [_lib.SYMBOLS, _lib.RECOVERY_SYMBOLS, _lib.MODES_SYMBOLS, _lib.HISTORY_SYMBOLS, _lib.ACOUSTIC_SYMBOLS, _lib.TEMPER_SYMBOLS,
              _lib.DRIFT_SYMBOLS, _lib.REGULARISE_SYMBOLS, _lib.QUANTILE_SYMBOLS, _lib.INNOVATION_SYMBOLS, _lib.INFORMATION_SYMBOLS]
    for t in others:
        assert not set(t) & set(NAMES)
    assert lib.mcl_abi_version() == 4
    assert ctypes.sizeof(_lib.Timing) == 15 * 16                 # no timing slot was added
    hdr = open(os.path.join(ROOT, 'include', 'mcl.h')).read()
    assert 'mcl_match' not in hdr                                # mcl.h is what it was


def test_the_records_have_the_declared_sizes_and_offsets(eng):
    from smarc_navigation_amd import _lib
    s, r, t, d = eng.MATCH_SUMS, eng.MATCH_RESULT, eng.MATCH_TRACE, eng.MATCH_DERIVED
    assert s.itemsize == 152 and [s.fields[f][1] for f in ('n', 'n_miss', 'n_jump', 'S', 'C', 's_rho', 's_rho2')] == [0, 8, 16, 24, 104, 136, 144]
    assert r.itemsize == 360 and [r.fields[f][1] for f in ('x', 'y', 'yaw', 'z', 'status', 'evaluations', 'accepted', 'j', 'dead',
                                                             'start', 'final')] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 56, 208]
    assert t.itemsize == 192 and [t.fields[f][1] for f in ('x', 'sums', 'j', 'accepted')] == [0, 32, 184, 188]
    assert d.itemsize == 192 and [d.fields[f][1] for f in ('rms', 'mean', 'chi2', 'J', 'cov', 'dead', 'm')] == [0, 8, 16, 24, 104, 184, 188]
    c = _lib.MatchConfig
    assert ctypes.sizeof(c) == 72 and [getattr(c, f).offset for f in ('dims', 'max_iter', 'min_beams', 'grad_floor_q', 'step_max_xy',
                                                                      'step_max_yaw', 'tol_xy', 'tol_yaw', 'steps')] == [0, 4, 8, 12, 16, 24, 32, 40, 48]
    # the header says the same
    src = open(os.path.join(ROOT, 'include', 'mcl_match.h')).read()
    for name in ('mcl_match_sums', 'mcl_match_config', 'mcl_match_result', 'mcl_match_trace', 'mcl_match_derived_t'):
        assert re.search(r'typedef struct %s \{' % name, src), name
    assert '#define MCL_MATCH_J0 (-10)' in src and '#define MCL_MATCH_MAX_POSES 65536' in src


# ------------------------------------------------------------------ solve, better, derived: bit for bit
def _check_solve(eng, rec, cfg, j):
    got, dead = eng.match_solve(rec_array(rec), c_cfg(cfg), j)
    want, wdead = solve_ref(rec, cfg, j)
    assert [_bits(v) for v in got] == [_bits(v) for v in want] and dead == wdead, (rec, cfg, j, list(got), want, dead, wdead)
    return want, wdead


def _check_derived(eng, rec, cfg, sigma):
    got = eng.match_derived(rec_array(rec), c_cfg(cfg), sigma)
    want = derived_ref(rec, cfg, sigma)
    for f in ('rms', 'mean', 'chi2'):
        assert _bits(got[f]) == _bits(want[f]), (f, rec)
    assert [_bits(v) for v in got['J']] == [_bits(v) for v in want['J']], rec
    assert [_bits(v) for v in got['cov']] == [_bits(v) for v in want['cov']], rec
    assert int(got['dead']) == want['dead'] and int(got['m']) == want['m']
    return want


def test_solve_and_derived_equal_the_restatement_bit_for_bit_on_random_records(eng):
    rs = np.random.RandomState(2)
    seen_clamped = seen_free = 0
    for trial in range(300):
        D = 3 + trial % 2
        cfg = default_cfg(dims=D, delta_xy=float(rs.choice([0.5, 0.25, 0.3])), delta_yaw=float(rs.choice([0.01, 0.003, 0.05])),
                          grad_floor_q=int(rs.choice([0, 2, 9])), step_max_xy=float(rs.choice([2.0, 0.3, 1e-3])),
                          step_max_yaw=float(rs.choice([0.1, 1e-3])))
        rec = random_record(rs, D)
        j = int(rs.randint(J_MIN, J_MAX + 3))
        delta, _ = _check_solve(eng, rec, cfg, j)
        h = math.sqrt(delta[0] * delta[0] + delta[1] * delta[1])
        tight = h > 0.999 * cfg['step_max_xy'] or abs(delta[2]) > 0.999 * cfg['step_max_yaw'] or abs(delta[3]) > 0.999 * cfg['step_max_xy']
        seen_clamped += tight
        seen_free += not tight
        assert h <= cfg['step_max_xy'] * (1 + 1e-15) and abs(delta[2]) <= cfg['step_max_yaw'] * (1 + 1e-15)
        assert abs(delta[3]) <= cfg['step_max_xy'] * (1 + 1e-15)
        _check_derived(eng, rec, cfg, float(rs.choice([0.05, 0.2, 3.7])))
    assert seen_clamped > 20 and seen_free > 20


def test_the_solution_solves_the_damped_normal_equations(eng):
    rs = np.random.RandomState(3)
    for D in (3, 4):
        cfg = default_cfg(dims=D, step_max_xy=1e9, step_max_yaw=1e9)
        rec = random_record(rs, D, n=300, scale=4096, rho_scale=400)
        for j in (-20, -10, 0, 6):
            delta, dead = eng.match_solve(rec_array(rec), c_cfg(cfg), j)
            assert dead == (8 if D == 3 else 0)
            A, y = _normal(rec, cfg, list(range(D)))
            full = np.zeros((D, D))
            for r in range(D):
                for c in range(r + 1):
                    full[r, c] = full[c, r] = A[packed(r, c)]
            full[np.diag_indices(D)] *= 1.0 + 2.0 ** j
            perm = [0, 1, 2, 3][:D]
            want = np.linalg.solve(full, np.array(y))
            assert np.allclose([delta[k] for k in perm], want, rtol=1e-8, atol=1e-12)


def test_dead_dimensions_at_the_gradient_floor_and_a_record_the_factor_kills(eng):
    cfg = default_cfg(grad_floor_q=2)
    m = 10
    base = [(4096 + 17 * k, 300 * ((k % 3) - 1), 40 * ((k % 5) - 2) + 3 * k, 50 * ((k % 4) - 1) + k) for k in range(m)]
    # S_yy = 0: y is dead, its step exactly +0.0
    rec = record_of([(x, 0, w, r) for x, _, w, r in base])
    delta, dead = _check_solve(eng, rec, cfg, J0)
    assert dead == 2 | 8 and _bits(delta[1]) == _bits(0.0) and delta[0] != 0.0 and delta[2] != 0.0
    # S_yy = m floor^2 exactly: dead; one above: live
    at = record_of([(x, 2, w, r) for x, _, w, r in base])
    assert at[3][packed(1, 1)] == m * 4
    delta, dead = _check_solve(eng, at, cfg, J0)
    assert dead & 2 and _bits(delta[1]) == _bits(0.0)
    above = list(at)
    S = list(at[3])
    S[packed(1, 1)] += 1
    above[3] = tuple(S)
    delta, dead = _check_solve(eng, tuple(above), cfg, J0)
    assert not dead & 2 and delta[1] != 0.0
    _check_derived(eng, at, cfg, SIGMA)
    assert derived_ref(at, cfg, SIGMA)['cov'][packed(1, 1)] == math.inf
    # yaw a multiple of x in every beam: the undamped factor (derived) kills the yaw column; the damped one cannot -- a
    # damping of 2^-20 or more leaves a pivot of about 2^-19 of its diagonal, above the factor's floor of 2^-26
    tied = record_of([(37 * k, 11 * ((k % 7) - 3), 74 * k, 13 * ((k % 5) - 2) + k) for k in range(1, 41)])
    delta, dead = _check_solve(eng, tied, cfg, J_MIN)
    assert dead == 8 and delta[2] != 0.0 and delta[0] != 0.0
    d = _check_derived(eng, tied, cfg, SIGMA)
    assert d['dead'] == 4 | 8 and d['cov'][packed(2, 2)] == math.inf and math.isfinite(d['cov'][packed(0, 0)]) and d['J'][packed(2, 2)] > 0.0
    # nothing live at all: every step 0, and the loop calls that CONVERGED
    none = record_of([(0, 1, 0, 5)] * 9)
    delta, dead = _check_solve(eng, none, cfg, J0)
    assert dead == 15 and all(_bits(v) == _bits(0.0) for v in delta)
    # no contributing beam
    empty = (5, 3, 2, (0,) * 10, (0,) * 4, 0, 0)
    assert _check_solve(eng, empty, cfg, J0)[1] == 15
    assert _check_derived(eng, empty, cfg, SIGMA)['rms'] == 0.0


def test_the_covariance_and_the_information_of_a_fix_are_symmetric_and_inverse_to_one_another(eng):
    """PingMatch.cov / .information: the full symmetric D x D matrices, sigma^2 A^-1 and A / sigma^2 -- their product is the
    identity over the live dimensions; a dead dimension has +inf on the diagonal of cov and zeros beside it"""
    rs = np.random.RandomState(6)
    for trial in range(40):
        D = 3 + trial % 2
        cfg = default_cfg(dims=D)
        rec = random_record(rs, D, n=int(rs.choice([64, 300])), scale=int(rs.choice([4096, 1 << 16])), rho_scale=400)
        if trial % 5 == 0:                      # no gradient in y: dead
            S, Cv = list(rec[3]), list(rec[4])
            for k in range(4):
                S[packed(max(k, 1), min(k, 1))] = 0
            Cv[1] = 0
            rec = rec[:3] + (tuple(S), tuple(Cv)) + rec[5:]
        res = np.zeros(1, eng.MATCH_RESULT)
        res['final'] = rec_array(rec)
        match = eng.PingMatch(res, c_cfg(cfg), SIGMA)
        cov, J = match.cov(0), match.information(0)
        want = derived_ref(rec, cfg, SIGMA)
        assert cov.shape == J.shape == (D, D)
        for r in range(D):
            for c in range(D):
                assert _bits(cov[r, c]) == _bits(want['cov'][packed(max(r, c), min(r, c))]), (trial, r, c)
                assert _bits(J[r, c]) == _bits(want['J'][packed(max(r, c), min(r, c))]), (trial, r, c)
        assert np.array_equal(cov, cov.T) and np.array_equal(J, J.T)
        live = [k for k in range(D) if not want['dead'] >> k & 1]
        assert len(live) == (D - 1 if trial % 5 == 0 else D)
        assert np.any(cov[np.ix_(live, live)][np.triu_indices(len(live), 1)] != 0.0)        # the upper triangle is there
        assert np.allclose(cov[np.ix_(live, live)].dot(J[np.ix_(live, live)]), np.identity(len(live)), rtol=0, atol=1e-8)
        for k in range(D):
            if k not in live:
                assert cov[k, k] == math.inf and not np.delete(cov[k], k).any() and not J[k].any()


def test_better_is_an_exact_compare_up_to_the_largest_legal_sums(eng):
    top = record_of([(D_MAX, -D_MAX, D_MAX, RHO_MAX)] * MAX_BEAMS)
    assert top[6] == 1 << 59 and top[3][0] == 1 << 57 and top[4][0] == 1 << 58
    less = record_of([(D_MAX, -D_MAX, D_MAX, RHO_MAX)] * (MAX_BEAMS - 1) + [(D_MAX, -D_MAX, D_MAX, RHO_MAX - 1)])
    fewer = record_of([(D_MAX, -D_MAX, D_MAX, RHO_MAX)] * (MAX_BEAMS - 1), n_miss=1)
    cases = [(top, top), (less, top), (top, less), (fewer, top), (top, fewer), (less, fewer), (fewer, less)]
    rs = np.random.RandomState(4)
    for _ in range(200):
        cases.append((random_record(rs), random_record(rs)))
    # products that differ by one unit in 2^70: s_rho2 m equal but for the last bit
    a = record_of([(1, 1, 1, RHO_MAX)] * 2047 + [(1, 1, 1, RHO_MAX - 1)])
    b = record_of([(1, 1, 1, RHO_MAX)] * 2047 + [(1, 1, 1, RHO_MAX - 2)])
    cases += [(a, b), (b, a), (a, a)]
    seen = set()
    for q, p in cases:
        for min_beams in (1, 8, 2048):
            want = better_ref(q, p, min_beams)
            assert eng.match_better(rec_array(q), rec_array(p), min_beams) == want, (q, p, min_beams)
            seen.add(want)
    assert seen == {True, False}
    assert eng.match_better(rec_array(less), rec_array(top), 8) and not eng.match_better(rec_array(top), rec_array(top), 8)
    assert not eng.match_better(rec_array(less), rec_array(top), 2049 - 1 + 1)       # too few beams
    cfg = default_cfg()
    _check_solve(eng, top, cfg, J_MAX)
    _check_derived(eng, top, cfg, SIGMA)


def test_impossible_records_configs_and_null_pointers_are_refused(eng, lib):
    from smarc_navigation_amd import _lib
    cfg = default_cfg()
    ok = record_of([(100, 50, 3, 7)] * 10)
    bad = [(-1,) + ok[1:], (2049,) + ok[1:], (10, 11, 0) + ok[3:], (10, 6, 5) + ok[3:], (10, -1, 0) + ok[3:],
           ok[:3] + ((-1,) + ok[3][1:],) + ok[4:], ok[:3] + (((10 << 46) + 1,) + ok[3][1:],) + ok[4:],
           ok[:4] + (((10 << 47) + 1, 0, 0, 0),) + ok[5:], ok[:5] + ((10 << 24) + 1, ok[6]), ok[:6] + (-1,), ok[:6] + ((10 << 48) + 1,)]
    for r in bad:
        with pytest.raises(eng.MclError) as ei:
            eng.match_solve(rec_array(r), c_cfg(cfg), J0)
        assert ei.value.status == ERR_INVALID, r
        with pytest.raises(eng.MclError):
            eng.match_derived(rec_array(r), c_cfg(cfg), SIGMA)
        with pytest.raises(eng.MclError):
            eng.match_better(rec_array(r), rec_array(ok), 8)
    for j in (J_MIN - 1, J_MAX + 3):
        with pytest.raises(eng.MclError):
            eng.match_solve(rec_array(ok), c_cfg(cfg), j)
    for s in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(eng.MclError):
            eng.match_derived(rec_array(ok), c_cfg(cfg), s)
    with pytest.raises(eng.MclError):
        eng.match_better(rec_array(ok), rec_array(ok), 0)
    assert eng.match_config_check(c_cfg(cfg), R_MAX) is None
    for k, vals in dict(dims=(2, 5), max_iter=(0, 33), min_beams=(0, -3), grad_floor_q=(-1, 4097), step_max_xy=(0.0, math.inf, math.nan),
                        step_max_yaw=(0.0, -1.0), tol_xy=(-1e-9, math.nan), tol_yaw=(-1.0, math.inf), delta_xy=(0.0, math.nan),
                        delta_yaw=(0.0, -0.01), jump_max=(0.0, R_MAX + 1.0)).items():
        for v in vals:
            c = c_cfg(cfg)
            if k in ('delta_xy', 'delta_yaw', 'jump_max'):
                setattr(c.steps, k, v)
            else:
                setattr(c, k, v if isinstance(v, int) else float(v))
            why = eng.match_config_check(c, R_MAX)
            assert why, (k, v)
            if k != 'jump_max':                 # (the steps against r_max are the device call's business alone)
                with pytest.raises(eng.MclError):
                    eng.match_solve(rec_array(ok), c, J0)
    assert eng.match_config_check(c_cfg(default_cfg(max_iter=32, tol_xy=0.0, grad_floor_q=0)), R_MAX) is None
    assert eng.match_config_check(c_cfg(cfg), 4096.5) and eng.match_config_check(None, R_MAX)
    buf = (ctypes.c_uint64 * 64)()
    i = ctypes.c_int32(0)
    c = c_cfg(cfg)
    assert lib.mcl_match_solve(None, ctypes.byref(c), 0, buf, ctypes.byref(i)) == ERR_INVALID
    assert lib.mcl_match_solve(buf, None, 0, buf, ctypes.byref(i)) == ERR_INVALID
    assert lib.mcl_match_solve(buf, ctypes.byref(c), 0, None, ctypes.byref(i)) == ERR_INVALID
    assert lib.mcl_match_solve(buf, ctypes.byref(c), 0, buf, None) == ERR_INVALID
    assert lib.mcl_match_solve(buf, ctypes.byref(c), 0, buf, ctypes.byref(i)) == 0
    assert lib.mcl_match_better(None, buf, 1, ctypes.byref(i)) == ERR_INVALID and lib.mcl_match_better(buf, buf, 1, None) == ERR_INVALID
    assert lib.mcl_match_derived(buf, ctypes.byref(c), SIGMA, None) == ERR_INVALID
    assert lib.mcl_match_ping(None, buf, 1, buf, buf, 1, SIGMA, R_MAX, None, ctypes.byref(c), buf, None, None) == ERR_INVALID
    assert _lib.MatchConfig().dims == 0


# ------------------------------------------------------------------ the restated loop on the oracle's casts
@pytest.mark.parametrize('kind', ['grid', 'mesh', 'tin'])
@pytest.mark.parametrize('dims', [3, 4])
def test_the_restated_loop_recovers_the_truth_on_rough_terrain(dims, kind):
    ref = rough_reference(dims, kind)
    errs = []
    for k, run in enumerate(ref['runs']):
        start = ref['starts'][:, k]
        d0 = math.hypot(start[0] - TRUTH[0], start[1] - TRUTH[1])
        err = horizontal_error(run)
        errs.append(err)
        print('%s dims %d start %d: %.2f m off -> status %d after %d evaluations, %.2e m off, rms %.1f quanta' % (
            kind, dims, k, d0, run['status'], run['evaluations'], err, math.sqrt(run['final'][6] / max(m_of(run['final']), 1))))
        assert run['status'] == CONVERGED and run['evaluations'] <= 13
        assert err < 2e-3 and abs(run['pose'][2] - TRUTH[5]) < 1e-3            # 2 mm: eight quanta of the ranges
        if dims == 4:
            assert abs(run['pose'][3] - TRUTH[2]) < 2e-3
        else:
            assert _bits(run['pose'][3]) == _bits(start[2])
        # the accept rule: the mean square residual never rises
        acc = [t for t in run['trace'] if t[3]]
        for a, b in zip(acc, acc[1:]):
            assert b[1][6] * m_of(a[1]) < a[1][6] * m_of(b[1])
    assert len(errs) == 8


def rms_quanta(rec):
    return math.sqrt(rec[6] / m_of(rec)) if m_of(rec) > 0 else 0.0


@pytest.mark.parametrize('dims', [3, 4])
def test_the_restated_loop_stops_in_a_local_minimum_from_a_start_far_away(dims):
    ref = rough_reference(dims)
    z, origin, _ = scene()
    _, omap = scene_map('grid', z, origin)
    run = loop_both(OracleEval(omap, ref['ba'], ref['meas'], ref['cfg']), LOCAL_STARTS[dims], ref['cfg'])
    print('dims %d local minimum: status %d after %d evaluations, %.2f m off, rms %.0f -> %.0f quanta' % (
        dims, run['status'], run['evaluations'], horizontal_error(run), rms_quanta(run['start']), rms_quanta(run['final'])))
    assert run['status'] == MAX_ITER and run['evaluations'] == 13 and horizontal_error(run) > 5.0
    assert 100.0 < rms_quanta(run['final']) <= rms_quanta(run['start'])          # its final cost tells it apart


def _grid_eval(z, pose_truth, cfg, B=64):
    from oracle import oracle as orc
    omap = orc.Grid(z, GRID_ORIGIN, 1.0)
    ba = synth.beam_angles(B)
    meas = ping_at(omap, pose_truth, ba, np.identity(4), [0] * 6, BC_RMAX)
    return OracleEval(omap, ba, meas, cfg, np.identity(4), [0] * 6, BC_RMAX)


def test_flat_seabed_x_y_and_yaw_keep_their_bits_and_z_is_recovered():
    cfg = default_cfg(dims=4, jump_max=BC_RMAX)
    truth = FLAT_START.copy()
    truth[2] = -2.0
    run = loop_both(_grid_eval(flat_grid(), truth, cfg), FLAT_START, cfg)
    print('flat: status %d, %d evaluations, z %.6f, dead %d' % (run['status'], run['evaluations'], run['pose'][3], run['dead']))
    assert run['status'] == CONVERGED and run['dead'] == 1 | 2 | 4
    assert [_bits(v) for v in run['pose'][:3]] == [_bits(FLAT_START[0]), _bits(FLAT_START[1]), _bits(FLAT_START[5])]
    assert abs(run['pose'][3] - truth[2]) < 1e-3
    for k in (0, 1, 2):
        assert run['final'][3][packed(k, k)] == 0 and run['start'][3][packed(k, k)] == 0      # their square sums are 0


def test_ridge_along_x_keeps_the_bits_of_x_and_recovers_y():
    cfg = default_cfg(dims=3, jump_max=BC_RMAX)
    run = loop_both(_grid_eval(ridge_grid(), RIDGE_TRUTH, cfg), RIDGE_START, cfg)
    print('ridge: status %d, %d evaluations, y %.6f (truth %.6f), dead %d' % (run['status'], run['evaluations'], run['pose'][1],
                                                                              RIDGE_TRUTH[1], run['dead']))
    assert run['status'] == CONVERGED and run['dead'] & 1
    assert _bits(run['pose'][0]) == _bits(RIDGE_START[0])
    assert abs(run['pose'][1] - RIDGE_TRUTH[1]) < 2e-3


def test_a_start_off_the_map_is_no_overlap():
    ref = rough_reference(3)
    z, origin, _ = scene()
    _, omap = scene_map('grid', z, origin)
    ev = OracleEval(omap, ref['ba'], ref['meas'], ref['cfg'])
    start = TRUTH.copy()
    start[0] += 280.0
    run = loop_both(ev, start, ref['cfg'])
    assert run['status'] == NO_OVERLAP and run['evaluations'] == 1 and ev.calls == 1 and m_of(run['start']) == 0
    assert [_bits(v) for v in run['pose']] == [_bits(start[0]), _bits(start[1]), _bits(start[5]), _bits(start[2])]


@pytest.mark.parametrize('kind', ['grid', 'mesh', 'tin'])
def test_the_oracle_alone_keeps_the_gpu_scene_within_the_outlier_cap_at_the_poses_of_the_match(kind):
    """the rays whose fp64 answer jumps when the sensor moves by 1 mm are the ones a fp32 cast may miss by more than 1e-3 m
    (helpers.outliers_explained excuses exactly those).  tests/test_gpu_match.py compares dumped ranges at the poses the
    kernel traces from the starts of starts_of(4) with a ping of 300 beams; here the loop -- restated, and decided once more
    by the library -- is traced from the same starts with the same ping on the oracle's casts, and at the 1 + 2 D variants
    of every pose it evaluates, and of the truth, the share of such rays stays under the cap"""
    from oracle import oracle as orc
    from tests.test_innovation_host import OUTLIER_CAP
    z, origin, _ = scene()
    _, omap = scene_map(kind, z, origin)
    ba = synth.beam_angles(300)
    cfg = default_cfg(dims=4)
    ev = OracleEval(omap, ba, ping_at(omap, TRUTH, ba), cfg)
    starts = starts_of(4)
    poses = [TRUTH]
    for k in range(starts.shape[1]):
        run = loop_both(ev, starts[:, k], cfg)
        assert run['status'] == CONVERGED
        poses += [[p[0], p[1], p[3], starts[3, k], starts[4, k], p[2]] for p, _, _, _ in run['trace']]
    poses = np.array(poses).T
    assert poses.shape[1] > 30
    base = np.ascontiguousarray(np.concatenate([variants(poses[:, k], cfg) for k in range(poses.shape[1])], axis=1))
    ref = orc.mbes_update(base, M2O, OFF, omap, ba, None, SIGMA, R_MAX)[1]
    moved = np.zeros(ref.shape, bool)
    for axis in range(3):
        for sgn in (1.0, -1.0):
            s_ = base.copy()
            s_[axis] += sgn * 1e-3
            moved |= np.abs(orc.mbes_update(s_, M2O, OFF, omap, ba, None, SIGMA, R_MAX)[1] - ref) > 0.1
    print('%s: %d of %d rays jump under a 1 mm shift; %.1f %% hit' % (kind, int(moved.sum()), moved.size, 100.0 * (ref < R_MAX).mean()))
    assert moved.mean() < OUTLIER_CAP and (ref < R_MAX).mean() > 0.99


def test_the_yaw_rule_and_the_pose_step():
    assert wrap_ref(3.0) == 3.0 and wrap_ref(-math.pi) == -math.pi
    assert abs(wrap_ref(math.pi + 0.25) - (-math.pi + 0.25)) < 1e-15 and abs(wrap_ref(-math.pi - 0.25) - (math.pi - 0.25)) < 1e-15
    q = next_pose_ref([-0.0, 1.0, 3.1, -2.0], [0.0, 0.5, 0.1, 0.0])
    assert _bits(q[0]) == _bits(-0.0) and q[1] == 1.5 and q[2] < -3.0 and _bits(q[3]) == _bits(-2.0)


# ------------------------------------------------------------------ the sanitizer driver
def test_the_host_arithmetic_runs_clean_under_the_sanitizers_as_a_program(tmp_path):
    """tests/host_san/match_driver.cpp: its own main over the device-free functions, g++ -fsanitize=address,undefined, run as
    a program (nothing loaded into Python runs under a sanitizer)"""
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no g++ / make')
    san = str(tmp_path / 'host_san')
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'smarc_navigation_amd', 'csrc'), 'host-asan-match', 'SAN_DIR=' + san],
                          stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(san, 'match_asan')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                       timeout=300, cwd=ROOT)
    for marker in ('AddressSanitizer', 'runtime error', 'LeakSanitizer'):
        assert marker not in p.stdout, p.stdout[-2000:]
    assert p.returncode == 0 and 'match_driver: ok' in p.stdout, p.stdout[-2000:]
