"""CPU tests of ESS-targeted tempering (include/mcl_temper.h): the seven symbols are exported at ABI version 4; the
exponent lattice, the 128-bit pass predicate and the round plan -- pure host functions -- against a restatement of the
header in Python integers, `decimal` and the oracle's det_exp; and the three-round search, driven only by
mcl_temper_candidates and mcl_temper_pass, against a linear scan of all 2049 levels.

The restatement (beta_ref, Cloud.sums, search_ref, linear_ref, case_lw) is what tests/test_gpu_temper.py holds the kernels
to as well."""
import ctypes
import decimal
import math

import numpy as np
import pytest

NAMES = ('mcl_temper_beta', 'mcl_temper_pass', 'mcl_temper_candidates', 'mcl_temper', 'mcl_temper_sums', 'mcl_temper_apply',
         'mcl_group_temper')
LEVELS = 2048
CASES = ('peaked', 'gps', 'flat', 'floor', 'two_maxima', 'peaked_nonfinite')
RATIOS = (0.5, 0.1)


# ------------------------------------------------------------------ the restatement of include/mcl_temper.h
def _table():
    ctx = decimal.Context(prec=80)
    return [float(ctx.power(decimal.Decimal(2), ctx.divide(decimal.Decimal(-i), decimal.Decimal(64)))) for i in range(64)]


_T = _table()   # float(Decimal) rounds correctly: the 64 correctly rounded doubles of 2^(-i / 64)


def beta_ref(j):
    return math.ldexp(_T[j % 64], -(j // 64))


def _orc():
    from oracle import oracle
    return oracle


def _q_sum(e, counts):
    """sum of counts * floor(det_exp(e) 2^32) as a Python integer (det_exp returns 0 below -700: those are not called)"""
    det_exp = _orc().det_exp
    live = e >= -700.0
    return sum(int(c) * int(det_exp(float(x)) * 4294967296.0) for x, c in zip(e[live], counts[live]))


class Cloud(object):
    """the log-weights of a whole cloud as the definition sees them: the finite values (distinct ones with their counts: the
    sums are integers, so this is exact), their maximum m, and S1, S2 per level, computed on demand and kept"""

    def __init__(self, lw, m=None):
        lw = np.asarray(lw, dtype=np.float64)
        fin = lw[np.isfinite(lw)]
        self.n, self.n_live = int(lw.size), int(fin.size)
        self.m = (float(fin.max()) if fin.size else -math.inf) if m is None else float(m)
        self.vals, self.counts = np.unique(fin, return_counts=True)
        self.memo = {}

    def sums(self, j):
        if j not in self.memo:
            if self.vals.size == 0 or self.m == -math.inf:
                self.memo[j] = (0, 0)
            else:
                d = self.vals - self.m              # one IEEE operation each
                e = beta_ref(j) * d
                self.memo[j] = (_q_sum(e, self.counts), _q_sum(2.0 * e, self.counts))
        return self.memo[j]


def pass_ref(s1, s2, n_t):
    return s1 * s1 >= n_t * s2 * (1 << 32)


def search_ref(sums, n_t):
    """the three rounds of the header over sums(j) -> (S1, S2): (j, floor_hit, levels_evaluated)"""
    def first(cands):
        for j in cands:
            if pass_ref(*sums(j), n_t):
                return j
        return None
    levels = 17
    j1 = first(range(0, LEVELS + 1, 128))
    if j1 is None:
        return LEVELS, 1, levels
    if j1 == 0:
        return 0, 0, levels
    levels += 15
    j2 = first(range(j1 - 120, j1, 8))
    j2 = j1 if j2 is None else j2
    levels += 7
    j3 = first(range(j2 - 7, j2))
    return (j2 if j3 is None else j3), 0, levels


def linear_ref(sums, n_t):
    for j in range(LEVELS + 1):
        if pass_ref(*sums(j), n_t):
            return j, 0
    return LEVELS, 1


def n_target_of(ratio, n):
    return max(1, int(math.ceil(ratio * n)))


def case_lw(name, n, seed=11, pool=None):
    """the log-weights of a named case; pool: draw the random cases from that many distinct values (large n)"""
    rs = np.random.RandomState(seed)
    k = n if pool is None else min(pool, n)

    def spread(v):
        return v if k == n else v[rs.randint(0, k, n)]
    if name in ('peaked', 'peaked_nonfinite'):
        x = 3.0 * rs.randn(k, 2)
        lw = spread(-256.0 * (x[:, 0] ** 2 + x[:, 1] ** 2))
        if name == 'peaked_nonfinite':
            lw[::3] = -np.inf
            lw[1::7] = np.nan
            lw[5::11] = np.inf
        return lw
    if name == 'gps':
        z = 2.0 * rs.randn(k)
        return spread(-0.5 * z * z)
    if name == 'flat':
        return np.full(n, -3.25)
    if name == 'floor':
        lw = np.full(n, -1e12)
        lw[0] = 0.0
        return lw
    if name == 'two_maxima':
        lw = np.full(n, -800.0)
        lw[0] = lw[n - 1] = -1.5
        return lw
    raise ValueError(name)


# ------------------------------------------------------------------ symbols
def test_temper_symbols_exported_and_bound_at_abi_4():
    from smarc_navigation_amd import _lib
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(raw, n), 'libmcl_hip.so does not export %s' % n
        assert n in _lib.TEMPER_SYMBOLS
    assert sorted(_lib.TEMPER_SYMBOLS) == sorted(NAMES)
    lib = _lib.load()
    assert lib.mcl_abi_version() == 4
    assert lib.mcl_temper_pass.argtypes is not None
    assert ctypes.sizeof(_lib.TemperRes) == 4 * 4 + 2 * 8 + 2 * 8


def test_header_declares_exactly_the_exported_symbols():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'include', 'mcl_temper.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert sorted(set(re.findall(r'\b(mcl_[a-z0-9_]+)\s*\(', src))) == sorted(NAMES)


# ------------------------------------------------------------------ the lattice
def test_beta_lattice():
    from smarc_navigation_amd import engine
    b = [engine.temper_beta(j) for j in range(LEVELS + 1)]
    assert b[0] == 1.0 and b[LEVELS] == 2.0 ** -32
    for j in range(LEVELS + 1):
        assert b[j] == beta_ref(j), j
        assert abs(b[j] - 2.0 ** (-j / 64.0)) <= 2.0 ** -52 * b[j], j
        if j >= 64:
            assert b[j - 64] == 2.0 * b[j], j
        if j >= 1:
            assert b[j] < b[j - 1], j
    for j in (-1, LEVELS + 1):
        with pytest.raises(engine.MclError) as ei:
            engine.temper_beta(j)
        assert ei.value.status == -1


# ------------------------------------------------------------------ the predicate
def test_pass_equals_the_big_integer_comparison():
    from smarc_navigation_amd import engine
    rs = np.random.RandomState(5)

    def u(bits):
        return int.from_bytes(rs.bytes(8), 'little') >> (64 - bits)
    triples = []
    for _ in range(400):                       # sums as the kernels can form them: below 2^56, n_t <= 2^24, ratio near 1
        s1 = u(56)
        n_t = int(rs.randint(1 << 16, (1 << 24) + 1))    # (s2 stays below 2^64)
        s2 = (s1 * s1) // (n_t << 32) + int(rs.randint(-3, 4))
        triples.append((s1, max(s2, 0), n_t))
    for _ in range(400):                       # anything 64 bits hold, n_t up to 2^62: the right side may pass 2^128
        triples.append((u(64), u(64), int(rs.randint(1, 1 << 31)) << int(rs.randint(0, 32))))
    triples += [(1 << 56, 1 << 56, 1 << 24), ((1 << 56) - 1, 1 << 56, 1 << 24), (0, 0, 1), (0, 1, 1), (1, 0, 1 << 24),
                ((1 << 64) - 1, (1 << 64) - 1, (1 << 63) - 1), ((1 << 64) - 1, 1, 1 << 32), ((1 << 64) - 1, (1 << 32) - 2, 1 << 32)]
    for s1, s2, n_t in triples:
        assert engine.temper_pass(s1, s2, n_t) == pass_ref(s1, s2, n_t), (s1, s2, n_t)
    # equality passes, one less fails: s1^2 = n_t s2 2^32 with s1 = 2^36 k, s2 = 2^40 k^2 / n_t
    for k, n_t in ((3, 9), (5, 1), (1 << 10, 1 << 20), (12345, 15)):
        s1 = k << 36
        assert (k * k << 40) % n_t == 0
        s2 = (k * k << 40) // n_t
        assert s1 * s1 == n_t * s2 << 32
        assert engine.temper_pass(s1, s2, n_t) and not engine.temper_pass(s1 - 1, s2, n_t) and not engine.temper_pass(s1, s2 + 1, n_t)
    assert engine.temper_pass(1 << 56, 1 << 56, 1 << 24)       # the extremes of a 2^24-particle cloud: equality
    for bad in (0, -1):
        with pytest.raises(engine.MclError):
            engine.temper_pass(1, 1, bad)


# ------------------------------------------------------------------ the round plan
def test_candidates_are_the_rounds_of_the_header():
    from smarc_navigation_amd import engine
    assert engine.temper_candidates(1) == list(range(0, LEVELS + 1, 128))
    assert engine.temper_candidates(1, 777) == list(range(0, LEVELS + 1, 128))
    for j1 in range(128, LEVELS + 1, 128):
        assert engine.temper_candidates(2, j1) == list(range(j1 - 120, j1, 8))
    for j2 in range(8, LEVELS + 1, 8):
        assert engine.temper_candidates(3, j2) == list(range(j2 - 7, j2))
    assert engine.temper_candidates(2, 0) == [] and engine.temper_candidates(3, 0) == []
    for rnd, jp in ((0, 0), (4, 0), (2, 64), (2, 2176), (3, 4), (3, -8), (2, -128)):
        with pytest.raises(engine.MclError):
            engine.temper_candidates(rnd, jp)


def search_abi(sums, n_t):
    """the search driven ONLY by mcl_temper_candidates and mcl_temper_pass, as a rank would drive it"""
    from smarc_navigation_amd import engine

    def first(cands):
        for j in cands:
            if engine.temper_pass(*sums(j), n_t):
                return j
        return None
    j1 = first(engine.temper_candidates(1))
    if j1 is None:
        return LEVELS, 1
    j2 = first(engine.temper_candidates(2, j1))
    j2 = j1 if j2 is None else j2
    j3 = first(engine.temper_candidates(3, j2))
    return (j2 if j3 is None else j3), 0


@pytest.mark.parametrize('n', [65, 1000])
@pytest.mark.parametrize('name', CASES)
def test_sectioning_search_equals_the_linear_scan(name, n):
    cloud = Cloud(case_lw(name, n))
    for ratio in RATIOS:
        n_t = n_target_of(ratio, n)
        want = linear_ref(cloud.sums, n_t)
        assert search_abi(cloud.sums, n_t) == want, (name, n, ratio)
        assert search_ref(cloud.sums, n_t)[:2] == want, (name, n, ratio)
        j = want[0]
        if j > 0 and not want[1]:
            assert not pass_ref(*cloud.sums(j - 1), n_t)       # the level below the result fails
