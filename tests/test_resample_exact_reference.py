"""CPU tests of the exact integer reference of the resamplers (tests/helpers.py: exact_resample) -- before it judges a
kernel (tests/test_gpu_resample_schemes.py) it must describe the operation of the reference project: its golden index
vectors under the project's rule, the decisions on a CDF edge written out as literals, the Philox
restatement against the oracle's, and numpy's chunked pairwise sum (what the residual scheme's renormalisation restates)
on both sides of a chunk border."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import helpers


def test_integer_reference_agrees_with_the_reference_golden_indices():
    """systematic / naive / stratified / multinomial golden vectors of resampling.py: exact for N <= 4096, at most 2
    differing indices per case at N = 65 536 (the reference's own fp64 cumsum rounding)."""
    g = helpers.load('resampling_kat')
    counts, total = {}, {}
    for tag in g['cases']:
        w = g[tag + '_w']
        n = w.size
        u = np.random.RandomState(int(g[tag + '_seed'])).random_sample(n)   # a prefix is what the scheme consumes
        q, _, _ = orc.fixed_weights(w, 2)
        U = helpers.u53_of(u)
        for scheme in helpers.EXACT_SCHEMES:
            key = tag + '_' + scheme + '_resample'
            if key not in g:
                continue
            idx = helpers.exact_resample(q, U, scheme)
            miss = int(np.count_nonzero(idx != g[key]))
            if n <= 4096:
                assert miss == 0, key
            else:
                assert miss <= 2, (key, miss)
                total[scheme] = total.get(scheme, 0) + miss
            counts[scheme] = counts.get(scheme, 0) + 1
    assert min(counts.get(s, 0) for s in helpers.EXACT_SCHEMES) >= 20, counts
    print('integer reference vs golden indices at N = 65 536, mismatches summed over the cases: %r' % (total,))


@pytest.mark.parametrize('n', [1, 2, 5, 64])
def test_decisions_on_a_cdf_edge_are_these(n):
    """What "evaluated exactly" means where a position sits ON an edge: equal weights and u = 0 put position i on
    C_{i-1}.  `<` (systematic, stratified) steps over the edge: arange(n).  `<=` (naive) stays: [0, 0, 1, .., n - 2]."""
    q = [1 << 40] * n
    assert helpers.exact_resample(q, [0], 'systematic').tolist() == list(range(n))
    assert helpers.exact_resample(q, [0] * n, 'stratified').tolist() == list(range(n))
    assert helpers.exact_resample(q, [0], 'naive').tolist() == [0] + list(range(n - 1))
    # multinomial on the edges U_i = m 2^53 / n: `C_j 2^53 >= U T` holds first at j = m - 1 (and at 0 for m = 0)
    if n == 64:
        U = [m * ((1 << 53) // n) for m in range(n)]
        assert helpers.exact_resample(q, U, 'multinomial').tolist() == [0] + list(range(n - 1))
    # one unit past the edge, every scheme steps over it
    assert helpers.exact_resample(q, [1], 'naive').tolist() == list(range(n))


def test_small_cases_by_hand():
    """q = (1, 2, 1): C = (1, 3, 4), T = 4, N = 3; positions (U + i 2^53) 4 against C_j 3 2^53."""
    q = [1, 2, 1]
    half = 1 << 52
    # u = 1/2: positions 1/6, 1/2, 5/6 against 1/4, 3/4, 1
    assert helpers.exact_resample(q, [half], 'systematic').tolist() == [0, 1, 2]
    # u = 3/4: positions 1/4 (on the first edge), 7/12, 11/12
    U = [3 << 51]
    assert helpers.exact_resample(q, U, 'systematic').tolist() == [1, 1, 2]
    assert helpers.exact_resample(q, U, 'naive').tolist() == [0, 1, 2]
    # multinomial: u = 1/4 sits on C_0 / T, u = 3/4 on C_1 / T, u just above 3/4 goes on
    assert helpers.exact_resample(q, [1 << 51, 3 << 51, (3 << 51) + 1], 'multinomial').tolist() == [0, 1, 2]
    # no weight at all: strict comparisons never hold (n - 1), non-strict ones hold at once (0)
    assert helpers.exact_resample([0, 0, 0], [5], 'systematic').tolist() == [2, 2, 2]
    assert helpers.exact_resample([0, 0, 0], [5] * 3, 'stratified').tolist() == [2, 2, 2]
    assert helpers.exact_resample([0, 0, 0], [5], 'naive').tolist() == [0, 0, 0]
    assert helpers.exact_resample([0, 0, 0], [5] * 3, 'multinomial').tolist() == [0, 0, 0]


def test_systematic_reference_equals_the_oracle_offspring_cdf():
    """the two statements of the systematic scheme -- min{j} over the positions here, the offspring CDF in
    oracle/mcl_oracle.c -- give the same indices, ragged sizes and underflowing particles included"""
    for n in (1, 2, 7, 1025, 4097):
        rs = np.random.RandomState(n)
        for mode in (0, 1):
            lw = -0.5 * (rs.randn(n) * 3.0) ** 2 - (300.0 if mode else 0.0)
            if n > 10:
                lw[rs.randint(0, n, size=n // 10)] = -1e4
            u = rs.random_sample()
            q, tot, _ = orc.fixed_weights(lw, mode)
            ref = orc.indices_from_ncum(orc.systematic_ncum(q, orc.u_to_u53(u), 0, tot, n))
            assert np.array_equal(helpers.exact_resample(q, helpers.u53_of(u), 'systematic'), ref), (n, mode)


def test_philox_restatement_equals_the_oracle():
    seed = 0x1234567890abcdef
    k = (seed & 0xffffffff, seed >> 32)
    ctr = [(0, 0, 0, 4), (1, 0, 2, 4), (65538, 0, 7, 4), (0xffffffff, 0, 3, 3), (12345, 1, 0xfffffffe, 6)]
    for c in ctr:
        got = [int(v) for v in helpers.philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1])]
        assert got == [int(v) for v in orc.philox(c, k)], c
    # and the draw rule on top of it: the systematic scheme's single uniform is the same rule at counter 0xffffffff, purpose 3
    x, y, _, _ = helpers.philox4x32_10(0xffffffff, 0, 5, 3, k[0], k[1])
    assert (((int(x) >> 5) << 26) | (int(y) >> 6)) == orc.native_u53(seed, 5)
    U = helpers.native_draws_u53(seed, 2, 70000)
    o = orc.philox((65538, 0, 2, 4), k)
    assert U[65538] == ((int(o[0]) >> 5) << 26) | (int(o[1]) >> 6) and all(0 <= v < (1 << 53) for v in U)
    assert U[:16] != helpers.native_draws_u53(seed, 3, 16)


@pytest.mark.parametrize('n', [7, 8, 129, 8191, 8192, 8193, 16389, 65536, 100003])
def test_numpy_sum_is_the_chunked_pairwise_sum(n):
    """oracle.numpy_sum (and with it mcl_resample_alt.h: k_np_chunk_sums / k_np_sum_final, the same recursion) is
    np.sum bit for bit on both sides of the 8192-element chunk border; the UNCHUNKED recursion is not"""
    rs = np.random.RandomState(n)
    differs = 0
    for rep in range(20):
        a = np.exp(-0.5 * (rs.randn(n) * 2.0) ** 2) + 1e-200
        want = float(np.sum(a))
        assert orc.numpy_sum(a) == want, (n, rep)
        if n > 8192:
            differs += _unchunked(a) != want
    if n > 8192:
        assert differs > 0   # (so a restatement without the chunks would not pass here)
        print('n = %d: the unchunked pairwise recursion differs from np.sum on %d of 20 vectors' % (n, differs))


def _unchunked(a):
    """numpy's pairwise recursion over the whole array, without the 8192-element chunks"""
    n = a.size
    if n <= 8192:
        return orc.numpy_sum(a)   # (one chunk: the plain recursion)
    n2 = n // 2
    n2 -= n2 % 8
    return _unchunked(a[:n2]) + _unchunked(a[n2:])
