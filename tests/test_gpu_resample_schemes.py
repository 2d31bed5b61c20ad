"""GPU tests of the non-systematic resampling schemes (NAIVE, STRATIFIED, MULTINOMIAL, RESIDUAL) through a handle.

The four CDF schemes (systematic, naive, stratified, multinomial) are compared, index for index and without a
tolerance, with the integer specification in tests/helpers.py (exact_resample: plain Python ints on the oracle's
fixed-point weights); positions exactly ON a CDF edge, the native Philox draws, degenerate weight vectors, NAIVE through
the sharded systematic machinery and the fused step with each scheme included.  RESIDUAL -- a literal fp64 restatement
of the reference -- is compared with the oracle's fp64 residual_ref on weights normalised by numpy: at most 2 differing
indices per case (the project's bound for fp64 references; the kernel's exp is the device library's, the
reference's numpy's), the observed count printed."""
import os
import re

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -4
SEED = 0x1234567890abcdef


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def eng():
    from smarc_navigation_amd import engine
    return engine


def _header_define(name):
    """an integer #define of csrc/mcl_kernels.h / mcl_resample.h (products of earlier ones resolved)"""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'smarc_navigation_amd', 'csrc')
    text = open(os.path.join(root, 'mcl_kernels.h')).read() + open(os.path.join(root, 'mcl_resample.h')).read()
    m = re.search(r'#define\s+%s\s+\(?([A-Za-z0-9_ *]+?)\)?\s*(//.*)?$' % name, text, re.M)
    val = 1
    for tok in m.group(1).split('*'):
        tok = tok.strip()
        val *= int(tok) if tok.isdigit() else _header_define(tok)
    return val


SCAN_TILE = _header_define('MCL_SCAN_TILE')
RS_TILE = _header_define('RS_TILE')
# one wave either side of 64, both sides of the scan tile and of the expansion tile, two tiles, many tiles
SIZES = sorted({1, 2, 7, 63, 64, 65, 2047, 2048, 2049, 4097, 65536 + 3, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1,
                2 * SCAN_TILE - 1, 2 * SCAN_TILE, 2 * SCAN_TILE + 1, RS_TILE - 1, RS_TILE, RS_TILE + 1})
CDF = ('naive', 'stratified', 'multinomial')


def scheme_id(eng, name):
    return getattr(eng, name.upper())


def uniforms_for(name, n, rs):
    return rs.random_sample(1 if name in ('systematic', 'naive') else n)


def expected_state(orc, soa, idx):
    """keep/lost/dupes of auv_pf.py:183-198 for an ancestor vector, zero noise"""
    lost, dupes = orc.lost_dupes(idx)
    ref = soa.copy()
    orc.reassign(ref, lost, dupes)
    return ref


def numpy_weights(lw, mode):
    """the weights as the reference node holds them before it resamples (auv_pf.py:165,172), numpy arithmetic"""
    w = np.exp(lw) + 1e-200 if mode == 0 else np.exp(lw - lw.max())
    return w / w.sum()


def residual_reference(orc, lw, mode, u):
    """(indices, k) of the oracle's fp64 residual_resample on numpy's weights; u: at least n - k uniforms"""
    w = numpy_weights(lw, mode)
    k = orc.residual_k(w)
    idx, k2 = orc.residual_ref(w, np.asarray(u[:w.size - k], dtype=np.float64))
    assert k == k2
    return idx, k


def ragged_log_weights(n, mode, rs):
    """the weights of test_fixed_point_resample_bit_exact_vs_oracle: both modes, a tenth of the particles at -1e4"""
    lw = -0.5 * (rs.randn(n) * 3.0) ** 2 + (2.0 if mode == 0 else -300.0)
    if n > 10:
        lw[rs.randint(0, n, size=n // 10)] = -1e4
    return lw


def replay_resample(eng, name, soa, lw, mode, u):
    """one REPLAY resample with zero noise through a handle of scheme `name`: (indices, state)"""
    n = lw.size
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY, resample_scheme=scheme_id(eng, name))
    e.set_particles(soa)
    e.set_log_weights(lw, mode)
    e.resample(u, np.zeros((n, 6)))
    out = e.last_indices(), e.get_particles()
    e.close()
    return out


# ------------------------------------------------------------------ a. sizes
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('name', CDF)
def test_indices_and_state_equal_the_integer_reference(name, n, eng, orc):
    for mode in (0, 1):
        rs = np.random.RandomState(n * 2 + mode)
        lw = ragged_log_weights(n, mode, rs)
        soa = rs.randn(6, n)
        u = uniforms_for(name, n, rs)
        idx, state = replay_resample(eng, name, soa, lw, mode, u)
        q, _, _ = orc.fixed_weights(lw, mode)
        ref = helpers.exact_resample(q, helpers.u53_of(u), name)
        assert np.array_equal(idx, ref), (name, n, mode, int(np.count_nonzero(idx != ref)))
        assert np.array_equal(state, expected_state(orc, soa, ref)), (name, n, mode)


@pytest.mark.parametrize('n', SIZES)
def test_residual_indices_and_state_at_ragged_sizes(n, eng, orc):
    """RESIDUAL at the same sizes (single-lane kernels: up to 65 539 particles): the state is exactly the reference's
    reassign of the handle's own indices; the indices are the oracle's on numpy's weights (<= 2 differ)"""
    for mode in (0, 1):
        rs = np.random.RandomState(n * 2 + mode)
        lw = ragged_log_weights(n, mode, rs)
        soa = rs.randn(6, n)
        e = eng.Engine(n, rng_mode=eng.RNG_REPLAY, resample_scheme=eng.RESIDUAL)
        e.set_particles(soa)
        e.set_log_weights(lw, mode)
        need = e.resample_prepare()
        u = rs.random_sample(n)
        e.resample(u[:need], np.zeros((n, 6)))
        idx = e.last_indices()
        assert idx.min() >= 0 and idx.max() < n
        assert np.array_equal(e.get_particles(), expected_state(orc, soa, idx)), (n, mode)
        ref, k = residual_reference(orc, lw, mode, u)
        miss = int(np.count_nonzero(idx != ref))
        print('residual n = %d mode %d: k = %d, %d indices differ from the fp64 reference' % (n, mode, k, miss))
        assert need == n - k and miss <= 2, (n, mode, need, n - k, miss)
        e.close()


@pytest.mark.parametrize('name', ['stratified', 'multinomial'])
def test_products_beyond_128_bits_at_a_million_particles(name, eng, orc):
    """n = 2^20 + 3, near-uniform weights: T ~ 2^61, (U + i 2^53) T passes 2^128 -- the carry into the third word of the
    192-bit comparison decides"""
    n = (1 << 20) + 3
    rs = np.random.RandomState(20)
    lw = rs.uniform(-1e-3, 0.0, n)
    soa = rs.randn(6, n)
    u = rs.random_sample(n)
    idx, state = replay_resample(eng, name, soa, lw, eng.WEIGHT_LOG_SHIFT, u)
    q, tot, _ = orc.fixed_weights(lw, 1)
    assert tot > 1 << 60 and (n << 53) * tot > 1 << 128
    ref = helpers.exact_resample(q, helpers.u53_of(u), name)
    assert np.array_equal(idx, ref), int(np.count_nonzero(idx != ref))
    assert np.array_equal(state, expected_state(orc, soa, ref))


# ------------------------------------------------------------------ b. positions exactly on a CDF edge
def tie_literal(name, n):
    return np.arange(n) if name in ('systematic', 'stratified') else np.concatenate([[0], np.arange(n - 1)])


@pytest.mark.parametrize('n', [64, RS_TILE, 2 * RS_TILE])
@pytest.mark.parametrize('name', ['systematic', 'naive', 'stratified', 'multinomial'])
def test_equal_weights_put_every_position_on_an_edge(name, n, eng, orc):
    """equal log-weights, u = 0 (multinomial: u_i = m_i / n, m a permutation): every position sits on an edge.  `<`
    steps over it (arange), `<=` / `>=` stay (naive: [0, 0, 1, .., n - 2]; multinomial: max(m_i - 1, 0))."""
    rs = np.random.RandomState(n)
    lw = np.full(n, -3.25)
    soa = rs.randn(6, n)
    if name == 'multinomial':
        m = rs.permutation(n)
        u = m / float(n)   # (n is a power of two: exact)
        literal = np.maximum(m - 1, 0)
    else:
        u = np.zeros(1 if name != 'stratified' else n)
        literal = tie_literal(name, n)
    q, _, _ = orc.fixed_weights(lw, 1)
    U = helpers.u53_of(u)
    assert helpers.exact_ties(q, U, name) >= n - 1
    ref = helpers.exact_resample(q, U, name)
    assert np.array_equal(ref, literal)
    idx, state = replay_resample(eng, name, soa, lw, eng.WEIGHT_LOG_SHIFT, u)
    assert np.array_equal(idx, ref), (name, n, int(np.count_nonzero(idx != ref)))
    # (naive: particle n - 1 has no offspring -- its slot takes the second copy of particle 0)
    assert np.array_equal(state, expected_state(orc, soa, ref)), (name, n)


def dyadic_weights(n, total_log2, rs):
    """n weights 2^k, k in 0 .. 10, that add up to 2^total_log2 exactly, shuffled: every fixed-point weight and every
    prefix sum is exact, and positions that are multiples of 2^-12 meet CDF edges"""
    head = [1 << int(k) for k in rs.randint(0, 11, size=(n * 3) // 4)]
    rest = (1 << total_log2) - sum(head)
    tail = [1024] * (rest // 1024) + [1 << b for b in range(10) if (rest % 1024) >> b & 1]
    assert rest > 0 and len(head) + len(tail) <= n
    while len(head) + len(tail) < n:   # split the largest piece in two until the count fits
        tail.sort()
        v = tail.pop()
        assert v > 1
        tail += [v // 2, v // 2]
    w = np.array(head + tail, dtype=np.float64)
    rs.shuffle(w)
    assert w.size == n and int(w.sum()) == 1 << total_log2
    return w


@pytest.mark.parametrize('name', ['systematic', 'naive', 'stratified', 'multinomial'])
def test_dyadic_weights_with_dyadic_uniforms_through_the_free_function(name, eng, orc):
    n = 4096
    rs = np.random.RandomState(77)
    w = dyadic_weights(n, 20, rs)
    if name == 'multinomial':
        # half of the draws on an edge C_j / T itself (T = 2^20: exact), half on multiples of 2^-12
        edges = np.cumsum(w)[rs.randint(0, n - 1, size=n)] / float(1 << 20)
        u = np.where(rs.rand(n) < 0.5, edges, rs.randint(0, 4096, size=n) / 4096.0)
    else:
        # (u + i) / n = C_j / T  <=>  16 C_j = 4096 (u + i): u a multiple of 16 / 4096
        u = rs.randint(0, 256, size=1 if name != 'stratified' else n) / 256.0
    q, _, _ = orc.fixed_weights(w, 2)
    assert np.array_equal(q, (w * float(1 << 41)).astype(np.uint64))   # 2^(s - 10), s = 63 - 12
    U = helpers.u53_of(u)
    ties = helpers.exact_ties(q, U, name)
    print('%s: %d of %d positions on a CDF edge' % (name, ties, n))
    assert ties >= 8
    ref = helpers.exact_resample(q, U, name)
    idx = eng.resample_indices(w, u, scheme=scheme_id(eng, name))
    assert np.array_equal(idx, ref), (name, int(np.count_nonzero(idx != ref)))


# ------------------------------------------------------------------ c. native draws
@pytest.mark.parametrize('n', [65, 5000, 65536 + 3])
@pytest.mark.parametrize('name', ['systematic', 'naive', 'stratified', 'multinomial', 'residual'])
def test_native_draws_equal_the_philox_restatement(name, n, eng, orc):
    """three consecutive NATIVE resamples: call k draws at step k -- explicit-index schemes U_i of counter i, purpose 4
    (k_make_u53); systematic / naive the one uniform of oracle.native_u53"""
    rs = np.random.RandomState(n + 1)
    e = eng.Engine(n, seed=SEED, resample_scheme=scheme_id(eng, name))
    soa = rs.randn(6, n)
    e.set_particles(soa)
    draws = []
    for step in range(3):
        lw = ragged_log_weights(n, 1, rs)
        e.set_log_weights(lw, eng.WEIGHT_LOG_SHIFT)
        e.resample()
        idx = e.last_indices()
        U = [orc.native_u53(SEED, step)] if name in ('systematic', 'naive') else helpers.native_draws_u53(SEED, step, n)
        draws.append(U[:64])
        if name == 'residual':
            ref, k = residual_reference(orc, lw, 1, np.array(U, dtype=np.float64) * 2.0 ** -53)
            miss = int(np.count_nonzero(idx != ref))
            print('residual native n = %d step %d: k = %d, %d indices differ from the fp64 reference' % (n, step, k, miss))
            assert miss <= 2, (n, step, miss)
        else:
            q, _, _ = orc.fixed_weights(lw, 1)
            ref = helpers.exact_resample(q, U, name)
            assert np.array_equal(idx, ref), (name, n, step, int(np.count_nonzero(idx != ref)))
        soa = expected_state(orc, soa, idx)
        assert np.array_equal(e.get_particles(), soa), (name, n, step)   # (resample_cov = 0: copies only)
    assert draws[0] != draws[1] and draws[1] != draws[2] and draws[0] != draws[2]
    e.close()


# ------------------------------------------------------------------ d. degenerate weights
def degenerate_log_weights(case, n, rs):
    if case == 'all_minus_inf':
        return np.full(n, -np.inf)
    if case == 'one_survivor':
        lw = np.full(n, -1e6)
        lw[1234] = -2.5
        return lw
    if case == 'nan_every_third':
        lw = -0.5 * rs.randn(n) ** 2
        lw[::3] = np.nan
        return lw
    if case == 'spread_1400':
        return rs.permutation(np.linspace(-1400.0, 0.0, n))
    if case == 'all_nan':
        return np.full(n, np.nan)
    raise ValueError(case)


@pytest.mark.parametrize('case', ['all_minus_inf', 'one_survivor', 'nan_every_third', 'spread_1400', 'all_nan'])
@pytest.mark.parametrize('name', ['systematic', 'naive', 'stratified', 'multinomial'])
def test_degenerate_weight_vectors(name, case, eng, orc):
    """whatever the oracle's quantiser makes of the vector is what the scheme resamples: no finite log-weight at all
    (all -inf, all NaN) is a uniform cloud, a NaN among finite log-weights is a particle without weight"""
    n = 4099
    for mode in (0, 1):
        rs = np.random.RandomState(len(case) + mode)
        lw = degenerate_log_weights(case, n, rs)
        soa = rs.randn(6, n)
        u = uniforms_for(name, n, rs)
        q, tot, _ = orc.fixed_weights(lw, mode)
        assert tot > 0
        if case in ('all_minus_inf', 'all_nan'):
            assert np.all(q == q[0]) and q[0] > 0
        if case == 'nan_every_third':
            assert np.all(q[::3] == 0)
        ref = helpers.exact_resample(q, helpers.u53_of(u), name)
        idx, state = replay_resample(eng, name, soa, lw, mode, u)
        assert np.array_equal(idx, ref), (name, case, mode, int(np.count_nonzero(idx != ref)))
        assert np.array_equal(state, expected_state(orc, soa, ref)), (name, case, mode)
        if case == 'one_survivor':
            assert np.all(ref == 1234) and np.array_equal(state, np.repeat(soa[:, 1234:1235], n, axis=1))


# ------------------------------------------------------------------ e. NAIVE through the sharded systematic machinery
def set_exchange(monkeypatch, exchange):
    if exchange == 'allgather':
        monkeypatch.setenv('MCL_EXCHANGE', 'allgather')
    else:
        monkeypatch.delenv('MCL_EXCHANGE', raising=False)


@pytest.mark.parametrize('exchange', ['p2p', 'allgather'])
def test_naive_sharded_equals_unsharded_bitwise(exchange, eng, orc, monkeypatch):
    set_exchange(monkeypatch, exchange)
    shards, nl = 4, 8192
    n = shards * nl
    cov = dict(init_cov=[2, 2, 0, 0, 0, 0.05], process_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5],
               resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4], meas_std=2.0, seed=99, resample_scheme=eng.NAIVE)
    one = eng.Engine(n, **cov)
    many = [eng.Engine(nl, rank=r, world=shards, n_global=n, global_offset=r * nl, **cov) for r in range(shards)]
    for e in [one] + many:
        e.init_particles()
    q4 = orc.quat_from_euler(0.01, 0.02, 0.3)
    for step in range(3):
        for e in [one] + many:
            e.predict([1.0, 0.05, 0.0], 0.02, q4, -2.0, 0.02)
            e.update_gps(0.1 * step, -0.05 * step)
        lw = one.get_log_weights()
        one.resample()
        eng.group_resample(many)
        assert np.array_equal(one.get_particles(), np.concatenate([e.get_particles() for e in many], axis=1)), step
        idx = one.last_indices()
        assert np.array_equal(idx, np.concatenate([e.last_indices() for e in many])), step
        assert np.array_equal(one.last_offspring_cdf(), many[0].last_offspring_cdf())
        assert np.array_equal(one.last_offspring_cdf(), many[-1].last_offspring_cdf())
        # and they are the naive scheme's indices at the handle's own draw
        qf, _, _ = orc.fixed_weights(lw, 0)
        assert np.array_equal(idx, helpers.exact_resample(qf, [orc.native_u53(99, step)], 'naive')), step


@pytest.mark.parametrize('exchange', ['p2p', 'allgather'])
def test_naive_tie_crosses_the_shards(exchange, eng, orc, monkeypatch):
    """equal weights, u = 0 over 4 shards: [0, 0, 1, .., n - 2] -- the cloud's last particle has no offspring, its slot
    (the last of the last shard) takes the second copy of shard 0's particle 0: exactly one particle crosses"""
    set_exchange(monkeypatch, exchange)
    shards, nl = 4, 8192
    n = shards * nl
    rs = np.random.RandomState(8)
    soa = rs.randn(6, n)
    lw = np.full(n, -1.5)
    one = eng.Engine(n, rng_mode=eng.RNG_REPLAY, resample_scheme=eng.NAIVE)
    many = [eng.Engine(nl, rank=r, world=shards, n_global=n, global_offset=r * nl, rng_mode=eng.RNG_REPLAY,
                       resample_scheme=eng.NAIVE) for r in range(shards)]
    one.set_particles(soa)
    one.set_log_weights(lw, eng.WEIGHT_LOG_SHIFT)
    one.resample([0.0], np.zeros((n, 6)))
    for r, e in enumerate(many):
        e.set_particles(np.ascontiguousarray(soa[:, r * nl:(r + 1) * nl]))
        e.set_log_weights(lw[r * nl:(r + 1) * nl], eng.WEIGHT_LOG_SHIFT)
    eng.group_resample(many, [0.0], [np.zeros((nl, 6))] * shards)
    literal = np.concatenate([[0], np.arange(n - 1)])
    want = soa.copy()
    want[:, n - 1] = soa[:, 0]
    for idx, state in ((one.last_indices(), one.get_particles()),
                       (np.concatenate([e.last_indices() for e in many]),
                        np.concatenate([e.get_particles() for e in many], axis=1))):
        assert np.array_equal(idx, literal)
        assert np.array_equal(state, want)
    if exchange == 'p2p':
        sent = [e.exchange_stats()[0] for e in many]
        lost = [e.exchange_stats()[1] for e in many]
        assert sent == [1, 0, 0, 0] and lost == [0, 0, 0, 1], (sent, lost)


def test_explicit_index_schemes_refuse_to_shard(eng, orc):
    from smarc_navigation_amd import synth
    shards, nl, B = 2, 4096, 16
    origin = (-64.0, -64.0)
    z = synth.bathymetry_grid(128, 128, 1.0, origin, seed=3)
    ba = synth.beam_angles(B)
    rs = np.random.RandomState(2)
    many = [eng.Engine(nl, rank=r, world=shards, n_global=shards * nl, global_offset=r * nl, seed=5,
                       resample_scheme=eng.STRATIFIED) for r in range(shards)]
    before = []
    for e in many:
        e.set_map_grid(z, origin, 1.0)
        soa = rs.randn(6, nl)
        e.set_particles(soa)
        e.set_log_weights(-0.5 * rs.randn(nl) ** 2, eng.WEIGHT_LOG_SHIFT)
        before.append(soa)
    with pytest.raises(eng.MclError) as ei:
        eng.group_resample(many)
    assert ei.value.status == ERR_UNSUPPORTED, ei.value
    with pytest.raises(eng.MclError) as ei:
        eng.group_step_mbes(many, [1.0, 0.0, 0.0], 0.02, orc.quat_from_euler(0.0, 0.0, 0.1), -2.0, 0.02,
                            np.full(B, 21.0, np.float32), ba, 0.5, 80.0)
    assert ei.value.status == ERR_UNSUPPORTED, ei.value
    for e, soa in zip(many, before):
        assert np.array_equal(e.get_particles(), soa)


# ------------------------------------------------------------------ f. the fused step with each scheme
@pytest.mark.parametrize('name', ['naive', 'stratified', 'multinomial', 'residual'])
def test_fused_step_equals_separate_calls_with_each_scheme(name, eng, orc):
    """mcl_step_mbes against predict + update_mbes + resample + mean_cov on a twin handle; between steps 2 and 3 one
    separate update + resample on both: nothing of an explicit-index resample inside a fused step may go stale"""
    from smarc_navigation_amd import synth
    n, B = 8192 + 77, 64
    origin = (-64.0, -64.0)
    z = synth.bathymetry_grid(128, 128, 1.0, origin, seed=3)
    ba = synth.beam_angles(B)
    cov = dict(init_cov=[1, 1, 0, 0, 0, 0.01], process_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5],
               resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4], seed=31, resample_scheme=scheme_id(eng, name))
    m2o = synth.rigid_matrix(0.5, -1.0, 0.0, 0.0, 0.0, 0.1)
    off = [0.2, 0.0, -0.1, 0.0, 0.01, 0.02]
    stream = synth.odom_stream(5)
    one = eng.Engine(1, rng_mode=eng.RNG_REPLAY, m2o=m2o)
    one.set_map_grid(z, origin, 1.0)
    a, b = eng.Engine(n, m2o=m2o, **cov), eng.Engine(n, m2o=m2o, **cov)
    for e in (a, b):
        e.set_map_grid(z, origin, 1.0)
        e.init_particles()
    for k in range(4):
        one.set_particles(stream['truth'][k][:, None].copy())
        ranges = one.mbes_expected(0, 1, ba, 80.0, off)[0]
        a.step_mbes(stream['v'][k], stream['wz'][k], stream['q'][k], stream['z'][k], stream['dt'], ranges, ba, 0.3, 80.0, off)
        ma = a.last_mean_cov()
        b.predict(stream['v'][k], stream['wz'][k], stream['q'][k], stream['z'][k], stream['dt'])
        b.update_mbes(ranges, ba, 0.3, 80.0, off)
        b.resample()
        mb = b.mean_cov()
        assert np.array_equal(a.get_particles(), b.get_particles()), (name, k)
        assert np.array_equal(a.last_indices(), b.last_indices()), (name, k)
        np.testing.assert_allclose(ma[0], mb[0], rtol=0, atol=1e-12)
        assert abs(ma[1] - mb[1]) <= 1e-12
        np.testing.assert_allclose(ma[2], mb[2], rtol=1e-9, atol=1e-15)
        m6, yaw, c9 = orc.mean_cov(a.get_particles())
        np.testing.assert_allclose(ma[0], m6, rtol=0, atol=1e-10)
        np.testing.assert_allclose(ma[2], c9, rtol=1e-8, atol=1e-15)
        if k == 1:
            for e in (a, b):
                e.update_mbes(ranges, ba, 0.3, 80.0, off)
                e.resample()
            assert np.array_equal(a.get_particles(), b.get_particles()), name
            assert np.array_equal(a.last_indices(), b.last_indices()), name


# ------------------------------------------------------------------ g. residual renormalisation above one numpy chunk
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n', [8193, 16389, 65536])
def test_residual_renormalises_like_numpy_above_one_chunk(n, mode, eng, orc):
    """through a handle, so that the 8192-element chunked pairwise sum runs (k_np_chunk_sums / k_np_sum_final)"""
    rs = np.random.RandomState(n + mode)
    lw = -0.5 * (rs.randn(n) * 2.0) ** 2 - (250.0 if mode else 0.0)
    soa = rs.randn(6, n)
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY, resample_scheme=eng.RESIDUAL)
    e.set_particles(soa)
    e.set_log_weights(lw, mode)
    need = e.resample_prepare()
    u = rs.random_sample(n)
    ref, k = residual_reference(orc, lw, mode, u)
    e.resample(u[:need], np.zeros((n, 6)))
    idx = e.last_indices()
    miss = int(np.count_nonzero(idx != ref))
    print('residual n = %d mode %d: k = %d (handle: %d), %d indices differ from the fp64 reference' % (n, mode, k, n - need, miss))
    assert need == n - k, (need, n - k)
    assert miss <= 2, miss
    assert np.array_equal(e.get_particles(), expected_state(orc, soa, idx))
    e.close()


@pytest.mark.parametrize('mode', [0, 1])
def test_residual_sum_rounds_where_the_8192_chunks_put_it(mode, eng, orc):
    """A weight vector on which the ORDER of numpy's sum decides how many copies residual resampling hands out, by a
    margin no last bit of an exp can move.  n = 2^14: 1024 particles of weight exactly 1 (lw = 0) in the first 8192-element
    chunk, whose other weights are 0 (+ 1e-200); every particle of the second chunk weighs 0.3 x 2^-54, 0.3 ulp(1024)
    per 4096 of them.  numpy adds chunk sums: 1024 + 0.6 ulp rounds UP, S = 1024 + 2^-42, n w = 16 (1 - 2^-52), 15
    copies each, k = 15 360.  Any summation that meets the two halves of the second chunk one after the other
    (4096-element chunks, a sequential sum) leaves S = 1024: 16 copies each, k = n."""
    n = 1 << 14
    rs = np.random.RandomState(14 + mode)
    lw = np.full(n, -np.inf)
    lw[rs.choice(8192, 1024, replace=False)] = 0.0
    lw[8192:] = np.log(0.3) - 54.0 * np.log(2.0)
    w = np.exp(lw) + 1e-200 if mode == 0 else np.exp(lw - lw.max())
    assert float(w.sum()) == 1024.0 + 2.0 ** -42 and float(w[:8192].sum()) == 1024.0
    assert abs(float(w[8192:12288].sum()) / (0.3 * 2.0 ** -42) - 1.0) < 1e-9
    soa = rs.randn(6, n)
    e = eng.Engine(n, rng_mode=eng.RNG_REPLAY, resample_scheme=eng.RESIDUAL)
    e.set_particles(soa)
    e.set_log_weights(lw, mode)
    need = e.resample_prepare()
    u = rs.random_sample(n)
    ref, k = residual_reference(orc, lw, mode, u)
    assert k == 15 * 1024
    assert need == n - k, (need, n - k)
    e.resample(u[:need], np.zeros((n, 6)))
    idx = e.last_indices()
    miss = int(np.count_nonzero(idx != ref))
    print('residual, order-sensitive sum, mode %d: k = %d, %d indices differ from the fp64 reference' % (mode, k, miss))
    assert miss <= 2, miss
    assert np.array_equal(e.get_particles(), expected_state(orc, soa, idx))
    e.close()


# ------------------------------------------------------------------ the free functions and unnormalised weights
def test_free_functions_with_weights_that_are_not_normalised(eng):
    """include/mcl.h, mcl_resample_indices: the four CDF schemes divide by the total themselves -- weights scaled by
    exactly 4 give the same indices; residual takes the weights as they are (they must sum to 1, like resampling.py's),
    but whatever it is given it returns n indices in [0, n)"""
    n = 5003
    rs = np.random.RandomState(6)
    w = rs.rand(n) ** 3
    w /= w.sum()
    u = rs.random_sample(n)
    for name in ('systematic', 'naive', 'stratified', 'multinomial'):
        a = eng.resample_indices(w, u, scheme=scheme_id(eng, name))
        b = eng.resample_indices(4.0 * w, u, scheme=scheme_id(eng, name))
        assert np.array_equal(a, b), name
    for scale in (1.0, 4.0, 0.25):
        idx = eng.resample_indices(scale * w, u, scheme=eng.RESIDUAL)
        assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < n, scale
