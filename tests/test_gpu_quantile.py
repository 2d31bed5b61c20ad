"""GPU tests of the exact order statistics (include/mcl_quantile.h; kernels csrc/mcl_quantile.h): value, key, M(K), S and
n_used of every query against the restatement of tests/test_quantile_host.py (numpy keys, Python-integer masses over the
oracle's det_exp, the 128-bit rule in unbounded integers) -- BITS, not tolerances --, the inverse question, shards against
the unsharded cloud, the untouched handle, the error codes and Engine.credible."""
import math

import numpy as np
import pytest

from tests.test_quantile_host import (Q_ABS_YAW_DEV, Q_RADIUS2, Q_X, Q_Y, Q_YAW_DEV, Selection, key_ref, masses_ref,
                                      quantity_ref, reached_ref, threshold_ref, value_ref)

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
SIZES = (1, 2, 63, 64, 65, 257, 4099)     # one lane, a wave edge, more than one workgroup, not a multiple of anything
CENTRE = (512.3, -87.1, 3.1)              # cyaw near pi
TINY = 2.0 ** -32


def probs_for(n):
    return [TINY, 1.0 / n, 0.5, 0.95, 1.0 - TINY, 1.0]


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


# ------------------------------------------------------------------ the clouds: (6, n) states and the quantities asked of each
def _base(n, seed):
    rs = np.random.RandomState(seed)
    soa = np.zeros((6, n))
    soa[0] = 512.3 + 0.05 * rs.randn(n)
    soa[1] = -87.1 + 0.05 * rs.randn(n)
    soa[5] = rs.uniform(-math.pi, math.pi, n)
    return soa, rs


def cloud(name, n):
    soa, rs = _base(n, 1000 + n)
    what = (Q_X,)
    if name == 'all_equal':
        soa[0] = 512.3
    elif name == 'one_to_rest':                       # two values split 1 : n - 1
        soa[0] = 7.25
        soa[0, rs.randint(n)] = -3.5
    elif name == 'lowest_bit':                        # values that differ only in the lowest key bit
        soa[0] = np.where(rs.rand(n) < 0.5, 512.3, np.nextafter(512.3, 1e9))
    elif name == 'sign_only':
        soa[0] = np.where(rs.rand(n) < 0.5, 512.3, -512.3)
    elif name == 'zeros':                             # a mix of -0 and +0
        soa[0] = np.where(rs.rand(n) < 0.5, 0.0, -0.0)
    elif name == 'denormals':                         # denormals beside 1e300
        soa[0] = rs.choice([5e-324, -5e-324, 1e-310, -1e-310, 1e300, -1e300, 2.2250738585072014e-308], n)
    elif name == 'nonfinite':                         # some NaN and +-inf coordinates
        k = rs.randint(0, 6, n)
        soa[0] = np.where(k == 0, np.nan, np.where(k == 1, np.inf, np.where(k == 2, -np.inf, soa[0])))
        soa[1] = np.where(rs.randint(0, 5, n) == 0, np.nan, soa[1])
        what = (Q_X, Q_Y, Q_RADIUS2)
    elif name == 'gaussian':                          # 5 cm wide at (512.3, -87.1)
        what = (Q_X, Q_Y, Q_RADIUS2)
    elif name == 'yaw_seam':                          # yaws on both sides of +-pi, cyaw near pi
        soa[5] = np.where(rs.rand(n) < 0.5, math.pi - 0.2 * rs.rand(n), -math.pi + 0.2 * rs.rand(n))
        soa[5, 0] = math.pi
        if n > 1:
            soa[5, 1] = -math.pi
        what = (Q_YAW_DEV, Q_ABS_YAW_DEV)
    else:
        raise KeyError(name)
    return soa, what


CLOUDS = ('all_equal', 'one_to_rest', 'lowest_bit', 'sign_only', 'zeros', 'denormals', 'nonfinite', 'gaussian', 'yaw_seam')


def lw_case(name, n, seed=5):
    rs = np.random.RandomState(seed + n)
    if name == 'spread600':                           # log-weights that spread over 600 nats (some masses are 0)
        lw = -600.0 * rs.rand(n) - 37.5
        lw[rs.randint(n)] = -37.5
        lw[rs.randint(0, 7, n) == 0] -= 200.0
    elif name == 'one_finite':
        lw = np.where(rs.rand(n) < 0.5, -np.inf, np.nan)
        lw[rs.randint(n)] = -12.25
    elif name == 'none_finite':
        lw = rs.choice([np.inf, -np.inf, np.nan], n)
    elif name == 'mixed':
        lw = -8.0 * rs.rand(n)
        k = rs.randint(0, 12, n)
        lw[k == 0], lw[k == 1], lw[k == 2] = np.inf, -np.inf, np.nan
    else:
        raise KeyError(name)
    return lw


def same(got, want_value, want_key, want_mass, total, n_used, tag):
    print(tag, 'got', got, 'want', (want_value, want_key, want_mass, total, n_used))
    assert got.total == total and got.n_used == n_used, tag
    if total == 0:
        assert math.isnan(got.value) and got.mass == 0, tag
        return
    assert bits([got.value])[0] == bits([want_value])[0] and got.key == want_key and got.mass == want_mass, tag


def check_query(eng, e, soa, quantity, centre, masses, tag, max_lw=None):
    """one call at the six probabilities against the restatement; then the inverse question at the answers"""
    n = soa.shape[1]
    sel = Selection(quantity_ref(soa, quantity, centre), masses)
    probs = probs_for(n)
    got = e.cloud_quantiles(quantity, probs, centre, weighted=masses is not None)
    assert len(got) == len(probs)
    for p, g in zip(probs, got):
        v, k, m = sel.quantile(p)
        same(g, v, k, m, sel.total, sel.n_used, '%s q%d p=%r' % (tag, quantity, p))
    if sel.total == 0:
        return got
    # cloud_mass at the returned value gives back M(K); one key below it stays below the threshold
    at = e.cloud_mass(quantity, [g.value for g in got], centre, weighted=masses is not None, max_lw=max_lw)
    assert at['mass'] == [g.mass for g in got] and at['total'] == sel.total and at['n_used'] == sel.n_used, tag
    # (the key -0 would have had is no value's key: below key(0) comes the key of the largest negative denormal)
    kbelow = [g.key - 2 if g.key == key_ref(0.0) else g.key - 1 for g in got]
    lower = [value_ref(k) for k in kbelow]
    keep = [i for i, v in enumerate(lower) if not math.isnan(v)]        # (below key(-inf) there is no value)
    under = e.cloud_mass(quantity, [lower[i] for i in keep], centre, weighted=masses is not None, max_lw=max_lw) if keep \
        else dict(mass=[])
    for i, m in zip(keep, under['mass']):
        assert key_ref(lower[i]) == kbelow[i]
        assert m == sel.mass_at(kbelow[i]) and not reached_ref(m, sel.total, threshold_ref(probs[i])), (tag, probs[i])
    return got


# ------------------------------------------------------------------ unweighted
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('name', CLOUDS)
def test_unweighted_quantiles_equal_the_restatement_bit_for_bit(eng, name, n):
    soa, what = cloud(name, n)
    e = eng.Engine(n)
    e.set_particles(soa)
    for quantity in what:
        a = check_query(eng, e, soa, quantity, CENTRE, None, '%s n=%d' % (name, n))
        b = e.cloud_quantiles(quantity, probs_for(n), CENTRE)                      # two identical calls agree
        assert [(bits([x.value])[0], x.key, x.mass, x.total, x.n_used) for x in a] == \
               [(bits([x.value])[0], x.key, x.mass, x.total, x.n_used) for x in b]
    e.close()


def test_unweighted_median_and_maximum_are_numpys(eng):
    n = 4099
    soa, _ = cloud('gaussian', n)
    e = eng.Engine(n)
    e.set_particles(soa)
    med, mx = e.cloud_quantiles('x', [0.5, 1.0])
    assert med.value == np.sort(soa[0])[(n - 1) // 2] and med.mass == (n + 1) // 2      # the lower median
    assert mx.value == soa[0].max() and mx.mass == mx.total == mx.n_used == n
    e.close()


@pytest.mark.parametrize('name,weights', [('gaussian', None), ('denormals', None), ('nonfinite', 'mixed')])
def test_eight_probabilities_in_one_call_equal_eight_single_calls(eng, name, weights):
    n = 4099
    soa, what = cloud(name, n)
    e = eng.Engine(n)
    e.set_particles(soa)
    if weights:
        e.set_log_weights(lw_case(weights, n))
    probs = [0.95, TINY, 0.5, 1.0, 0.25, 1.0 / n, 0.5, 1.0 - TINY]                     # any order, a repeat
    for quantity in what:
        many = e.cloud_quantiles(quantity, probs, CENTRE, weighted=bool(weights))
        for p, g in zip(probs, many):
            one = e.cloud_quantiles(quantity, [p], CENTRE, weighted=bool(weights))[0]
            assert (bits([one.value])[0], one.key, one.mass, one.total, one.n_used) == \
                   (bits([g.value])[0], g.key, g.mass, g.total, g.n_used), (name, quantity, p)
    e.close()


# ------------------------------------------------------------------ weighted
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('wname', ['spread600', 'one_finite', 'none_finite', 'mixed'])
def test_weighted_quantiles_equal_the_restatement_as_integers(eng, wname, n):
    soa, _ = cloud('nonfinite' if wname == 'mixed' else 'gaussian', n)
    lw = lw_case(wname, n)
    masses, m = masses_ref(lw)
    e = eng.Engine(n)
    e.set_particles(soa)
    e.set_log_weights(lw)
    for quantity in (Q_X, Q_RADIUS2):
        got = check_query(eng, e, soa, quantity, CENTRE, masses, '%s n=%d' % (wname, n), m)
        if wname == 'none_finite':
            assert all(math.isnan(g.value) and g.total == 0 for g in got)            # S = 0: NaN, and MCL_OK
        if wname == 'one_finite':
            assert all(g.total == 1 << 32 for g in got) and len({g.key for g in got}) == 1
    assert np.array_equal(bits(e.get_log_weights()), bits(lw))
    e.close()


def test_weighted_needs_pending_log_weights_that_are_logarithms(eng):
    n = 65
    soa, _ = cloud('gaussian', n)
    e = eng.Engine(n)
    e.set_particles(soa)
    expect_status(eng, ERR_STATE, e.cloud_quantiles, 'x', [0.5], weighted=True)        # no pending weights
    expect_status(eng, ERR_STATE, e.cloud_mass, 'x', [0.0], weighted=True, max_lw=0.0)
    expect_status(eng, ERR_STATE, e.cloud_key_hist, 'x', 0, 0, weighted=True)
    assert e.cloud_quantiles('x', [0.5])[0].n_used == n                                 # unweighted needs none
    e.set_log_weights(np.full(n, 0.5), eng.WEIGHT_LINEAR)
    expect_status(eng, ERR_STATE, e.cloud_quantiles, 'x', [0.5], weighted=True)        # linear weights are no logarithms
    e.set_log_weights(np.zeros(n), eng.WEIGHT_LOG_SHIFT)
    assert e.cloud_quantiles('x', [0.5], weighted=True)[0].total == n << 32
    e.resample()
    expect_status(eng, ERR_STATE, e.cloud_quantiles, 'x', [0.5], weighted=True)        # resampled away
    e.close()


def test_error_codes(eng):
    n = 64
    e = eng.Engine(n)
    expect_status(eng, ERR_STATE, e.cloud_quantiles, 'x', [0.5])                       # no particles yet
    expect_status(eng, ERR_STATE, e.cloud_mass, 'x', [0.0])
    expect_status(eng, ERR_STATE, e.cloud_key_hist, 'x', 0, 0)
    expect_status(eng, ERR_STATE, eng.group_cloud_quantiles, [e], 'x', [0.5])
    e.init_particles()
    for bad in ([], [0.5] * 9, [0.0], [TINY / 2], [1.0 + 2.0 ** -52], [math.nan], [0.5, -1.0]):
        expect_status(eng, ERR_INVALID, e.cloud_quantiles, 'x', bad)
    expect_status(eng, ERR_INVALID, e.cloud_quantiles, 5, [0.5])
    expect_status(eng, ERR_INVALID, e.cloud_quantiles, -1, [0.5])
    expect_status(eng, ERR_INVALID, e.cloud_quantiles, 'radius2', [0.5], (math.nan, 0.0, 0.0))
    expect_status(eng, ERR_INVALID, e.cloud_quantiles, 'yaw_dev', [0.5], (0.0, 0.0, math.inf))
    expect_status(eng, ERR_INVALID, e.cloud_mass, 'x', [math.nan])
    expect_status(eng, ERR_INVALID, e.cloud_mass, 'x', [0.0] * 9)
    expect_status(eng, ERR_INVALID, e.cloud_mass, 'x', [])
    expect_status(eng, ERR_INVALID, e.cloud_key_hist, 'x', 0, 4)
    expect_status(eng, ERR_INVALID, e.cloud_key_hist, 'x', 0, 64)
    expect_status(eng, ERR_INVALID, e.cloud_key_hist, 'x', 256, 8)
    e.set_log_weights(np.zeros(n))
    for bad in (math.nan, math.inf):
        expect_status(eng, ERR_INVALID, e.cloud_mass, 'x', [0.0], weighted=True, max_lw=bad)
        expect_status(eng, ERR_INVALID, e.cloud_key_hist, 'x', 0, 0, weighted=True, max_lw=bad)
    assert e.cloud_mass('x', [math.inf], weighted=True, max_lw=-math.inf)['total'] == 0
    e.close()
    shard = eng.Engine(1024, rank=1, world=2, n_global=2048, global_offset=1024)
    shard.init_particles()
    expect_status(eng, ERR_UNSUPPORTED, shard.cloud_quantiles, 'x', [0.5])            # a shard of a LOCAL group
    assert shard.cloud_mass('x', [math.inf])['mass'] == [1024]                         # the split calls serve it
    shard.close()


def test_where_the_hist_and_mass_launches_stride(eng):
    """one particle more than QUANT_GRID workgroups of 256 cover in one pass (the range launch strides past 2048 x 256 only:
    its loop is the same); the log-weights drawn from 512 distinct values, so that the restatement's det_exp stays cheap"""
    n = 1024 * 256 + 1
    soa, _ = cloud('gaussian', n)
    rs = np.random.RandomState(9)
    pool = -40.0 * rs.rand(512)
    pick = rs.randint(0, 512, n)
    lw = pool[pick]
    qpool, m = masses_ref(pool, float(lw.max()))
    masses = [qpool[i] for i in pick]
    e = eng.Engine(n)
    e.set_particles(soa)
    e.set_log_weights(lw)
    check_query(eng, e, soa, Q_RADIUS2, CENTRE, None, 'stride unweighted')
    check_query(eng, e, soa, Q_X, CENTRE, masses, 'stride weighted', m)
    e.close()


# ------------------------------------------------------------------ the handle is untouched
def test_a_resample_after_the_calls_gives_the_indices_it_gives_without_them(eng):
    n = 4099
    soa, _ = cloud('gaussian', n)
    lw = lw_case('mixed', n)
    lw[~np.isfinite(lw)] = -30.0
    kw = dict(resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4], seed=17)
    a, b = eng.Engine(n, **kw), eng.Engine(n, **kw)
    for e in (a, b):
        e.set_particles(soa)
        e.set_log_weights(lw)
    for weighted in (False, True):
        a.cloud_quantiles('radius2', [0.5, 0.95], CENTRE, weighted)
        a.cloud_quantiles('abs_yaw_dev', [0.95], CENTRE, weighted)
        a.cloud_mass('x', [512.3], None, weighted)
        a.cloud_key_hist('x', 0, 0, None, weighted, 0.0)
        eng.group_cloud_quantiles([a], 'y', [0.5], None, weighted)
    a.credible((0.5, 0.95), CENTRE)
    assert np.array_equal(bits(a.get_particles()), bits(soa)) and np.array_equal(bits(a.get_log_weights()), bits(lw))
    for e in (a, b):
        e.resample()
    assert np.array_equal(a.last_indices(), b.last_indices())
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    a.close()
    b.close()


# ------------------------------------------------------------------ shards
SPLITS = ((1, 4098), (2049, 2050), (5, 1000, 64, 2773, 257))


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('split', SPLITS)
def test_shards_give_the_unsharded_bits_for_any_split(eng, split, weighted):
    n = 4099
    assert sum(split) == n
    soa, _ = cloud('nonfinite', n)
    lw = lw_case('spread600', n)
    whole = eng.Engine(n)
    whole.set_particles(soa)
    whole.set_log_weights(lw)
    parts, at = [], 0
    for k in split:
        e = eng.Engine(k)
        e.set_particles(np.ascontiguousarray(soa[:, at:at + k]))
        e.set_log_weights(lw[at:at + k])
        parts.append(e)
        at += k
    probs = probs_for(n)
    m = float(lw.max())
    for quantity in (Q_X, Q_RADIUS2, Q_ABS_YAW_DEV):
        want = whole.cloud_quantiles(quantity, probs, CENTRE, weighted)
        got = eng.group_cloud_quantiles(parts[::-1], quantity, probs, CENTRE, weighted)      # (any order)
        for p, w, g in zip(probs, want, got):
            assert (bits([w.value])[0], w.key, w.mass, w.total, w.n_used) == \
                   (bits([g.value])[0], g.key, g.mass, g.total, g.n_used), (split, quantity, p)
        # the split calls: the shards' integers simply add
        vals = [w.value for w in want if not math.isnan(w.value)]
        sums = [e.cloud_mass(quantity, vals, CENTRE, weighted, m) for e in parts]
        one = whole.cloud_mass(quantity, vals, CENTRE, weighted, m)
        assert [sum(s['mass'][i] for s in sums) for i in range(len(vals))] == one['mass']
        assert sum(s['total'] for s in sums) == one['total'] and sum(s['n_used'] for s in sums) == one['n_used']
    for e in parts + [whole]:
        e.close()


def test_key_hist_is_the_histogram_of_the_next_eight_key_bits(eng):
    n = 4099
    soa, _ = cloud('nonfinite', n)
    lw = lw_case('mixed', n)
    masses, m = masses_ref(lw)
    e = eng.Engine(n)
    e.set_particles(soa)
    e.set_log_weights(lw)
    v = quantity_ref(soa, Q_X)
    used = ~np.isnan(v)
    keys = [key_ref(x) for x in v[used]]
    for weighted in (False, True):
        q = [masses[i] for i in np.nonzero(used)[0]] if weighted else [1] * len(keys)
        med = e.cloud_quantiles('x', [0.5], None, weighted)[0].key
        for bits_ in (0, 8, 24, 56):
            prefix = med >> (64 - bits_) if bits_ else 0
            want = [0] * 256
            for k, w in zip(keys, q):
                if bits_ == 0 or k >> (64 - bits_) == prefix:
                    want[(k >> (56 - bits_)) & 255] += w
            assert e.cloud_key_hist('x', prefix, bits_, None, weighted, m) == want, (weighted, bits_)
    e.close()


# ------------------------------------------------------------------ the engine's credible region
def test_credible_radius_is_the_root_of_numpys_selected_r2(eng):
    n = 4099
    soa, _ = cloud('gaussian', n)
    e = eng.Engine(n)
    e.set_particles(soa)
    c = e.credible((0.5, 0.95), CENTRE)
    r2 = np.sort(quantity_ref(soa, Q_RADIUS2, CENTRE))
    for p in (0.5, 0.95):
        k = -((-threshold_ref(p) * n) >> 32)                      # the least count that reaches
        assert c.radius[p] == math.sqrt(r2[k - 1]), p
        assert c.yaw_halfwidth[p] == np.sort(quantity_ref(soa, Q_ABS_YAW_DEV, CENTRE))[k - 1], p
    h = (n + 1) // 2
    assert c.median[0] == np.sort(soa[0])[h - 1] and c.median[1] == np.sort(soa[1])[h - 1]
    assert c.median[2] == CENTRE[2] + np.sort(quantity_ref(soa, Q_YAW_DEV, CENTRE))[h - 1]
    assert c.n_used == n and c.centre == CENTRE
    med = e.credible((0.95,), 'median')
    assert med.centre[:2] == (c.median[0], c.median[1]) and med.median[:2] == med.centre[:2]
    assert 0.0 < med.radius[0.95] < 0.3                            # 5 cm wide: R95 is about 12 cm
    mean = e.credible((0.95,), 'mean')
    mu = e.mean_cov()[0]
    assert mean.centre[:2] == (mu[0], mu[1]) and abs(mean.radius[0.95] - med.radius[0.95]) < 0.02
    e.close()
