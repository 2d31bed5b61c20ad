"""The sensor resetting (include/mcl_reseed.h) restated in numpy, for tests/test_reseed_host.py and tests/test_gpu_reseed.py:
the draws (Philox4x32-10 from tests/helpers.py, the word-to-double rule, the library's Box-Muller with its deterministic
log and sincos), the component rule in integers, the apply rule one IEEE operation at a time, and the selection of a
mixture from match results.  No GPU, no library call except where the definition itself names a library function
(mcl_swath_derived, mcl_regularise_factor)."""
import math

import numpy as np

from tests.helpers import philox4x32_10

TWO53 = 9007199254740992.0
PI = math.pi


# ------------------------------------------------------------------ an exact fused multiply-add on float64 arrays
# (numpy has none; det_log and det_sincos2pi of mcl_device.h are sequences of them.)  Boldo and Melquiond, "Emulation of a
# FMA and correctly rounded sums: proved algorithms using rounding to odd" (2008): a b = uh + ul exactly (Dekker / Veltkamp),
# c + uh = th + tl exactly (Knuth), v = the sum tl + ul ROUNDED TO ODD, result = th + v rounded to nearest.  No operand here
# comes near overflow or the subnormals.
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _sum_to_odd(a, b):
    s, e = _two_sum(a, b)
    s = np.array(s, dtype=np.float64, ndmin=1)
    e = np.broadcast_to(np.asarray(e, dtype=np.float64), s.shape)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0.0) & even
    toward = np.where(e > 0.0, np.inf, -np.inf)
    return np.where(fix, np.nextafter(s, toward), s)


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    return th + _sum_to_odd(tl, ul).reshape(th.shape)


def det_log(x):
    """det_log of mcl_device.h (orc_det_log of the oracle), x positive normal doubles"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    bits = x.view(np.uint64)
    e = (bits >> np.uint64(52)).astype(np.int64) - 1023
    m = ((bits & np.uint64(0x000fffffffffffff)) | np.uint64(0x3ff0000000000000)).view(np.float64)
    big = m > 1.41421356237309514547
    m = np.where(big, m * 0.5, m)
    e = e + big
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    p = np.full_like(s, 1.0 / 23.0)
    for d in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = fma(p, s2, 1.0 / d)
    p = fma(p, s2, 1.0)
    lm = 2.0 * s * p
    ed = e.astype(np.float64)
    return fma(ed, 6.93147180369123816490e-01, fma(ed, 1.90821492927058770002e-10, lm))


def det_sincos2pi(u):
    """det_sincos2pi of mcl_device.h: (sin, cos) of 2 pi u, u in [0, 1]"""
    u = np.asarray(u, dtype=np.float64)
    k = np.rint(u * 4.0)
    r = fma(-k, 0.25, u)
    th = r * 6.28318530717958647693
    t2 = th * th
    ps = np.full_like(th, -1.0 / 355687428096000.0)
    for c in (1.0 / 1307674368000.0, -1.0 / 6227020800.0, 1.0 / 39916800.0, -1.0 / 362880.0, 1.0 / 5040.0, -1.0 / 120.0, 1.0 / 6.0):
        ps = fma(ps, t2, c)
    s0 = fma(-(th * t2), ps, th)
    pc = np.full_like(th, 1.0 / 6402373705728000.0)
    for c in (-1.0 / 20922789888000.0, 1.0 / 87178291200.0, -1.0 / 479001600.0, 1.0 / 3628800.0, -1.0 / 40320.0, 1.0 / 720.0,
              -1.0 / 24.0, 0.5):
        pc = fma(pc, t2, c)
    c0 = fma(-t2, pc, 1.0)
    q = k.astype(np.int64) & 3
    sn = np.where(q == 0, s0, np.where(q == 1, c0, np.where(q == 2, -s0, -c0)))
    cs = np.where(q == 0, c0, np.where(q == 1, -s0, np.where(q == 2, -c0, s0)))
    return sn, cs


def box_muller(a, b):
    """box_muller of mcl_device.h on two arrays of 32-bit words: (n0, n1)"""
    u1 = (np.asarray(a, np.uint64).astype(np.float64) + 0.5) * (1.0 / 4294967296.0)
    u2 = (np.asarray(b, np.uint64).astype(np.float64) + 0.5) * (1.0 / 4294967296.0)
    r = np.sqrt(-2.0 * det_log(u1))
    sn, cs = det_sincos2pi(u2)
    return r * cs, r * sn


# ------------------------------------------------------------------ the draws of mcl_inject_gaussian, NATIVE mode
def native_block0(seed, step, gids):
    """(u_select (float64), t (uint64, 53 bits)) of the particles `gids` at injection counter `step`: purpose 9, block 0"""
    a = philox4x32_10(np.asarray(gids, np.uint64), 0, step, 9, seed & 0xffffffff, seed >> 32)
    u_select = (((a[0] >> np.uint64(5)) << np.uint64(26)) | (a[1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53
    t = ((a[2] >> np.uint64(5)) << np.uint64(26)) | (a[3] >> np.uint64(6))
    return u_select, t


def native_block1(seed, step, gids):
    """xi (3, len(gids)): block 1, (xi_0, xi_1) = box_muller(b0, b1), (xi_2, unused) = box_muller(b2, b3)"""
    b = philox4x32_10(np.asarray(gids, np.uint64), 1, step, 9, seed & 0xffffffff, seed >> 32)
    x0, x1 = box_muller(b[0], b[1])
    x2, _ = box_muller(b[2], b[3])
    return np.stack([x0, x1, x2])


def restate_native(state, comps, fraction, seed, step, gid0=0):
    """restate_inject with the NATIVE draws; block 1 only for the selected particles, as the kernel"""
    n = np.asarray(state).shape[1]
    gids = gid0 + np.arange(n, dtype=np.uint64)
    u_select, t = native_block0(seed, step, gids)
    sel = u_select < fraction
    xi = np.zeros((3, n))
    xi[:, sel] = native_block1(seed, step, gids[sel])
    return restate_inject(state, comps, fraction, u_select, t, xi)


# ------------------------------------------------------------------ the component rule
def rank_int(t, W):
    """r = (t W) >> 53 in Python integers"""
    return (int(t) * int(W)) >> 53


def component_int(t, masses):
    """the component a 53-bit draw picks, in Python integers: the first c with cum_c > r"""
    W = sum(int(m) for m in masses)
    r, acc = rank_int(t, W), 0
    for c, m in enumerate(masses):
        acc += int(m)
        if acc > r:
            return c
    raise AssertionError('r >= W')


def components_of(t, masses):
    """component_int for an array of draws (uint64): the 84-bit product in two 64-bit halves, then a bisection over cum"""
    t = np.asarray(t, np.uint64)
    W = np.uint64(sum(int(m) for m in masses))
    lo = (t & np.uint64(0xffffffff)) * W
    hi = (t >> np.uint64(32)) * W + (lo >> np.uint64(32))
    r = hi >> np.uint64(21)
    cum = np.cumsum(np.asarray(masses, np.uint64))
    return np.searchsorted(cum, r, side='right')


# ------------------------------------------------------------------ the apply rule
def wrap_yaw(v):
    """kept when -pi <= v < pi, else ((v + pi) mod 2 pi) - pi with the floored modulo"""
    v = np.asarray(v, np.float64)
    return np.where((v >= -PI) & (v < PI), v, np.mod(v + PI, 2.0 * PI) - PI)


def apply_rule(mean, chol, xi):
    """v_r = mean_r + sum_{c <= r} L_rc xi_c (c increasing, from the first product; a row of zeros: the mean's bits); yaw
    wrapped.  mean (3, n), chol (6, n) packed, xi (3, n) -> (x, y, yaw)"""
    out = []
    for r in range(3):
        base = r * (r + 1) // 2
        z = chol[base] * xi[0]
        some = chol[base] != 0.0
        for c in range(1, r + 1):
            z = z + chol[base + c] * xi[c]
            some = some | (chol[base + c] != 0.0)
        out.append(np.where(some, mean[r] + z, mean[r]))
    out[2] = wrap_yaw(out[2])
    return out


def restate_inject(state, comps, fraction, u_select, t, xi):
    """the state mcl_inject_gaussian leaves, and the number of replaced particles.  comps: records with mean, chol, mass."""
    sel = u_select < fraction
    c = components_of(t[sel], comps['mass'])
    x, y, yaw = apply_rule(comps['mean'][c].T, comps['chol'][c].T, xi[:, sel])
    out = np.array(state, dtype=np.float64, copy=True)
    out[0, sel], out[1, sel], out[5, sel] = x, y, yaw
    return out, int(sel.sum()), sel, c


# ------------------------------------------------------------------ the selection
def select_ref(eng, results, mcfg, sigma, cfg):
    """mcl_reseed_select restated: (components, indices).  mcl_swath_derived and mcl_regularise_factor are the library's
    (the definition names them); everything else is here."""
    cand = []
    for i, r in enumerate(results):
        if int(r['status']) != 0:
            continue
        d = eng.swath_derived(r['final'], mcfg, sigma)
        if int(d['m']) >= cfg.min_beams and float(d['rms']) <= cfg.max_rms:
            cand.append((float(d['rms']), i, d))
    cand.sort(key=lambda c: (c[0], c[1]))
    comps, idx = [], []
    for rms, i, d in cand:
        if len(comps) == cfg.max_components:
            break
        r = results[i]
        near = False
        for k in comps:
            dx, dy = np.float64(r['x']) - k['mean'][0], np.float64(r['y']) - k['mean'][1]
            dist = np.sqrt(dx * dx + dy * dy)
            dyaw = float(wrap_yaw(np.float64(r['yaw']) - k['mean'][2]))
            if dist <= cfg.sep_xy and abs(dyaw) <= cfg.sep_yaw:
                near = True
                break
        if near:
            continue
        cov = np.zeros((3, 3))
        cov[np.tril_indices(3)] = np.float64(cfg.cov_scale) * np.asarray(d['cov'][:6], np.float64)
        for k in range(3):
            if (int(d['dead']) >> k) & 1:
                cov[k, :] = 0.0
                cov[:, k] = 0.0
                s = np.float64(cfg.dead_std_yaw if k == 2 else cfg.dead_std_xy)
                cov[k, k] = s * s
        for k in range(3):
            s = np.float64(cfg.add_std_yaw if k == 2 else cfg.add_std_xy)
            cov[k, k] = cov[k, k] + s * s
        L, _ = eng.regularise_factor(cov)
        rec = np.zeros(1, eng.ReseedComponent)[0]
        rec['mean'] = (r['x'], r['y'], r['yaw'])
        rec['chol'] = L[np.tril_indices(3)]
        rec['mass'] = 1
        comps.append(rec)
        idx.append(i)
    return (np.array(comps, dtype=eng.ReseedComponent) if comps else np.zeros(0, eng.ReseedComponent)), np.array(idx, np.int64)
