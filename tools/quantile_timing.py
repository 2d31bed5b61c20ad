#!/usr/bin/env python3
"""tools/quantile_timing.py -- what the exact order statistics (include/mcl_quantile.h) cost on the GPU, at the bench's
particle count: 1 048 576 particles, no map (none of the launches reads one).

HIP events of the library (mcl_timing_enable / mcl_timing_get: device time of the timed region `mean_cov`), median of --reps
after --warmup warm-up calls, from ONE handle per cloud in one run:
  * mcl_cloud_quantiles: unweighted and weighted, MCL_Q_X and MCL_Q_RADIUS2, 1 and 8 probabilities, on a converged cloud
    (5 cm wide at (512.3, -87.1)), a healthy one (decimetres) and one uniform over a 1 km map -- the converged cloud is the
    atomic-contention case the wave aggregation is there for, and the one whose keys share the most leading bytes;
  * mcl_cloud_mass with 8 values: the one-pass inverse question;
  * mcl_mean_cov and mcl_pose_modes on the same state in the same run: the yardsticks (both are timed under `mean_cov` too).
Every figure also reports `rounds`: the radix rounds that ran (8 minus the leading key bytes the cloud shares).
Appends one JSON line per figure to profiles/quantile_timing.jsonl (and prints it); every number carries its source.
Run it under `timeout` on the GPU box:  timeout -k 10 400 python3 tools/quantile_timing.py"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smarc_navigation_amd import engine  # noqa: E402

CENTRE = (512.3, -87.1, 0.3)
PROBS8 = [0.05, 0.25, 0.5, 0.68, 0.9, 0.95, 0.99, 1.0]
CLOUDS = (('converged', 0.05), ('healthy', 0.3), ('uniform', None))


def make_cloud(name, width, n, rs):
    soa = np.zeros((6, n))
    if width is None:
        soa[0], soa[1] = rs.uniform(0.0, 1000.0, n), rs.uniform(-500.0, 500.0, n)
        soa[5] = rs.uniform(-np.pi, np.pi, n)
    else:
        soa[0], soa[1] = CENTRE[0] + width * rs.randn(n), CENTRE[1] + width * rs.randn(n)
        soa[5] = CENTRE[2] + 0.02 * rs.randn(n)
    # log-weights of a ping of a few beams: -chi^2 / 2 about the centre, a few tens of nats across the cloud
    lw = -0.5 * ((soa[0] - CENTRE[0]) ** 2 + (soa[1] - CENTRE[1]) ** 2) / (width or 300.0) ** 2 * 4.0
    return soa, lw


def rounds_run(key_lo, key_hi):
    """the radix rounds a call runs: 8 minus the leading bytes the smallest and the largest key share, at least one"""
    r = 0
    while r < 7 and (key_lo >> (56 - 8 * r)) == (key_hi >> (56 - 8 * r)):
        r += 1
    return 8 - r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=30, help='timed calls per figure (at least 20)')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'quantile_timing.jsonl'))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error('--reps: at least 20')
    n = a.particles
    src = ('measured: HIP events around the launches (mcl_timing_get after every call, region mean_cov), median of %d after %d '
           'warm-ups, one handle per cloud, %d particles' % (a.reps, a.warmup, n))
    lines = []

    def report(name, ms, **kw):
        ms = np.array(ms)
        row = dict(figure=name, median_us=round(float(np.median(ms)) * 1e3, 2), p10_us=round(float(np.quantile(ms, 0.1)) * 1e3, 2),
                   p90_us=round(float(np.quantile(ms, 0.9)) * 1e3, 2), source=src, **kw)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    rs = np.random.RandomState(11)
    for cname, width in CLOUDS:
        soa, lw = make_cloud(cname, width, n, rs)
        e = engine.Engine(n, seed=5)
        e.set_particles(soa)
        e.set_log_weights(lw)
        e.timing_enable(True)

        def timed(fn):
            for _ in range(a.warmup):
                fn()
            e.timing_get()
            out = []
            for _ in range(a.reps):
                fn()
                t = e.timing_get()['mean_cov']
                assert t[1] >= 1, t
                out.append(t[0])
            return out

        for weighted in (False, True):
            for qname in ('x', 'radius2'):
                ends = e.cloud_quantiles(qname, [2.0 ** -32, 1.0], CENTRE, False)
                rounds = rounds_run(ends[0].key, ends[1].key)
                for probs in ([0.95], PROBS8):
                    report('%s_%s_%s_%dp' % (cname, 'weighted' if weighted else 'unweighted', qname, len(probs)),
                           timed(lambda: e.cloud_quantiles(qname, probs, CENTRE, weighted)), cloud=cname, weighted=weighted,
                           quantity=qname, n_probs=len(probs), rounds=rounds,
                           what='mcl_cloud_quantiles: k_quant_range, k_quant_plan, 8 x (k_quant_hist, k_quant_pick)')
            vals = [r.value for r in e.cloud_quantiles('radius2', PROBS8, CENTRE, weighted)]
            report('%s_%s_mass_8v' % (cname, 'weighted' if weighted else 'unweighted'),
                   timed(lambda: e.cloud_mass('radius2', vals, CENTRE, weighted, 0.0)), cloud=cname, weighted=weighted,
                   quantity='radius2', what='mcl_cloud_mass: one memset and k_quant_mass')
        report('%s_mean_cov' % cname, timed(e.mean_cov), cloud=cname, what='mcl_mean_cov: the yardstick')
        grid = e.mode_grid(2.0, 16, box=(0.0, 1000.0, -500.0, 500.0))
        report('%s_pose_modes' % cname, timed(lambda: e.pose_modes(None, k=4, grid=grid)), cloud=cname,
               what='mcl_pose_modes, 500 x 500 x 16 cells, k = 4: the yardstick')
        e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
