#!/usr/bin/env python3
"""tools/acoustic_timing.py -- what the delayed acoustic updates (include/mcl_acoustic.h) cost on the GPU: device time of
mcl_update_fix at 1 048 576 particles, evaluated at the current state (lag -1) and at lags 0, 8 and 64 of a ring of 65
recorded frames, with 1 and with 4 resamples between two records (more resamples leave fewer distinct ancestors, but
scatter the link further: which of the two wins is what the figures say).  No map is involved: the update reads the state,
the link and the frames.

HIP events of the library (mcl_timing_enable / mcl_timing_get: region MCL_K_UPDATE_GPS, one region per call), median of
--reps calls after 3 warm-ups.  Besides the plain fix: lag 8 with frac 0.5 (two frames), lag 8 with a lever arm (yaw, one
sincos and the rotation), four beacon ranges at lag 8, and mcl_update_gps on the same cloud as the yardstick of a pure
stream.  n_unique (mcl_history_smooth) says how many distinct ancestors the cloud has left at the deepest lag.
Appends one JSON line per figure to profiles/acoustic_timing.jsonl (and prints it); every number carries its source.
Run it under `timeout` on the GPU box:  timeout -k 10 600 python3 tools/acoustic_timing.py"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smarc_navigation_amd import engine  # noqa: E402

Q0 = [0.0, 0.0, 0.0, 1.0]
ZRP = [-2.0, 0.02, -0.01]
BEACONS = [[60.0, -10.0, -30.0], [-40.0, -40.0, -28.0], [45.0, 55.0, -31.0], [-30.0, 60.0, -25.0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--depth', type=int, default=65)
    ap.add_argument('--lags', type=int, nargs='*', default=[-1, 0, 8, 64])
    ap.add_argument('--between', type=int, nargs='*', default=[1, 4], help='resamples between two records')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'acoustic_timing.jsonl'))
    a = ap.parse_args()
    n = a.particles
    src = ('measured: HIP events around the launch (mcl_timing_get, region update_gps, one region per call), median of %d '
           'calls after 3 warm-ups, %d particles, ring of %d frames' % (a.reps, n, a.depth))
    lines = []

    def timed(name, call, **kw):
        ms = []
        for r in range(a.reps + 3):
            e.timing_get()
            call()
            t = e.timing_get()['update_gps']
            assert t[1] == 1, t
            if r >= 3:
                ms.append(t[0])
        ms = np.array(ms)
        row = dict(figure=name, median_us=round(float(np.median(ms)) * 1e3, 2), p10_us=round(float(np.quantile(ms, 0.1)) * 1e3, 2),
                   p90_us=round(float(np.quantile(ms, 0.9)) * 1e3, 2), source=src, **kw)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    for between in a.between:
        e = engine.Engine(n, seed=5, init_cov=[4.0, 4.0, 0.0, 0.0, 0.0, 0.01], process_cov=[1e-2, 1e-2, 0.0, 0.0, 0.0, 1e-5],
                          resample_cov=[1e-2, 1e-2, 0.0, 0.0, 0.0, 1e-5])
        e.init_particles()
        e.history_enable(a.depth)
        x = 0.0
        for k in range(a.depth):
            e.predict([1.5, 0.0, 0.0], 0.0, Q0, ZRP[0], 1.0)
            x += 1.5
            for _ in range(between):      # a fix of two sigmas of the cloud's spread: a resample that does select
                e.update_fix([x, 0.0], 2.0)
                e.resample()
            e.history_record(float(k))
        e.update_fix([x, 0.0], 2.0)
        e.resample()                      # the link is not the identity
        held = e.history_frames()[0]
        uniq = e.history_smooth(held)
        e.sync()
        e.timing_enable(True)
        kw = dict(resamples_between_records=between)
        timed('update_gps', lambda: e.update_gps(x, 0.0), what='the GPS update: a pure stream over the state', **kw)
        for lag in a.lags:
            if lag >= held:
                continue
            nu = dict(n_unique_at_lag=uniq[lag].n_unique) if lag >= 0 else {}
            timed('update_fix_lag_%d' % lag, lambda: e.update_fix([x, 0.0], 1.0, zrp=ZRP, lag=lag), lag=lag, **dict(kw, **nu))
        if held > 9:
            nu = dict(n_unique_at_lag=uniq[8].n_unique)
            timed('update_fix_lag_8_frac', lambda: e.update_fix([x, 0.0], 1.0, zrp=ZRP, lag=8, frac=0.5), lag=8, frac=0.5,
                  **dict(kw, **nu))
            timed('update_fix_lag_8_arm', lambda: e.update_fix([x, 0.0], 1.0, offset=[0.4, 0.0, 0.3], zrp=ZRP, lag=8), lag=8,
                  what='with a lever arm', **dict(kw, **nu))
            timed('update_beacon_ranges_4_lag_8', lambda: e.update_beacon_ranges(BEACONS, [70.0, 65.0, 80.0, 75.0], 1.0, zrp=ZRP, lag=8),
                  lag=8, what='four slant ranges', **dict(kw, **nu))
        e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
