#!/usr/bin/env python3
"""tools/history_timing.py -- what the particle genealogy (include/mcl_history.h) costs on the GPU, at the bench's
workload: 1 048 576 particles x 512 beams on the bench's default map (bench.py's own map, pings, covariances and seed).

HIP events of the library (mcl_timing_enable / mcl_timing_get: device time, every region of a call added up), median of
--reps after --warmup warm-up steps, from ONE handle in one run, alternating block by block so that drift hits both alike:
  * the fused step (mcl_step_mbes) with history off,
  * the fused step with history on (one compose behind the gather) plus one mcl_history_record per step,
  * mcl_history_smooth at lags 1, 8 and 64 (regions MCL_K_MEAN_COV) after 64 recorded steps, with n_unique at the
    deepest lag -- whether skipping the zero counts makes the older frames cheap shows in lag 64 against lag 8.
Appends one JSON line per figure to profiles/history_timing.jsonl (and prints it); every number carries its source.
Run it under `timeout` on the GPU box:  timeout -k 10 900 python3 tools/history_timing.py"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workload's definition: build_map, make_ranges, COV, SIGMA, R_MAX)
from smarc_navigation_amd import engine, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=int, default=1 << 20)
    ap.add_argument('--beams', type=int, default=512)
    ap.add_argument('--reps', type=int, default=200, help='timed steps per leg')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--block', type=int, default=25, help='steps before the legs alternate')
    ap.add_argument('--depth', type=int, default=64)
    ap.add_argument('--smooth-reps', type=int, default=20)
    ap.add_argument('--map', default='mesh')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'history_timing.jsonl'))
    a = ap.parse_args()
    n, B = a.particles, a.beams
    src = ('measured: HIP events around the launches (mcl_timing_get after every call, all regions added), median of %d '
           'after %d warm-ups, %d particles x %d beams, bench map %r' % (a.reps, a.warmup, n, B, a.map))
    lines = []

    def report(name, ms, **kw):
        ms = np.array(ms)
        row = dict(figure=name, median_us=round(float(np.median(ms)) * 1e3, 2), p10_us=round(float(np.quantile(ms, 0.1)) * 1e3, 2),
                   p90_us=round(float(np.quantile(ms, 0.9)) * 1e3, 2), source=src, **kw)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    total = a.warmup + 2 * a.reps + a.depth + 8
    m = bench.build_map(a.map)
    stream = synth.odom_stream(total)
    ba = synth.beam_angles(B)
    ranges = bench.make_ranges(engine, m, stream['truth'], ba, bench.SIGMA, bench.R_MAX)
    e = engine.Engine(n, seed=5, **bench.COV)
    bench.attach_map(e, m)
    e.init_particles()
    step = [0]

    def one_step(record):
        k = step[0]
        step[0] += 1
        e.step_mbes(stream['v'][k], stream['wz'][k], stream['q'][k], stream['z'][k], stream['dt'], ranges[k], ba,
                    bench.SIGMA, bench.R_MAX)
        if record:
            e.history_record(float(k))
        t = e.timing_get()
        return sum(ms for ms, _ in t.values()) - t['mbes_main'][0]   # (mbes_main is nested inside update_mbes)

    for _ in range(a.warmup):
        one_step(False)
    e.sync()
    e.timing_enable(True)
    e.timing_get()
    rows = {'off': [], 'on': []}
    while len(rows['on']) < a.reps:
        for leg in ('off', 'on'):
            if leg == 'on':
                e.history_enable(a.depth)
            for _ in range(a.block):
                if len(rows[leg]) < a.reps:
                    rows[leg].append(one_step(leg == 'on'))
            if leg == 'on':
                e.history_disable()
    report('step_mbes_history_off', rows['off'], what='fused step, device time')
    report('step_mbes_history_on_plus_record', rows['on'], what='fused step + compose + one record, device time',
           depth=a.depth, bytes_enabled=e.history_bytes(a.depth))
    report('history_on_cost', np.array(rows['on']) - np.median(rows['off']), what='the row above minus the median of history off')

    # the smoother after `depth` recorded steps
    e.history_enable(a.depth)
    for _ in range(a.depth):
        one_step(True)
    for lags in (1, 8, 64):
        if lags > a.depth:
            continue
        ms, est = [], None
        for r in range(a.smooth_reps + 3):
            e.timing_get()
            est = e.history_smooth(lags)
            t = e.timing_get()['mean_cov']
            assert t[1] == 1, t
            if r >= 3:
                ms.append(t[0])
        report('history_smooth_lags_%d' % lags, ms, region='mean_cov', lags=lags, n_unique_newest=est[0].n_unique,
               n_unique_oldest=est[-1].n_unique,
               reps='median of %d calls after 3 warm-ups (not the step legs\' counts)' % a.smooth_reps)
    e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
