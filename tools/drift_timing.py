#!/usr/bin/env python3
"""tools/drift_timing.py -- what the per-particle drift states (include/mcl_drift.h) cost on the GPU, at the bench's
workload: 1 048 576 particles x 512 beams on the bench's default map (bench.py's own map, pings, covariances and seed).

HIP events of the library (mcl_timing_enable / mcl_timing_get: device time of the timed regions), median of --reps after
--warmup warm-up steps, from ONE handle in one run, the legs alternating block by block so that clock drift hits all alike:
  * mcl_drift_advance alone, beside mcl_predict alone (both region `predict`: the yardstick moves the same 96 B per
    particle and draws the same four normals),
  * mcl_resample (systematic, on the log-weights a ping of the workload leaves) with nothing on, with the drift on (one
    gather behind the resample's own) and with the history on (k_history_compose: the yardstick), region `resample`, with
    the lost-slot fraction of those resamples,
  * the fused step (mcl_step_mbes) with the drift off, and with it on plus one mcl_drift_advance per step,
  * mcl_drift_mean_cov (region `mean_cov`).
Appends one JSON line per figure to profiles/drift_timing.jsonl (and prints it); every number carries its source.
Run it under `timeout` on the GPU box:  timeout -k 10 900 python3 tools/drift_timing.py"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workload's definition: build_map, make_ranges, COV, SIGMA, R_MAX)
from smarc_navigation_amd import engine, resampling, synth  # noqa: E402

INIT_STD, WALK_STD = (0.2, 0.2, 1e-3), (0.005, 0.005, 1e-5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=int, default=1 << 20)
    ap.add_argument('--beams', type=int, default=512)
    ap.add_argument('--reps', type=int, default=50, help='timed calls per leg')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--block', type=int, default=10, help='calls before the legs alternate')
    ap.add_argument('--map', default='mesh')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'drift_timing.jsonl'))
    a = ap.parse_args()
    n, B = a.particles, a.beams
    src = ('measured: HIP events around the launches (mcl_timing_get after every call), median of %d after %d warm-ups, legs '
           'alternating in blocks of %d on one handle, %d particles x %d beams, bench map %r'
           % (a.reps, a.warmup, a.block, n, B, a.map))
    lines = []

    def report(name, ms, **kw):
        ms = np.array(ms)
        row = dict(figure=name, median_us=round(float(np.median(ms)) * 1e3, 2), p10_us=round(float(np.quantile(ms, 0.1)) * 1e3, 2),
                   p90_us=round(float(np.quantile(ms, 0.9)) * 1e3, 2), source=src, **kw)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    total = 3 * a.warmup + 8 * a.reps + 16
    m = bench.build_map(a.map)
    stream = synth.odom_stream(total)
    ba = synth.beam_angles(B)
    ranges = bench.make_ranges(engine, m, stream['truth'], ba, bench.SIGMA, bench.R_MAX)
    e = engine.Engine(n, seed=5, **bench.COV)
    bench.attach_map(e, m)
    e.init_particles()
    step = [0]

    def odo():
        k = step[0]
        step[0] += 1
        return k, (stream['v'][k], stream['wz'][k], stream['q'][k], stream['z'][k], stream['dt'])

    def all_regions(t):
        return sum(ms for ms, _ in t.values()) - t['mbes_main'][0]   # (mbes_main is nested inside update_mbes)

    def fused(drift):
        k, od = odo()
        if drift:
            e.drift_advance(stream['dt'])
        e.step_mbes(*od, ranges[k], ba, bench.SIGMA, bench.R_MAX)
        return all_regions(e.timing_get())

    def alternate(legs, call, before=None, after=None):
        rows = {leg: [] for leg in legs}
        while min(len(r) for r in rows.values()) < a.reps:
            for leg in legs:
                if before:
                    before(leg)
                for _ in range(a.block):
                    if len(rows[leg]) < a.reps:
                        rows[leg].append(call(leg))
                if after:
                    after(leg)
        return rows

    def on(leg):
        if leg == 'drift':
            e.drift_enable(INIT_STD, WALK_STD)
        if leg == 'history':
            e.history_enable(1)

    def off(leg):
        if leg == 'drift':
            e.drift_disable()
        if leg == 'history':
            e.history_disable()

    for _ in range(a.warmup):
        k, od = odo()
        e.step_mbes(*od, ranges[k], ba, bench.SIGMA, bench.R_MAX)
    e.sync()
    e.timing_enable(True)
    e.timing_get()

    # ---- the fused step, drift off / on (+ one advance per step)
    rows = alternate(('off', 'drift'), lambda leg: fused(leg == 'drift'), on, off)
    report('step_mbes_drift_off', rows['off'], what='fused step, device time')
    report('step_mbes_drift_on_plus_advance', rows['drift'], what='fused step + gather + one advance, device time',
           bytes_enabled=e.drift_bytes())
    report('drift_on_cost_per_step', np.array(rows['drift']) - np.median(rows['off']),
           what='the row above minus the median of drift off')

    # ---- the advance beside the predict
    e.drift_enable(INIT_STD, WALK_STD)

    def adv_or_predict(leg):
        _, od = odo()
        if leg == 'advance':
            e.drift_advance(stream['dt'])
        else:
            e.predict(*od)
        t = e.timing_get()['predict']
        assert t[1] == 1, t
        return t[0]
    rows = alternate(('predict', 'advance'), adv_or_predict)
    report('predict_alone', rows['predict'], region='predict', what='mcl_predict (k_predict): the yardstick')
    report('drift_advance', rows['advance'], region='predict', what='mcl_drift_advance (k_drift_advance)')

    # ---- mean and covariance
    ms = []
    for r in range(a.reps + 3):
        e.timing_get()
        e.drift_mean_cov()
        t = e.timing_get()['mean_cov']
        assert t[1] == 1, t
        if r >= 3:
            ms.append(t[0])
    report('drift_mean_cov', ms, region='mean_cov', what='k_drift_moments + k_sum_final')
    e.drift_disable()

    # ---- a resample with nothing / the drift / the history behind it, on the log-weights a ping leaves
    lost = []

    def resample(leg):
        k, od = odo()
        e.predict(*od)
        e.update_mbes(ranges[k], ba, bench.SIGMA, bench.R_MAX)
        e.timing_get()
        e.resample()
        t = e.timing_get()['resample'][0]
        if len(lost) < 4:
            A = resampling.slot_ancestors(e.last_indices())
            lost.append(float(np.count_nonzero(A != np.arange(n))) / n)
        return t
    rows = alternate(('off', 'drift', 'history'), resample, on, off)
    frac = round(float(np.mean(lost)), 4)
    report('resample_plain', rows['off'], region='resample', lost_fraction=frac)
    report('resample_drift_on', rows['drift'], region='resample', lost_fraction=frac, what='+ k_drift_gather')
    report('resample_history_on', rows['history'], region='resample', lost_fraction=frac,
           what='+ k_history_compose: the yardstick')
    report('drift_gather_cost', np.array(rows['drift']) - np.median(rows['off']), what='drift on minus the median of plain')
    report('history_compose_cost', np.array(rows['history']) - np.median(rows['off']), what='history on minus the median of plain')
    e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
