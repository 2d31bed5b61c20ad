#!/usr/bin/env python3
"""tools/swath_timing.py -- what one mcl_match_swath (include/mcl_swath.h) costs on the GPU, and in the same run what
mcl_match_ping costs at the shapes of a swath of one ping.

The maps of tools/match_timing.py -- the 512 x 512 height grid, the 708 x 708 lattice mesh, the irregular TIN over the same
terrain and that TIN cast as a triangle soup --, K = 1, 8 and 32 pings 1 m apart along the heading behind the anchor, B = 64
and 512 beams, M = 1, 64 and 4096 start poses around a track point (x, y sigma 2 m, yaw sigma 0.05 rad; roll and pitch the
track's, which is what the offsets carry, so that the ping match at K = 1 is the same fit bit for bit), D = 4, noise-free
pings the library itself expects at the pings' poses, max_iter = 12.

  * `call_us`: the host's wall time of the whole Engine.match_swath (figures swath_*) or Engine.match_ping (figures ping_*,
    K = 1 shapes only) call -- uploads, memset, the kernel, the copy back and its one synchronisation --, median of --reps
    after --warmup calls.
  * `kernel_us` (the profiler's clock): run the tool under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3
    tools/swath_timing.py --plan DIR/plan.json`, then `python3 tools/swath_timing.py --from-trace DIR --plan DIR/plan.json`:
    the k_swath_match and k_ping_match dispatches of the trace, in order, are dealt to the cases by the plan, and every
    K = 1 swath figure gains `kernel_over_ping_match`, its kernel time over k_ping_match's at the same shape in that run.
Appends one JSON line per figure to profiles/swath_timing.jsonl (and prints it); every number carries its source.  Nothing
is asserted about the numbers.  Run it under `timeout` on the GPU box:  timeout -k 10 500 python3 tools/swath_timing.py"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIGMA, R_MAX = 0.2, 60.0
PINGS = (1, 8, 32)
BEAMS = (64, 512)
POSES = (1, 64, 4096)
SPACING = 1.0


def _median_us(call, warmup, reps):
    us, res = [], None
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        res = call()
        if k >= warmup:
            us.append((time.perf_counter() - t0) * 1e6)
    us = np.array(us)
    return res, round(float(np.median(us)), 1), round(float(np.quantile(us, 0.1)), 1), round(float(np.quantile(us, 0.9)), 1)


def run_cases(a):
    from smarc_navigation_amd import engine, synth
    from ranges_timing import cloud, maps
    src = 'measured: host clock around each call, median of %d after %d warm-up calls' % (a.reps, a.warmup)
    lines, plan = [], []
    truth = np.array([40.0, 10.0, -2.0, 0.0, 0.0, 0.3])
    kmax = max(PINGS)
    back = SPACING * (kmax - 1 - np.arange(kmax))
    track = np.repeat(truth[:, None], kmax, axis=1)          # the vehicle's poses at the pings, the newest last
    track[0] -= back * np.cos(truth[5])
    track[1] -= back * np.sin(truth[5])
    for mname, m in maps(a.maps.split(',')):
        e = engine.Engine(kmax, rng_mode=engine.RNG_REPLAY)
        if 'z' in m:
            e.set_map_grid(m['z'], m['origin'], 1.0)
        else:
            e.set_map_mesh(m['verts'], m['tris'], general=m.get('general', False))
        e.set_particles(track)
        for B in BEAMS:
            ba = synth.beam_angles(B)
            pings = e.mbes_expected(0, kmax, ba, R_MAX).astype(np.float32)
            for M in POSES:
                poses = np.ascontiguousarray(cloud(M))
                poses[3], poses[4] = truth[3], truth[4]      # the attitude the offsets carry: the ping match does the swath's work

                def row_of(name, kind, K, res, call_us, p10, p90):
                    plan.append(dict(figure=name, kernel='k_%s_match' % kind, calls=a.warmup + a.reps, warmup=a.warmup,
                                     shape='%s_M%d_B%d' % (mname, M, B), pings=K))
                    lines.append(json.dumps(dict(
                        figure=name, map=mname, pings=K, poses=M, beams=B, dims=4, call_us=call_us, p10_us=p10, p90_us=p90,
                        evaluations_mean=round(float(res.results['evaluations'].mean()), 2),
                        converged_share=round(float((res.status == 0).mean()), 4), rms_median=round(float(np.median(res.rms)), 5), source=src)))
                    print(lines[-1], flush=True)
                res, us, p10, p90 = _median_us(lambda: e.match_ping(poses, pings[-1], ba, SIGMA, R_MAX, fit_z=True), a.warmup, a.reps)
                row_of('ping_%s_M%d_B%d' % (mname, M, B), 'ping', 1, res, us, p10, p90)
                for K in PINGS:
                    off = engine.swath_offsets(track[:, kmax - K:])
                    rng = np.ascontiguousarray(pings[kmax - K:])
                    res, us, p10, p90 = _median_us(lambda: e.match_swath(poses, rng, ba, off, SIGMA, R_MAX, fit_z=True), a.warmup, a.reps)
                    row_of('swath_%s_K%d_M%d_B%d' % (mname, K, M, B), 'swath', K, res, us, p10, p90)
        e.close()
    if a.plan:
        with open(a.plan, 'w') as f:
            json.dump(plan, f)
    return lines


def from_trace(a):
    """the device durations of the k_swath_match / k_ping_match dispatches of a rocprofv3 kernel trace, dealt to the plan's
    cases in order; the K = 1 swath cases against the ping match at the same shape"""
    plan = json.load(open(a.plan))
    rows = []
    for p in sorted(glob.glob(os.path.join(a.from_trace, '**', '*kernel_trace.csv'), recursive=True)):
        for r in csv.DictReader(open(p)):
            for kernel in ('k_swath_match', 'k_ping_match'):
                if kernel in r['Kernel_Name']:
                    rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), kernel))
    rows.sort()
    need = sum(c['calls'] for c in plan)
    if len(rows) != need:
        raise SystemExit('the trace holds %d match dispatches, the plan %d calls' % (len(rows), need))
    src = 'measured: rocprofv3 --kernel-trace, device duration of each dispatch, median per case, warm-ups dropped'
    lines, at, ping_us = [], 0, {}
    for c in plan:
        mine = rows[at:at + c['calls']]
        at += c['calls']
        if any(k != c['kernel'] for _, _, k in mine):
            raise SystemExit('%s: the trace is not in the order of the plan' % c['figure'])
        d = np.array([(e - s) / 1e3 for s, e, _ in mine[c['warmup']:]])
        row = dict(figure=c['figure'], kernel_us=round(float(np.median(d)), 2), p10_us=round(float(np.quantile(d, 0.1)), 2),
                   p90_us=round(float(np.quantile(d, 0.9)), 2), dispatches=int(d.size), source=src)
        if c['kernel'] == 'k_ping_match':
            ping_us[c['shape']] = row['kernel_us']
        elif c['pings'] == 1:
            row['kernel_over_ping_match'] = round(row['kernel_us'] / ping_us[c['shape']], 3)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--maps', default='grid,mesh,tin,soup')
    ap.add_argument('--plan', help='write (run) or read (--from-trace) the cases and their call counts here')
    ap.add_argument('--from-trace', metavar='DIR', help='no GPU run: read the rocprofv3 kernel trace under DIR')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'swath_timing.jsonl'))
    a = ap.parse_args()
    if a.from_trace and not a.plan:
        ap.error('--from-trace needs --plan')
    lines = from_trace(a) if a.from_trace else run_cases(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
