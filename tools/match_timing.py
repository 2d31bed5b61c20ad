#!/usr/bin/env python3
"""tools/match_timing.py -- what one mcl_match_ping (include/mcl_match.h) costs on the GPU, and what the same work costs the
only way the library allowed before it.

The maps of tools/information_timing.py -- the 512 x 512 height grid, the 708 x 708 lattice mesh, the irregular TIN over the
same terrain and that TIN cast as a triangle soup --, M = 1, 64 and 4096 start poses around a track point (x, y sigma 2 m,
yaw sigma 0.05 rad), B = 64 and 512 beams, D = 3 and 4, a noise-free ping the library itself expects at the track point,
max_iter = 12.

  * `call_us`: the host's wall time of the whole Engine.match_ping call -- uploads, memset, k_ping_match, the copy back and
    its one synchronisation --, median of --reps after --warmup calls.
  * `host_loop_us`: per evaluation the kernel ran on average (rounded up), one round trip of the calls the library had:
    set_particles of the M poses, mbes_expected of them (the ranges at the pose itself), pose_information of them (the
    sums of the central differences).  That is less than a host loop needs -- those calls do not hand back sum d rho, and a
    fix of z would need a second set of poses --, so the ratio `host_loop_over_call` flatters the host loop.
  * `kernel_us` (the profiler's clock): run the tool under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3
    tools/match_timing.py --no-host-loop --plan DIR/plan.json`, then `python3 tools/match_timing.py --from-trace DIR --plan
    DIR/plan.json`: the k_ping_match dispatches of the trace, in order, are dealt to the cases by the plan.
Appends one JSON line per figure to profiles/match_timing.jsonl (and prints it); every number carries its source.  Nothing
is asserted about the numbers.  Run it under `timeout` on the GPU box:  timeout -k 10 400 python3 tools/match_timing.py"""
import argparse
import csv
import glob
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIGMA, R_MAX = 0.2, 60.0
POSES = (1, 64, 4096)
BEAMS = (64, 512)


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
    src = ('measured: host clock around each call, median of %d after %d warm-up calls; call_us: Engine.match_ping; '
           'host_loop_us: set_particles + mbes_expected + pose_information per evaluation' % (a.reps, a.warmup))
    lines, plan = [], []
    truth = np.array([40.0, 10.0, -2.0, 0.0, 0.0, 0.3])
    for mname, m in maps(a.maps.split(',')):
        def mapped(n):
            e = engine.Engine(n, rng_mode=engine.RNG_REPLAY)
            if 'z' in m:
                e.set_map_grid(m['z'], m['origin'], 1.0)
            else:
                e.set_map_mesh(m['verts'], m['tris'], general=m.get('general', False))
            return e
        one = mapped(1)
        one.set_particles(truth[:, None])
        for B in BEAMS:
            ba = synth.beam_angles(B)
            meas = one.mbes_expected(0, 1, ba, R_MAX)[0].astype(np.float32)
            for M in POSES:
                poses = np.ascontiguousarray(cloud(M))
                loop = mapped(M)
                for fit_z in (False, True):
                    name = '%s_M%d_B%d_D%d' % (mname, M, B, 4 if fit_z else 3)
                    res, call_us, p10, p90 = _median_us(lambda: one.match_ping(poses, meas, ba, SIGMA, R_MAX, fit_z=fit_z), a.warmup, a.reps)
                    evals = float(res.results['evaluations'].mean())
                    row = dict(figure=name, map=mname, poses=M, beams=B, dims=4 if fit_z else 3, call_us=call_us, p10_us=p10, p90_us=p90,
                               evaluations_mean=round(evals, 2), converged_share=round(float((res.status == 0).mean()), 4),
                               rms_median=round(float(np.median(res.rms)), 5), source=src)
                    plan.append(dict(figure=name, calls=a.warmup + a.reps, warmup=a.warmup))
                    if a.host_loop:
                        rounds = int(math.ceil(evals))

                        def host_loop():
                            for _ in range(rounds):
                                loop.set_particles(poses)
                                loop.mbes_expected(0, M, ba, R_MAX)
                                loop.pose_information(poses, ba, SIGMA, R_MAX)
                        _, loop_us, _, _ = _median_us(host_loop, min(a.warmup, 2), max(a.reps // 4, 3))
                        row.update(host_loop_us=loop_us, host_loop_rounds=rounds, host_loop_over_call=round(loop_us / call_us, 2))
                    lines.append(json.dumps(row))
                    print(lines[-1], flush=True)
                loop.close()
        one.close()
    if a.plan:
        with open(a.plan, 'w') as f:
            json.dump(plan, f)
    return lines


def from_trace(a):
    """the device durations of the k_ping_match dispatches of a rocprofv3 kernel trace, dealt to the plan's cases in order"""
    plan = json.load(open(a.plan))
    rows = []
    for p in sorted(glob.glob(os.path.join(a.from_trace, '**', '*kernel_trace.csv'), recursive=True)):
        for r in csv.DictReader(open(p)):
            if 'k_ping_match' in r['Kernel_Name']:
                rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp'])))
    rows.sort()
    need = sum(c['calls'] for c in plan)
    if len(rows) != need:
        raise SystemExit('the trace holds %d k_ping_match dispatches, the plan %d calls' % (len(rows), need))
    src = 'measured: rocprofv3 --kernel-trace, device duration of each k_ping_match dispatch, median per case, warm-ups dropped'
    lines, at = [], 0
    for c in plan:
        d = np.array([(e - s) / 1e3 for s, e in rows[at + c['warmup']:at + c['calls']]])
        at += c['calls']
        lines.append(json.dumps(dict(figure=c['figure'], kernel_us=round(float(np.median(d)), 2), p10_us=round(float(np.quantile(d, 0.1)), 2),
                                     p90_us=round(float(np.quantile(d, 0.9)), 2), dispatches=int(d.size), source=src)))
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--maps', default='grid,mesh,tin,soup')
    ap.add_argument('--no-host-loop', dest='host_loop', action='store_false', help='skip the host loop (a profiler run)')
    ap.add_argument('--plan', help='write (run) or read (--from-trace) the cases and their call counts here')
    ap.add_argument('--from-trace', metavar='DIR', help='no GPU run: read the rocprofv3 kernel trace under DIR')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'match_timing.jsonl'))
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
