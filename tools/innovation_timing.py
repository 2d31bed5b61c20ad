#!/usr/bin/env python3
"""tools/innovation_timing.py -- what one mcl_ping_innovation (include/mcl_innovation.h) costs on the GPU.

The matrix of tools/ranges_timing.py's maps -- the 512 x 512 height grid, the 708 x 708 lattice mesh, the irregular TIN over
the same terrain and that TIN cast as a triangle soup -- with B = 64 and 512 beams and max_samples = 1024 / 4096 / 32768, on
1 048 576 particles around a track point; then, on the grid, the default case (4096 samples x 512 beams) for several group
sizes G (MCL_INNOVATION_GROUP, particles per workgroup of k_innovation; the records do not depend on it).

The launches have no timing region of the library (MCL_K_COUNT stays 15), so two clocks are used:
  * the host's: wall time of the whole call -- beam table upload, memset, k_innovation, the copy back and its one
    synchronisation --, median of --reps after --warmup calls (`call_us`);
  * the profiler's: run the tool under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3
    tools/innovation_timing.py --plan DIR/plan.json`, then `python3 tools/innovation_timing.py --from-trace DIR --plan
    DIR/plan.json`: the k_innovation dispatches of the trace, in order, are dealt to the cases by the plan and their device
    durations reported (`kernel_us`, warm-up dispatches dropped).
Appends one JSON line per figure to profiles/innovation_timing.jsonl (and prints it); every number carries its source.
Run it under `timeout` on the GPU box:  timeout -k 10 400 python3 tools/innovation_timing.py"""
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
GROUPS = (2, 4, 8, 16, 32, 64)


def run_cases(a):
    from smarc_navigation_amd import engine, synth
    from ranges_timing import cloud, maps
    soa = cloud(a.particles)
    src = ('measured: host clock around each Engine.ping_innovation call (upload, memset, k_innovation, copy back, one '
           'synchronisation), median of %d after %d warm-up calls, %d particles' % (a.reps, a.warmup, a.particles))
    lines, plan = [], []

    def one(e, name, B, ms, **kw):
        ba = synth.beam_angles(B)
        ranges = e.mbes_expected(0, 1, ba, R_MAX)[0] + np.float32(0.05)
        us = []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            inn = e.ping_innovation(ranges, ba, SIGMA, R_MAX, max_samples=ms)
            if k >= a.warmup:
                us.append((time.perf_counter() - t0) * 1e6)
        us = np.array(us)
        row = dict(figure=name, beams=B, max_samples=ms, n_sampled=inn.n_sampled, rays=int(inn.n.sum()),
                   call_us=round(float(np.median(us)), 1), p10_us=round(float(np.quantile(us, 0.1)), 1),
                   p90_us=round(float(np.quantile(us, 0.9)), 1), mean_nis=round(inn.mean_nis(), 4), source=src, **kw)
        plan.append(dict(figure=name, calls=a.warmup + a.reps, warmup=a.warmup))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    for mname, m in maps(a.maps.split(',')):
        e = engine.Engine(a.particles, rng_mode=engine.RNG_REPLAY)
        if 'z' in m:
            e.set_map_grid(m['z'], m['origin'], 1.0)
        else:
            e.set_map_mesh(m['verts'], m['tris'], general=m.get('general', False))
        e.set_particles(soa)
        for B in (64, 512):
            for ms in (1024, 4096, 32768):
                one(e, '%s_B%d_S%d' % (mname, B, ms), B, ms, map=mname)
        e.close()
    if a.groups:
        mname, m = maps(['grid'])[0]
        for g in GROUPS:
            os.environ['MCL_INNOVATION_GROUP'] = str(g)      # (read when the handle is created)
            e = engine.Engine(a.particles, rng_mode=engine.RNG_REPLAY)
            e.set_map_grid(m['z'], m['origin'], 1.0)
            e.set_particles(soa)
            one(e, '%s_B512_S4096_G%d' % (mname, g), 512, 4096, map=mname, group=g)
            e.close()
        del os.environ['MCL_INNOVATION_GROUP']
    if a.plan:
        with open(a.plan, 'w') as f:
            json.dump(plan, f)
    return lines


def from_trace(a):
    """the device durations of the k_innovation dispatches of a rocprofv3 kernel trace, dealt to the plan's cases in order"""
    plan = json.load(open(a.plan))
    rows = []
    for p in sorted(glob.glob(os.path.join(a.from_trace, '**', '*kernel_trace.csv'), recursive=True)):
        for r in csv.DictReader(open(p)):
            if 'k_innovation' in r['Kernel_Name']:
                rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp'])))
    rows.sort()
    need = sum(c['calls'] for c in plan)
    if len(rows) != need:
        raise SystemExit('the trace holds %d k_innovation dispatches, the plan %d calls' % (len(rows), need))
    src = 'measured: rocprofv3 --kernel-trace, device duration of each k_innovation dispatch, median per case, warm-ups dropped'
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
    ap.add_argument('--particles', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--maps', default='grid,mesh,tin,soup')
    ap.add_argument('--no-groups', dest='groups', action='store_false', help='skip the group-size sweep')
    ap.add_argument('--plan', help='write (run) or read (--from-trace) the cases and their call counts here')
    ap.add_argument('--from-trace', metavar='DIR', help='no GPU run: read the rocprofv3 kernel trace under DIR')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'innovation_timing.jsonl'))
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
