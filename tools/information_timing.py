#!/usr/bin/env python3
"""tools/information_timing.py -- what one mcl_ping_information / mcl_pose_information (include/mcl_information.h) costs on
the GPU.

The maps of tools/innovation_timing.py -- the 512 x 512 height grid, the 708 x 708 lattice mesh, the irregular TIN over the
same terrain and that TIN cast as a triangle soup -- with B = 64 and 512 beams at the default 4096 samples, on 1 048 576
particles around a track point; on each map the raster of 256 x 256 poses (Engine.pose_information, 65 536 poses at the
vehicle's depth, B = 64 and 512); then, on the grid, the default case and the raster for several group sizes G (MCL_INFORMATION_GROUP, poses
per workgroup of k_information; the records do not depend on it).

The launches have no timing region of the library (MCL_K_COUNT stays 15), so two clocks are used:
  * the host's: wall time of the whole call -- beam table (and pose) upload, memset, k_information, the copy back, its one
    synchronisation and the derived quantities --, median of --reps after --warmup calls (`call_us`);
  * the profiler's: run the tool under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3
    tools/information_timing.py --plan DIR/plan.json`, then `python3 tools/information_timing.py --from-trace DIR --plan
    DIR/plan.json`: the k_information dispatches of the trace, in order, are dealt to the cases by the plan and their device
    durations reported (`kernel_us`, warm-up dispatches dropped).
Appends one JSON line per figure to profiles/information_timing.jsonl (and prints it); every number carries its source.
Run it under `timeout` on the GPU box:  timeout -k 10 400 python3 tools/information_timing.py"""
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
GROUPS = (1, 2, 4, 7, 10)
RASTER = 256


def run_cases(a):
    from smarc_navigation_amd import engine, synth
    from ranges_timing import cloud, maps
    soa = cloud(a.particles)
    src = ('measured: host clock around each Engine call (uploads, memset, k_information, copy back, one synchronisation, '
           'mcl_information_matrix), median of %d after %d warm-up calls, %d particles' % (a.reps, a.warmup, a.particles))
    lines, plan = [], []

    def timed(name, call, describe, **kw):
        us = []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            res = call()
            if k >= a.warmup:
                us.append((time.perf_counter() - t0) * 1e6)
        us = np.array(us)
        row = dict(figure=name, call_us=round(float(np.median(us)), 1), p10_us=round(float(np.quantile(us, 0.1)), 1),
                   p90_us=round(float(np.quantile(us, 0.9)), 1), source=src, **kw)
        row.update(describe(res))
        plan.append(dict(figure=name, calls=a.warmup + a.reps, warmup=a.warmup))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def ping(e, name, B, **kw):
        ba = synth.beam_angles(B)
        timed(name, lambda: e.ping_information(ba, SIGMA, R_MAX),
              lambda r: dict(n_sampled=r.n_sampled, pairs=int(r.beams['n'].sum()), hit_share=round(r.hit_share, 4),
                             crlb_strong=round(r.crlb_strong, 4), crlb_weak=round(min(r.crlb_weak, 1e9), 4)), beams=B, **kw)

    def raster(e, name, B, **kw):
        ba = synth.beam_angles(B)
        c = soa[:, :1].mean(axis=1)
        xs, ys = np.meshgrid(c[0] + 1.5 * (np.arange(RASTER) - RASTER / 2), c[1] + 1.5 * (np.arange(RASTER) - RASTER / 2))
        poses = np.zeros((6, RASTER * RASTER))
        poses[0], poses[1], poses[2] = xs.ravel(), ys.ravel(), c[2]
        timed(name, lambda: e.pose_information(poses, ba, SIGMA, R_MAX),
              lambda r: dict(poses=int(r.poses.size), pairs=int(r.poses['n'].sum()), hit_share=round(float(r.hit_share.mean()), 4),
                             rank2_share=round(float((r.rank_pos == 2).mean()), 4)), beams=B, **kw)

    for mname, m in maps(a.maps.split(',')):
        e = engine.Engine(a.particles, rng_mode=engine.RNG_REPLAY)
        if 'z' in m:
            e.set_map_grid(m['z'], m['origin'], 1.0)
        else:
            e.set_map_mesh(m['verts'], m['tris'], general=m.get('general', False))
        e.set_particles(soa)
        for B in (64, 512):
            ping(e, '%s_B%d_S4096' % (mname, B), B, map=mname)
        for B in (64, 512):
            raster(e, '%s_B%d_raster%d' % (mname, B, RASTER), B, map=mname)
        e.close()
    if a.groups:
        mname, m = maps(['grid'])[0]
        for g in GROUPS:
            os.environ['MCL_INFORMATION_GROUP'] = str(g)      # (read when the handle is created)
            e = engine.Engine(a.particles, rng_mode=engine.RNG_REPLAY)
            e.set_map_grid(m['z'], m['origin'], 1.0)
            e.set_particles(soa)
            ping(e, '%s_B512_S4096_G%d' % (mname, g), 512, map=mname, group=g)
            raster(e, '%s_B512_raster%d_G%d' % (mname, RASTER, g), 512, map=mname, group=g)
            e.close()
        del os.environ['MCL_INFORMATION_GROUP']
    if a.plan:
        with open(a.plan, 'w') as f:
            json.dump(plan, f)
    return lines


def from_trace(a):
    """the device durations of the k_information dispatches of a rocprofv3 kernel trace, dealt to the plan's cases in order"""
    plan = json.load(open(a.plan))
    rows = []
    for p in sorted(glob.glob(os.path.join(a.from_trace, '**', '*kernel_trace.csv'), recursive=True)):
        for r in csv.DictReader(open(p)):
            if 'k_information' in r['Kernel_Name']:
                rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp'])))
    rows.sort()
    need = sum(c['calls'] for c in plan)
    if len(rows) != need:
        raise SystemExit('the trace holds %d k_information dispatches, the plan %d calls' % (len(rows), need))
    src = 'measured: rocprofv3 --kernel-trace, device duration of each k_information dispatch, median per case, warm-ups dropped'
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'information_timing.jsonl'))
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
