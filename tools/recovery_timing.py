#!/usr/bin/env python3
"""tools/recovery_timing.py -- device time of the recovery calls (include/mcl_recovery.h) on the GPU, 1 048 576 particles.

HIP events of the library (mcl_timing_enable / mcl_timing_get), median of --reps after --warmup warm-up rounds:
  * mcl_weight_stats (its two launches, MCL_K_NORMALISE) beside the normalise region of the resample of the same round --
    both read the same 8 MB of log-weights;
  * mcl_init_particles_uniform, mcl_inject_uniform at fraction 0.05 and 1 (with and without the count), beside k_add_noise
    as mcl_init_particles runs it (all MCL_K_NOISE);
  * the MBES update (MCL_K_UPDATE_MBES) of the headline lattice mesh in a tracking filter: a normal step, the step after an
    injection that replaces next to nothing (fraction 1e-6: only the visiting order is voided), and the step after an
    injection of 5 % over the map's footprint.
Prints one JSON line per figure; every number carries its source.
Run it under `timeout` on the GPU box:  timeout -k 10 600 python3 tools/recovery_timing.py"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smarc_navigation_amd import engine, synth  # noqa: E402


def report(name, ms, src, **kw):
    ms = np.array(ms)
    print(json.dumps(dict(figure=name, median_us=round(float(np.median(ms)) * 1e3, 2), p10_us=round(float(np.quantile(ms, 0.1)) * 1e3, 2),
                          p90_us=round(float(np.quantile(ms, 0.9)) * 1e3, 2), source=src, **kw)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    a = ap.parse_args()
    n = a.particles
    src = 'measured: HIP events around the launches (mcl_timing_get after every call), median of %d after %d warm-ups, %d particles' % (
        a.reps, a.warmup, n)
    origin = (-64.0, -354.0)
    z = synth.bathymetry_grid(708, 708, 1.0, origin, seed=3)
    verts, tris = synth.mesh_from_grid(z, 1.0, origin)
    ba = synth.beam_angles(512)
    e = engine.Engine(n, init_cov=[4.0, 4.0, 0, 0, 0, 0.0025], process_cov=[1e-4, 1e-4, 0, 0, 0, 1e-6],
                      resample_cov=[0.01, 0.01, 0, 0, 0, 1e-5], seed=3)
    e.set_map_mesh(verts, tris)
    box = e.map_bounds()
    q = synth.quat_from_rpy(0.0, 0.0, 0.3)
    t = engine.Engine(64)
    t.set_map_mesh(verts, tris)
    truth = np.zeros((6, 64))
    truth[0], truth[1], truth[2], truth[5] = 40.0, 10.0, -2.0, 0.3
    t.set_particles(truth)
    ranges = t.mbes_expected(0, 1, ba, 60.0)[0]
    t.close()

    def cloud():
        e.init_particles()
        s = e.get_particles()
        s[0] += 40.0
        s[1] += 10.0
        s[5] += 0.3
        e.set_particles(s)

    # ---- the state-writing kernels
    e.timing_enable(True)
    rows = {k: [] for k in ('add_noise_init', 'init_uniform', 'inject_0.05_counted', 'inject_0.05', 'inject_1_counted', 'inject_1')}
    for r in range(a.warmup + a.reps):
        e.timing_get()
        for name, call in (('add_noise_init', lambda: e.init_particles()),
                           ('init_uniform', lambda: e.init_particles_uniform(box)),
                           ('inject_0.05_counted', lambda: e.inject_uniform(0.05, box)),
                           ('inject_0.05', lambda: e.inject_uniform(0.05, box, count=False)),
                           ('inject_1_counted', lambda: e.inject_uniform(1.0, box)),
                           ('inject_1', lambda: e.inject_uniform(1.0, box, count=False))):
            call()
            tm = e.timing_get()['noise']
            assert tm[1] == 1, (name, tm)
            if r >= a.warmup:
                rows[name].append(tm[0])
    for name in rows:
        report(name, rows[name], src, region='noise')

    # ---- weight statistics beside the resample's normalise, and the MBES update after an injection
    cloud()
    ws, norm = [], []
    upd = {'normal': [], 'order_voided': [], 'injected_5_per_cent': []}
    kinds = ['normal', 'normal', 'order_voided', 'normal', 'normal', 'injected_5_per_cent']
    rounds = a.warmup + 3 * a.reps
    for r in range(rounds):
        kind = kinds[r % len(kinds)] if r >= a.warmup else 'normal'
        if kind == 'order_voided':
            e.inject_uniform(1e-6, box, count=False)
        elif kind == 'injected_5_per_cent':
            e.inject_uniform(0.05, box, count=False)
        e.predict([0.0, 0.0, 0.0], 0.0, q, -2.0, 0.02)    # (at rest: the cloud stays over the ping's ground)
        e.timing_get()
        e.update_mbes(ranges, ba, 0.2, 60.0)
        tu = e.timing_get()['update_mbes']
        st = e.weight_stats()
        tw = e.timing_get()['normalise']
        e.resample()
        tn = e.timing_get()['normalise']
        assert tu[1] == 1 and tw[1] == 1 and tn[1] >= 1, (tu, tw, tn)
        if r >= a.warmup:
            upd[kind].append(tu[0])
            ws.append(tw[0])
            norm.append(tn[0])
        if kind == 'injected_5_per_cent':
            cloud()                                          # (back to a tracking cloud for the next rounds)
            for _ in range(2):
                e.predict([0.0, 0.0, 0.0], 0.0, q, -2.0, 0.02)
                e.update_mbes(ranges, ba, 0.2, 60.0)
                e.resample()
    report('weight_stats', ws, src, region='normalise', launches=2, n_eff_last=st.n_eff)
    report('resample_normalise', norm, src, region='normalise')
    for kind in upd:
        report('update_mbes_' + kind, upd[kind], src, region='update_mbes', map='lattice_mesh_708', beams=512, rounds=len(upd[kind]))
    e.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
