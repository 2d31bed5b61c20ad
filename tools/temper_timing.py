#!/usr/bin/env python3
"""tools/temper_timing.py -- device time of mcl_temper (include/mcl_temper.h) on the GPU, 1 048 576 particles.

HIP events of the library (mcl_timing_enable / mcl_timing_get, region MCL_K_NORMALISE), median of --reps after --warmup
warm-up rounds, the same log-weights planted again before every call:
  * peaked: the log-weights one real 512-beam MBES update of the headline lattice mesh leaves (all three rounds);
  * flat:   equal log-weights (beta = 1: round 1 alone decides, rounds 2 and 3 and the apply return at once);
  * floor:  one particle holds all the weight (not even beta = 2^-32 reaches the target: round 1 alone);
each with and without the apply, with `levels_evaluated`, the level and the launches next to the time, and beside them
mcl_weight_stats (one pass over the same 8 MB) and the normalise region of the resample that follows.
Prints one JSON line per figure; every number carries its source.
Run it under `timeout` on the GPU box:  timeout -k 10 600 python3 tools/temper_timing.py"""
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
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--ess-ratio', type=float, default=0.5)
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
    t = engine.Engine(64)
    t.set_map_mesh(verts, tris)
    truth = np.zeros((6, 64))
    truth[0], truth[1], truth[2], truth[5] = 40.0, 10.0, -2.0, 0.3
    t.set_particles(truth)
    ranges = t.mbes_expected(0, 1, ba, 60.0)[0]
    t.close()
    e.init_particles()
    s = e.get_particles()
    s[0] += 40.0
    s[1] += 10.0
    s[5] += 0.3
    e.set_particles(s)
    e.predict([0.0, 0.0, 0.0], 0.0, synth.quat_from_rpy(0.0, 0.0, 0.3), -2.0, 0.02)
    e.update_mbes(ranges, ba, 0.2, 60.0)
    floor = np.full(n, -1e12)
    floor[0] = 0.0
    clouds = (('peaked_512_beam_update', e.get_log_weights()), ('flat', np.full(n, -3.25)), ('floor', floor))
    e.timing_enable(True)
    for name, lw in clouds:
        for apply in (False, True):
            ms, res = [], None
            for r in range(a.warmup + a.reps):
                e.set_log_weights(lw)
                e.timing_get()
                res = e.temper(a.ess_ratio, apply=apply)
                tm = e.timing_get()['normalise']
                assert tm[1] == 1, tm
                if r >= a.warmup:
                    ms.append(tm[0])
            report('temper_%s%s' % (name, '_applied' if apply else ''), ms, src, region='normalise', launches=9 if apply else 8,
                   j=res.j, beta=res.beta, levels_evaluated=res.levels_evaluated, floor_hit=res.floor_hit, n_target=res.n_target)
    ws, norm = [], []
    for r in range(a.warmup + a.reps):
        e.set_log_weights(clouds[0][1])
        e.timing_get()
        e.weight_stats()
        tw = e.timing_get()['normalise']
        e.resample()
        tn = e.timing_get()['normalise']
        if r >= a.warmup:
            ws.append(tw[0])
            norm.append(tn[0])
    report('weight_stats', ws, src, region='normalise', launches=2)
    report('resample_normalise', norm, src, region='normalise')
    e.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
