#!/usr/bin/env python3
"""tools/modes_timing.py -- device time of mcl_pose_modes (include/mcl_modes.h) on the GPU, 1 048 576 particles.

HIP events of the library (mcl_timing_enable / mcl_timing_get, region MCL_K_MEAN_COV), median of --reps after --warmup
warm-up rounds, on the 192 m footprint of the recovery scenario (191 x 191 cells of 1 m, 36 yaw bins, k = 4 and k = 1) for
  * a uniform cloud (mcl_init_particles_uniform over the footprint, the full circle),
  * a tracking cloud (sigma 2 m, 0.1 rad),
  * a cloud collapsed into ONE cell (every add of the histogram on one address but for the wave aggregation),
and beside each, from the same handle in the same run, mcl_mean_cov (its two regions added): existing code that streams
the same state.  Prints one JSON line per figure; every number carries its source.
Run it under `timeout` on the GPU box:  timeout -k 10 600 python3 tools/modes_timing.py"""
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
    ap.add_argument('--cell', type=float, default=1.0)
    ap.add_argument('--n-yaw', type=int, default=36)
    a = ap.parse_args()
    n = a.particles
    src = 'measured: HIP events around the launches (mcl_timing_get after every call), median of %d after %d warm-ups, %d particles' % (
        a.reps, a.warmup, n)
    origin = (-96.0, -96.0)
    z = synth.bathymetry_grid(192, 192, 1.0, origin, seed=2, swell=2.0, fbm_amp=3.0)
    e = engine.Engine(n, seed=17)
    e.set_map_grid(z, origin, 1.0)
    lattice = e.mode_grid(a.cell, a.n_yaw)
    cells = lattice.nx * lattice.ny * lattice.n_yaw
    rs = np.random.RandomState(1)

    def uniform():
        e.init_particles_uniform()

    def tracking():
        s = np.zeros((6, n))
        s[0], s[1], s[5] = -40.0 + 2.0 * rs.randn(n), -30.0 + 2.0 * rs.randn(n), 0.5 + 0.1 * rs.randn(n)
        e.set_particles(s)

    def collapsed():
        s = np.zeros((6, n))
        s[0], s[1], s[5] = -40.0 + 0.9 * rs.rand(n), -30.0 + 0.9 * rs.rand(n), 0.01 + 0.15 * rs.rand(n)
        e.set_particles(s)

    e.timing_enable(True)
    for name, make in (('uniform', uniform), ('tracking', tracking), ('collapsed', collapsed)):
        make()
        rows = {'pose_modes_k4': [], 'pose_modes_k1': [], 'mean_cov': []}
        info = {}
        for r in range(a.warmup + a.reps):
            e.timing_get()
            for fig, k in (('pose_modes_k4', 4), ('pose_modes_k1', 1)):
                modes, n_out = e.pose_modes(None, k=k, grid=lattice)
                tm = e.timing_get()['mean_cov']
                assert tm[1] == 1, (fig, tm)
                if r >= a.warmup:
                    rows[fig].append(tm[0])
                info[fig] = dict(n_modes=len(modes), n_outside=n_out, mode0_count=modes[0].count if modes else 0)
            e.mean_cov()
            tm = e.timing_get()['mean_cov']
            assert tm[1] == 2, tm
            if r >= a.warmup:
                rows['mean_cov'].append(tm[0])
        for fig in rows:
            report('%s_%s' % (fig, name), rows[fig], src, region='mean_cov', cloud=name, cells=cells, **info.get(fig, {}))
    e.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
