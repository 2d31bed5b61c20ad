#!/usr/bin/env python3
"""tools/ranges_timing.py -- device time of one DVL / altimeter range update (mcl_update_ranges) on the GPU.

For every map of the matrix -- the 512 x 512 height grid, the 708 x 708 lattice mesh, the irregular TIN over the same
terrain (synth.mesh_tin) and that TIN cast as a triangle soup (MCL_MESH_GENERAL) -- and for B = 1 (the altitude) and
B = 4 (Janus beams 25 degrees off vertical): 1 048 576 particles around a track point, warm-up updates, then --reps
updates, each timed by the library's HIP events (mcl_timing_enable / mcl_timing_get: one MCL_K_UPDATE_MBES region per
update).  Prints one JSON line per case with the median and the 10 / 90 % quantiles; every number carries its source.
Run it under `timeout` on the GPU box:  timeout -k 10 600 python3 tools/ranges_timing.py"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smarc_navigation_amd import engine, synth  # noqa: E402


def janus(tilt_deg=25.0):
    t = math.radians(tilt_deg)
    return np.array([[math.sin(t) * math.cos(a), math.sin(t) * math.sin(a), -math.cos(t)]
                     for a in (0.25 * math.pi, 0.75 * math.pi, 1.25 * math.pi, 1.75 * math.pi)], np.float32)


def maps(which):
    out = []
    if 'grid' in which:
        origin = (-64.0, -256.0)
        out.append(('grid_512', dict(z=synth.bathymetry_grid(512, 512, 1.0, origin, seed=3), origin=origin)))
    origin = (-64.0, -354.0)
    z = synth.bathymetry_grid(708, 708, 1.0, origin, seed=3)
    if 'mesh' in which:
        v, t = synth.mesh_from_grid(z, 1.0, origin)
        out.append(('lattice_mesh_708', dict(verts=v, tris=t)))
    if 'tin' in which or 'soup' in which:
        v, t = synth.mesh_tin(z, 1.0, origin, seed=7)
        if 'tin' in which:
            out.append(('tin_708', dict(verts=v, tris=t)))
        if 'soup' in which:
            out.append(('tin_708_as_soup', dict(verts=v, tris=t, general=True)))
    return out


def cloud(n, seed=1):
    """a cloud around a track point of the bench (x, y sigma 2 m, 2 m deep, small attitudes, yaw +-0.05 rad)"""
    rs = np.random.RandomState(seed)
    soa = np.zeros((6, n))
    soa[0] = 40.0 + 2.0 * rs.randn(n)
    soa[1] = 10.0 + 2.0 * rs.randn(n)
    soa[2] = -2.0 + 0.1 * rs.randn(n)
    soa[3] = 0.02 * rs.randn(n)
    soa[4] = 0.02 * rs.randn(n)
    soa[5] = 0.3 + 0.05 * rs.randn(n)
    return soa


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--maps', default='grid,mesh,tin,soup')
    a = ap.parse_args()
    soa = cloud(a.particles)
    src = 'measured: HIP events around each mcl_update_ranges launch (mcl_timing_get after every update), median of %d after %d warm-up updates' % (
        a.reps, a.warmup)
    for name, m in maps(a.maps.split(',')):
        e = engine.Engine(a.particles, rng_mode=engine.RNG_REPLAY)
        if 'z' in m:
            e.set_map_grid(m['z'], m['origin'], 1.0)
        else:
            e.set_map_mesh(m['verts'], m['tris'], general=m.get('general', False))
        e.set_particles(soa)
        for B, dirs in ((1, np.array([[0.0, 0.0, -1.0]], np.float32)), (4, janus())):
            ranges = e.ranges_expected(0, 1, dirs, 60.0)[0] + np.float32(0.05)
            e.timing_enable(True)
            for _ in range(a.warmup):
                e.update_ranges(ranges, dirs, 0.2, 60.0)
            e.timing_get()
            ms = []
            for _ in range(a.reps):
                e.update_ranges(ranges, dirs, 0.2, 60.0)
                t = e.timing_get()['update_mbes']
                assert t[1] == 1, t
                ms.append(t[0])
            e.timing_enable(False)
            lw = e.get_log_weights()
            ms = np.array(ms)
            print(json.dumps(dict(map=name, particles=a.particles, beams=B, median_ms=round(float(np.median(ms)), 5),
                                  p10_ms=round(float(np.quantile(ms, 0.1)), 5), p90_ms=round(float(np.quantile(ms, 0.9)), 5),
                                  rays_per_s=float('%.3g' % (a.particles * B / (np.median(ms) * 1e-3))),
                                  lw_finite=bool(np.isfinite(lw).all()), source=src)), flush=True)
        e.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
