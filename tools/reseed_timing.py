#!/usr/bin/env python3
"""tools/reseed_timing.py -- what the sensor resetting (include/mcl_reseed.h) costs on the GPU, and how wide the basin of
the swath match is that its start lattice has to cover.

  * inject_*: Engine.inject_gaussian at 2^20 particles for fraction 0.01 / 0.1 / 1 and 1 / 16 / 256 components, beside
    Engine.inject_uniform at the same fractions in the same run.  `kernel_us`: the library's own events around the launch
    (mcl_timing_get, slot MCL_K_NOISE; the calls made with count=False, so the region holds the one kernel), `call_us`: the
    host's wall time of the whole call with count=True (the table's upload, both launches, the count's copy back and its one
    synchronisation); medians of --reps after --warmup calls.
  * step_*: the whole recovery.SensorResetting step (starts -> match_swath -> reseed_select -> inject_gaussian) at K = 4 and
    64 beams, a fraction of 0.1, 65 536 particles, 4 yaws in a window of +-0.4 rad: on the 192 x 192 grid of the closed-loop
    tests (pitch 4 m: 9 216 starts) and on the 708 x 708 TIN of the other timing tools (pitch 8 m: 31 684 starts; pitch 4 m
    would be above the 65 536 starts one match call takes).  Host wall time, median of --step-reps.
  * basin_*: on the 192 x 192 grid, K = 4, noise-free pings at --basin-points track points: of the lattice starts (pitch 2 /
    4 / 8 m) within one pitch of the truth, with the yaw 0.1 / 0.2 / 0.4 rad off either way, the share that ends CONVERGED
    within 0.5 m of the truth.  The defaults of recovery.SensorResetting and of tests/test_gpu_reseed.py are read off it.
Appends one JSON line per figure to profiles/reseed_timing.jsonl (and prints it); every number carries its source.  Nothing
is asserted about the numbers.  Run it under `timeout` on the GPU box:  timeout -k 10 500 python3 tools/reseed_timing.py"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N = 1 << 20
FRACTIONS = (0.01, 0.1, 1.0)
COMPONENTS = (1, 16, 256)
BOX = (-90.0, 90.0, -90.0, 90.0)
SIGMA, R_MAX, K, BEAMS = 1.5, 80.0, 4, 64
GRID_ORIGIN = (-96.0, -96.0)


def _median(vals):
    v = np.array(vals)
    return round(float(np.median(v)), 1), round(float(np.quantile(v, 0.1)), 1), round(float(np.quantile(v, 0.9)), 1)


def _table(engine, n_comp, seed=3):
    rs = np.random.RandomState(seed)
    c = np.zeros(n_comp, engine.ReseedComponent)
    c['mean'][:, 0], c['mean'][:, 1] = rs.uniform(-90, 90, n_comp), rs.uniform(-90, 90, n_comp)
    c['mean'][:, 2] = rs.uniform(-math.pi, math.pi, n_comp)
    c['chol'][:, 0], c['chol'][:, 2], c['chol'][:, 5] = 0.5, 0.5, 0.05
    c['chol'][:, 1], c['chol'][:, 3], c['chol'][:, 4] = 0.1, 0.01, -0.01
    c['mass'] = 1
    return c


def inject_cases(a, engine):
    src = ('measured: kernel_us = mcl_timing_get (events around the launch, MCL_K_NOISE) of calls without a count; call_us = host '
           'clock around the call with its count; medians of %d after %d warm-up calls' % (a.reps, a.warmup))
    e = engine.Engine(N, seed=5, init_cov=[4, 4, 0, 0, 0, 0.1])
    e.init_particles()
    e.timing_enable(True)
    lines = []

    def measure(name, call, extra):
        kern, wall = [], []
        for k in range(a.warmup + a.reps):
            e.timing_get()                           # (reading the slots empties them)
            call(False)
            ms = e.timing_get()['noise'][0]
            t0 = time.perf_counter()
            call(True)
            dt = (time.perf_counter() - t0) * 1e6
            if k >= a.warmup:
                kern.append(ms * 1e3)
                wall.append(dt)
        ku, k10, k90 = _median(kern)
        cu, c10, c90 = _median(wall)
        lines.append(json.dumps(dict(figure=name, particles=N, kernel_us=ku, kernel_p10_us=k10, kernel_p90_us=k90, call_us=cu,
                                     call_p10_us=c10, call_p90_us=c90, source=src, **extra)))
        print(lines[-1], flush=True)

    for f in FRACTIONS:
        measure('inject_uniform_f%g' % f, lambda count, f=f: e.inject_uniform(f, BOX, frame='odom', count=count), dict(fraction=f))
        for nc in COMPONENTS:
            comps = _table(engine, nc)
            measure('inject_gaussian_f%g_c%d' % (f, nc), lambda count, f=f, comps=comps: e.inject_gaussian(f, comps, count=count),
                    dict(fraction=f, components=nc))
    e.close()
    return lines


class _Always(object):
    """an AugmentedMCL that always asks for the same fraction"""

    def __init__(self, f):
        self.f = f

    def fraction(self):
        return self.f

    def injected(self):
        pass


def _pings(e, synth, truth6, ba):
    """K noise-free pings 1 m apart along the heading behind the anchor `truth6`: (ranges K x B, poses 6 x K, newest last)"""
    back = K - 1 - np.arange(K)
    track = np.repeat(np.asarray(truth6, np.float64)[:, None], K, axis=1)
    track[0] -= back * math.cos(truth6[5])
    track[1] -= back * math.sin(truth6[5])
    e.set_particles(np.concatenate([track, np.repeat(track[:, -1:], e.n - K, axis=1)], axis=1))
    return e.mbes_expected(0, K, ba, R_MAX).astype(np.float32), track


def step_cases(a, engine, synth):
    from smarc_navigation_amd.recovery import SensorResetting
    from ranges_timing import maps
    src = 'measured: host clock around SensorResetting.step, median of %d after 1 warm-up step' % a.step_reps
    lines = []
    ba = synth.beam_angles(BEAMS)
    scenes = [('grid_192', dict(z=synth.bathymetry_grid(192, 192, 1.0, GRID_ORIGIN, seed=2, swell=2.0, fbm_amp=3.0), origin=GRID_ORIGIN),
               4.0, [-10.0, 5.0, -2.0, 0.0, 0.0, 0.5])]
    scenes += [(name, m, 8.0, [40.0, 10.0, -2.0, 0.0, 0.0, 0.3]) for name, m in maps(['tin'])]
    for name, m, pitch, truth in scenes:
        e = engine.Engine(1 << 16, seed=7)
        if 'z' in m:
            e.set_map_grid(m['z'], m['origin'], 1.0)
        else:
            e.set_map_mesh(m['verts'], m['tris'], heightfield=True)
        rng, track = _pings(e, synth, truth, ba)
        e.init_particles_uniform()
        sr = SensorResetting(_Always(0.1), engine.make_reseed_select_config(dead_std_xy=pitch), pitch, 4, yaw_window=0.4, pings=K)
        for k in range(K):
            sr.push(rng[k], track[:, k])
        us = []
        for k in range(1 + a.step_reps):
            t0 = time.perf_counter()
            sr.step(e, ba, SIGMA, R_MAX)
            e.sync()
            if k:
                us.append((time.perf_counter() - t0) * 1e6)
        med, p10, p90 = _median(us)
        first = sr.last['match'].results[sr.last['indices'][0]] if sr.last['components'] else None
        lines.append(json.dumps(dict(
            figure='step_%s' % name, map=name, pitch=pitch, n_yaw=4, yaw_window=0.4, pings=K, beams=BEAMS, particles=1 << 16,
            starts=sr.last['starts'], components=sr.last['components'], injected=sr.last['injected'],
            first_component_error_m=None if first is None else round(math.hypot(first['x'] - truth[0], first['y'] - truth[1]), 4),
            step_us=med, p10_us=p10, p90_us=p90, source=src)))
        print(lines[-1], flush=True)
        e.close()
    return lines


def basin_cases(a, engine, synth):
    src = ('measured: Engine.match_swath on the 192 x 192 grid, K = 4, 64 beams, noise-free pings at %d track points; starts = the '
           'lattice nodes within one pitch of the truth, the yaw off by the offset either way' % a.basin_points)
    z = synth.bathymetry_grid(192, 192, 1.0, GRID_ORIGIN, seed=2, swell=2.0, fbm_amp=3.0)
    ba = synth.beam_angles(BEAMS)
    e = engine.Engine(64)
    e.set_map_grid(z, GRID_ORIGIN, 1.0)
    st = synth.odom_stream(n_steps=90, dt=1.0, x0=-40.0, y0=-30.0, yaw0=0.5)
    at = np.linspace(K, 89, a.basin_points).astype(int)
    lines = []
    for pitch in (2.0, 4.0, 8.0):
        for off in (0.1, 0.2, 0.4):
            good = total = 0
            for k in at:
                ring = range(k - K + 1, k + 1)
                e.set_particles(np.concatenate([st['truth'][list(ring)].T, np.repeat(st['truth'][k][:, None], 64 - K, axis=1)], axis=1))
                rng = e.mbes_expected(0, K, ba, R_MAX).astype(np.float32)
                truth = st['truth'][k]
                offsets = engine.swath_offsets(st['truth'][list(ring)].T, -1)
                lat = e.reseed_starts(None, pitch, (truth[5], truth[5]), 1, z=truth[2])
                near = np.hypot(lat[0] - truth[0], lat[1] - truth[1]) <= pitch
                starts = np.concatenate([lat[:, near], lat[:, near]], axis=1)
                starts[5, :near.sum()] += off
                starts[5, near.sum():] -= off
                m = e.match_swath(starts, rng, ba, offsets, SIGMA, R_MAX)
                err = np.hypot(m.results['x'] - truth[0], m.results['y'] - truth[1])
                good += int(np.sum((m.status == 0) & (err <= 0.5)))
                total += starts.shape[1]
            lines.append(json.dumps(dict(figure='basin_p%g_y%g' % (pitch, off), pitch=pitch, yaw_offset=off, starts=total,
                                         share_within_half_a_metre=round(good / max(total, 1), 4), source=src)))
            print(lines[-1], flush=True)
    e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--step-reps', type=int, default=3)
    ap.add_argument('--basin-points', type=int, default=12)
    ap.add_argument('--only', default='inject,step,basin')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reseed_timing.jsonl'))
    a = ap.parse_args()
    from smarc_navigation_amd import engine, synth
    lines = []
    if 'inject' in a.only:
        lines += inject_cases(a, engine)
    if 'basin' in a.only:
        lines += basin_cases(a, engine, synth)
    if 'step' in a.only:
        lines += step_cases(a, engine, synth)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
